"""mmf_clip_train_epoch_trials / mmf_clip_contrastive_eval_trials (csrc/clip_train.hip) and
mmf_amd.clip_training.ClipProjectionTuner on the MI355X.

There is no tolerance in this file.  Every reduction of clip_train.hip has a fixed order and a trial's workgroups
read nothing of another trial's, so a trial trained beside others must give the BITS of the same trial trained
alone through mmf_clip_train_epoch / mmf_clip_contrastive_eval, whose distance to float64 tests/test_gpu_clip_train.py
owns.  Inputs are tests/clip_train_refs.py's draws / initial_params.
"""
import os
import sys

import numpy as np
import pytest
import torch

from tests import clip_train_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22
STRIDE, TMAX = 655364, 16
SENT = -7.0          # what the output buffers hold before a call
PAD = 1234.5         # the three floats between two trials' parameters


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _lib():
    import mmf_amd.hip as hip
    return hip, hip.load()


def _buf(dev, nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device=dev)


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, np.int32))


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, np.float64))


def _nsteps(N, b):
    return -(-N // b)


def stack(rows, dev):
    """float32 [T][P] -> device [T, STRIDE], PAD in the three floats after each trial's parameters."""
    out = np.full((len(rows), STRIDE), PAD, np.float32)
    for t, r in enumerate(rows):
        out[t, :R.N_PARAMS] = r
    return _t(out, dev)


def single_epoch(img, txt, perm, batch, lr, wd, max_norm, step0, p, m, v):
    """mmf_clip_train_epoch of one trial alone on device tensors [N_PARAMS] (in place) -> (loss, gnorm) numpy."""
    hip, lib = _lib()
    n = _nsteps(len(perm), batch)
    sl = torch.full((n,), SENT, dtype=torch.float32, device=p.device)
    sg = torch.full((n,), SENT, dtype=torch.float32, device=p.device)
    need = int(lib.mmf_clip_train_ws_bytes(batch))
    ws = _buf(p.device, need)
    permd = _t(perm, p.device)
    rc = lib.mmf_clip_train_epoch(hip.ptr(img), hip.ptr(txt), len(perm), hip.ptr(permd), batch, lr, R.BETAS[0],
                                  R.BETAS[1], R.EPS, wd, max_norm, step0, hip.ptr(p), hip.ptr(m), hip.ptr(v),
                                  hip.ptr(sl), hip.ptr(sg), None, hip.ptr(ws), need, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return sl.cpu().numpy(), sg.cpu().numpy()


def trials_epoch(img, txt, perms, batch, lr, wd, max_norm, step0, active, P, M, V, S, ws=None, trials=None,
                 ws_bytes=None, params_ptr=None):
    """mmf_clip_train_epoch_trials on stacked device tensors (in place) -> (rc, loss [T, S], gnorm [T, S], ws)."""
    hip, lib = _lib()
    T = P.shape[0] if trials is None else trials
    dev = P.device
    sl = torch.full((P.shape[0], S), SENT, dtype=torch.float32, device=dev)
    sg = torch.full((P.shape[0], S), SENT, dtype=torch.float32, device=dev)
    need = int(lib.mmf_clip_train_trials_ws_bytes(P.shape[0], 64))
    if ws is None:
        ws = _buf(dev, need)
    permd = _t(np.stack(perms).astype(np.int32), dev)
    b, l, w, mn, s0 = _i32(batch), _f64(lr), _f64(wd), _f64(max_norm), _i32(step0)
    a = None if active is None else _i32(active)
    rc = lib.mmf_clip_train_epoch_trials(
        hip.ptr(img), hip.ptr(txt), img.shape[0], T, hip.ptr(permd), b.ctypes.data, l.ctypes.data, w.ctypes.data,
        mn.ctypes.data, s0.ctypes.data, None if a is None else a.ctypes.data, R.BETAS[0], R.BETAS[1], R.EPS,
        hip.ptr(P) if params_ptr is None else params_ptr, hip.ptr(M), hip.ptr(V), hip.ptr(sl), hip.ptr(sg), S,
        hip.ptr(ws), need if ws_bytes is None else ws_bytes, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, sl.cpu().numpy(), sg.cpu().numpy(), ws


def _same_as_single(P, M, V, sl, sg, t, single):
    p, m, v, l, g = single
    n = len(l)
    for name, got, want in (("params", P[t, :R.N_PARAMS], p), ("exp_avg", M[t, :R.N_PARAMS], m),
                            ("exp_avg_sq", V[t, :R.N_PARAMS], v)):
        assert torch.equal(got, want), (t, name)
    assert np.array_equal(sl[t, :n], l) and np.array_equal(sg[t, :n], g), t
    assert (sl[t, n:] == SENT).all() and (sg[t, n:] == SENT).all(), t  # nothing past the trial's own steps
    for X in (P, M, V):  # nor between two trials' slices
        assert (X[t, R.N_PARAMS:] == (PAD if X is P else 0)).all(), t


def test_uneven_trials_are_bit_identical_to_single_runs_and_an_inactive_trial_is_untouched():
    """N = 37; batches 5 / 16 / 64 / 1: 8 / 3 / 1 / 37 steps, a 5-row and a 2-row tail, a 1-row minibatch (loss and
    gradient exactly 0); each trial its own lr, weight decay, max_norm and step0; two epochs, step0 carried over.  In
    a third call trial 1 is inactive (with a batch that would be rejected were it read)."""
    dev = _dev()
    N, T, S = 37, 4, 40
    batch, lr, wd = [5, 16, 64, 1], [1e-4, 3e-5, 1e-3, 1e-5], [0.01, 0.0, 0.05, 0.01]
    max_norm, step0 = [1.0, 0.5, 2.0, 1.0], [0, 3, 10, 100]
    img, txt = R.draws(N, 3)
    imgd, txtd = _t(img, dev), _t(txt, dev)
    g = np.random.default_rng(3)
    p0 = [R.initial_params(3 + t) for t in range(T)]
    P = stack(p0, dev)
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    alone = [[_t(p0[t], dev), torch.zeros(R.N_PARAMS, device=dev), torch.zeros(R.N_PARAMS, device=dev)] for t in range(T)]
    s0 = list(step0)
    ws = None
    for epoch in range(2):
        perms = [g.permutation(N).astype(np.int32) for _ in range(T)]
        rc, sl, sg, ws = trials_epoch(imgd, txtd, perms, batch, lr, wd, max_norm, s0, None, P, M, V, S, ws)
        assert rc == 0
        for t in range(T):
            l, n = single_epoch(imgd, txtd, perms[t], batch[t], lr[t], wd[t], max_norm[t], s0[t], *alone[t])
            assert len(l) == _nsteps(N, batch[t])
            _same_as_single(P, M, V, sl, sg, t, alone[t] + [l, n])
            s0[t] += len(l)
        assert (sl[3, :37] == 0).all() and (sg[3, :37] == 0).all()  # the 1-row minibatches
        assert np.isfinite(sl[:3, 0]).all() and (sl[:3, 0] > 0).all()
    # ---- trial 1 inactive ----
    hip, lib = _lib()
    image = int(lib.mmf_clip_train_ws_bytes(64))
    before = [X[1].clone() for X in (P, M, V)] + [ws[image:2 * image].clone()]
    perms = [g.permutation(N).astype(np.int32) for _ in range(T)]
    rc, sl, sg, ws = trials_epoch(imgd, txtd, perms, [5, 99, 64, 1], lr, wd, max_norm, s0, [1, 0, 1, 1], P, M, V, S, ws)
    assert rc == 0
    for a, b in zip(before, [X[1] for X in (P, M, V)] + [ws[image:2 * image]]):
        assert torch.equal(a, b)
    assert (sl[1] == SENT).all() and (sg[1] == SENT).all()
    for t in (0, 2, 3):  # and its neighbours did not notice
        l, n = single_epoch(imgd, txtd, perms[t], batch[t], lr[t], wd[t], max_norm[t], s0[t], *alone[t])
        _same_as_single(P, M, V, sl, sg, t, alone[t] + [l, n])


def test_sixteen_trials_are_bit_identical_to_single_runs():
    """The full width: T = 16, N = 17, batch 16 (a 16-row minibatch and a 1-row one); trials 3 and 11 have the
    same settings, permutation and starting point and so the same bits."""
    dev = _dev()
    N, T, S = 17, TMAX, 2
    img, txt = R.draws(N, 9)
    imgd, txtd = _t(img, dev), _t(txt, dev)
    g = np.random.default_rng(9)
    lr = list(np.exp(g.uniform(np.log(1e-5), np.log(1e-3), T)))
    perms = [g.permutation(N).astype(np.int32) for _ in range(T)]
    p0 = [R.initial_params(20 + t) for t in range(T)]
    lr[11], perms[11], p0[11] = lr[3], perms[3], p0[3]
    P = stack(p0, dev)
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    rc, sl, sg, _ = trials_epoch(imgd, txtd, perms, [16] * T, lr, [R.WD] * T, [R.MAX_NORM] * T, [0] * T, None, P, M, V, S)
    assert rc == 0
    for t in range(T):
        one = [_t(p0[t], dev), torch.zeros(R.N_PARAMS, device=dev), torch.zeros(R.N_PARAMS, device=dev)]
        l, n = single_epoch(imgd, txtd, perms[t], 16, lr[t], R.WD, R.MAX_NORM, 0, *one)
        _same_as_single(P, M, V, sl, sg, t, one + [l, n])
    for X in (P, M, V):
        assert torch.equal(X[3], X[11])
    assert np.array_equal(sl[3], sl[11]) and np.array_equal(sg[3], sg[11])
    assert not torch.equal(P[3], P[4])


def test_eval_trials_are_bit_identical_to_single_evals():
    hip, lib = _lib()
    dev = _dev()
    N, T, batch = 21, 3, [8, 16, 5]
    img, txt = R.draws(N, 5)
    imgd, txtd = _t(img, dev), _t(txt, dev)
    p0 = [R.initial_params(5 + t) for t in range(T)]
    P = stack(p0, dev)
    ref = P.clone()
    S = 6
    bl = torch.full((T, S), SENT, dtype=torch.float32, device=dev)
    rcos = torch.full((T, N), SENT, dtype=torch.float32, device=dev)
    need = int(lib.mmf_clip_train_trials_ws_bytes(T, 64))
    ws = _buf(dev, need)
    b = _i32(batch)
    rc = lib.mmf_clip_contrastive_eval_trials(hip.ptr(imgd), hip.ptr(txtd), N, T, b.ctypes.data, None, hip.ptr(P),
                                              hip.ptr(bl), hip.ptr(rcos), S, hip.ptr(ws), need, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(P, ref)  # forward only
    need1 = int(lib.mmf_clip_train_ws_bytes(64))
    ws1 = _buf(dev, need1)
    for t in range(T):
        nb = _nsteps(N, batch[t])
        l1 = torch.full((nb,), SENT, dtype=torch.float32, device=dev)
        c1 = torch.full((N,), SENT, dtype=torch.float32, device=dev)
        p = _t(p0[t], dev)
        assert lib.mmf_clip_contrastive_eval(hip.ptr(imgd), hip.ptr(txtd), N, batch[t], hip.ptr(p), hip.ptr(l1),
                                             hip.ptr(c1), hip.ptr(ws1), need1, hip.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(bl[t, :nb], l1) and torch.equal(rcos[t], c1), t
        assert (bl[t, nb:] == SENT).all() and not (l1 == SENT).any() and not (c1 == SENT).any()
    # an inactive trial's rows stay as they were
    bl.fill_(SENT)
    rcos.fill_(SENT)
    a = _i32([1, 0, 1])
    rc = lib.mmf_clip_contrastive_eval_trials(hip.ptr(imgd), hip.ptr(txtd), N, T, b.ctypes.data, a.ctypes.data,
                                              hip.ptr(P), hip.ptr(bl), hip.ptr(rcos), S, hip.ptr(ws), need,
                                              hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and (bl[1] == SENT).all() and (rcos[1] == SENT).all() and not (rcos[[0, 2]] == SENT).any()


def test_rejected_calls_are_einval_with_nothing_launched():
    hip, lib = _lib()
    dev = _dev()
    N, T, S = 32, 2, 4
    img, txt = R.draws(N, 4)
    imgd, txtd = _t(img, dev), _t(txt, dev)
    perms = [np.arange(N, dtype=np.int32)] * (TMAX + 1)
    assert lib.mmf_clip_train_trials_ws_bytes(0, 64) == 0 and lib.mmf_clip_train_trials_ws_bytes(17, 64) == 0
    assert lib.mmf_clip_train_trials_ws_bytes(2, 65) == 0 and lib.mmf_clip_train_trials_ws_bytes(2, 0) == 0
    assert lib.mmf_clip_train_trials_ws_bytes(3, 16) == 3 * lib.mmf_clip_train_ws_bytes(16)
    # buffers for 17 trials' worth of arguments, so that a call that was NOT rejected would stay inside them
    big = TMAX + 1
    P = stack([R.initial_params(4)] * big, dev)
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    refP = P.clone()
    ws = _buf(dev, int(lib.mmf_clip_train_ws_bytes(64)) * big)
    need2 = int(lib.mmf_clip_train_trials_ws_bytes(T, 64))
    shifted = hip.ptr(P) + 4  # a stacked params 4 bytes off its boundary
    cases = (dict(trials=0), dict(trials=big), dict(batch=[16, 65]), dict(ws_bytes=need2 - 1),
             dict(params_ptr=shifted), dict(batch=[0, 16]), dict(S=1))
    for kw in cases:
        trials = kw.get("trials", T)
        n = max(trials, T)
        batch = kw.get("batch", [16] * n)
        rc, sl, sg, _ = trials_epoch(imgd, txtd, perms[:big], batch, [1e-4] * n, [R.WD] * n, [1.0] * n, [0] * n, None,
                                     P, M, V, kw.get("S", S), ws, trials=trials,
                                     ws_bytes=kw.get("ws_bytes", ws.numel() if trials != T else need2),
                                     params_ptr=kw.get("params_ptr"))
        assert rc == EINVAL, kw
        assert lib.mmf_last_error()
        assert torch.equal(P, refP) and not M.any() and not V.any() and (sl == SENT).all() and (sg == SENT).all(), kw
        assert not ws.any(), kw
    # the eval call's
    bl = torch.full((big, S), SENT, dtype=torch.float32, device=dev)
    rcos = torch.full((big, N), SENT, dtype=torch.float32, device=dev)
    for trials, batch, nbytes, pp in ((0, [16, 16], need2, hip.ptr(P)), (big, [16] * big, ws.numel(), hip.ptr(P)),
                                      (T, [16, 65], need2, hip.ptr(P)), (T, [16, 16], need2 - 1, hip.ptr(P)),
                                      (T, [16, 16], need2, shifted)):
        b = _i32(batch)
        assert lib.mmf_clip_contrastive_eval_trials(hip.ptr(imgd), hip.ptr(txtd), N, trials, b.ctypes.data, None, pp,
                                                    hip.ptr(bl), hip.ptr(rcos), S, hip.ptr(ws), nbytes,
                                                    hip.stream_ptr()) == EINVAL, (trials, batch, nbytes)
    torch.cuda.synchronize()
    assert (bl == SENT).all() and (rcos == SENT).all() and not ws.any() and torch.equal(P, refP)


# ---- end to end: ClipProjectionTuner on a synthetic-weights MisinfoForensics ----
def _forensics(golden, golden_inputs, det_sd, clip_sd):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    rob = {"sample text 0": golden["rob_ids"][0, :golden_inputs["rob_lens"][0]].tolist()}
    clp = {"sample text 0": golden["clip_ids"][0, :golden_inputs["clip_lens"][0]].tolist()}
    return MisinfoForensics(fusion_weights="/nonexistent", faiss_index_path="/nonexistent",
                            roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=TableClipProcessor(clp),
                            detector_state=det_sd, clip_state=dict(clip_sd), max_batch=24, verbose=False)


def test_tuner_end_to_end(golden, golden_inputs, det_sd, clip_sd, tmp_path):
    _dev()
    import mmf_amd.clip_training as CT
    import mmf_amd.synthetic as syn
    import mmf_amd.vault_builder as VB
    from mmf_amd.engine import Engine
    f = _forensics(golden, golden_inputs, det_sd, clip_sd)
    eng = f.engine
    N = 24
    imgs = syn.images(N, 17)
    cid, cm = syn.clip_ids(N, 77, 17)
    ti, tt = (t.cpu().numpy() for t in eng.clip_pooled(imgs, cid, cm))
    labels = np.arange(N) % 2
    start = {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v)) for k, v in f.clip_state.items()
             if k in CT.KEYS}
    trials = [{"lr": 1e-4, "batch_size": 8, "epochs": 3}, {"lr": 5e-4, "batch_size": 16, "epochs": 2},
              {"lr": 3e-5, "batch_size": 12, "epochs": 1, "seed": 5, "weight_decay": 0.0}]
    # every trial alone through fit, from the same starting heads (fit installs its result)
    alone = []
    for tr in trials:
        f.clip_state.update({k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v)) for k, v in start.items()})
        alone.append(CT.ClipProjectionTrainer(f, batch_size=tr["batch_size"], epochs=tr["epochs"], lr=tr["lr"],
                                              weight_decay=tr.get("weight_decay", 0.01),
                                              seed=tr.get("seed", 1)).fit((ti, tt), (ti, tt), labels))
    # the starting heads again, in forensics and in the engine's towers
    f.clip_state.update(start)
    CT.ClipProjectionTrainer(f)._install(CT.split_heads(CT.flatten_heads(f.clip_state)))
    nbytes = eng.device_bytes
    ck_path = str(tmp_path / "clip_detective_best.pth")
    res = CT.ClipProjectionTuner(f, trials=trials, seed=1).tune((ti, tt), (ti, tt), labels, checkpoint_path=ck_path)
    assert eng.device_bytes == nbytes
    assert [t["number"] for t in res["trials"]] == [0, 1, 2]
    for t, hist in zip(res["trials"], alone):
        assert t["history"] == hist, (t["number"], t["history"], hist)
    # the study's rule: the loss at the best-accuracy epoch (the first epoch reaching it), minimised, ties low
    values = []
    for hist in alone:
        best = max(hist, key=lambda h: (h["val_accuracy"], -h["epoch"]))
        values.append(best["val_loss"] if best["val_accuracy"] > 0 else float("inf"))
    assert [t["value"] for t in res["trials"]] == values
    assert res["best_trial"] == int(np.argmin(values)) and res["best_value"] == min(values)
    assert res["best_params"] == {k: trials[res["best_trial"]][k] for k in ("lr", "batch_size", "epochs")}
    # the checkpoint is the winner's best epoch, and a fresh engine on it gives the tuned engine's bits
    sd, meta = VB.load_clip_detective_checkpoint(ck_path)
    win = alone[res["best_trial"]]
    assert meta["epoch"] == max(win, key=lambda h: (h["val_accuracy"], -h["epoch"]))["epoch"]
    assert np.array_equal(CT.flatten_heads(sd).numpy(), CT.flatten_heads(f.clip_state).numpy())
    assert not np.array_equal(CT.flatten_heads(sd).numpy(), CT.flatten_heads(start).numpy())
    cons = eng.clip_consistency(imgs, cid, cm)["sim"].clone()
    fresh = Engine(0, None, sd, eos_token_id=golden_inputs["eos"], max_batch=24)
    assert torch.equal(fresh.clip_consistency(imgs, cid, cm)["sim"], cons)
    fresh.close()
    eng.close()
