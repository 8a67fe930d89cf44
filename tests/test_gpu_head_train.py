"""mmf_head_train_epoch / mmf_head_eval (csrc/head_train.hip), mmf_text_pooled and mmf_amd/head_training.py on the
MI355X.

Kernel references are the float64 restatement of tests/head_train_refs.py (equal to a real torch loop:
tests/test_head_train_refs_cpu.py); bounds are derived there, never from what the kernel returned.

Multi-step bound: K = max |kernel - float64| over all parameters must stay within 8 x max(e32, FLOOR x steps, cond):
e32 = the float32 restatement's same error, FLOOR = 2^-27 per step (two half-ulps of a parameter below 0.125) and
cond = the float64 run's conditioning number (head_train_refs' docstring).  The CPU test asserts on the reference
alone that this bound is below a tenth of the distance the parameters move.

Pooled rows: tests/test_gpu_clip_train.py's bar for LayerNorm rows of an fp16-stream tower, relative to the row
norm: |pooled - reference| <= sqrt(2e-4) |reference|.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import head_train_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22
REL = float(np.sqrt(2e-4))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _keep(keep, dev):
    return None if keep is None else _t(keep.view(np.int64), dev)


_WS = {}


def _ws(dev, batch=16):
    import mmf_amd.hip as hip
    need = int(hip.load().mmf_head_train_ws_bytes(batch))
    assert need > 0
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
    return _WS["ws"], need


def launch(feat, labels, perm, keep, batch, lrs, step0, p, m, v, grad=False, N=None, ws_bytes=None, p_drop=R.P_DROP,
           max_norm=R.MAX_NORM):
    """One mmf_head_train_epoch on device tensors (p, m, v updated in place) -> (rc, loss, correct, gnorm, grad)
    numpy."""
    import mmf_amd.hip as hip
    lib = hip.load()
    N = len(perm) if N is None else N
    nsteps = max(1, -(-N // max(batch, 1)))
    lrs = np.ascontiguousarray(np.broadcast_to(np.asarray(lrs, np.float64), (nsteps,)))
    sl = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    sg = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    sc = torch.full((nsteps,), -7, dtype=torch.int32, device=p.device)
    g = torch.zeros(R.N_PARAMS, dtype=torch.float32, device=p.device) if grad else None
    ws, need = _ws(p.device)
    rc = lib.mmf_head_train_epoch(hip.ptr(feat), hip.ptr(labels), N, hip.ptr(perm), hip.ptr(keep), p_drop, batch,
                                  lrs.ctypes.data, R.BETAS[0], R.BETAS[1], R.EPS, R.WD, max_norm, step0, hip.ptr(p),
                                  hip.ptr(m), hip.ptr(v), hip.ptr(sl), hip.ptr(sc), hip.ptr(sg), hip.ptr(g),
                                  hip.ptr(ws), need if ws_bytes is None else ws_bytes, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, sl.cpu().numpy(), sc.cpu().numpy(), sg.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _state(dev, p0):
    p = _t(p0, dev)
    return p, torch.zeros_like(p), torch.zeros_like(p)


def _all(p, m, v):
    return [t.cpu().numpy().copy() for t in (p, m, v)]


# ---- single step, per element ----
@pytest.mark.parametrize("dropout", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("regime", ["clip", "noclip"])
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_single_step_gradient_per_element(B, regime, dropout):
    dev = _dev()
    feat, labels, perm, keep, p0, max_norm, b, seed = R.single_case(B, regime, dropout)
    # both branches decided by the reference alone
    assert b["relu_ok"] and ((b["norm"] > 1.5 * max_norm) if regime == "clip" else (b["norm"] < 0.67 * max_norm))
    lr = 1e-3
    p, m, v = _state(dev, p0)
    rc, sl, sc, sg, g = launch(_t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), B, lr, 0, p, m, v,
                               grad=True, max_norm=max_norm)
    assert rc == 0
    err, tol = np.abs(g - b["grad"]), b["grad_tol"]
    nz = tol > 0
    print(f"B={B} {regime} keep={dropout} (seed {seed}): norm {b['norm']:.4g} coef {b['coef']:.3g}; max grad err "
          f"{err.max():.3g} (largest err / bound {(err[nz] / tol[nz]).max():.3g}), loss err "
          f"{abs(sl[0] - b['loss']):.3g} (bound {b['loss_tol']:.3g}), norm err {abs(sg[0] - b['norm']):.3g} (bound "
          f"{b['norm_tol']:.3g})")
    assert (err <= tol).all(), int((err > tol).sum())
    assert abs(float(sl[0]) - b["loss"]) <= b["loss_tol"]
    assert abs(float(sg[0]) - b["norm"]) <= b["norm_tol"]
    assert sc[0] == b["r"]["correct"]
    # and the step it took is the float64 one's, at the multi-step bound of ONE step
    p64, p32 = p0.astype(np.float64), p0.copy()
    for dt, q in ((np.float64, p64), (np.float32, p32)):
        R.epoch(feat, labels, perm, keep, B, [lr], 0, q, np.zeros_like(q), np.zeros_like(q), dt, max_norm=max_norm)
    K, e32 = np.abs(p.cpu().numpy() - p64).max(), np.abs(p32 - p64).max()
    print(f"  one step: K = {K:.3g}, e32 = {e32:.3g}")
    assert K <= 8 * max(e32, R.FLOOR), (K, e32)


def test_a_step_with_lr_zero_moves_the_moments_only():
    """The schedule's first value is 0 (warmup): parameters bit-unchanged, moments updated."""
    dev = _dev()
    feat, labels, perm, keep, p0, max_norm, b, _ = R.single_case(16, "clip", True)
    p, m, v = _state(dev, p0)
    rc, sl, _, sg, _ = launch(_t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), 16, 0.0, 0, p, m, v)
    assert rc == 0 and np.isfinite(sl).all()
    assert np.array_equal(p.cpu().numpy(), p0)
    m64, v64 = (1 - R.BETAS[0]) * b["grad"], (1 - R.BETAS[1]) * b["grad"] ** 2
    # m = (1 - beta1) g and v = (1 - beta2) g^2 of a gradient within its per-element bound (+ 4 U of the value)
    tol, ag = b["grad_tol"], np.abs(b["grad"])
    assert m.cpu().numpy().any() and v.cpu().numpy().any()
    assert (np.abs(m.cpu().numpy() - m64) <= (1 - R.BETAS[0]) * tol + 4 * R.U * np.abs(m64)).all()
    assert (np.abs(v.cpu().numpy() - v64) <= (1 - R.BETAS[1]) * (2 * ag * tol + tol * tol) + 4 * R.U * v64).all()


# ---- multi-step ----
@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: f"N{c[0]}-b{c[1]}-e{c[2]}")
def test_multi_step_tracks_float64(case):
    dev = _dev()
    N, batch, epochs = case
    p64, m64, v64, l64, n64, plan, cond, p0 = R.run_case(*case, np.float64)
    p32, m32, v32 = R.run_case(*case, np.float32)[:3]
    steps = sum(len(l) for l in l64)
    feat, labels = R.draws(N, R.MULTI_SEED)
    featd, labd = _t(feat, dev), _t(labels, dev)
    p, m, v = _state(dev, p0)
    step0 = 0
    for e, (perm, keep, lrs) in enumerate(plan):
        rc, sl, sc, sg, _ = launch(featd, labd, _t(perm, dev), _keep(keep, dev), batch, lrs, step0, p, m, v)
        assert rc == 0
        step0 += len(sl)
        assert np.isfinite(sl).all() and np.isfinite(sg).all()
        np.testing.assert_allclose(sl, l64[e], rtol=0, atol=2e-2)  # coarse: the per-element test owns the loss
        np.testing.assert_allclose(sg, n64[e], rtol=2e-2, atol=0)
    assert step0 == steps
    e32 = float(np.abs(p32 - p64).max())
    bound = 8 * max(e32, R.FLOOR * steps, cond)
    K = float(np.abs(p.cpu().numpy() - p64).max())
    Km, Kv = float(np.abs(m.cpu().numpy() - m64).max()), float(np.abs(v.cpu().numpy() - v64).max())
    moved = float(np.abs(p64 - p0).max())
    print(f"case {case}: K = {K:.3g}, e32 = {e32:.3g}, cond = {cond:.3g}, steps = {steps}, bound = {bound:.3g} "
          f"({bound / moved:.3g} of the movement {moved:.3g}); moments: {Km:.3g} (f32 {np.abs(m32 - m64).max():.3g}), "
          f"{Kv:.3g} (f32 {np.abs(v32 - v64).max():.3g})")
    assert K <= bound, (K, e32, cond)


# ---- invariance ----
def _epoch(N=37, seed=3):
    feat, labels = R.draws(N, seed)
    g = np.random.default_rng(seed)
    return (feat, labels, g.permutation(N).astype(np.int32), R.pack_keep(g.random((N, R.H)) >= R.P_DROP),
            R.initial_params(seed))


def test_same_launch_twice_is_bit_identical():
    dev = _dev()
    feat, labels, perm, keep, p0 = _epoch(N=130)
    outs = []
    for _ in range(2):
        p, m, v = _state(dev, p0)
        rc, sl, sc, sg, g = launch(_t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), 64,
                                   [1e-3, 5e-4, 2e-4], 4, p, m, v, grad=True)
        assert rc == 0 and len(sl) == 3
        outs.append(_all(p, m, v) + [sl, sc, sg, g])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_an_epoch_split_into_two_launches_is_bit_identical():
    dev = _dev()
    feat, labels, perm, keep, p0 = _epoch(N=32)
    lrs = np.array([0.0, 1e-3])
    p, m, v = _state(dev, p0)
    rc, sl, sc, sg, _ = launch(_t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), 16, lrs, 5, p, m, v)
    assert rc == 0 and len(sl) == 2
    q, qm, qv = _state(dev, p0)
    parts = []
    for h in range(2):  # 16 positions each: their rows and masks gathered, the identity permutation, step0 carried
        rows = perm[16 * h:16 * h + 16]
        rc, l, c, n, _ = launch(_t(feat[rows], dev), _t(labels[rows], dev), _t(np.arange(16, dtype=np.int32), dev),
                                _keep(keep[16 * h:16 * h + 16], dev), 16, lrs[h:h + 1], 5 + h, q, qm, qv)
        assert rc == 0
        parts.append((l, c, n))
    for a, b in zip(_all(p, m, v), _all(q, qm, qv)):
        assert np.array_equal(a, b)
    for k, whole in enumerate((sl, sc, sg)):
        assert np.array_equal(whole, np.concatenate([part[k] for part in parts]))


def test_tail_minibatch_gives_the_bits_of_a_whole_batch():
    """N = 37, batch = 16: the third minibatch has 5 rows.  Run alone from the state after two steps -- once as the
    tail of a 16-row batch size, once as a whole minibatch of 5 -- it gives the same bits."""
    dev = _dev()
    feat, labels, perm, keep, p0 = _epoch(N=37)
    lrs = np.array([1e-3, 8e-4, 6e-4])
    p, m, v = _state(dev, p0)
    rc, sl, sc, sg, g = launch(_t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), 16, lrs, 0, p, m, v,
                               grad=True)
    assert rc == 0 and len(sl) == 3
    q, qm, qv = _state(dev, p0)
    rows = perm[:32]
    rc = launch(_t(feat[rows], dev), _t(labels[rows], dev), _t(np.arange(32, dtype=np.int32), dev),
                _keep(keep[:32], dev), 16, lrs[:2], 0, q, qm, qv)[0]
    assert rc == 0
    tails = []
    rows = perm[32:]
    for batch in (16, 5):
        t, tm, tv = q.clone(), qm.clone(), qv.clone()
        rc, l, c, n, gt = launch(_t(feat[rows], dev), _t(labels[rows], dev), _t(np.arange(5, dtype=np.int32), dev),
                                 _keep(keep[32:], dev), batch, lrs[2:], 2, t, tm, tv, grad=True)
        assert rc == 0 and len(l) == 1
        tails.append(_all(t, tm, tv) + [l, c, n, gt])
    for a, b in zip(*tails):
        assert np.array_equal(a, b)
    for a, b in zip(_all(p, m, v) + [sl[2:], sc[2:], sg[2:], g], tails[0]):
        assert np.array_equal(a, b)


def test_out_of_range_permutation_entries_are_clamped_and_labels_masked():
    dev = _dev()
    feat, labels, perm, keep, p0 = _epoch(N=37)
    wild = perm.copy()
    wild[[0, 7, 20, 36]] = [-5, 37, 2 ** 31 - 1, -2 ** 31]
    odd = labels.copy()
    odd[::3] += 2 * np.arange(len(odd[::3]), dtype=np.int32)  # read as label & 1
    outs = []
    for pr, lb in ((wild, odd), (np.clip(wild, 0, 36), labels)):
        p, m, v = _state(dev, p0)
        rc, sl, sc, sg, _ = launch(_t(feat, dev), _t(lb, dev), _t(pr, dev), _keep(keep, dev), 16, 1e-3, 0, p, m, v)
        assert rc == 0
        outs.append(_all(p, m, v) + [sl, sc, sg])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_bad_arguments_are_einval_with_nothing_launched():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    feat, labels, perm, keep, p0 = _epoch(N=32)
    fd, ld, pd, kd = _t(feat, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev)
    p, m, v = _state(dev, p0)
    ref = p.clone()
    _, need = _ws(dev)
    assert lib.mmf_head_train_ws_bytes(0) == 0 and lib.mmf_head_train_ws_bytes(65) == 0
    assert lib.mmf_head_train_ws_bytes(1) > R.N_PARAMS * 4 and lib.mmf_head_train_ws_bytes(64) > R.N_PARAMS * 4
    for kw in (dict(batch=0), dict(batch=65), dict(N=0), dict(ws_bytes=need - 1), dict(batch=-3), dict(N=-1),
               dict(ws_bytes=0), dict(p_drop=1.0), dict(p_drop=-0.1), dict(p_drop=float("nan"))):
        args = dict(batch=16, N=None, ws_bytes=None, p_drop=R.P_DROP)
        args.update(kw)
        rc, sl, sc, sg, _ = launch(fd, ld, pd, kd, args["batch"], 1e-3, 0, p, m, v, N=args["N"],
                                   ws_bytes=args["ws_bytes"], p_drop=args["p_drop"])
        assert rc == EINVAL, kw
        assert lib.mmf_last_error()
        assert torch.equal(p, ref) and not m.any() and not v.any()
        assert (sl == -7).all() and (sg == -7).all() and (sc == -7).all()
    sl = torch.zeros(2, dtype=torch.float32, device=dev)
    sg = torch.zeros(2, dtype=torch.float32, device=dev)
    sc = torch.zeros(2, dtype=torch.int32, device=dev)
    ws, need = _ws(dev)
    lrs = np.array([1e-3, 1e-3])
    ptrs = [hip.ptr(t) for t in (fd, ld, pd)] + [lrs.ctypes.data] + [hip.ptr(t) for t in (p, m, v, sl, sc, sg, ws)]

    def call(a, ws_ptr=None):
        return lib.mmf_head_train_epoch(a[0], a[1], 32, a[2], hip.ptr(kd), 0.3, 16, a[3], 0.9, 0.999, 1e-8, 0.01, 1.0, 0,
                                        a[4], a[5], a[6], a[7], a[8], a[9], None, a[10] if ws_ptr is None else ws_ptr,
                                        need, hip.stream_ptr())
    for missing in range(11):  # each required pointer in turn (keep and grad_out may be NULL)
        a = list(ptrs)
        a[missing] = None
        assert call(a) == EINVAL, missing
    big = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    assert call(ptrs, ws_ptr=hip.ptr(big) + 4) == EINVAL  # a misaligned workspace
    bl, lg = torch.zeros(2, device=dev), torch.zeros(32, 2, device=dev)
    for batch, N, nb in ((0, 32, need), (65, 32, need), (16, 0, need), (16, 32, need - 1)):
        assert lib.mmf_head_eval(hip.ptr(fd), hip.ptr(ld), N, batch, hip.ptr(p), hip.ptr(bl), hip.ptr(lg), hip.ptr(ws),
                                 nb, hip.stream_ptr()) == EINVAL
    ev = [hip.ptr(t) for t in (fd, ld, p, bl, lg, ws)]
    for missing in range(6):
        a = list(ev)
        a[missing] = None
        assert lib.mmf_head_eval(a[0], a[1], 32, 16, a[2], a[3], a[4], a[5], need, hip.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(p, ref) and not m.any() and not v.any() and not bl.any() and not lg.any()
    assert not sl.any() and not sg.any() and not sc.any()


# ---- eval ----
def _eval(feat, labels, batch, p, dev):
    import mmf_amd.hip as hip
    N = len(labels)
    bl = torch.zeros(-(-N // batch), dtype=torch.float32, device=dev)
    lg = torch.zeros(N, 2, dtype=torch.float32, device=dev)
    ws, need = _ws(dev)
    fd, ld = _t(feat, dev), _t(labels, dev)  # (named: alive until the synchronise)
    rc = hip.load().mmf_head_eval(hip.ptr(fd), hip.ptr(ld), N, batch, hip.ptr(p), hip.ptr(bl), hip.ptr(lg),
                                  hip.ptr(ws), need, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return bl.cpu().numpy(), lg.cpu().numpy()


def test_eval_against_float64():
    dev = _dev()
    N, batch = 21, 8
    feat, labels = R.draws(N, 5)
    p0 = R.initial_params(5)
    want_loss, want_lg = R.evaluate(feat, labels, batch, p0)
    p = _t(p0, dev)
    bl, lg = _eval(feat, labels, batch, p, dev)
    for k, a in enumerate(range(0, N, batch)):
        x = feat[a:a + batch]
        b = R.step_bounds(x, np.ones((len(x), R.H)), p0.astype(np.float64), labels[a:a + batch],
                          check_branches=False)  # the forward's bounds need neither branch
        assert abs(b["loss"] - want_loss[k]) < 1e-12
        d = np.abs(lg[a:a + batch] - want_lg[a:a + batch])
        print(f"eval batch {k}: loss err {abs(float(bl[k]) - want_loss[k]):.3g} (bound {b['loss_tol']:.3g}), max logit "
              f"err {d.max():.3g} (largest err / bound {(d / b['lg_tol']).max():.3g})")
        assert abs(float(bl[k]) - want_loss[k]) <= b["loss_tol"]
        assert (d <= b["lg_tol"]).all()
    assert torch.equal(p, _t(p0, dev))  # forward only


# ---- mmf_text_pooled, on the golden eight rows ----
@pytest.fixture(scope="module")
def engine(det_sd, golden_inputs):
    """text_precision "precise" keeps every layout's weights packed, so text_hilo can be switched."""
    _dev()
    from mmf_amd.engine import Engine
    eng = Engine(0, det_sd, None, max_batch=8, max_text_len=256, text_precision="precise")
    yield eng
    eng.close()


def _head_params(det_sd, head):
    return np.concatenate([np.asarray(det_sd[f"{head}.{k}"], np.float64).reshape(-1)
                           for k in ("0.weight", "0.bias", "3.weight", "3.bias")])


def _check_logits_agree(eng, det_sd, ids, mask, what):
    """text_forward's logits against the float64 heads on text_pooled's rows, within the fp32 bound of the head
    kernel's arithmetic; text_forward unchanged by the call in between."""
    before = [t.clone() for t in eng.text_forward(ids, mask)]
    cls = eng.text_pooled(ids, mask)
    after = eng.text_forward(ids, mask)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    cls = cls.cpu().numpy()
    assert cls.shape == (len(ids), 768) and np.isfinite(cls).all()
    for head, got in (("ai_head", before[0]), ("misinfo_head", before[1])):
        lg, tol = R.deployed_head_bounds(cls, _head_params(det_sd, head))
        d = np.abs(got.cpu().numpy() - lg)
        print(f"{what} {head}: max |text_forward - float64 head(pooled)| {d.max():.3g} (largest err / bound "
              f"{(d / tol).max():.3g})")
        assert (d <= tol).all(), (what, head)
    return cls


def test_text_pooled_on_the_golden_rows(engine, det_sd, golden):
    ids, mask = golden["rob_ids"], golden["rob_mask"]
    engine.set_option("text_hilo", 0)
    cls = _check_logits_agree(engine, det_sd, ids, mask, "fp16 stream").astype(np.float64)
    want = golden["cls_hidden"].astype(np.float64)
    rel = np.linalg.norm(cls - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"pooled CLS rows vs the reference run: max relative distance {rel.max():.3g} (bar {REL:.3g})")
    assert (rel <= REL).all(), rel
    for head, key in (("ai_head", "ai_logits"), ("misinfo_head", "misinfo_logits")):
        lg = R.deployed_head_bounds(cls, _head_params(det_sd, head))[0]
        d = np.abs(lg - golden[key]).max()
        print(f"float64 {head} on the pooled rows vs golden[{key}]: {d:.3g}")
        assert d <= 5e-3
    # the other stream layouts, and rows of a smaller batch
    for mode, name in ((1, "split stream"), (2, "precise mode")):
        engine.set_option("text_hilo", mode)
        assert engine.get_option("text_hilo_effective") == mode
        c = _check_logits_agree(engine, det_sd, ids, mask, name).astype(np.float64)
        rel = np.linalg.norm(c - want, axis=1) / np.linalg.norm(want, axis=1)
        print(f"  {name}: max relative distance {rel.max():.3g}")
        assert (rel <= REL).all(), (name, rel)
    engine.set_option("text_hilo", 0)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp16", "split", "precise"])
def test_text_pooled_long_sequences(engine, det_sd, mode):
    """Two rows at L = 130: the long-sequence attention path."""
    import mmf_amd.synthetic as syn
    ids, mask = syn.roberta_ids(2, 130, 41, [130, 77])
    engine.set_option("text_hilo", mode)
    try:
        _check_logits_agree(engine, det_sd, ids, mask, f"L=130 text_hilo={mode}")
    finally:
        engine.set_option("text_hilo", 0)


# ---- end to end: extract_text_features, HeadTrainer, the checkpoint the constructor loads ----
def _forensics(golden, golden_inputs, det_sd, clip_sd, **kw):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    rob = {}
    for i in range(golden["rob_ids"].shape[0]):
        rob[f"sample text {i}"] = golden["rob_ids"][i, :golden_inputs["rob_lens"][i]].tolist()
    first = rob["sample text 0"]
    rob["long text"] = first[:60] + first[1:60] + first[1:]  # 246 tokens
    args = dict(fusion_weights="/nonexistent", faiss_index_path="/nonexistent",
                roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=None, detector_state=det_sd,
                clip_state=dict(clip_sd), max_batch=24, verbose=False)
    args.update(kw)
    return MisinfoForensics(**args), rob


def test_extract_train_checkpoint_end_to_end(golden, golden_inputs, det_sd, clip_sd, tmp_path):
    dev = _dev()
    import mmf_amd.head_training as HT
    import mmf_amd.synthetic as syn
    f, rob = _forensics(golden, golden_inputs, det_sd, clip_sd)
    eng, det = f.engine, f.detector
    # ---- extract_text_features on the golden texts; a text longer than max_length equals its truncation ----
    texts = [f"sample text {i}" for i in range(8)]
    fe = HT.extract_text_features(f, texts + ["long text"], max_length=200)
    assert fe.shape == (9, 768) and fe.dtype == np.float32
    want = golden["cls_hidden"].astype(np.float64)
    assert (np.linalg.norm(fe[:8] - want, axis=1) <= REL * np.linalg.norm(want, axis=1)).all()
    cut = np.asarray([rob["long text"][:200]], np.int32)
    trunc = eng.text_pooled(cut, np.ones_like(cut))[0].cpu().numpy()
    assert np.linalg.norm(fe[8] - trunc) <= REL * np.linalg.norm(trunc)
    whole = np.asarray([rob["long text"]], np.int32)
    assert not np.array_equal(eng.text_pooled(whole, np.ones_like(whole))[0].cpu().numpy(), trunc)

    # ---- 24 synthetic rows, 2 epochs, batch 8 ----
    N = 24
    ids, mask = syn.roberta_ids(N, 64, 17)
    feats = eng.text_pooled(ids, mask).cpu().numpy()
    labels = (np.arange(N) % 2).astype(np.int32)
    before = HT.flatten_head(det.ai_head).cpu().numpy()
    mi_before = HT.flatten_head(det.misinfo_head).cpu().numpy()
    uploads, nbytes = dict(det.uploads), eng.device_bytes
    path = str(tmp_path / "ai_head_best.pth")
    hist = HT.HeadTrainer(f, head="ai_head", batch_size=8, epochs=2, lr=1e-3, seed=1).fit(
        feats, labels, feats, labels, checkpoint_path=path, save_full_model=False)
    assert [h["epoch"] for h in hist] == [1, 2] and all(np.isfinite(h["train_loss"]) for h in hist)
    after = HT.flatten_head(det.ai_head).cpu().numpy()
    assert not np.array_equal(before, after)
    assert np.array_equal(HT.flatten_head(det.misinfo_head).cpu().numpy(), mi_before)
    assert det.uploads["text"] == uploads["text"] + 1
    assert det.uploads["fusion"] == uploads["fusion"] and det.uploads["effnet"] == uploads["effnet"]
    assert eng.device_bytes == nbytes
    loss0 = R.evaluate(feats, labels, N, before.astype(np.float64))[0][0]
    loss1 = R.evaluate(feats, labels, N, after.astype(np.float64))[0][0]
    print(f"fit: float64 eval loss of the cached features {loss0:.4f} -> {loss1:.4f}; history {hist}")
    assert loss1 < loss0

    # ---- mmf_head_eval on the cached rows against detector.forward_text on the same ids, after installation ----
    _, lg = _eval(feats, labels, 8, _t(after, dev), dev)
    ai, mi = det.forward_text(ids, mask)
    assert det.uploads["text"] == uploads["text"] + 1  # nothing left to re-pack
    want_lg, tol_dep = R.deployed_head_bounds(feats, after.astype(np.float64))
    tol_eval = np.concatenate([R.step_bounds(feats[a:a + 8], np.ones((8, R.H)), after.astype(np.float64),
                                             labels[a:a + 8], check_branches=False)["lg_tol"] for a in range(0, N, 8)])
    d = np.abs(lg - ai.cpu().numpy())
    print(f"head_eval vs forward_text after the install: max {d.max():.3g} (largest err / bound "
          f"{(d / (tol_dep + tol_eval)).max():.3g})")
    assert (np.abs(lg - want_lg) <= tol_eval).all() and (d <= tol_dep + tol_eval).all()

    # ---- the checkpoint: the constructor's fallback path loads it ----
    ck = torch.load(path, map_location="cpu", weights_only=True)
    best = min(hist, key=lambda h: (h["val_loss"], h["epoch"]))
    assert ck["epoch"] == best["epoch"] and ck["val_loss"] == best["val_loss"]
    assert np.array_equal(torch.cat([ck["model_state_dict"][f"ai_head.{k}"].reshape(-1) for k in HT.PARAM_KEYS]).numpy(),
                          after)
    fresh, _ = _forensics(golden, golden_inputs, det_sd, clip_sd, ai_head_weights=path)
    assert np.array_equal(HT.flatten_head(fresh.detector.ai_head).cpu().numpy(), after)
    ai2, mi2 = fresh.detector.forward_text(ids, mask)
    assert torch.equal(ai2, ai) and torch.equal(mi2, mi)
    for x in (fresh, f):
        x.engine.close()
