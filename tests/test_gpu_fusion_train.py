"""mmf_fusion_train_epoch (csrc/fusion_train.hip) and mmf_amd/fusion_training.py on the MI355X.

Kernel: initial parameters = W.synthetic_detector_state(0)'s fusion_layer.*, scores drawn as SURVEY 8d's C1
distribution (tests/fusion_train_refs.py).  References are the float64 restatement (equal to a real torch loop:
tests/test_fusion_train_refs_cpu.py); bounds are derived there, never from what the kernel returned.

Multi-step bound: K = max |kernel - float64| over all parameters must stay within 8 x max(e32, 1e-7 x steps),
e32 = the float32 restatement's same error (8: another summation order and expf; the floor is a couple of
half-ulps of parameters below 1 per step, so a luckily small e32 does not tighten the bound).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import fusion_train_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev)


def launch(x, y, perm, keep, batch, lr, step0, p, m, v, p_drop=R.P_DROP, grad=False, N=None):
    """One mmf_fusion_train_epoch on device tensors (p, m, v updated in place) -> (loss, correct, grad) numpy."""
    import mmf_amd.hip as hip
    lib = hip.load()
    N = len(y) if N is None else N
    nsteps = max(1, -(-N // max(batch, 1)))
    sl = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    sc = torch.full((nsteps,), -7, dtype=torch.int32, device=p.device)
    g = torch.zeros(R.N_PARAMS, dtype=torch.float32, device=p.device) if grad else None
    rc = lib.mmf_fusion_train_epoch(hip.ptr(x), hip.ptr(y), N, hip.ptr(perm), hip.ptr(keep), p_drop, batch, lr,
                                    R.BETAS[0], R.BETAS[1], R.EPS, R.WD, step0, hip.ptr(p), hip.ptr(m), hip.ptr(v),
                                    hip.ptr(sl), hip.ptr(sc), hip.ptr(g), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, sl.cpu().numpy(), sc.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _state(dev, p0=None):
    p = _t(R.initial_params() if p0 is None else p0, dev)
    return p, torch.zeros_like(p), torch.zeros_like(p)


# ---- single step, per element ----
@pytest.mark.parametrize("masked", [True, False], ids=["masks", "nokeep"])
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_single_step_gradient_per_element(B, masked):
    dev = _dev()
    x, y = R.draws(B, R.SINGLE_SEED)
    perm = np.random.default_rng(B).permutation(B).astype(np.int32)
    mask = R.masks(B, R.SINGLE_SEED) if masked else None  # row i: the row at POSITION i
    b = R.step_bounds(x[perm], y[perm].astype(np.int64), mask, R.P_DROP, R.initial_params().astype(np.float64))
    lg = b["r"]["logits"]
    assert (np.abs(lg[:, 1] - lg[:, 0]) > b["margin_tol"]).all(), "the reference's margins do not decide step_correct"
    p, m, v = _state(dev)
    keep = _t(R.pack_keep(mask), dev) if masked else None
    rc, sl, sc, g = launch(_t(x, dev), _t(y, dev), _t(perm, dev), keep, B, 1e-2, 0, p, m, v, grad=True)
    assert rc == 0
    err = np.abs(g - b["grad"])
    print(f"B={B} masked={masked}: max grad err {err.max():.3g} (largest err / bound {(err[b['grad_tol'] > 0] / b['grad_tol'][b['grad_tol'] > 0]).max():.3g}),"
          f" loss err {abs(sl[0] - b['r']['loss']):.3g} (bound {b['loss_tol']:.3g})")
    assert (err <= b["grad_tol"]).all(), int((err > b["grad_tol"]).sum())
    assert abs(float(sl[0]) - b["r"]["loss"]) <= b["loss_tol"]
    assert int(sc[0]) == b["r"]["correct"]
    # and the step it took is the float64 one's, at the multi-step bound of ONE step
    p64 = R.initial_params().astype(np.float64)
    p32 = R.initial_params()
    for dt, q in ((np.float64, p64), (np.float32, p32)):
        R.epoch(x, y, perm, None if mask is None else R.pack_keep(mask), R.P_DROP, B, 1e-2, 0, q, np.zeros_like(q),
                np.zeros_like(q), dt)
    K, e32 = np.abs(p.cpu().numpy() - p64).max(), np.abs(p32 - p64).max()
    assert K <= 8 * max(e32, 1e-7), (K, e32)


# ---- multi-step ----
@functools.lru_cache(maxsize=None)
def _case_refs(case):
    return R.run_case(*case, np.float64), R.run_case(*case, np.float32)


@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: f"N{c[0]}-b{c[1]}-e{c[2]}")
def test_multi_step_tracks_float64(case):
    dev = _dev()
    N, batch, epochs, lr = case
    (p64, m64, v64, l64, c64, margin, plan, cond), (p32, m32, v32, _, _, _, _, _) = _case_refs(case)
    assert margin > 1e-4, margin  # so step_correct must be exact
    assert cond <= 8e-7 * sum(len(l) for l in l64), cond  # a well-conditioned reference (fusion_train_refs)
    x, y = R.draws(N)
    xd, yd = _t(x, dev), _t(y, dev)
    p, m, v = _state(dev)
    step0 = 0
    for e, (perm, keep) in enumerate(plan):
        rc, sl, sc, _ = launch(xd, yd, _t(perm, dev), _t(keep, dev), batch, lr, step0, p, m, v)
        assert rc == 0
        step0 += len(sl)
        assert np.array_equal(sc, c64[e]), (e, sc, c64[e])
        assert np.isfinite(sl).all()
    e32 = float(np.abs(p32 - p64).max())
    K = float(np.abs(p.cpu().numpy() - p64).max())
    Km, Kv = float(np.abs(m.cpu().numpy() - m64).max()), float(np.abs(v.cpu().numpy() - v64).max())
    print(f"case {case}: K = {K:.3g}, e32 = {e32:.3g}, steps = {step0}, bound = {8 * max(e32, 1e-7 * step0):.3g}; "
          f"moments: {Km:.3g} (f32 {np.abs(m32 - m64).max():.3g}), {Kv:.3g} (f32 {np.abs(v32 - v64).max():.3g})")
    assert K <= 8 * max(e32, 1e-7 * step0), (K, e32)


# ---- invariance ----
def _epoch32(dev, N=32, batch=16, seed=3):
    x, y = R.draws(N)
    g = np.random.default_rng(seed)
    perm = g.permutation(N).astype(np.int32)
    keep = R.pack_keep(g.uniform(size=(N, 64)) >= R.P_DROP)
    return x, y, perm, keep


def _all(p, m, v):
    return [t.cpu().numpy().copy() for t in (p, m, v)]


def test_same_launch_twice_is_bit_identical():
    dev = _dev()
    x, y, perm, keep = _epoch32(dev, N=300, batch=64)
    outs = []
    for _ in range(2):
        p, m, v = _state(dev)
        rc, sl, sc, g = launch(_t(x, dev), _t(y, dev), _t(perm, dev), _t(keep, dev), 64, 1e-2, 4, p, m, v, grad=True)
        assert rc == 0
        outs.append(_all(p, m, v) + [sl, sc, g])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_an_epoch_split_into_two_launches_is_bit_identical():
    dev = _dev()
    x, y, perm, keep = _epoch32(dev)
    p, m, v = _state(dev)
    rc, sl, sc, _ = launch(_t(x, dev), _t(y, dev), _t(perm, dev), _t(keep, dev), 16, 1e-2, 5, p, m, v)
    assert rc == 0 and len(sl) == 2
    q, qm, qv = _state(dev)
    parts = []
    for h in range(2):  # 16 positions each: their rows gathered, the identity permutation, their masks
        rows = perm[16 * h:16 * h + 16]
        rc, l, c, _ = launch(_t(x[rows], dev), _t(y[rows], dev), _t(np.arange(16, dtype=np.int32), dev),
                             _t(keep[16 * h:16 * h + 16], dev), 16, 1e-2, 5 + h, q, qm, qv)
        assert rc == 0
        parts.append((l, c))
    for a, b in zip(_all(p, m, v), _all(q, qm, qv)):
        assert np.array_equal(a, b)
    assert np.array_equal(sl, np.concatenate([l for l, _ in parts]))
    assert np.array_equal(sc, np.concatenate([c for _, c in parts]))


def test_tail_minibatch_uses_its_own_row_count():
    """N = 37, batch = 16: the third minibatch has 5 rows.  Run alone from the state after two steps -- once as
    the tail of a 16-row batch size, once as a whole minibatch of 5 -- it gives the same bits, and its loss is
    the float64 mean over 5 rows."""
    dev = _dev()
    x, y, perm, keep = _epoch32(dev, N=37)
    p, m, v = _state(dev)
    rc, sl, sc, g = launch(_t(x, dev), _t(y, dev), _t(perm, dev), _t(keep, dev), 16, 1e-2, 0, p, m, v, grad=True)
    assert rc == 0 and len(sl) == 3
    q, qm, qv = _state(dev)
    rows = perm[:32]
    rc, _, _, _ = launch(_t(x[rows], dev), _t(y[rows], dev), _t(np.arange(32, dtype=np.int32), dev),
                         _t(keep[:32], dev), 16, 1e-2, 0, q, qm, qv)
    assert rc == 0
    before_tail = q.cpu().numpy().astype(np.float64)
    tails = []
    for batch in (16, 5):
        t, tm, tv = q.clone(), qm.clone(), qv.clone()
        rows = perm[32:]
        rc, l, c, gt = launch(_t(x[rows], dev), _t(y[rows], dev), _t(np.arange(5, dtype=np.int32), dev),
                              _t(keep[32:], dev), batch, 1e-2, 2, t, tm, tv, grad=True)
        assert rc == 0 and len(l) == 1
        tails.append(_all(t, tm, tv) + [l, c, gt])
    for a, b in zip(*tails):
        assert np.array_equal(a, b)
    for a, b in zip(_all(p, m, v) + [sl[2:], sc[2:], g], tails[0]):
        assert np.array_equal(a, b)
    b = R.step_bounds(x[perm[32:]], y[perm[32:]].astype(np.int64), R.unpack_keep(keep[32:]), R.P_DROP, before_tail)
    assert abs(float(sl[2]) - b["r"]["loss"]) <= b["loss_tol"]
    assert (np.abs(g - b["grad"]) <= b["grad_tol"]).all()


def test_out_of_range_permutation_entries_are_clamped():
    dev = _dev()
    x, y, perm, keep = _epoch32(dev, N=37)
    wild = perm.copy()
    wild[[0, 7, 20, 36]] = [-5, 37, 2 ** 31 - 1, -2 ** 31]
    outs = []
    for pr in (wild, np.clip(wild, 0, 36)):
        p, m, v = _state(dev)
        rc, sl, sc, _ = launch(_t(x, dev), _t(y, dev), _t(pr, dev), _t(keep, dev), 16, 1e-2, 0, p, m, v)
        assert rc == 0
        outs.append(_all(p, m, v) + [sl, sc])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_bad_arguments_are_einval_with_nothing_launched():
    import mmf_amd.hip as hip
    dev = _dev()
    x, y, perm, keep = _epoch32(dev)
    xd, yd, pd, kd = _t(x, dev), _t(y, dev), _t(perm, dev), _t(keep, dev)
    p, m, v = _state(dev)
    p0 = p.clone()
    for kw in (dict(batch=0), dict(batch=257), dict(N=0), dict(p_drop=1.0), dict(batch=-3), dict(p_drop=-0.1),
               dict(p_drop=float("nan")), dict(N=-1)):
        args = dict(batch=16, p_drop=R.P_DROP, N=None)
        args.update(kw)
        rc, sl, sc, _ = launch(xd, yd, pd, kd, args["batch"], 1e-2, 0, p, m, v, p_drop=args["p_drop"], N=args["N"])
        assert rc == EINVAL, kw
        assert hip.load().mmf_last_error()
        assert torch.equal(p, p0) and not m.any() and not v.any() and (sl == -7).all() and (sc == -7).all()
    lib = hip.load()
    sl = torch.zeros(2, dtype=torch.float32, device=dev)
    sc = torch.zeros(2, dtype=torch.int32, device=dev)
    ptrs = [hip.ptr(t) for t in (xd, yd, pd, p, m, v, sl, sc)]
    for missing in range(8):
        a = list(ptrs)
        a[missing] = None
        rc = lib.mmf_fusion_train_epoch(a[0], a[1], 32, a[2], hip.ptr(kd), R.P_DROP, 16, 1e-2, 0.9, 0.999, 1e-8, 0.01, 0,
                                        a[3], a[4], a[5], a[6], a[7], None, hip.stream_ptr())
        assert rc == EINVAL, missing
    torch.cuda.synchronize()
    assert torch.equal(p, p0)


# ---- end to end: extract_scores, FusionTrainer, checkpoint ----
SCORE_KEYS = ("ai_score", "misinfo_score", "deepfake_score", "clip_similarity", "vault_discrepancy")


def _tables(golden, gi):
    rob, clp = {}, {}
    for i in range(golden["rob_ids"].shape[0]):
        t = f"sample text {i}"
        rob[t] = golden["rob_ids"][i, :gi["rob_lens"][i]].tolist()
        clp[t] = golden["clip_ids"][i, :gi["clip_lens"][i]].tolist()
    for j, ids in enumerate(gi["title_ids"]):
        clp[f"Guardian article {j}"] = ids.tolist()
    for extra in ("missing file", "truncated file"):
        rob[extra], clp[extra] = rob["sample text 0"], clp["sample text 0"]
    first = clp["sample text 1"]
    rob["long caption"] = rob["sample text 1"]
    clp["long caption"] = [first[0]] + [first[1]] * 78 + [first[-1]]  # 80 CLIP tokens
    return rob, clp


def _forensics(golden, golden_inputs, det_sd, clip_sd, fusion_weights="/nonexistent"):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    rob, clp = _tables(golden, golden_inputs)
    mf = MisinfoForensics(fusion_weights=fusion_weights, faiss_index_path="/nonexistent",
                          roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=TableClipProcessor(clp),
                          detector_state=det_sd, clip_state=clip_sd, max_batch=16, verbose=False)
    mf.set_vault(golden_inputs["vault"], golden_inputs["meta"])
    return mf


def test_extract_train_checkpoint_end_to_end(golden, golden_json, golden_inputs, det_sd, clip_sd, tmp_path):
    _dev()
    from PIL import Image
    import mmf_amd.fusion_training as FT
    forensics = _forensics(golden, golden_inputs, det_sd, clip_sd)
    texts, paths, labels = [], [], []
    for i in range(8):
        p = str(tmp_path / f"img{i}.png")
        Image.fromarray(golden_inputs["imgs"][i]).save(p)
        texts.append(f"sample text {i}")
        paths.append(p)
        labels.append(i % 2)
    cut = str(tmp_path / "cut.png")
    whole = open(paths[0], "rb").read()
    open(cut, "wb").write(whole[:len(whole) // 2])
    # the three bad rows in between the good ones
    texts[3:3] = ["missing file"]
    paths[3:3] = [str(tmp_path / "nope.png")]
    texts[6:6] = ["long caption"]
    paths[6:6] = [paths[1]]
    texts.append("truncated file")
    paths.append(cut)
    good = [i for i in range(11) if i not in (3, 6, 10)]

    want = np.array([[ref["scores"][k] for k in SCORE_KEYS] for ref in golden_json["analyze"][:8]])
    # without the undecodable file: one batched chunk, no single-image ViT pass
    v0 = forensics.vit_passes
    scores, ok = FT.extract_scores(forensics, texts[:10], paths[:10])
    assert forensics.vit_passes == v0, "the batched path was not taken"
    assert ok.tolist() == [i in good for i in range(10)]
    assert (scores[[3, 6]] == 0).all()
    d_gold = float(np.abs(scores[good] - want).max())
    rows = np.array([FT._row_scores(forensics, texts[i], paths[i]) for i in good], np.float32)
    d_rows = float(np.abs(scores[good] - rows).max())
    print(f"extract_scores: max |batched - golden.json| = {d_gold:.3g}, max |batched - per-row| = {d_rows:.3g}")
    assert d_gold < 1e-3 and d_rows < 1e-3
    # with it: the chunk raises while it is staged and is redone row by row
    scores_all, ok_all = FT.extract_scores(forensics, texts, paths)
    assert forensics.vit_passes > v0 + 8
    assert ok_all.tolist() == [i in good for i in range(11)]
    assert (scores_all[[3, 6, 10]] == 0).all()
    assert np.array_equal(scores_all[good], rows)
    assert float(np.abs(scores_all[good] - want).max()) < 1e-3

    # ---- FusionTrainer.fit: 3 epochs at batch 4 ----
    det = forensics.detector
    before = {k: v.clone() for k, v in det.fusion_layer.state_dict().items()}
    forensics.fusion_verdict(dict(zip(SCORE_KEYS, scores[0].tolist())))
    up_f, up_t = det.uploads["fusion"], det.uploads["text"]
    ck_path = str(tmp_path / "forensics_master_final.pth")
    hist = FT.FusionTrainer(forensics, batch_size=4, epochs=3, lr=1e-2, seed=1).fit(scores[good], labels,
                                                                                    checkpoint_path=ck_path)
    assert len(hist) == 3 and all(np.isfinite(h["loss"]) for h in hist)
    after = det.fusion_layer.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    assert all(v.device == forensics.device for v in after.values())
    det.eval()
    with torch.no_grad():
        p_ref = torch.softmax(det.forward_fusion(torch.from_numpy(scores[good]).to(forensics.device)), 1).cpu().numpy()
    for n, i in enumerate(good):
        vd = forensics.fusion_verdict(dict(zip(SCORE_KEYS, scores[i].tolist())))
        assert abs(vd["fake_probability"] - p_ref[n, 1]) < 1e-5 and abs(vd["real_probability"] - p_ref[n, 0]) < 1e-5
    assert det.uploads["fusion"] > up_f and det.uploads["text"] == up_t

    # ---- the checkpoint, found by a fresh system's constructor ----
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "fusion_layer_state_dict", "full_model_state_dict", "optimizer_state_dict",
                       "scheduler_state_dict", "loss", "accuracy"}
    opt = torch.optim.AdamW(det.fusion_layer.parameters())
    opt.load_state_dict(ck["optimizer_state_dict"])
    assert all(float(opt.state[p]["step"]) == 2 * ck["epoch"] for p in det.fusion_layer.parameters())
    # the layer now holds the LAST epoch's parameters; the file the best epoch's: compare through the file
    det.load_state_dict(ck["full_model_state_dict"])
    pairs_before = forensics.analyze_pairs([texts[i] for i in good], [paths[i] for i in good])
    forensics.engine.close()
    fresh = _forensics(golden, golden_inputs, det_sd, clip_sd, fusion_weights=ck_path)
    for k, v in fresh.detector.fusion_layer.state_dict().items():
        assert torch.equal(v.cpu(), ck["fusion_layer_state_dict"][k]), k
    pairs_after = fresh.analyze_pairs([texts[i] for i in good], [paths[i] for i in good])
    for a, b in zip(pairs_before, pairs_after):
        assert a["verdict"] == b["verdict"] and a["scores"] == b["scores"]
    fresh.engine.close()
