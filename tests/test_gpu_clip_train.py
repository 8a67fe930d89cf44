"""mmf_clip_train_epoch / mmf_clip_contrastive_eval (csrc/clip_train.hip), mmf_clip_pooled,
mmf_set_clip_projections and mmf_amd/clip_training.py on the MI355X.

Kernel references are the float64 restatement of tests/clip_train_refs.py (equal to a real torch loop:
tests/test_clip_train_refs_cpu.py); bounds are derived there, never from what the kernel returned.

Multi-step bound: K = max |kernel - float64| over all parameters must stay within 8 x max(e32, FLOOR x steps),
e32 = the float32 restatement's same error and FLOOR = 2^-22 per step (two half-ulps of logit_scale ~ 2.66:
clip_train_refs' docstring), the rule of tests/test_gpu_fusion_train.py with this module's floor.

Pooled rows: tests/test_gpu_parity.py demands cos > 1 - 1e-4 of the unit CLIP embeddings of these towers, i.e.
|a - b| < sqrt(2e-4) for unit rows.  A LayerNorm output is not unit-norm, so the same bar is stated relative to
the row norm: |pooled - reference| <= sqrt(2e-4) |reference|.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import clip_train_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22
REL = float(np.sqrt(2e-4))  # the parity bar of unit embeddings as a relative distance


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_WS = {}


def _ws(dev, batch=16):
    import mmf_amd.hip as hip
    need = int(hip.load().mmf_clip_train_ws_bytes(batch))
    assert need > 0
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
    return _WS["ws"], need


def launch(img, txt, perm, batch, lr, step0, p, m, v, grad=False, N=None, ws_bytes=None):
    """One mmf_clip_train_epoch on device tensors (p, m, v updated in place) -> (rc, loss, gnorm, grad) numpy."""
    import mmf_amd.hip as hip
    lib = hip.load()
    N = len(perm) if N is None else N
    nsteps = max(1, -(-N // max(batch, 1)))
    sl = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    sg = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    g = torch.zeros(R.N_PARAMS, dtype=torch.float32, device=p.device) if grad else None
    ws, need = _ws(p.device)
    rc = lib.mmf_clip_train_epoch(hip.ptr(img), hip.ptr(txt), N, hip.ptr(perm), batch, lr, R.BETAS[0], R.BETAS[1],
                                  R.EPS, R.WD, R.MAX_NORM, step0, hip.ptr(p), hip.ptr(m), hip.ptr(v), hip.ptr(sl),
                                  hip.ptr(sg), hip.ptr(g), hip.ptr(ws), need if ws_bytes is None else ws_bytes,
                                  hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, sl.cpu().numpy(), sg.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _state(dev, p0):
    p = _t(p0, dev)
    return p, torch.zeros_like(p), torch.zeros_like(p)


def _all(p, m, v):
    return [t.cpu().numpy().copy() for t in (p, m, v)]


# ---- single step, per element ----
@pytest.mark.parametrize("regime", ["clip", "noclip"])
@pytest.mark.parametrize("B", R.SINGLE_BATCHES)
def test_single_step_gradient_per_element(B, regime):
    dev = _dev()
    img, txt, p0 = R.single_case(B, regime)
    perm = np.random.default_rng(B).permutation(B).astype(np.int32)
    b = R.step_bounds(img[perm], txt[perm], p0.astype(np.float64))
    if B > 1:  # both clipping regimes, decided by the reference alone
        assert (b["norm"] > 1.5) if regime == "clip" else (b["norm"] < 0.67), b["norm"]
    p, m, v = _state(dev, p0)
    rc, sl, sg, g = launch(_t(img, dev), _t(txt, dev), _t(perm, dev), B, 1e-4, 0, p, m, v, grad=True)
    assert rc == 0
    err, tol = np.abs(g - b["grad"]), b["grad_tol"]
    nz = tol > 0
    print(f"B={B} {regime}: norm {b['norm']:.4g} coef {b['coef']:.3g}; max grad err {err.max():.3g} (largest err / "
          f"bound {(err[nz] / tol[nz]).max() if nz.any() else 0:.3g}), loss err {abs(sl[0] - b['loss']):.3g} (bound "
          f"{b['loss_tol']:.3g}), norm err {abs(sg[0] - b['norm']):.3g} (bound {b['norm_tol']:.3g})")
    assert (err <= tol).all(), int((err > tol).sum())
    assert abs(float(sl[0]) - b["loss"]) <= b["loss_tol"]
    assert abs(float(sg[0]) - b["norm"]) <= b["norm_tol"]
    if B == 1:  # loss 0 and gradient 0, exactly; AdamW still decays
        assert sl[0] == 0 and sg[0] == 0 and not g.any()
        assert np.array_equal(p.cpu().numpy(), p0 * np.float32(1.0 - 1e-4 * R.WD))
    # and the step it took is the float64 one's, at the multi-step bound of ONE step
    p64, p32 = p0.astype(np.float64), p0.copy()
    for dt, q in ((np.float64, p64), (np.float32, p32)):
        R.epoch(img, txt, perm, B, 1e-4, 0, q, np.zeros_like(q), np.zeros_like(q), dt)
    K, e32 = np.abs(p.cpu().numpy() - p64).max(), np.abs(p32 - p64).max()
    print(f"  one step: K = {K:.3g}, e32 = {e32:.3g}")
    assert K <= 8 * max(e32, R.FLOOR), (K, e32)


# ---- multi-step ----
@functools.lru_cache(maxsize=None)
def _case_refs(case):
    return R.run_case(*case, np.float64), R.run_case(*case, np.float32)


@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: f"N{c[0]}-b{c[1]}-e{c[2]}")
def test_multi_step_tracks_float64(case):
    dev = _dev()
    N, batch, epochs = case
    (p64, m64, v64, l64, n64, plan, cond), (p32, m32, v32, _, _, _, _) = _case_refs(case)
    steps = sum(len(l) for l in l64)
    assert cond <= R.FLOOR * steps, cond  # a well-conditioned reference (clip_train_refs)
    img, txt = R.draws(N, R.MULTI_SEED)
    imgd, txtd = _t(img, dev), _t(txt, dev)
    p, m, v = _state(dev, R.initial_params(R.MULTI_SEED))
    step0 = 0
    for e, perm in enumerate(plan):
        rc, sl, sg, _ = launch(imgd, txtd, _t(perm, dev), batch, R.MULTI_LR, step0, p, m, v)
        assert rc == 0
        step0 += len(sl)
        assert np.isfinite(sl).all() and np.isfinite(sg).all()
        np.testing.assert_allclose(sl, l64[e], rtol=0, atol=2e-2)  # coarse: the per-element test owns the loss
    assert step0 == steps
    e32 = float(np.abs(p32 - p64).max())
    K = float(np.abs(p.cpu().numpy() - p64).max())
    Km, Kv = float(np.abs(m.cpu().numpy() - m64).max()), float(np.abs(v.cpu().numpy() - v64).max())
    print(f"case {case}: K = {K:.3g}, e32 = {e32:.3g}, steps = {steps}, bound = {8 * max(e32, R.FLOOR * steps):.3g}, "
          f"cond = {cond:.3g}; moments: {Km:.3g} (f32 {np.abs(m32 - m64).max():.3g}), {Kv:.3g} "
          f"(f32 {np.abs(v32 - v64).max():.3g})")
    assert K <= 8 * max(e32, R.FLOOR * steps), (K, e32)


# ---- invariance ----
def _epoch(N=37, seed=3):
    img, txt = R.draws(N, seed)
    return img, txt, np.random.default_rng(seed).permutation(N).astype(np.int32), R.initial_params(seed)


def test_same_launch_twice_is_bit_identical():
    dev = _dev()
    img, txt, perm, p0 = _epoch(N=130)
    outs = []
    for _ in range(2):
        p, m, v = _state(dev, p0)
        rc, sl, sg, g = launch(_t(img, dev), _t(txt, dev), _t(perm, dev), 64, 1e-4, 4, p, m, v, grad=True)
        assert rc == 0 and len(sl) == 3
        outs.append(_all(p, m, v) + [sl, sg, g])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_an_epoch_split_into_two_launches_is_bit_identical():
    dev = _dev()
    img, txt, perm, p0 = _epoch(N=32)
    p, m, v = _state(dev, p0)
    rc, sl, sg, _ = launch(_t(img, dev), _t(txt, dev), _t(perm, dev), 16, 1e-4, 5, p, m, v)
    assert rc == 0 and len(sl) == 2
    q, qm, qv = _state(dev, p0)
    parts = []
    for h in range(2):  # 16 positions each: their rows gathered, the identity permutation
        rows = perm[16 * h:16 * h + 16]
        rc, l, n, _ = launch(_t(img[rows], dev), _t(txt[rows], dev), _t(np.arange(16, dtype=np.int32), dev), 16, 1e-4,
                             5 + h, q, qm, qv)
        assert rc == 0
        parts.append((l, n))
    for a, b in zip(_all(p, m, v), _all(q, qm, qv)):
        assert np.array_equal(a, b)
    assert np.array_equal(sl, np.concatenate([l for l, _ in parts]))
    assert np.array_equal(sg, np.concatenate([n for _, n in parts]))


def test_tail_minibatch_gives_the_bits_of_a_whole_batch():
    """N = 37, batch = 16: the third minibatch has 5 rows.  Run alone from the state after two steps -- once as the
    tail of a 16-row batch size, once as a whole minibatch of 5 -- it gives the same bits."""
    dev = _dev()
    img, txt, perm, p0 = _epoch(N=37)
    p, m, v = _state(dev, p0)
    rc, sl, sg, g = launch(_t(img, dev), _t(txt, dev), _t(perm, dev), 16, 1e-4, 0, p, m, v, grad=True)
    assert rc == 0 and len(sl) == 3
    q, qm, qv = _state(dev, p0)
    rows = perm[:32]
    rc, _, _, _ = launch(_t(img[rows], dev), _t(txt[rows], dev), _t(np.arange(32, dtype=np.int32), dev), 16, 1e-4, 0,
                         q, qm, qv)
    assert rc == 0
    tails = []
    rows = perm[32:]
    for batch in (16, 5):
        t, tm, tv = q.clone(), qm.clone(), qv.clone()
        rc, l, n, gt = launch(_t(img[rows], dev), _t(txt[rows], dev), _t(np.arange(5, dtype=np.int32), dev), batch,
                              1e-4, 2, t, tm, tv, grad=True)
        assert rc == 0 and len(l) == 1
        tails.append(_all(t, tm, tv) + [l, n, gt])
    for a, b in zip(*tails):
        assert np.array_equal(a, b)
    for a, b in zip(_all(p, m, v) + [sl[2:], sg[2:], g], tails[0]):
        assert np.array_equal(a, b)


def test_out_of_range_permutation_entries_are_clamped():
    dev = _dev()
    img, txt, perm, p0 = _epoch(N=37)
    wild = perm.copy()
    wild[[0, 7, 20, 36]] = [-5, 37, 2 ** 31 - 1, -2 ** 31]
    outs = []
    for pr in (wild, np.clip(wild, 0, 36)):
        p, m, v = _state(dev, p0)
        rc, sl, sg, _ = launch(_t(img, dev), _t(txt, dev), _t(pr, dev), 16, 1e-4, 0, p, m, v)
        assert rc == 0
        outs.append(_all(p, m, v) + [sl, sg])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_bad_arguments_are_einval_with_nothing_launched():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    img, txt, perm, p0 = _epoch(N=32)
    imgd, txtd, pd = _t(img, dev), _t(txt, dev), _t(perm, dev)
    p, m, v = _state(dev, p0)
    ref = p.clone()
    _, need = _ws(dev)
    assert lib.mmf_clip_train_ws_bytes(0) == 0 and lib.mmf_clip_train_ws_bytes(65) == 0
    assert lib.mmf_clip_train_ws_bytes(1) > R.N_PARAMS * 4 and lib.mmf_clip_train_ws_bytes(64) > R.N_PARAMS * 4
    for kw in (dict(batch=0), dict(batch=65), dict(N=0), dict(ws_bytes=need - 1), dict(batch=-3), dict(N=-1),
               dict(ws_bytes=0)):
        args = dict(batch=16, N=None, ws_bytes=None)
        args.update(kw)
        rc, sl, sg, _ = launch(imgd, txtd, pd, args["batch"], 1e-4, 0, p, m, v, N=args["N"], ws_bytes=args["ws_bytes"])
        assert rc == EINVAL, kw
        assert lib.mmf_last_error()
        assert torch.equal(p, ref) and not m.any() and not v.any() and (sl == -7).all() and (sg == -7).all()
    sl = torch.zeros(2, dtype=torch.float32, device=dev)
    sg = torch.zeros(2, dtype=torch.float32, device=dev)
    ws, need = _ws(dev)
    ptrs = [hip.ptr(t) for t in (imgd, txtd, pd, p, m, v, sl, sg, ws)]
    for missing in range(9):
        a = list(ptrs)
        a[missing] = None
        rc = lib.mmf_clip_train_epoch(a[0], a[1], 32, a[2], 16, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1.0, 0, a[3], a[4], a[5],
                                      a[6], a[7], None, a[8], need, hip.stream_ptr())
        assert rc == EINVAL, missing
    bl, rcos = torch.zeros(2, device=dev), torch.zeros(32, device=dev)
    for batch, N, nb in ((0, 32, need), (65, 32, need), (16, 0, need), (16, 32, need - 1)):
        assert lib.mmf_clip_contrastive_eval(hip.ptr(imgd), hip.ptr(txtd), N, batch, hip.ptr(p), hip.ptr(bl),
                                             hip.ptr(rcos), hip.ptr(ws), nb, hip.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(p, ref) and not bl.any() and not rcos.any()


# ---- eval ----
def test_contrastive_eval_against_float64():
    import mmf_amd.hip as hip
    dev = _dev()
    N, batch = 21, 8
    img, txt = R.draws(N, 5)
    p0 = R.initial_params(5)
    want_loss, want_cos = R.evaluate(img, txt, batch, p0)
    bl = torch.zeros(3, dtype=torch.float32, device=dev)
    rcos = torch.zeros(N, dtype=torch.float32, device=dev)
    ws, need = _ws(dev)
    p, imgd, txtd = _t(p0, dev), _t(img, dev), _t(txt, dev)  # (named: alive until the synchronise)
    rc = hip.load().mmf_clip_contrastive_eval(hip.ptr(imgd), hip.ptr(txtd), N, batch, hip.ptr(p),
                                              hip.ptr(bl), hip.ptr(rcos), hip.ptr(ws), need, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    # the bounds of the forward, batch by batch, from the float64 run (max_norm far below every norm: the clamp,
    # which the eval does not have, is never borderline)
    got_cos = rcos.cpu().numpy()
    for k, a in enumerate(range(0, N, batch)):
        b = R.step_bounds(img[a:a + batch], txt[a:a + batch], p0.astype(np.float64), max_norm=1e-9)
        assert abs(b["loss"] - want_loss[k]) < 1e-12
        d = np.abs(got_cos[a:a + batch] - want_cos[a:a + batch])
        print(f"eval batch {k}: loss err {abs(float(bl[k]) - want_loss[k]):.3g} (bound {b['loss_tol']:.3g}), max cos err "
              f"{d.max():.3g} (bound {b['cos_tol'].min():.3g})")
        assert abs(float(bl[k]) - want_loss[k]) <= b["loss_tol"], (k, float(bl[k]), want_loss[k], b["loss_tol"])
        assert (d <= b["cos_tol"]).all()
    assert torch.equal(p, _t(p0, dev))  # forward only


# ---- mmf_clip_pooled and mmf_set_clip_projections, on the golden eight rows ----
@pytest.fixture(scope="module")
def engine(clip_sd, golden_inputs):
    _dev()
    from mmf_amd.engine import Engine
    eng = Engine(0, None, clip_sd, eos_token_id=golden_inputs["eos"], max_batch=8)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def pooled_ref(clip_sd, golden, golden_inputs):
    """post_layernorm(CLS) [8, 768] and final_layer_norm(EOS) [8, 512] from the unmodified oracle, called with
    selector projections: rows of the identity pick the pooled channels."""
    from oracle import models as M
    csd = dict(M.to_torch(clip_sd))
    eye = torch.eye(768)
    px = M.clip_preprocess(torch.as_tensor(golden_inputs["imgs"]))
    halves = []
    with torch.no_grad():
        for lo in (0, 256):
            csd["visual_projection.weight"] = eye[lo:lo + 512].clone()
            halves.append(M.clip_image_features(csd, px).numpy())
        csd["text_projection.weight"] = torch.eye(512)
        txt = M.clip_text_features(csd, torch.as_tensor(golden["clip_ids"]), torch.as_tensor(golden["clip_mask"]),
                                   golden_inputs["eos"]).numpy()
    assert np.array_equal(halves[0][:, 256:], halves[1][:, :256])  # the two calls agree where they overlap
    return np.concatenate([halves[0], halves[1][:, 256:]], 1), txt


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_pooled_rows_against_the_oracle(engine, pooled_ref, clip_sd, golden, golden_inputs):
    imgs, ids, mask = golden_inputs["imgs"], golden["clip_ids"], golden["clip_mask"]
    before = {k: v.clone() for k, v in engine.clip_consistency(imgs, ids, mask).items()}
    ip, tp = engine.clip_pooled(imgs, ids, mask)
    after = engine.clip_consistency(imgs, ids, mask)
    for k in before:
        assert torch.equal(before[k], after[k]), k  # existing outputs unchanged
    ip, tp = ip.cpu().numpy().astype(np.float64), tp.cpu().numpy().astype(np.float64)
    for got, want, name in ((ip, pooled_ref[0], "image"), (tp, pooled_ref[1], "text")):
        rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
        print(f"pooled {name}: max relative distance {rel.max():.3g} (bar {REL:.3g})")
        assert got.shape == want.shape and (rel <= REL).all(), (name, rel)
    # one tower alone gives the same bits
    assert torch.equal(engine.clip_pooled(imgs, None, None)[0].cpu(), torch.from_numpy(ip.astype(np.float32)))
    assert torch.equal(engine.clip_pooled(None, ids, mask)[1].cpu(), torch.from_numpy(tp.astype(np.float32)))
    # normalise(pooled W^T) is what clip_image / clip_text return, at the same bar
    Wv = np.asarray(clip_sd["visual_projection.weight"], np.float64)
    Wt = np.asarray(clip_sd["text_projection.weight"], np.float64)
    ie, te = engine.clip_image(imgs).cpu().numpy(), engine.clip_text(ids, mask).cpu().numpy()
    assert (_unit(ip @ Wv.T) * ie).sum(1).min() > 1 - 1e-4
    assert (_unit(tp @ Wt.T) * te).sum(1).min() > 1 - 1e-4


def test_set_clip_projections(engine, clip_sd, golden, golden_inputs):
    imgs, ids, mask = golden_inputs["imgs"], golden["clip_ids"], golden["clip_mask"]
    ip, tp = (t.cpu().numpy().astype(np.float64) for t in engine.clip_pooled(imgs, ids, mask))
    ie0, te0 = engine.clip_image(imgs).clone(), engine.clip_text(ids, mask).clone()
    nbytes = engine.device_bytes
    g = np.random.default_rng(11)
    Wv0 = np.asarray(clip_sd["visual_projection.weight"], np.float32)
    Wt0 = np.asarray(clip_sd["text_projection.weight"], np.float32)
    Wv = (Wv0 + 0.01 * g.standard_normal(Wv0.shape)).astype(np.float32)
    Wt = (Wt0 + 0.01 * g.standard_normal(Wt0.shape)).astype(np.float32)
    try:
        engine.set_clip_projections(Wv, Wt)
        ie, te = engine.clip_image(imgs).cpu().numpy(), engine.clip_text(ids, mask).cpu().numpy()
        want_i = _unit(ip @ Wv.astype(np.float16).astype(np.float64).T)
        want_t = _unit(tp @ Wt.astype(np.float16).astype(np.float64).T)
        ci, ct = (want_i * ie).sum(1).min(), (want_t * te).sum(1).min()
        print(f"set projections: min cos image {ci:.8f}, text {ct:.8f}; against the old ones "
              f"{(ie0.cpu().numpy() * ie).sum(1).min():.4f}")
        assert ci > 1 - 1e-4 and ct > 1 - 1e-4
        assert (ie0.cpu().numpy() * ie).sum(1).min() < 1 - 1e-3  # the perturbation is visible at this bar
        engine.set_clip_projections(None, Wt0)  # either may be None
        assert torch.equal(engine.clip_text(ids, mask), te0)
        assert not torch.equal(engine.clip_image(imgs), ie0)
    finally:
        engine.set_clip_projections(Wv0, Wt0)
    assert torch.equal(engine.clip_image(imgs), ie0) and torch.equal(engine.clip_text(ids, mask), te0)
    assert engine.device_bytes == nbytes
    with pytest.raises(ValueError):
        engine.set_clip_projections(Wv0[:, :512], None)


# ---- end to end: extract_features, ClipProjectionTrainer, checkpoint, vault builder ----
def _forensics(golden, golden_inputs, det_sd, clip_sd):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    rob, clp = {}, {}
    for i in range(golden["rob_ids"].shape[0]):
        t = f"sample text {i}"
        rob[t] = golden["rob_ids"][i, :golden_inputs["rob_lens"][i]].tolist()
        clp[t] = golden["clip_ids"][i, :golden_inputs["clip_lens"][i]].tolist()
    for j, ids in enumerate(golden_inputs["title_ids"][:16]):
        clp[f"Guardian article {j}"] = ids.tolist()
    first = clp["sample text 1"]
    clp["long caption"] = [first[0]] + [first[1]] * 78 + [first[-1]]  # 80 CLIP tokens
    mf = MisinfoForensics(fusion_weights="/nonexistent", faiss_index_path="/nonexistent",
                          roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=TableClipProcessor(clp),
                          detector_state=det_sd, clip_state=dict(clip_sd), max_batch=24, verbose=False)
    mf.set_vault(golden_inputs["vault"][:16], golden_inputs["meta"][:16])
    return mf, clp


def test_extract_train_checkpoint_end_to_end(golden, golden_inputs, det_sd, clip_sd, tmp_path):
    _dev()
    from PIL import Image
    import mmf_amd.clip_training as CT
    import mmf_amd.synthetic as syn
    import mmf_amd.vault_builder as VB
    from mmf_amd.engine import Engine
    f, clp = _forensics(golden, golden_inputs, det_sd, clip_sd)
    eng = f.engine
    # ---- extract_features on the golden rows as files: a missing image is black, a long caption truncated ----
    texts, paths = [], []
    for i in range(8):
        p = str(tmp_path / f"img{i}.png")
        Image.fromarray(golden_inputs["imgs"][i]).save(p)
        texts.append(f"sample text {i}")
        paths.append(p)
    fi, ft = CT.extract_features(f, texts + ["long caption"], paths + [str(tmp_path / "nope.png")])
    ip, tp = eng.clip_pooled(golden_inputs["imgs"], golden["clip_ids"], golden["clip_mask"])
    assert fi.shape == (9, 768) and ft.shape == (9, 512)
    # (chunks of other sizes take the same rows through the same kernels: rows of batches >= 8 are bit-identical)
    for got, want in ((fi[:8], ip.cpu().numpy()), (ft[:8], tp.cpu().numpy())):
        assert (np.linalg.norm(got - want, axis=1) <= REL * np.linalg.norm(want, axis=1)).all()
    black = eng.clip_pooled(np.zeros((1, 224, 224, 3), np.uint8), None, None)[0].cpu().numpy()
    cut = np.asarray([clp["long caption"][:77]], np.int32)
    trunc = eng.clip_pooled(None, cut, np.ones_like(cut))[1].cpu().numpy()
    assert np.linalg.norm(fi[8] - black[0]) <= REL * np.linalg.norm(black[0])
    assert np.linalg.norm(ft[8] - trunc[0]) <= REL * np.linalg.norm(trunc[0])

    # ---- 24 synthetic pairs, 2 epochs ----
    N = 24
    imgs = syn.images(N, 17)
    cid, cm = syn.clip_ids(N, 77, 17)
    ti, tt = (t.cpu().numpy() for t in eng.clip_pooled(imgs, cid, cm))
    labels = np.arange(N) % 2
    before = CT.flatten_heads(f.clip_state).numpy()
    titles_before = eng.clip_text(*_title_ids(golden, golden_inputs)).clone()
    vault_sets, set_vault = [], f.set_vault
    f.set_vault = lambda emb, meta: (vault_sets.append(len(meta)), set_vault(emb, meta))
    nbytes = eng.device_bytes
    ck_path = str(tmp_path / "clip_detective_best.pth")
    hist = CT.ClipProjectionTrainer(f, batch_size=8, epochs=2, lr=1e-4, seed=1).fit((ti, tt), (ti, tt), labels,
                                                                                  checkpoint_path=ck_path)
    assert [h["epoch"] for h in hist] == [0, 1] and all(np.isfinite(h["train_loss"]) for h in hist)
    after = CT.flatten_heads(f.clip_state).numpy()
    assert not np.array_equal(before, after) and eng.device_bytes == nbytes
    loss0 = R.evaluate(ti, tt, N, before.astype(np.float64))[0][0]
    loss1 = R.evaluate(ti, tt, N, after.astype(np.float64))[0][0]
    print(f"fit: float64 loss of the cached features {loss0:.4f} -> {loss1:.4f}; history {hist}")
    assert loss1 < loss0
    # the loaded vault was set again (its title embeddings are recomputed), and titles embed differently now
    assert vault_sets == [16]
    assert not torch.equal(eng.clip_text(*_title_ids(golden, golden_inputs)), titles_before)

    # ---- the checkpoint ----
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "val_loss",
                       "val_accuracy", "train_loss"}
    best = max(hist, key=lambda h: (h["val_accuracy"], -h["epoch"]))
    assert ck["epoch"] == best["epoch"] and ck["val_accuracy"] == best["val_accuracy"]
    sd, meta = VB.load_clip_detective_checkpoint(ck_path)
    assert set(sd) == set(clip_sd) and meta["epoch"] == best["epoch"]
    assert np.array_equal(CT.flatten_heads(sd).numpy(), after)  # the engine holds the best epoch's heads
    cons = eng.clip_consistency(imgs, cid, cm)["sim"].clone()
    fresh = Engine(0, None, sd, eos_token_id=golden_inputs["eos"], max_batch=24)
    assert torch.equal(fresh.clip_consistency(imgs, cid, cm)["sim"], cons)
    fresh.close()
    # ---- and the vault builder takes it ----
    arts = [{"article_id": f"a{i}", "text_content": texts[i], "image_local_path": paths[i]} for i in range(8)]
    jf = str(tmp_path / "seed.json")
    json.dump(arts, open(jf, "w"))
    db = VB.generate_embeddings_database(ck_path, jf, str(tmp_path / "db.pkl"), processor=f.clip_processor,
                                         eos_token_id=golden_inputs["eos"], batch=8)
    assert db["image_embeddings"].shape == (8, 512) and db["metadata"]["val_accuracy"] == ck["val_accuracy"]
    want = eng.clip_text(golden["clip_ids"], golden["clip_mask"]).cpu().numpy()
    assert (db["text_embeddings"] * want).sum(1).min() > 1 - 1e-4
    eng.close()


def _title_ids(golden, golden_inputs, n=16):
    mask = np.zeros((n, 77), np.int32)
    for j in range(n):
        mask[j, :len(golden_inputs["title_ids"][j])] = 1
    return golden["title_clip_ids"][:n], mask
