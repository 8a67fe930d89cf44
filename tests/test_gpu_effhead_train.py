"""mmf_effhead_train_epoch / mmf_effhead_eval (csrc/effhead_train.hip), mmf_effnet_trunk and
mmf_amd/cifake_training.py's HeadStageTrainer on the MI355X.

Kernel references are the float64 restatement of tests/effhead_train_refs.py (equal to a real torch loop:
tests/test_effhead_train_refs_cpu.py); bounds are derived there, never from what the kernel returned.

Multi-step bound, per tensor: K = max |kernel - float64| over the tensor must stay within 8 x max(e32, FLOOR x steps,
cond): e32 = the float32 restatement's same error, FLOOR = two half-ulps at the tensor's magnitude and cond = the float64
run's conditioning number over the tensor (effhead_train_refs.multi_bounds).

The trunk rows.  The head stage applied in float64 numpy to mmf_effnet_trunk's rows, then pooled, against
mmf_effnet_pooled's row relative to that row's largest entry: on the fp32 tower within the forward bound of
step_bounds (pooled_tol); on the fp16 tower within TRUNK_BAR = twice the largest difference measured on golden images
0 .. 2 (the tower's own head GEMM reads the same fp16 trunk, rounds its folded weights to fp16 and its output to
fp16 before the pool).  Against the oracle's features within test_gpu_effcls_train.py's POOLED_BAR.
"""
import os

import numpy as np
import pytest
import torch

from tests import effhead_train_refs as R
from tests.test_gpu_effcls_train import POOLED_BAR, _forensics

pytestmark = pytest.mark.gpu
EINVAL = -22
# max |pool(head stage in float64 on the trunk rows) - mmf_effnet_pooled| / max |pooled row| on golden images 0 .. 2 of
# the fp16 tower: measured 2.67e-4; the run is deterministic, the factor 2 covers other images
TRUNK_BAR = 2 * 2.67e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _keep(keep, dev):
    return None if keep is None else _t(keep.view(np.int64), dev)


def _ws(batch, dev, short=0):
    import mmf_amd.hip as hip
    need = int(hip.load().mmf_effhead_ws_bytes(int(batch)))
    return torch.empty(max(need - short, 16), dtype=torch.uint8, device=dev), need


def launch(trunk, labels, perm, keep, batch, lr, step0, p, m, v, mean, var, grad=False, R_=None, N=None,
           p_drop=R.P_DROP, wd=0.0, bn_eps=R.BN_EPS, ws=None):
    """One mmf_effhead_train_epoch on device tensors (p, m, v updated in place) -> (rc, loss, correct, grad) numpy."""
    import mmf_amd.hip as hip
    lib = hip.load()
    N = len(perm) if N is None else N
    R_ = len(labels) if R_ is None else R_
    nsteps = max(1, -(-N // max(batch, 1)))
    sl = torch.full((nsteps,), -7.0, dtype=torch.float32, device=p.device)
    sc = torch.full((nsteps,), -7, dtype=torch.int32, device=p.device)
    g = torch.zeros(R.N_PARAMS, dtype=torch.float32, device=p.device) if grad else None
    if ws is None:
        ws = _ws(min(max(batch, 1), 64), p.device)[0]
    rc = lib.mmf_effhead_train_epoch(hip.ptr(trunk), hip.ptr(labels), R_, hip.ptr(perm), N, hip.ptr(keep), p_drop, batch,
                                     hip.ptr(mean), hip.ptr(var), bn_eps, lr, R.BETAS[0], R.BETAS[1], R.EPS, wd, step0,
                                     hip.ptr(p), hip.ptr(m), hip.ptr(v), hip.ptr(sl), hip.ptr(sc), hip.ptr(g),
                                     hip.ptr(ws), ws.numel(), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, sl.cpu().numpy(), sc.cpu().numpy(), (g.cpu().numpy() if grad else None)


def _state(dev, p0):
    p = _t(p0, dev)
    return p, torch.zeros_like(p), torch.zeros_like(p)


def _all(p, m, v):
    return [t.cpu().numpy().copy() for t in (p, m, v)]


def _ratio(err, tol):
    nz = tol > 0
    assert (err[~nz] == 0).all()
    return float((err[nz] / tol[nz]).max()) if nz.any() else 0.0


# ---- single step, per element ----
@pytest.mark.parametrize("wd", R.SINGLE_WDS, ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("dropout", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("n", R.SINGLE_BATCHES)
def test_single_step_per_element(n, dropout, wd):
    """M = 49 n = 49, 98, 245, 784, 3136 rows: the forward's row tile is one image; the backward's 32-row chunks are
    straddled by every image, and M is a multiple of 32 only at n = 32 k."""
    dev = _dev()
    trunk, labels, perm, keep, p0, mean, var, b, seed = R.single_case(n, dropout, wd)
    assert b["margin_ok"] and len(labels) == 2 * n + 3 and perm.max() >= n + 2  # the upper half of the bank
    p, m, v = _state(dev, p0)
    rc, sl, sc, g = launch(_t(trunk, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), n, R.SINGLE_LR, 0, p, m, v,
                           _t(mean, dev), _t(var, dev), grad=True, wd=wd)
    assert rc == 0
    errs = {"grad": (np.abs(g - b["grad"]), b["grad_tol"]), "exp_avg": (np.abs(m.cpu().numpy() - b["m"]), b["m_tol"]),
            "exp_avg_sq": (np.abs(v.cpu().numpy() - b["v"]), b["v_tol"]),
            "params": (np.abs(p.cpu().numpy() - b["p"]), b["p_tol"])}
    print(f"n={n} keep={dropout} wd={wd} (seed {seed}): loss err {abs(sl[0] - b['loss']):.3g} (bound "
          f"{b['loss_tol']:.3g}); largest err / bound: " + ", ".join(f"{k} {_ratio(*e):.3g}" for k, e in errs.items()) +
          "; grad per tensor: " + ", ".join(f"{_ratio(errs['grad'][0][x], errs['grad'][1][x]):.3g}"
                                            for x in R.SLICES.values()))
    for k, (err, tol) in errs.items():
        assert (err <= tol).all(), (k, int((err > tol).sum()))
    assert abs(float(sl[0]) - b["loss"]) <= b["loss_tol"]
    assert sc[0] == b["r"]["correct"]


# ---- multi-step ----
@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: f"N{c[0]}-b{c[1]}-e{c[2]}")
def test_multi_step_tracks_float64(case):
    dev = _dev()
    N, batch, epochs = case
    seed = R.MULTI_SEEDS[case]
    p64, m64, v64, l64, plan, cond, p0, mean, var = R.run_case(*case, np.float64, seed)
    steps = sum(len(l) for l in l64)
    trunk, labels = R.draws(N, seed)
    td, labd, md, vd = _t(trunk, dev), _t(labels, dev), _t(mean, dev), _t(var, dev)
    p, m, v = _state(dev, p0)
    step0 = 0
    for e, (perm, keep) in enumerate(plan):
        rc, sl, sc, _ = launch(td, labd, _t(perm, dev), _keep(keep, dev), batch, R.MULTI_LR, step0, p, m, v, md, vd)
        assert rc == 0
        step0 += len(sl)
        assert np.isfinite(sl).all()
        np.testing.assert_allclose(sl, l64[e], rtol=0, atol=1e-3)  # coarse: the per-element test owns the loss
    assert step0 == steps
    got = p.cpu().numpy()
    for k, (bound, e32, floor, cnd, moved) in R.multi_bounds(case, seed).items():
        K = float(np.abs(got[R.SLICES[k]] - p64[R.SLICES[k]]).max())
        print(f"case {case} {k}: K = {K:.3g}, e32 = {e32:.3g}, cond = {cnd:.3g}, floor x steps = {floor:.3g}, bound = "
              f"{bound:.3g} ({bound / moved:.3g} of the movement {moved:.3g})")
        assert K <= bound, (k, K, bound)


# ---- repeatability and step0 ----
def _epoch(N=37, seed=3, R_=None):
    R_ = N if R_ is None else R_
    trunk, labels = R.draws(R_, seed)
    g = np.random.default_rng(seed)
    return (trunk, labels, g.permutation(N).astype(np.int32), R.pack_keep(g.random((N, R.CH)) >= R.P_DROP)) + \
        R.initial_params(seed)


def test_same_launch_twice_is_bit_identical():
    dev = _dev()
    trunk, labels, perm, keep, p0, mean, var = _epoch(N=70)
    outs = []
    for _ in range(2):
        p, m, v = _state(dev, p0)
        rc, sl, sc, g = launch(_t(trunk, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), 64, 1e-4, 4, p, m, v,
                               _t(mean, dev), _t(var, dev), grad=True, wd=1e-2)
        assert rc == 0 and len(sl) == 2
        outs.append(_all(p, m, v) + [sl, sc, g])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_two_epochs_equal_one_call_each_with_step0_carried_and_a_split_epoch():
    """The state after an epoch is all that the next one reads: an epoch split at a minibatch boundary into two calls
    (perm and keep sliced, step0 carried) gives the bits of the whole call; and clamped, label-masked entries behave
    as their clamped, masked values."""
    dev = _dev()
    trunk, labels, perm, keep, p0, mean, var = _epoch(N=37, R_=45)
    wild = perm.copy()
    wild[[0, 20, 36]] = [-5, 2 ** 31 - 1, -2 ** 31]
    odd = labels.copy()
    odd[::3] += 2 * np.arange(len(odd[::3]), dtype=np.int32)  # read as label & 1
    td, md, vd = _t(trunk, dev), _t(mean, dev), _t(var, dev)
    p, m, v = _state(dev, p0)
    rc, sl, sc, g = launch(td, _t(odd, dev), _t(wild, dev), _keep(keep, dev), 16, 1e-4, 5, p, m, v, md, vd, grad=True)
    assert rc == 0 and len(sl) == 3
    q, qm, qv = _state(dev, p0)
    parts = []
    clamped = np.clip(wild, 0, 44).astype(np.int32)
    for a, b, s0 in ((0, 16, 5), (16, 37, 6)):
        rc, l, c, gq = launch(td, _t(labels, dev), _t(clamped[a:b], dev), _keep(keep[a:b], dev), 16, 1e-4, s0, q, qm, qv,
                              md, vd, grad=True)
        assert rc == 0
        parts.append((l, c))
    for x, y in zip(_all(p, m, v) + [g], _all(q, qm, qv) + [gq]):
        assert np.array_equal(x, y)
    for k, whole in enumerate((sl, sc)):
        assert np.array_equal(whole, np.concatenate([part[k] for part in parts]))


# ---- eval ----
def _eval(trunk, labels, batch, p, mean, var, dev):
    import mmf_amd.hip as hip
    N = len(labels)
    bl = torch.zeros(-(-N // batch), dtype=torch.float32, device=dev)
    lg = torch.zeros(N, 2, dtype=torch.float32, device=dev)
    td, ld, md, vd = _t(trunk, dev), _t(labels, dev), _t(mean, dev), _t(var, dev)
    ws = _ws(batch, dev)[0]
    rc = hip.load().mmf_effhead_eval(hip.ptr(td), hip.ptr(ld), N, batch, hip.ptr(p), hip.ptr(md), hip.ptr(vd), R.BN_EPS,
                                     hip.ptr(bl), hip.ptr(lg), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return bl.cpu().numpy(), lg.cpu().numpy()


@pytest.mark.parametrize("rows,batch", [(1, 1), (17, 16), (130, 64)])
def test_eval_against_float64(rows, batch):
    dev = _dev()
    trunk, labels = R.draws(rows, 5)
    p0, mean, var = R.initial_params(5)
    p = _t(p0, dev)
    bl, lg = _eval(trunk, labels, batch, p, mean, var, dev)
    for k, b in enumerate(R.eval_bounds(trunk, labels, batch, p0.astype(np.float64), mean, var)):
        a = k * batch
        d = np.abs(lg[a:a + batch] - b["lg"])
        print(f"eval R={rows} batch {k}: loss err {abs(float(bl[k]) - b['loss']):.3g} (bound {b['loss_tol']:.3g}), max "
              f"logit err {d.max():.3g} (largest err / bound {(d / b['lg_tol']).max():.3g})")
        assert abs(float(bl[k]) - b["loss"]) <= b["loss_tol"]
        assert (d <= b["lg_tol"]).all()
    assert torch.equal(p, _t(p0, dev))  # forward only


def test_eval_logits_do_not_depend_on_the_batch_size():
    dev = _dev()
    trunk, labels = R.draws(17, 6)
    p0, mean, var = R.initial_params(6)
    p = _t(p0, dev)
    rows = [_eval(trunk, labels, batch, p, mean, var, dev)[1] for batch in (1, 16, 64)]
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2]) and np.isfinite(rows[0]).all()


# ---- argument errors ----
def test_bad_arguments_are_einval_with_nothing_launched():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    trunk, labels, perm, keep, p0, mean, var = _epoch(N=8)
    td, ld, pd, kd, md, vd = _t(trunk, dev), _t(labels, dev), _t(perm, dev), _keep(keep, dev), _t(mean, dev), _t(var, dev)
    p, m, v = _state(dev, p0)
    ref = p.clone()
    assert lib.mmf_effhead_ws_bytes(0) == 0 and lib.mmf_effhead_ws_bytes(65) == 0
    assert lib.mmf_effhead_ws_bytes(16) == 4 * (16 * 49 * 1280 + 2 * 16 * 1280 + 2 * 1280)
    short = _ws(4, dev, short=16)[0]
    for kw in (dict(batch=0), dict(batch=65), dict(N=0), dict(R_=0), dict(batch=-3), dict(N=-1), dict(R_=-1),
               dict(p_drop=1.0), dict(p_drop=-0.1), dict(p_drop=float("nan")), dict(bn_eps=0.0), dict(bn_eps=-1e-5),
               dict(bn_eps=float("nan")), dict(bn_eps=float("inf")), dict(bn_eps=1e-50), dict(bn_eps=1e300),
               dict(ws=short)):  # (1e-50 and 1e300 are 0 and inf as the fp32 value the kernels use)
        args = dict(batch=4, N=None, R_=None, p_drop=R.P_DROP, bn_eps=R.BN_EPS, ws=None)
        args.update(kw)
        rc, sl, sc, _ = launch(td, ld, pd, kd, args["batch"], 1e-4, 0, p, m, v, md, vd, N=args["N"], R_=args["R_"],
                               p_drop=args["p_drop"], bn_eps=args["bn_eps"], ws=args["ws"])
        assert rc == EINVAL, kw
        assert lib.mmf_last_error()
        assert torch.equal(p, ref) and not m.any() and not v.any()
        assert (sl == -7).all() and (sc == -7).all()
    sl = torch.zeros(2, dtype=torch.float32, device=dev)
    sc = torch.zeros(2, dtype=torch.int32, device=dev)
    ws, need = _ws(4, dev)
    ptrs = [hip.ptr(t) for t in (td, ld, pd, md, vd, p, m, v, sl, sc, ws)]

    def call(a, keep_ptr=hip.ptr(kd), nbytes=need):
        return lib.mmf_effhead_train_epoch(a[0], a[1], 8, a[2], 8, keep_ptr, 0.2, 4, a[3], a[4], 1e-5, 1e-4, 0.9, 0.999,
                                           1e-8, 0.0, 0, a[5], a[6], a[7], a[8], a[9], None, a[10], nbytes,
                                           hip.stream_ptr())
    for missing in range(11):  # each required pointer in turn (keep and grad_out may be NULL)
        a = list(ptrs)
        a[missing] = None
        assert call(a) == EINVAL, missing
    a = list(ptrs)
    a[0] += 4
    assert call(a) == EINVAL                               # a misaligned bank
    a = list(ptrs)
    a[10] += 4
    assert call(a) == EINVAL                               # a misaligned workspace
    assert call(ptrs, keep_ptr=hip.ptr(kd) + 4) == EINVAL  # a misaligned mask
    assert call(ptrs, nbytes=need - 1) == EINVAL           # a short workspace
    bl, lg = torch.zeros(2, device=dev), torch.zeros(8, 2, device=dev)
    ev = [hip.ptr(t) for t in (td, ld, p, md, vd, bl, lg, ws)]

    def evaluate(a, rows=8, batch=4, eps=1e-5, nbytes=need):
        return lib.mmf_effhead_eval(a[0], a[1], rows, batch, a[2], a[3], a[4], eps, a[5], a[6], a[7], nbytes,
                                    hip.stream_ptr())
    for kw in (dict(batch=0), dict(batch=65), dict(rows=0), dict(eps=0.0), dict(eps=float("nan")), dict(eps=1e-50), dict(eps=1e300),
               dict(nbytes=need - 1)):
        assert evaluate(ev, **kw) == EINVAL, kw
    for missing in range(8):
        a = list(ev)
        a[missing] = None
        assert evaluate(a) == EINVAL, missing
    torch.cuda.synchronize()
    assert torch.equal(p, ref) and not m.any() and not v.any() and not bl.any() and not lg.any()
    assert not sl.any() and not sc.any()


# ---- mmf_effnet_trunk, on the golden images ----
@pytest.fixture(scope="module")
def engine(det_sd):
    _dev()
    from mmf_amd.engine import Engine
    eng = Engine(0, det_sd, None, max_batch=8, max_text_len=64)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle_rows(det_sd, golden_inputs):
    from oracle import models as M
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in det_sd.items() if k.startswith("efficientnet.")}
    with torch.no_grad():
        _, feat = M.effnet_forward(sd, M.effnet_preprocess(torch.as_tensor(golden_inputs["imgs"][:3])),
                                   return_features=True)
    return feat.double().numpy()


def _head_params(det_sd):
    keys = ("features.8.0.weight", "features.8.1.weight", "features.8.1.bias", "classifier.1.weight", "classifier.1.bias")
    flat = np.concatenate([np.asarray(det_sd["efficientnet." + k], np.float64).reshape(-1) for k in keys])
    assert flat.shape == (R.N_PARAMS,)
    return (flat, np.asarray(det_sd["efficientnet.features.8.1.running_mean"], np.float32),
            np.asarray(det_sd["efficientnet.features.8.1.running_var"], np.float32))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp16_tower", "fp32_tower"])
def test_effnet_trunk_on_the_golden_images(engine, det_sd, golden_inputs, oracle_rows, fp32, B):
    imgs = golden_inputs["imgs"][:B]
    engine.set_option("effnet_fp32", fp32)
    try:
        before = [t.clone() for t in engine.effnet_forward(imgs)]
        trunk = engine.effnet_trunk(imgs)
        again = engine.effnet_trunk(imgs)
        pooled = engine.effnet_pooled(imgs).cpu().numpy()
        after = engine.effnet_forward(imgs)
        for a, b in zip(before, after):
            assert torch.equal(a, b)
        assert torch.equal(trunk, again) and engine.get_option("effnet_fp32") == fp32
    finally:
        engine.set_option("effnet_fp32", engine.ledger.last("effnet_fp32", 0))
    trunk = trunk.cpu().numpy()
    assert trunk.shape == (B, 49, 320) and trunk.dtype == np.float32 and np.isfinite(trunk).all()
    if not fp32:  # every value is an fp16 value, converted exactly
        assert np.array_equal(trunk, trunk.astype(np.float16).astype(np.float32))
    p64, mean, var = _head_params(det_sd)
    h = R.stage(trunk, p64, mean.astype(np.float64), var.astype(np.float64), np.float64)
    rel_pooled = np.abs(h["pooled"] - pooled).max(1) / np.abs(pooled).max(1)
    want = oracle_rows[:B]
    rel_oracle = np.abs(h["pooled"] - want).max(1) / np.abs(want).max(1)
    print(f"effnet_fp32={fp32} B={B}: max |stage64(trunk) - pooled| / max |pooled row| {rel_pooled.max():.3g}"
          f"{'' if fp32 else f' (bar {TRUNK_BAR:.3g})'}; against the oracle {rel_oracle.max():.3g} (bar "
          f"{POOLED_BAR[fp32]:.3g})")
    if fp32:
        tol = 2 * R.stage_bounds(h, p64)["e_pooled"]
        d = np.abs(h["pooled"] - pooled)
        print(f"fp32 tower B={B}: largest |stage64(trunk) - pooled| / bound {(d / tol).max():.3g}")
        assert (d <= tol).all()
    else:
        assert (rel_pooled <= TRUNK_BAR).all(), rel_pooled
    assert (rel_oracle <= POOLED_BAR[fp32]).all(), rel_oracle


# ---- end to end: extract_image_features(level="trunk"), HeadStageTrainer, the file the constructor loads ----
def test_head_stage_trainer_end_to_end(det_sd, clip_sd, tmp_path):
    _dev()
    import mmf_amd.cifake_training as CT
    from PIL import Image
    g = np.random.default_rng(11)
    paths, labels = [], []
    for i in range(24):
        px = np.clip(g.integers(40, 180, (32, 32, 3)) + np.array((60, 0, 0) if i % 2 else (0, 0, 60)), 0, 255)
        paths.append(str(tmp_path / f"img{i:02d}.png"))
        Image.fromarray(px.astype(np.uint8)).save(paths[-1])
        labels.append(i % 2)
    f = _forensics(det_sd, clip_sd)
    before = [f.analyze_image(p)["deepfake_score"] for p in paths[:4]]
    jit = CT.jitter_params(18, 2, 0)
    xt, xf, ok = CT.extract_image_features(f, paths[:18], flip=True, jitter=jit, level="trunk")
    xv, okv = CT.extract_image_features(f, paths[18:], level="trunk")
    assert ok.all() and okv.all() and xt.shape == xf.shape == (2, 18, 49, 320) and xt.is_cuda
    path = str(tmp_path / CT.DEFAULT_FILE)
    hist = CT.HeadStageTrainer(f, batch_size=8, epochs=2, seed=1, flip=True, jitter_views=2).fit(
        (xt, xf), np.asarray(labels[:18], np.int32), xv, np.asarray(labels[18:], np.int32), checkpoint_path=path)
    assert [h["epoch"] for h in hist] == [1, 2]
    assert all(np.isfinite([h["train_loss"], h["val_loss"], h["train_acc"], h["val_acc"]]).all() for h in hist)
    installed = CT.flatten_head_stage(f.detector)[0].cpu().numpy()
    after = [f.analyze_image(p)["deepfake_score"] for p in paths[:4]]
    assert all(np.isfinite(after)) and after != before
    assert os.path.exists(path)  # written on a strictly higher validation accuracy
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == set(CT.HEAD_PARAM_KEYS)
    assert np.array_equal(torch.cat([ck[k].reshape(-1) for k in CT.HEAD_PARAM_KEYS]).numpy(), installed)
    fresh = _forensics(det_sd, clip_sd, efficientnet_weights=path)
    assert np.array_equal(CT.flatten_head_stage(fresh.detector)[0].cpu().numpy(), installed)
    assert [fresh.analyze_image(p)["deepfake_score"] for p in paths[:4]] == after
    for x in (fresh, f):
        x.engine.close()
