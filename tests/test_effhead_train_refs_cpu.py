"""CPU checks of the head-stage training pieces that need no GPU: the float64 restatement of mmf_effhead_train_epoch
(tests/effhead_train_refs.py) against a real torch training loop -- Conv2d(320, 1280, 1, bias=False),
BatchNorm2d(1280).eval(), SiLU, AdaptiveAvgPool2d(1), the given mask times scale, Linear, CrossEntropyLoss,
torch.optim.Adam -- the conditions the GPU tests assert on the reference alone, and the Python layer
(mmf_amd/cifake_training.py: extract_image_features(level="trunk"), flatten_head_stage, HeadStageTrainer,
train_cifake(unfreeze=...)) on a stub engine."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mmf_amd.cifake_training as CT
import mmf_amd.weights as W
from tests import effhead_train_refs as R
from tests.test_effcls_train_refs_cpu import _StubEngine, _cifake_tree, _detector, _fake_forensics, _stub_forensics


# ---- the restatement against torch ----
class _TorchStage(nn.Module):
    def __init__(self, p0, mean, var, train_bn=False):
        super().__init__()
        Wt, gamma, beta, Wc, bc = R.unpack(p0.astype(np.float64))
        self.conv = nn.Conv2d(320, 1280, 1, bias=False).double()
        self.bn = nn.BatchNorm2d(1280, eps=R.BN_EPS).double()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.lin = nn.Linear(1280, 2).double()
        with torch.no_grad():
            self.conv.weight.copy_(torch.from_numpy(np.array(Wt)).reshape(1280, 320, 1, 1))
            self.bn.weight.copy_(torch.from_numpy(np.array(gamma)))
            self.bn.bias.copy_(torch.from_numpy(np.array(beta)))
            self.bn.running_mean.copy_(torch.from_numpy(mean.astype(np.float64)))
            self.bn.running_var.copy_(torch.from_numpy(var.astype(np.float64)))
            self.lin.weight.copy_(torch.from_numpy(np.array(Wc)))
            self.lin.bias.copy_(torch.from_numpy(np.array(bc)))
        self.bn.train(train_bn)

    def forward(self, x, mult):
        """x [n, 49, 320] (positions row-major over 7 x 7, channels innermost) -> logits."""
        img = x.reshape(-1, 7, 7, 320).permute(0, 3, 1, 2)
        a = nn.functional.silu(self.bn(self.conv(img)))
        return self.lin(self.pool(a).flatten(1) * mult)

    def tensors(self):
        return (self.conv.weight, self.bn.weight, self.bn.bias, self.lin.weight, self.lin.bias)

    def flat(self, what=lambda p: p.detach()):
        return torch.cat([what(t).reshape(-1) for t in self.tensors()]).numpy()


def _torch_run(N, batch, epochs, wd, train_bn=False, seed=4):
    """(restatement's params / moments / last gradient / losses, torch's) after `epochs` epochs over a two-view bank."""
    trunk, labels = R.draws(2 * N, seed)
    labels[N:] = labels[:N]
    p0, mean, var = R.initial_params(seed)
    p = p0.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    net = _TorchStage(p0, mean, var, train_bn)
    opt = torch.optim.Adam(net.tensors(), lr=1e-4, weight_decay=wd)
    crit = nn.CrossEntropyLoss()
    y = torch.from_numpy(labels.astype(np.int64))
    step0, out = 0, []
    for perm, keep, _ in CT.plan(N, batch, epochs, seed=3, flip=True):
        assert perm.max() >= N and perm.min() < N
        ls, cs, g_last = R.epoch(trunk, labels, perm, keep, batch, 1e-4, step0, p, m, v, mean.astype(np.float64),
                                 var.astype(np.float64), np.float64, wd=wd)
        step0 += len(ls)
        mask = R.unpack_keep(keep)
        for s in range(len(ls)):
            pos = np.arange(s * batch, min(N, (s + 1) * batch))
            mult = torch.from_numpy(mask[pos].astype(np.float64) * R.SCALE)
            opt.zero_grad()
            logits = net(torch.from_numpy(trunk[perm[pos]]).double(), mult)
            loss = crit(logits, y[perm[pos]])
            loss.backward()
            g_torch = net.flat(lambda q: q.grad)
            opt.step()
            out.append((ls[s], loss.item(), cs[s], int((torch.max(logits, 1)[1] == y[perm[pos]]).sum())))
    st = opt.state
    moments = [np.concatenate([st[q][key].reshape(-1).numpy() for q in net.tensors()])
               for key in ("exp_avg", "exp_avg_sq")]
    return (p, m, v, g_last), (net.flat(), moments[0], moments[1], g_torch), out, p0


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_restatement_equals_torch_loop(wd):
    """Three optimizer steps, the last minibatch short (N = 5, batch 2), over a two-view bank: the gradient of all
    five tensors, both moments and the parameters to 1e-11 relative."""
    ours, theirs, steps, _ = _torch_run(5, 2, 1, wd)
    assert len(steps) == 3
    for l_ref, l_torch, c_ref, c_torch in steps:
        assert abs(l_ref - l_torch) <= 1e-11 * abs(l_torch) and c_ref == c_torch
    for k, sl in R.SLICES.items():
        for what, a, b in zip(("params", "exp_avg", "exp_avg_sq", "grad"), ours, theirs):
            assert _rel(a[sl], b[sl]) <= 1e-11, (k, what)


def test_wrong_statements_do_not_equal_the_torch_loop():
    """Train-mode BatchNorm in the torch loop, AdamW's decoupled decay, or a pool without its / 49 in the restatement:
    each parts from the other side by far more than the 1e-11 of the test above."""
    ours, theirs, _, _ = _torch_run(5, 2, 1, 0.0, train_bn=True)
    assert _rel(ours[3], theirs[3]) > 1e-3
    trunk, labels = R.draws(10, 4)
    p0, mean, var = R.initial_params(4)
    mean, var = mean.astype(np.float64), var.astype(np.float64)
    perm, keep, _ = CT.plan(5, 2, 1, seed=3, flip=True)[0]
    runs = {}
    for broken, wd in (("", 1e-2), ("adamw", 1e-2), ("pool", 1e-2)):
        p = p0.astype(np.float64)
        m, v = np.zeros_like(p), np.zeros_like(p)
        _, _, g = R.epoch(trunk, labels, perm, keep, 2, 1e-4, 0, p, m, v, mean, var, np.float64, wd=wd, broken=broken)
        runs[broken] = (p, g)
    moved = np.abs(runs[""][0] - p0).max()
    assert np.abs(runs["adamw"][0] - runs[""][0]).max() > 1e-3 * moved
    assert _rel(runs["pool"][1], runs[""][1]) > 1.0


def test_eval_restatement_equals_torch():
    trunk, labels = R.draws(5, 5)
    p0, mean, var = R.initial_params(5)
    net = _TorchStage(p0, mean, var)
    losses, lg = R.evaluate(trunk, labels, 2, p0, mean, var)
    with torch.no_grad():
        for k, a in enumerate(range(0, 5, 2)):
            out = net(torch.from_numpy(trunk[a:a + 2]).double(), torch.ones(1, 1280, dtype=torch.float64))
            np.testing.assert_allclose(lg[a:a + 2], out.numpy(), rtol=1e-11, atol=1e-13)
            want = nn.functional.cross_entropy(out, torch.from_numpy(labels[a:a + 2].astype(np.int64)))
            assert abs(want.item() - losses[k]) < 1e-12


# ---- the bounds cannot hide a failure ----
# the share of a tensor's entries whose parameter bound stays under a tenth of the step (the rest are entries whose
# gradient is smaller than its own bound: their first step's sign is open to any fp32 evaluation)
DECIDED = {"features.8.0.weight": 0.75, "features.8.1.weight": 0.98, "features.8.1.bias": 0.98,
           "classifier.1.weight": 0.99, "classifier.1.bias": 1.0}
GRAD_MEDIAN = {"features.8.0.weight": 0.01, "classifier.1.bias": 0.025}  # of the tensor's largest gradient; others 0.005


@pytest.mark.parametrize("n", R.SINGLE_BATCHES)
def test_float32_restatement_sits_inside_the_single_step_bounds(n):
    """The derived bounds are bounds of any fp32 evaluation, and the reference alone decides every argmax (margin_ok).

    The bounds cannot hide a failure: for EVERY tensor the single-step parameter bound stays below a tenth of the
    distance the parameters move.  The first Adam step moves every parameter by lr (it is the gradient's sign), and the
    bound's median is at most 0.0012 lr for each of the five tensors, the conv weight included (measured on the twenty
    cases: 7e-5 .. 1.2e-4 lr for features.8.0.weight, 0.0012 lr for gamma, 8.5e-5, 8.1e-5 and 1.8e-5 lr for beta and
    the classifier's two); asserted below at 0.01 lr, ten times under the issue's tenth.  As in effcls_train_refs the
    statistic is the median: an entry whose gradient is smaller than the rounding error of ANY fp32 evaluation has an
    open sign and a bound of 2 lr whatever the derivation, and a tensor of 409,600 entries always holds some.  DECIDED
    asserts how few: at least 0.78 of the conv weight's entries (0.78 .. 0.96 measured) and 0.99 of every other
    tensor's stay under a tenth of the step.  With z's chain bounded by 320 U sum |terms| instead of its partial sums
    (effhead_train_refs.chain_partials) the conv weight's median was 2 lr and its share 0.16 .. 0.63: that form hid
    most of the tensor, which is why it is not used."""
    for dropout in (True, False):
        for wd in R.SINGLE_WDS:
            trunk, labels, perm, keep, p0, mean, var, b, seed = R.single_case(n, dropout, wd)
            assert b["margin_ok"] and len(labels) == 2 * n + 3 and perm.max() >= n + 2
            q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
            ls, cs, g32 = R.epoch(trunk, labels, perm, keep, n, R.SINGLE_LR, 0, q, m, v, mean, var, np.float32, wd=wd)
            assert (np.abs(g32 - b["grad"]) <= b["grad_tol"]).all(), (n, dropout, wd)
            assert abs(ls[0] - b["loss"]) <= b["loss_tol"] and cs[0] == b["r"]["correct"]
            assert (np.abs(m - b["m"]) <= b["m_tol"]).all() and (np.abs(v - b["v"]) <= b["v_tol"]).all()
            assert (np.abs(q - b["p"]) <= b["p_tol"]).all(), (n, dropout, wd)
            assert b["loss_tol"] < 5e-3 and b["lg_tol"].max() < 5e-3
            assert (b["pooled_tol"] < 1e-4 * np.abs(b["pooled"]).max()).all()
            moved = np.abs(b["p"] - p0)
            for k, sl in R.SLICES.items():
                assert np.median(b["grad_tol"][sl]) < GRAD_MEDIAN.get(k, 0.005) * np.abs(b["grad"][sl]).max(), k
                assert abs(moved[sl].max() / R.SINGLE_LR - 1) < 0.05, k  # the step is lr
                frac = float((b["p_tol"][sl] < 0.1 * moved[sl].max()).mean())
                print(f"n={n} keep={dropout} wd={wd} {k}: median p_tol / lr {np.median(b['p_tol'][sl]) / R.SINGLE_LR:.3g}, "
                      f"elements with p_tol < 0.1 x the movement: {frac:.6f}")
                assert np.median(b["p_tol"][sl]) < 0.1 * 0.1 * moved[sl].max(), k
                assert frac >= DECIDED[k], (k, frac)


def test_multi_step_cases_qualify():
    """What the GPU test's bound 8 x max(e32, FLOOR x steps, cond) per tensor rests on, asserted on the reference
    alone: float32 sits inside it, and it stays below a tenth of the distance the float64 run moved that tensor, so a
    kernel that trains differently (AdamW's decoupled decay for Adam's L2) lands outside.  MULTI_SEEDS are chosen
    here, per case.  What decides is features.8.0.weight's cond, the LARGEST conditioning number over 409,600 weights:
    bound / movement over the seeds tried was 0.07 .. 0.38 for (37, 16, 2) (seeds 1 .. 12; 10 and 12 qualify),
    0.013 .. 0.18 for (10, 1, 1) (seeds 1 .. 12; nine qualify) and 0.05 .. 1.06 for (70, 64, 2), whose four steps move
    a weight by 4e-4 only (seeds 1 .. 37; 37 alone qualifies).  The other four tensors sit at 0.0002 .. 0.015."""
    for case in R.MULTI_CASES:
        p64, _, _, l64, plan, cond, p0 = R.run_case(*case, np.float64)[:7]
        steps = sum(len(l) for l in l64)
        assert steps == -(-case[0] // case[1]) * case[2] and len(plan) == case[2]
        fl = R.floors(p0, float(np.abs(p64 - p0).max()))
        for k, (bound, e32, floor, cnd, moved) in R.multi_bounds(case).items():
            # the floor's premise: the tensor stays below the power of two the floor was derived from
            assert np.abs(p64[R.SLICES[k]]).max() < fl[k] * 2.0 ** 24
            print(f"case {case} {k}: e32 = {e32:.3g}, cond = {cnd:.3g}, floor = {floor:.3g}, bound = {bound:.3g}, "
                  f"moved = {moved:.3g}, ratio = {bound / moved:.3g}")
            assert cnd > 0 and e32 <= bound
            assert bound <= 0.1 * moved, (case, k, bound, moved)
    case = R.MULTI_CASES[1]
    l2 = R.run_case(*case, np.float64, broken="l2")
    aw = R.run_case(*case, np.float64, broken="adamw")
    k = "features.8.1.weight"  # gamma is of order 1: Adam's L2 term 1e-2 gamma outweighs its gradient, AdamW's does not
    bound, _, _, _, moved = R.multi_bounds(case, broken="l2")[k]
    assert bound <= 0.1 * moved
    assert np.abs(aw[0][R.SLICES[k]] - l2[0][R.SLICES[k]]).max() > bound


# ---- the Python layer on a stub engine ----
class _HeadStub(_StubEngine):
    """effhead_train_epoch / effhead_eval by the float32 restatement; effnet_trunk as a plain function of the pixels."""

    def __init__(self):
        super().__init__()
        self.trunk_batches, self.head_calls = [], []

    def effnet_trunk(self, img):
        self.trunk_batches.append(int(img.shape[0]))
        x = img.float().reshape(img.shape[0], -1)[:, :49 * 320 * 9].reshape(-1, 49, 320, 9).mean(-1) / 255.0 - 0.5
        return (x + 0.05 * torch.sin(torch.arange(320.0))).contiguous()

    def effhead_train_epoch(self, trunk, labels, perm, keep, p_drop, batch, mean, var, bn_eps, lr, betas, eps, wd, step0,
                            params, m, v, grad_out=None):
        assert p_drop == 0.2 and betas == (0.9, 0.999) and eps == 1e-8 and bn_eps == W.BN_EPS
        self.head_calls.append((step0, tuple(trunk.shape), int(perm.shape[0])))
        self.bank_ptr = trunk.data_ptr()
        ls, cs, _ = R.epoch(trunk.numpy(), labels.numpy(), perm.numpy(), keep.numpy().view(np.uint64), batch, lr, step0,
                            params.numpy(), m.numpy(), v.numpy(), mean.numpy(), var.numpy(), np.float32, wd=wd)
        return torch.from_numpy(ls.astype(np.float32)), torch.from_numpy(cs.astype(np.int32))

    def effhead_eval(self, trunk, labels, batch, params, mean, var, bn_eps):
        bl, lg = R.evaluate(trunk.numpy(), labels.numpy(), batch, params.numpy(), mean.numpy(), var.numpy(), np.float32)
        return torch.from_numpy(bl.astype(np.float32)), torch.from_numpy(lg.astype(np.float32))


def _head_forensics():
    fs = _stub_forensics()
    fs.engine = _HeadStub()
    fs.detector.bind(fs.engine)
    return fs


def test_trunk_level_bank_layout_with_flip_and_views(tmp_path):
    root = tmp_path / "cifake"
    _cifake_tree(root, n_real=3, n_fake=(2, 1))
    (root / "broken.png").write_bytes(b"not a png")
    tp, _, vp, _ = CT.load_cifake_data(str(root))
    paths = tp + vp + [str(root / "broken.png")]
    fs = _head_forensics()
    N = len(paths)
    feats, flipped, ok = CT.extract_image_features(fs, paths, flip=True, level="trunk")
    assert torch.is_tensor(feats) and feats.shape == flipped.shape == (N, 49, 320) and feats.dtype == torch.float32
    assert ok.tolist() == [True] * (N - 1) + [False] and not feats[-1].any() and not flipped[-1].any()
    assert torch.equal(feats[0], flipped[0])  # a uniform image is its own mirror
    assert max(fs.engine.trunk_batches) <= fs.engine.max_batch and not fs.engine.pooled_batches
    # the same staging and tower inputs as the pooled level: only the final call differs
    fs2 = _head_forensics()
    pooled, pf, ok2 = CT.extract_image_features(fs2, paths, flip=True)
    assert fs2.engine.pooled_batches == fs.engine.trunk_batches and np.array_equal(ok, ok2)
    assert pooled.shape == (N, 1280) and not fs2.engine.trunk_batches
    # views: [K, N, 49, 320], view v from draw v; K = 2 with the jitter stubbed out as the identity
    fs.engine.color_jitter = lambda x, ops, fac, hue: x
    jit = CT.jitter_params(N, 2, 0)
    fv, ffv, okv = CT.extract_image_features(fs, paths, flip=True, jitter=jit, level="trunk")
    assert fv.shape == ffv.shape == (2, N, 49, 320) and torch.equal(fv[0], feats) and torch.equal(fv[1], feats)
    assert not fv[:, -1].any()
    # the two results are views of one allocation in the bank's order: fit trains on it without a copy
    labels = np.arange(N) % 2
    CT.HeadStageTrainer(fs, batch_size=4, epochs=1, flip=True, jitter_views=2).fit((fv, ffv), labels, feats, labels)
    assert fs.engine.head_calls[-1][1] == (4 * N, 49, 320) and fs.engine.bank_ptr == fv.data_ptr()
    assert CT.HeadStageTrainer._bank([fv[0], ffv[0], fv[1], ffv[1]], fv.device).data_ptr() == fv.data_ptr()
    copied = CT.HeadStageTrainer._bank([fv[0], fv[1]], fv.device)  # not adjacent: copied together
    assert copied.data_ptr() != fv.data_ptr() and torch.equal(copied[N:], fv[1])
    whole = CT.HeadStageTrainer._bank([fv[0], ffv[0], fv[1], ffv[1]], fv.device)
    assert torch.equal(whole[N:2 * N], ffv[0]) and torch.equal(whole[2 * N:3 * N], fv[1])
    one, ok1 = CT.extract_image_features(fs, paths[:1], level="trunk")
    assert torch.equal(one[0], feats[0]) and ok1.all()
    assert CT.extract_image_features(fs, [], level="trunk")[0].shape == (0, 49, 320)
    with pytest.raises(ValueError):
        CT.extract_image_features(fs, paths, level="head")


def _trunk_views(N, seed):
    x, y = R.draws(2 * N, seed)
    return (x[:N], x[N:]), y[:N]


def test_head_stage_trainer_argument_errors():
    fs = _head_forensics()
    train, yt = _trunk_views(6, 9)
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, batch_size=65)
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, jitter_views=-1)
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, flip=True).fit(train[0], yt, train[0], yt)  # one view where two are needed
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, flip=False).fit(train[0][:, :, :300], yt, train[0], yt)
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, flip=False).fit(train[0].reshape(6, -1), yt, train[0], yt)  # pooled-style rows
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, flip=False).fit(train[0], yt + 2, train[0], yt)
    with pytest.raises(ValueError):
        CT.HeadStageTrainer(fs, flip=False, jitter_views=2).fit(train[0], yt, train[0], yt)
    with pytest.raises(ValueError):
        CT.train_cifake("/nonexistent", forensics=fs, unfreeze="backbone")


@pytest.mark.parametrize("full", [False, True], ids=["head_stage", "full_model"])
def test_checkpoint_holds_the_five_tensors_and_the_fallback_path_applies_them(full, tmp_path):
    fs = _head_forensics()
    det = fs.detector
    train, yt = _trunk_views(6, 9)
    val, yv = R.draws(4, 10)
    flat0, mean0, var0 = CT.flatten_head_stage(det)
    assert flat0.shape == (CT.HEAD_N_PARAMS,) == (414722,) and mean0.shape == var0.shape == (1280,)
    sd0 = det.efficientnet.state_dict()
    assert torch.equal(flat0[:409600].reshape(1280, 320, 1, 1), sd0["features.8.0.weight"])
    assert torch.equal(flat0[-2:], sd0["classifier.1.bias"]) and torch.equal(var0, sd0["features.8.1.running_var"])
    uploads = dict(det.uploads)
    before = {k: v.clone() for k, v in det.state_dict().items()}
    path = str(tmp_path / CT.DEFAULT_FILE)
    trainer = CT.HeadStageTrainer(fs, batch_size=4, epochs=2, lr=1e-4, seed=2, flip=True)
    hist = trainer.fit(train, yt, val, yv, checkpoint_path=path, save_full_model=full)
    assert [h["epoch"] for h in hist] == [1, 2] and all(np.isfinite(h["train_loss"]) for h in hist)
    assert fs.engine.head_calls == [(0, (12, 49, 320), 6), (2, (12, 49, 320), 6)]  # the two-view bank, step0 carried
    assert det.uploads["effnet"] == uploads["effnet"] + 1 and fs.engine.calibrated == ["effnet"]
    assert det.uploads["text"] == uploads["text"] and det.uploads["fusion"] == uploads["fusion"]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    eff_keys = set(det.efficientnet.state_dict())
    assert set(ck) == (eff_keys if full else set(CT.HEAD_PARAM_KEYS)) and set(CT.HEAD_PARAM_KEYS) <= eff_keys
    shapes = {"features.8.0.weight": (1280, 320, 1, 1), "features.8.1.weight": (1280,), "features.8.1.bias": (1280,),
              "classifier.1.weight": (2, 1280), "classifier.1.bias": (2,)}
    assert {k: tuple(ck[k].shape) for k in CT.HEAD_PARAM_KEYS} == shapes
    # the detector holds the saved tensors; everything else, the running statistics included, is unchanged
    trained = {k: v.clone() for k, v in det.state_dict().items()}
    changed = {"efficientnet." + k for k in CT.HEAD_PARAM_KEYS}
    for k, v in before.items():
        assert torch.equal(trained[k], v) == (k not in changed), k
    for k in CT.HEAD_PARAM_KEYS:
        assert torch.equal(trained["efficientnet." + k], ck[k]), k
    # a fresh detector takes exactly those tensors from the file through the constructor's fallback path
    det2 = _detector()
    _fake_forensics(det2)._load_individual_weights("/nonexistent", "/nonexistent", path, "/nonexistent")
    after = det2.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], trained[k]), k
    assert torch.equal(after["efficientnet.features.8.1.running_mean"], before["efficientnet.features.8.1.running_mean"])
    assert torch.equal(after["efficientnet.features.8.1.running_var"], before["efficientnet.features.8.1.running_var"])


def test_train_cifake_unfreeze_selects_the_trainer(tmp_path, capsys, monkeypatch):
    root = tmp_path / "cifake"
    _cifake_tree(root, n_real=6, n_fake=(3, 3))
    made = []
    for cls in (CT.ClassifierTrainer, CT.HeadStageTrainer):
        init = cls.__init__
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _i=init, _c=cls, **k: (made.append(_c), _i(self, *a, **k))[1])
    fs = _head_forensics()
    hist = CT.train_cifake(str(root), batch_size=4, epochs=1, forensics=fs, checkpoint_path=None)
    assert made == [CT.ClassifierTrainer] and len(hist) == 1 and fs.engine.train_calls and not fs.engine.head_calls
    made.clear()
    fs = _head_forensics()
    path = str(tmp_path / "head.pth")
    hist = CT.train_cifake(str(root), batch_size=4, epochs=1, forensics=fs, checkpoint_path=path, unfreeze="head")
    assert made[0] is CT.HeadStageTrainer and len(hist) == 1 and fs.engine.head_calls and not fs.engine.train_calls
    assert not fs.engine.pooled_batches and sum(fs.engine.trunk_batches) == 2 * 9 + 3
    assert set(torch.load(path, map_location="cpu", weights_only=True)) == set(CT.HEAD_PARAM_KEYS)
    assert "Best validation accuracy" in capsys.readouterr().out
