"""CPU checks of the deepfake-classifier training pieces that need no GPU: the float64 restatement of
mmf_effcls_train_epoch (tests/effcls_train_refs.py) against a real torch training loop, the conditions the GPU tests
assert on the reference alone, the epoch plan, the CIFAKE directory contract, the checkpoint -- the counterpart of
SURVEY quirk Q3: a file this trainer writes IS applied by the constructor's fallback path -- and train_cifake end to
end on a stub engine (mmf_amd/cifake_training.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import mmf_amd.cifake_training as CT
import mmf_amd.weights as W
from mmf_amd.api import MisinfoForensics, MultiModalMisinfoDetector
from tests import effcls_train_refs as R


def _torch_classifier(p0):
    Wt, b = R.unpack(p0.astype(np.float64))
    lin = nn.Linear(1280, 2).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.array(Wt)))
        lin.bias.copy_(torch.from_numpy(np.array(b)))
    return lin


def _flat(lin, what=lambda p: p.detach()):
    return torch.cat([what(lin.weight).reshape(-1), what(lin.bias).reshape(-1)]).numpy()


@pytest.mark.parametrize("N,batch,epochs,wd", [(37, 16, 2, 0.0), (21, 4, 2, 1e-2)])
def test_restatement_equals_torch_loop(N, batch, epochs, wd):
    """nn.Linear(1280, 2) on x * mask / (1 - p), CrossEntropyLoss, autograd and torch.optim.Adam (with and without
    weight_decay) in float64, against epoch(dtype=float64) on the plan's perm / keep over the two-view bank: float64
    round-off."""
    feat, labels = R.draws(2 * N, 4)
    labels[N:] = labels[:N]  # the bank: rows N .. 2N - 1 are the mirrored views of rows 0 .. N - 1
    p = R.initial_params(4).astype(np.float64)
    lin = _torch_classifier(p)
    opt = torch.optim.Adam(lin.parameters(), lr=1e-4, weight_decay=wd)
    crit = nn.CrossEntropyLoss()
    m, v = np.zeros_like(p), np.zeros_like(p)
    step0 = 0
    y = torch.from_numpy(labels.astype(np.int64))
    for perm, keep, flipped in CT.plan(N, batch, epochs, seed=3, flip=True):
        assert perm.max() >= N and perm.min() < N
        ls, cs, g_last = R.epoch(feat, labels, perm, keep, batch, 1e-4, step0, p, m, v, np.float64, wd=wd)
        step0 += len(ls)
        mask = R.unpack_keep(keep)
        for s in range(len(ls)):
            pos = np.arange(s * batch, min(N, (s + 1) * batch))
            mult = torch.from_numpy(mask[pos].astype(np.float64) * R.SCALE)
            opt.zero_grad()
            logits = lin(torch.from_numpy(feat[perm[pos]]).double() * mult)
            loss = crit(logits, y[perm[pos]])
            loss.backward()
            if s == len(ls) - 1:
                np.testing.assert_allclose(g_last, _flat(lin, lambda q: q.grad), rtol=0, atol=1e-13)
            opt.step()
            assert abs(loss.item() - ls[s]) < 1e-13
            assert int((torch.max(logits, 1)[1] == y[perm[pos]]).sum()) == cs[s]
    np.testing.assert_allclose(p, _flat(lin), rtol=0, atol=1e-12)
    st = opt.state
    for arr, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
        np.testing.assert_allclose(arr, np.concatenate([st[q][key].reshape(-1).numpy() for q in (lin.weight, lin.bias)]),
                                   rtol=0, atol=1e-13)


def test_eval_restatement_equals_torch():
    feat, labels = R.draws(21, 5)
    p0 = R.initial_params(5)
    lin = _torch_classifier(p0)
    losses, lg = R.evaluate(feat, labels, 8, p0)
    with torch.no_grad():
        for k, a in enumerate(range(0, 21, 8)):
            out = lin(torch.from_numpy(feat[a:a + 8]).double())
            np.testing.assert_allclose(lg[a:a + 8], out.numpy(), rtol=0, atol=1e-14)
            want = nn.functional.cross_entropy(out, torch.from_numpy(labels[a:a + 8].astype(np.int64)))
            assert abs(want.item() - losses[k]) < 1e-13


def test_float32_restatement_sits_inside_the_single_step_bounds():
    """The derived bounds are bounds of any fp32 evaluation, the reference alone decides every argmax, and the
    bounds say something."""
    for B in R.SINGLE_BATCHES:
        for dropout in (True, False):
            for wd in R.SINGLE_WDS:
                feat, labels, perm, keep, p0, b, seed = R.single_case(B, dropout, wd)
                assert b["margin_ok"] and len(labels) == 2 * B + 3 and perm.max() >= B + 2
                q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
                ls, cs, g32 = R.epoch(feat, labels, perm, keep, B, R.SINGLE_LR, 0, q, m, v, np.float32, wd=wd)
                assert (np.abs(g32 - b["grad"]) <= b["grad_tol"]).all(), (B, dropout, wd)
                assert abs(ls[0] - b["loss"]) <= b["loss_tol"] and cs[0] == b["r"]["correct"]
                assert (np.abs(m - b["m"]) <= b["m_tol"]).all() and (np.abs(v - b["v"]) <= b["v_tol"]).all()
                assert (np.abs(q - b["p"]) <= b["p_tol"]).all(), (B, dropout, wd)
                assert b["loss_tol"] < 1e-4 and b["lg_tol"].max() < 1e-4
                assert np.median(b["grad_tol"]) < 1e-4 * np.abs(b["grad"]).max()
                # the step is lr per parameter; its bound stays far below it for all but a handful of tiny gradients
                assert np.median(b["p_tol"]) < 1e-3 * R.SINGLE_LR


def test_multi_step_cases_qualify():
    """What the GPU test's bound 8 x max(e32, FLOOR x steps, cond) rests on, asserted on the reference alone: the
    parameters stay below 1 / 16 (the floor's premise), float32 sits inside the bound, and the bound stays below a
    tenth of the distance the float64 run moved its parameters, so a kernel that trains differently lands outside.
    MULTI_SEED: of seeds 1 .. 8 every one but 8 qualifies (bound / movement 3e-4 .. 5e-4; seed 8's 17-row case
    0.014); 3 is the one whose weight-decay run below has the smallest bound as well (3.5e-6)."""
    assert R.FLOOR == 2.0 ** -28 and R.MULTI_SEED == 3
    for case in R.MULTI_CASES:
        p64, _, _, l64, plan, cond, p0 = R.run_case(*case, np.float64)
        p32 = R.run_case(*case, np.float32)[0]
        steps = sum(len(l) for l in l64)
        assert steps == -(-case[0] // case[1]) * case[2] and len(plan) == case[2]
        assert np.abs(p64).max() < 0.0625 and np.abs(p32).max() < 0.0625
        e32 = float(np.abs(p32 - p64).max())
        bound = 8 * max(e32, R.FLOOR * steps, cond)
        moved = float(np.abs(p64 - p0).max())
        print(f"case {case}: e32 = {e32:.3g}, cond = {cond:.3g}, floor = {R.FLOOR * steps:.3g}, bound = {bound:.3g}, "
              f"moved = {moved:.3g}, ratio = {bound / moved:.3g}")
        assert cond > 0 and e32 <= bound
        assert bound <= 0.1 * moved, (case, bound, moved)
    # two broken restatements end outside the bound: no dropout scale; AdamW's decoupled decay for Adam's L2
    case = R.MULTI_CASES[0]
    p64, _, _, _, _, cond, _ = R.run_case(*case, np.float64)
    bound = 8 * max(float(np.abs(R.run_case(*case, np.float32)[0] - p64).max()), R.FLOOR * 6, cond)
    assert np.abs(R.run_case(*case, np.float64, broken="scale")[0] - p64).max() > bound
    l2 = R.run_case(*case, np.float64, broken="l2")
    bound = 8 * max(float(np.abs(R.run_case(*case, np.float32, broken="l2")[0] - l2[0]).max()), R.FLOOR * 6, l2[5])
    moved = float(np.abs(l2[0] - l2[6]).max())
    assert bound <= 0.1 * moved
    assert np.abs(R.run_case(*case, np.float64, broken="adamw")[0] - l2[0]).max() > bound


def test_plan_masks_flips_and_pack_keep():
    N, bs, epochs = 50, 16, 3
    pl = CT.plan(N, bs, epochs, seed=5, flip=True)
    assert len(pl) == epochs
    g = torch.Generator().manual_seed(5)
    for perm, keep, flipped in pl:
        order = torch.randperm(N, generator=g).numpy()
        fl = (torch.rand(N, generator=g) < 0.5).numpy()
        mask = (torch.rand(N, 1280, generator=g) >= 0.2).numpy()
        assert perm.dtype == np.int32 and keep.dtype == np.uint64 and keep.shape == (N, 20)
        assert np.array_equal(flipped, fl) and 0 < fl.sum() < N
        # row or row + N, exactly where the flip draw of that DATA-SET row says
        assert np.array_equal(perm % N, order) and np.array_equal(perm >= N, fl[order])
        assert np.array_equal(CT.unpack_keep(keep), mask) and np.array_equal(CT.pack_keep(mask), keep)
        assert np.array_equal(R.unpack_keep(keep), mask) and np.array_equal(R.pack_keep(mask), keep)
    assert bool(keep[3, 7] >> np.uint64(5) & np.uint64(1)) == bool(mask[3, 64 * 7 + 5])  # word w bit j = channel 64 w + j
    again = CT.plan(N, bs, epochs, seed=5, flip=True)
    assert all(np.array_equal(a[i], b[i]) for a, b in zip(pl, again) for i in range(3))
    assert not np.array_equal(pl[0][0], CT.plan(N, bs, epochs, seed=6, flip=True)[0][0])
    for perm, keep, flipped in CT.plan(N, bs, 2, seed=5, flip=False):
        assert perm.max() == N - 1 and not flipped.any() and sorted(perm.tolist()) == list(range(N))
    rng = np.random.default_rng(0)
    mask = rng.random((7, 1280)) < 0.5
    assert np.array_equal(CT.unpack_keep(CT.pack_keep(mask)), mask)


def _png(path, colour, size=(32, 32)):
    from PIL import Image
    Image.new("RGB", size, colour).save(path)


def _cifake_tree(root, n_real=7, n_fake=(5, 6)):
    """test/REAL bright images, train/FAKE + test/FAKE dark ones, a .txt and a sub-directory to ignore."""
    os.makedirs(root / "test" / "REAL")
    os.makedirs(root / "train" / "FAKE")
    os.makedirs(root / "test" / "FAKE")
    os.makedirs(root / "test" / "REAL" / "nested.png")  # a directory with an image's name
    (root / "test" / "REAL" / "notes.txt").write_text("not an image")
    exts = (".png", ".PNG", ".jpg", ".JPEG")
    for i in range(n_real):
        _png(root / "test" / "REAL" / f"r{i}{exts[i % 4]}", (200 + i, 180, 160 + 2 * i))
    for k, folder in enumerate(("train", "test")):
        for i in range(n_fake[k]):
            _png(root / folder / "FAKE" / f"f{k}{i}{exts[i % 4]}", (20 + i, 40 + 3 * k, 30))


def test_load_cifake_data(tmp_path):
    root = tmp_path / "cifake"
    _cifake_tree(root)
    tp, ty, vp, vy = CT.load_cifake_data(str(root), sample_per_label=5)
    assert len(tp) == 8 and len(vp) == 2 and len(ty) == 8 and len(vy) == 2
    assert (ty + vy).count(0) == 5 and (ty + vy).count(1) == 5  # min(5, 7, 11) per label
    assert len(set(tp + vp)) == 10
    whole = CT.load_cifake_data(str(root))  # min(2500, 7, 11) = 7 per label, split 11 / 3
    assert (whole[1] + whole[3]).count(0) == 7 and (whole[1] + whole[3]).count(1) == 7 and len(whole[0]) == 11
    for p, y in zip(tp + vp, ty + vy):
        assert os.path.isfile(p) and (os.sep + "REAL" + os.sep in p) == (y == 0)
        assert not p.endswith(".txt") and "nested" not in p
    assert CT.load_cifake_data(str(root), sample_per_label=5) == (tp, ty, vp, vy)
    assert CT.load_cifake_data(str(root), sample_per_label=5, seed=7) != (tp, ty, vp, vy)
    a = CT.load_cifake_data(str(root), sample_per_label=2)
    assert len(a[0]) == 3 and len(a[2]) == 1
    for name in os.listdir(root / "test" / "REAL"):
        if os.path.isfile(root / "test" / "REAL" / name):
            os.remove(root / "test" / "REAL" / name)
    with pytest.raises(ValueError):
        CT.load_cifake_data(str(root))


# ---- the trainer on a stub engine (float32 restatement on CPU tensors) ----
class _StubEngine:
    """Engine.effcls_train_epoch / effcls_eval by the float32 restatement; effnet_pooled / hflip / resize_images as
    plain functions of the pixels; and the calls detector.sync makes."""
    device = torch.device("cpu")
    max_batch = 4

    def __init__(self):
        self.finalized, self.pooled_batches, self.train_calls = 0, [], []

    def load_state(self, sd, prefix=""):
        pass

    def finalize(self):
        self.finalized += 1

    def calibrate(self, names):
        self.calibrated = list(names)

    def effcls_train_epoch(self, feat, labels, perm, keep, p_drop, batch, lr, betas, eps, wd, step0, params, m, v,
                           grad_out=None):
        assert p_drop == 0.2 and betas == (0.9, 0.999) and eps == 1e-8 and wd == 0.0
        self.train_calls.append((step0, int(feat.shape[0]), int(perm.shape[0])))
        ls, cs, _ = R.epoch(feat.numpy(), labels.numpy(), perm.numpy(), keep.numpy().view(np.uint64), batch, lr, step0,
                            params.numpy(), m.numpy(), v.numpy(), np.float32)  # views: updated in place
        return torch.from_numpy(ls.astype(np.float32)), torch.from_numpy(cs.astype(np.int32))

    def effcls_eval(self, feat, labels, batch, params):
        bl, lg = R.evaluate(feat.numpy(), labels.numpy(), batch, params.numpy(), np.float32)
        return torch.from_numpy(bl.astype(np.float32)), torch.from_numpy(lg.astype(np.float32))

    def resize_supported(self, w, h):
        return True

    def resize_images(self, rgb):
        from PIL import Image
        eff = np.stack([np.asarray(Image.fromarray(a[..., :3]).resize((224, 224), Image.BILINEAR)) for a in rgb])
        return torch.from_numpy(eff), torch.from_numpy(eff.copy())

    def hflip(self, img):
        return torch.flip(img, dims=[2])

    def effnet_pooled(self, img):
        self.pooled_batches.append(int(img.shape[0]))
        x = img.float().reshape(img.shape[0], -1)[:, :1280 * 117].reshape(-1, 1280, 117).mean(-1) / 255.0
        return (x + 0.05 * torch.sin(torch.arange(1280.0))).contiguous()


def _detector(seed=0):
    det = MultiModalMisinfoDetector()
    det.load_state_dict({k: torch.as_tensor(v) for k, v in W.synthetic_detector_state(seed).items()}, strict=False)
    return det


def _stub_forensics():
    fs = object.__new__(MisinfoForensics)
    fs._verbose = False
    fs.device = torch.device("cpu")
    fs.device_jpeg, fs._jpeg = False, None
    fs.detector = _detector()
    fs.engine = _StubEngine()
    fs.detector.bind(fs.engine)
    return fs


def _fake_forensics(det):
    fs = object.__new__(MisinfoForensics)
    fs._verbose = False
    fs.detector = det
    return fs


def _two_views(N, seed):
    feat, labels = R.draws(2 * N, seed)
    return (feat[:N], feat[N:]), labels[:N]


@pytest.mark.parametrize("full", [False, True], ids=["classifier", "full_model"])
def test_checkpoint_is_a_raw_state_dict_the_fallback_path_applies(full, tmp_path):
    """Q3's counterpart.  The script's own file -- a raw timm-named state dict (train_cifake_forensics.py:374) --
    changes nothing in the detector (tests/test_checkpoint_cpu.py::test_q2_q3_fallback_files_load_nothing, and again
    below); the file ClassifierTrainer writes changes efficientnet.classifier.1.* to exactly the trained tensors and
    nothing else."""
    fs = _stub_forensics()
    det = fs.detector
    train, yt = _two_views(32, 9)
    val, yv = R.draws(8, 10)
    uploads = dict(det.uploads)
    before = {k: v.clone() for k, v in det.state_dict().items()}
    path = str(tmp_path / CT.DEFAULT_FILE)
    trainer = CT.ClassifierTrainer(fs, batch_size=8, epochs=3, lr=1e-4, seed=2, flip=True)
    hist = trainer.fit(train, yt, val, yv, checkpoint_path=path, save_full_model=full)
    assert [h["epoch"] for h in hist] == [1, 2, 3]
    assert set(hist[0]) == {"epoch", "train_loss", "train_acc", "val_loss", "val_acc"}
    assert det.uploads["effnet"] == uploads["effnet"] + 1 and fs.engine.calibrated == ["effnet"]
    assert det.uploads["text"] == uploads["text"] and det.uploads["fusion"] == uploads["fusion"]
    assert fs.engine.train_calls == [(0, 64, 32), (4, 64, 32), (8, 64, 32)]  # the two-view bank, step0 carried
    ck = torch.load(path, map_location="cpu", weights_only=True)
    eff_keys = set(det.efficientnet.state_dict())
    assert set(ck) == (eff_keys if full else set(CT.PARAM_KEYS)) and set(CT.PARAM_KEYS) <= eff_keys
    assert ck["classifier.1.weight"].shape == (2, 1280) and ck["classifier.1.bias"].shape == (2,)
    # saved on a strictly higher validation accuracy: the file is the FIRST epoch that reached the best one
    best = max(h["val_acc"] for h in hist)
    assert trainer.best_val_acc == best
    # the detector holds the saved classifier; everything else is unchanged
    trained = {k: v.clone() for k, v in det.state_dict().items()}
    for k, v in before.items():
        assert torch.equal(trained[k], v) == (not k.startswith("efficientnet.classifier.1.")), k
    for k in CT.PARAM_KEYS:
        assert torch.equal(trained["efficientnet." + k], ck[k]), k
    # ... and a fresh detector takes exactly those tensors from the file through the fallback path
    det2 = _detector()
    _fake_forensics(det2)._load_individual_weights("/nonexistent", "/nonexistent", path, "/nonexistent")
    after = det2.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], trained[k]), k
    # ... while the script's own timm-named file still changes nothing
    g = torch.Generator().manual_seed(0)
    timm = str(tmp_path / "timm.pth")
    torch.save({"efficientnet.conv_stem.weight": torch.randn(32, 3, 3, 3, generator=g),
                "efficientnet.classifier.weight": torch.randn(1, 1280, generator=g),
                "efficientnet.classifier.bias": torch.randn(1, generator=g),
                "fusion_layer.0.weight": torch.randn(512, 1538, generator=g)}, timm)
    det3 = _detector()
    _fake_forensics(det3)._load_individual_weights("/nonexistent", "/nonexistent", timm, "/nonexistent")
    for k, v in det3.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_trainer_argument_errors_and_non_finite_loss():
    fs = _stub_forensics()
    train, yt = _two_views(12, 9)
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, batch_size=65)
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, flip=True).fit(train[0], yt, train[0], yt)  # one view where two are needed
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, flip=False).fit(train[0][:, :700], yt, train[0], yt)
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, flip=False).fit(train[0], yt + 2, train[0], yt)
    hist = CT.ClassifierTrainer(fs, batch_size=4, epochs=1, flip=False).fit(train[0], yt, train[0], yt)
    assert len(hist) == 1 and fs.engine.train_calls[-1] == (0, 12, 12)
    fs.engine.effcls_eval = lambda *a: (torch.tensor([float("nan")]), torch.zeros(12, 2))
    with pytest.raises(FloatingPointError):
        CT.ClassifierTrainer(fs, batch_size=4, epochs=1, flip=False).fit(train[0], yt, train[0], yt)


def test_train_cifake_end_to_end_on_a_stub_engine(tmp_path, capsys):
    root = tmp_path / "cifake"
    _cifake_tree(root, n_real=12, n_fake=(7, 6))
    (root / "train" / "FAKE" / "broken.png").write_bytes(b"not a png at all")
    fs = _stub_forensics()
    path = str(tmp_path / "eff.pth")
    before = CT.flatten_classifier(fs.detector).clone()
    hist = CT.train_cifake(str(root), batch_size=4, lr=1e-3, epochs=3, forensics=fs, checkpoint_path=path)
    out = capsys.readouterr().out
    assert "Loaded 19 training samples" in out and "Loaded 5 validation samples" in out
    assert "Best validation accuracy" in out
    tp, ty, vp, vy = CT.load_cifake_data(str(root))
    broken = sum(p.endswith("broken.png") for p in tp + vp)
    assert ("Dropped 1 unreadable images" in out) == (broken == 1)
    assert len(hist) == 3 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert max(fs.engine.pooled_batches) <= fs.engine.max_batch
    assert sum(fs.engine.pooled_batches) == 2 * 19 + 5  # two views of the training images, one of the others
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]
    assert not torch.equal(CT.flatten_classifier(fs.detector), before)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == set(CT.PARAM_KEYS)
    # extract_image_features: an unreadable image gives ok False and zero rows, in both views
    feats, flipped, ok = CT.extract_image_features(fs, [tp[0], str(root / "train" / "FAKE" / "broken.png"), vp[0]],
                                                   flip=True)
    assert ok.tolist() == [True, False, True] and not feats[1].any() and not flipped[1].any()
    assert feats[0].any() and feats.shape == flipped.shape == (3, 1280) and feats.dtype == np.float32
    assert np.array_equal(feats[0], flipped[0])  # a uniform image is its own mirror
    f2, ok2 = CT.extract_image_features(fs, [tp[0]])
    assert np.array_equal(f2[0], feats[0]) and ok2.all()
    assert CT.extract_image_features(fs, [])[0].shape == (0, 1280)
