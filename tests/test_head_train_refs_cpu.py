"""CPU checks of the text-head training pieces that need no GPU: the float64 restatement of mmf_head_train_epoch
(tests/head_train_refs.py) against a real torch training loop, the conditions the GPU tests assert on the
reference alone, the epoch plan, the split, the checkpoint dict -- the counterpart of SURVEY quirk Q2: a file
this trainer writes IS loaded by the constructor's fallback path -- and train_head's CSV rules
(mmf_amd/head_training.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mmf_amd.head_training as HT
import mmf_amd.weights as W
from mmf_amd.api import MisinfoForensics, MultiModalMisinfoDetector
from tests import head_train_refs as R


class _MaskedDropout(nn.Module):
    """Dropout with a given mask: x * keep * 1 / (1 - p), the mask set before each forward (None: identity)."""

    def __init__(self):
        super().__init__()
        self.mult = None

    def forward(self, x):
        return x if self.mult is None else x * self.mult


def _torch_head(p0):
    W1, b1, W2, b2 = R.unpack(p0.astype(np.float64))
    net = nn.Sequential(nn.Linear(768, 256), nn.ReLU(), _MaskedDropout(), nn.Linear(256, 2)).double()
    with torch.no_grad():
        for p, src in zip(net.parameters(), (W1, b1, W2, b2)):
            p.copy_(torch.from_numpy(np.array(src)))
    return net


def _flat(net, what=lambda p: p.detach()):
    return torch.cat([what(p).reshape(-1) for p in net.parameters()]).numpy()


@pytest.mark.parametrize("N,batch,epochs,lr", [(37, 16, 2, 1e-3), (45, 3, 2, 1e-3)])
def test_restatement_equals_torch_loop(N, batch, epochs, lr):
    """The deployed nn.Sequential (Dropout replaced by the given mask x 1 / (1 - p)), autograd, clip_grad_norm_,
    AdamW and the real warmup-cosine scheduler stepped per minibatch, in float64, against epoch(dtype=float64) on
    the plan's perm / keep / lr_steps: float64 round-off."""
    from transformers import get_cosine_schedule_with_warmup
    feat, labels = R.draws(N, 4)
    p = R.initial_params(4).astype(np.float64)
    net = _torch_head(p)
    assert [k for k, _ in net.named_parameters()] == list(HT.PARAM_KEYS)
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=R.WD)
    spe = -(-N // batch)
    sched = get_cosine_schedule_with_warmup(opt, int(spe * epochs * 0.1), spe * epochs)
    m, v = np.zeros_like(p), np.zeros_like(p)
    step0 = 0
    y = torch.from_numpy(labels.astype(np.int64))
    for perm, keep, lrs in HT.plan(N, batch, epochs, lr, seed=3):
        ls, cs, ns, g_last = R.epoch(feat, labels, perm, keep, batch, lrs, step0, p, m, v, np.float64)
        step0 += len(ls)
        mask = R.unpack_keep(keep)
        for s in range(len(ls)):
            pos = np.arange(s * batch, min(N, (s + 1) * batch))
            assert lrs[s] == opt.param_groups[0]["lr"]
            net[2].mult = torch.from_numpy(mask[pos].astype(np.float64) * R.SCALE)
            opt.zero_grad()
            logits = net(torch.from_numpy(feat[perm[pos]]).double())
            loss = nn.functional.cross_entropy(logits, y[perm[pos]])
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=R.MAX_NORM)
            if s == len(ls) - 1:
                np.testing.assert_allclose(g_last, _flat(net, lambda q: q.grad), rtol=0, atol=1e-13)
            opt.step()
            sched.step()
            assert abs(loss.item() - ls[s]) < 1e-13
            assert abs(norm.item() - ns[s]) < 1e-12
            assert int((logits.argmax(-1) == y[perm[pos]]).sum()) == cs[s]
    np.testing.assert_allclose(p, _flat(net), rtol=0, atol=1e-12)
    st = opt.state
    np.testing.assert_allclose(m, np.concatenate([st[q]["exp_avg"].reshape(-1).numpy() for q in net.parameters()]),
                               rtol=0, atol=1e-13)
    np.testing.assert_allclose(v, np.concatenate([st[q]["exp_avg_sq"].reshape(-1).numpy() for q in net.parameters()]),
                               rtol=0, atol=1e-13)


def test_eval_restatement_equals_torch():
    feat, labels = R.draws(21, 5)
    p0 = R.initial_params(5)
    net = _torch_head(p0).eval()
    losses, lg = R.evaluate(feat, labels, 8, p0)
    with torch.no_grad():
        for k, a in enumerate(range(0, 21, 8)):
            out = net(torch.from_numpy(feat[a:a + 8]).double())
            np.testing.assert_allclose(lg[a:a + 8], out.numpy(), rtol=0, atol=1e-14)
            want = nn.functional.cross_entropy(out, torch.from_numpy(labels[a:a + 8].astype(np.int64)))
            assert abs(want.item() - losses[k]) < 1e-13


def test_float32_restatement_sits_inside_the_single_step_bounds():
    """The derived bounds are bounds of any fp32 evaluation, and the reference alone decides both branches: the
    norm above 1.5 x ("clip") or below 0.67 x ("noclip") max_norm, every |pre| above its own forward bound."""
    for B in R.SINGLE_BATCHES:
        for regime in ("clip", "noclip"):
            for dropout in (True, False):
                feat, labels, perm, keep, p0, max_norm, b, seed = R.single_case(B, regime, dropout)
                assert b["relu_ok"] and b["clamp_ok"], (B, regime, dropout)
                assert (b["norm"] > 1.5 * max_norm) if regime == "clip" else (b["norm"] < 0.67 * max_norm)
                assert (b["coef"] < 1) == (regime == "clip")
                W1, b1, W2, b2 = R.unpack(p0)
                mult = R._mult(keep, np.arange(B), np.float32)
                r32 = R.forward_backward(feat[perm], mult, W1, b1, W2, b2, labels[perm], np.float32)
                assert np.array_equal(r32["live"], b["r"]["live"])  # no hidden unit on the other side
                g32 = R.flat(r32["grads"])
                n32 = np.sqrt((g32 * g32).sum(dtype=np.float32))
                g32 = g32 * R.clip_coef(n32, max_norm, np.float32)
                assert (np.abs(g32 - b["grad"]) <= b["grad_tol"]).all(), (B, regime, dropout)
                assert abs(float(r32["loss"]) - b["loss"]) <= b["loss_tol"]
                assert abs(float(n32) - b["norm"]) <= b["norm_tol"]
                assert (np.abs(r32["lg"] - b["lg"]) <= b["lg_tol"]).all()
                # the bounds say something
                assert b["loss_tol"] < 1e-3 and b["norm_tol"] < 5e-3 * b["norm"] and b["lg_tol"].max() < 1e-3
                assert np.median(b["grad_tol"]) < 1e-3 * np.abs(b["grad"]).max()


def test_multi_step_cases_qualify():
    """What the GPU test's bound 8 x max(e32, FLOOR x steps, cond) rests on, asserted on the reference alone: the
    parameters stay below 0.125 (the floor's premise), float32 sits inside the bound, and the bound stays below a
    tenth of the distance the float64 run moved its parameters, so a kernel that trains differently lands outside."""
    assert R.FLOOR == 2.0 ** -27
    for case in R.MULTI_CASES:
        p64, _, _, l64, _, plan, cond, p0 = R.run_case(*case, np.float64)
        p32 = R.run_case(*case, np.float32)[0]
        steps = sum(len(l) for l in l64)
        assert steps == -(-case[0] // case[1]) * case[2] and len(plan) == case[2]
        assert np.abs(p64).max() < 0.125 and np.abs(p32).max() < 0.125
        e32 = float(np.abs(p32 - p64).max())
        bound = 8 * max(e32, R.FLOOR * steps, cond)
        moved = float(np.abs(p64 - p0).max())
        print(f"case {case}: e32 = {e32:.3g}, cond = {cond:.3g}, floor = {R.FLOOR * steps:.3g}, bound = {bound:.3g}, "
              f"moved = {moved:.3g}, ratio = {bound / moved:.3g}")
        assert cond > 0 and e32 <= bound
        assert bound <= 0.1 * moved, (case, bound, moved)
    # a trainer without the dropout scale, or with the bias correction of the wrong step, ends outside the bound
    case = R.MULTI_CASES[0]
    p64, _, _, l64, _, plan, cond, p0 = R.run_case(*case, np.float64)
    bound = 8 * max(float(np.abs(R.run_case(*case, np.float32)[0] - p64).max()), R.FLOOR * 6, cond)
    feat, labels = R.draws(case[0], R.MULTI_SEED)
    for wrong in ("scale", "step"):
        q = p0.astype(np.float64)
        m, v = np.zeros_like(q), np.zeros_like(q)
        step0 = 0
        scale = R.SCALE
        try:
            if wrong == "scale":
                R.SCALE = 1.0
            for perm, keep, lrs in plan:
                R.epoch(feat, labels, perm, keep, case[1], lrs, step0 + (wrong == "step"), q, m, v, np.float64)
                step0 += len(lrs)
        finally:
            R.SCALE = scale
        assert np.abs(q - p64).max() > bound, wrong


def test_plan_learning_rates_masks_and_split():
    from transformers import get_cosine_schedule_with_warmup
    N, bs, epochs, lr = 100, 16, 3, 1e-3
    pl = HT.plan(N, bs, epochs, lr, seed=5)
    assert len(pl) == epochs
    opt = torch.optim.AdamW([nn.Parameter(torch.zeros(1))], lr=lr)
    sched = get_cosine_schedule_with_warmup(opt, num_warmup_steps=int(21 * 0.1), num_training_steps=21)
    want = []
    for _ in range(21):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    got = np.concatenate([p[2] for p in pl])
    assert got.dtype == np.float64 and got.tolist() == want and got[0] == 0.0 and got.max() == lr
    np.testing.assert_allclose(R.lr_schedule(21, lr), want, rtol=1e-13, atol=0)  # the refs' restatement
    g = torch.Generator().manual_seed(5)
    for perm, keep, lrs in pl:
        assert perm.dtype == np.int32 and np.array_equal(perm, torch.randperm(N, generator=g).numpy())
        mask = (torch.rand(N, 256, generator=g) >= 0.3).numpy()
        assert keep.dtype == np.uint64 and keep.shape == (N, 4)
        assert np.array_equal(R.unpack_keep(keep), mask) and np.array_equal(R.pack_keep(mask), keep)
        assert len(lrs) == 7
    assert bool(keep[3, 1] >> np.uint64(5) & np.uint64(1)) == bool(mask[3, 64 + 5])  # word w bit j = unit 64 w + j
    assert [np.array_equal(a[0], b[0]) for a, b in zip(pl, HT.plan(N, bs, epochs, lr, seed=5))] == [True] * 3
    # the split: torch.utils.data.random_split with manual_seed(42)
    from torch.utils.data import random_split
    for n in (10, 37, 101):
        tr, va = random_split(range(n), [n - int(0.2 * n), int(0.2 * n)], generator=torch.Generator().manual_seed(42))
        a, b = HT.split_indices(n)
        assert a.tolist() == list(tr.indices) and b.tolist() == list(va.indices)


# ---- the trainer on a stub engine (float32 restatement on CPU tensors) ----
class _StubEngine:
    """Engine.head_train_epoch / head_eval / text_pooled by the float32 restatement, and the calls detector.sync
    makes."""
    device = torch.device("cpu")
    max_batch, max_text_len, max_clip_len = 4, 128, 77

    def __init__(self):
        self.finalized, self.pooled_shapes, self.train_calls = 0, [], []

    def load_state(self, sd, prefix=""):
        pass

    def finalize(self):
        self.finalized += 1

    def calibrate(self, names):
        pass

    def head_train_epoch(self, feat, labels, perm, keep, p_drop, batch, lr_steps, betas, eps, wd, max_norm, step0,
                         params, m, v, grad_out=None):
        assert p_drop == 0.3 and betas == (0.9, 0.999) and eps == 1e-8
        self.train_calls.append((step0, list(lr_steps)))
        p, mm, vv = params.numpy(), m.numpy(), v.numpy()  # views: updated in place
        ls, cs, ns, _ = R.epoch(feat.numpy(), labels.numpy(), perm.numpy(), keep.numpy().view(np.uint64), batch,
                                lr_steps, step0, p, mm, vv, np.float32, wd=wd, max_norm=max_norm)
        return (torch.from_numpy(ls.astype(np.float32)), torch.from_numpy(cs.astype(np.int32)),
                torch.from_numpy(ns.astype(np.float32)))

    def head_eval(self, feat, labels, batch, params):
        bl, lg = R.evaluate(feat.numpy(), labels.numpy(), batch, params.numpy(), np.float32)
        return torch.from_numpy(bl.astype(np.float32)), torch.from_numpy(lg.astype(np.float32))

    def text_pooled(self, ids, mask):
        ids, mask = np.asarray(ids), np.asarray(mask)
        self.pooled_shapes.append(ids.shape)
        out = np.zeros((ids.shape[0], 768), np.float32)
        for i in range(ids.shape[0]):  # a function of the unpadded ids alone
            n = int(mask[i].sum())
            g = np.random.default_rng(ids[i, :n].astype(np.int64))
            out[i] = g.standard_normal(768) + (1.5 if ids[i, 1] % 2 else -1.5) * np.sin(np.arange(768))
        return torch.from_numpy(out)


class _Tok:
    """text -> [0, 3 + parity marker, word hashes ..., 2]; truncation cuts, as the table tokenizer."""

    def __call__(self, text, return_tensors="pt", max_length=512, truncation=True, padding=True):
        texts = [text] if isinstance(text, str) else list(text)
        seqs = []
        for t in texts:
            words = t.split()
            s = [0, 4 if "machine" in t else 3] + [5 + (sum(map(ord, w)) % 1000) for w in words] + [2]
            seqs.append(s[:max_length] if truncation else s)
        L = max(len(s) for s in seqs)
        ids = torch.full((len(seqs), L), 1, dtype=torch.long)
        mask = torch.zeros((len(seqs), L), dtype=torch.long)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.tensor(s)
            mask[i, :len(s)] = 1
        return {"input_ids": ids, "attention_mask": mask}


def _detector(seed=0):
    det = MultiModalMisinfoDetector()
    det.load_state_dict({k: torch.as_tensor(v) for k, v in W.synthetic_detector_state(seed).items()}, strict=False)
    return det


def _stub_forensics():
    fs = object.__new__(MisinfoForensics)
    fs._verbose = False
    fs.detector = _detector()
    fs.engine = _StubEngine()
    fs.detector.bind(fs.engine)
    fs.roberta_tokenizer = _Tok()
    return fs


def _fake_forensics(det):
    fs = object.__new__(MisinfoForensics)
    fs._verbose = False
    fs.detector = det
    return fs


@pytest.mark.parametrize("head", HT.HEADS)
def test_checkpoint_is_the_references_dict_and_the_fallback_path_loads_it(head, tmp_path):
    """Q2's counterpart.  tests/test_checkpoint_cpu.py::test_q2_q3_fallback_files_load_nothing pins that the file
    train_ai_head.py writes changes nothing; the file HeadTrainer writes changes the trained head to exactly the
    trained tensors and nothing else."""
    fs = _stub_forensics()
    det = fs.detector
    N = 40
    feat, labels = R.draws(N, 9)
    tr, va = HT.split_indices(N)
    uploads = dict(det.uploads)
    before = {k: v.clone() for k, v in det.state_dict().items()}
    path = str(tmp_path / HT.DEFAULT_FILES[head])
    trainer = HT.HeadTrainer(fs, head=head, batch_size=8, epochs=3, lr=1e-3, seed=2)
    hist = trainer.fit(feat[tr], labels[tr], feat[va], labels[va], checkpoint_path=path, save_full_model=False)
    assert [h["epoch"] for h in hist] == [1, 2, 3]
    assert det.uploads["text"] == uploads["text"] + 1 and det.uploads["fusion"] == uploads["fusion"]
    # per-step learning rates of the whole run went to the engine, step0 carried over
    assert [c[0] for c in fs.engine.train_calls] == [0, 4, 8]
    assert sum((c[1] for c in fs.engine.train_calls), []) == np.concatenate(
        [p[2] for p in HT.plan(32, 8, 3, 1e-3, 2)]).tolist()
    best = min(hist, key=lambda h: (h["val_loss"], h["epoch"]))
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "val_loss",
                       "val_acc", "train_loss", "train_acc"}
    assert ck["epoch"] == best["epoch"] and ck["val_loss"] == best["val_loss"] and ck["val_acc"] == best["val_acc"]
    assert ck["train_loss"] == best["train_loss"] and ck["train_acc"] == best["train_acc"]
    assert set(ck["model_state_dict"]) == {f"{head}.{k}" for k in HT.PARAM_KEYS}
    assert ck["scheduler_state_dict"]["last_epoch"] == 4 * best["epoch"]
    # the optimizer dict loads into a real AdamW over a head's parameters
    fresh = nn.Sequential(nn.Linear(768, 256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 2))
    opt = torch.optim.AdamW(fresh.parameters(), lr=1e-3, weight_decay=0.01)
    opt.load_state_dict(ck["optimizer_state_dict"])
    assert [int(opt.state[p]["step"]) for p in fresh.parameters()] == [4 * best["epoch"]] * 4
    assert opt.state[fresh[0].weight]["exp_avg"].shape == (256, 768) and opt.state[fresh[0].weight]["exp_avg"].any()
    assert opt.param_groups[0]["initial_lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 0.01
    # the detector holds the best epoch's head; everything else is unchanged
    trained = {k: v.clone() for k, v in det.state_dict().items()}
    for k, v in before.items():
        assert torch.equal(trained[k], v) == (not k.startswith(head + ".")), k
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(trained[k], v), k
    # ... and a fresh detector takes exactly those tensors from the file through the fallback path
    det2 = _detector()
    args = ["/nonexistent"] * 4
    args[HT.HEADS.index(head)] = path
    _fake_forensics(det2)._load_individual_weights(*args)
    after = det2.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], trained[k]), k
        assert torch.equal(after[k], v) == (not k.startswith(head + ".")), k


def test_full_model_checkpoint_and_non_finite_loss(tmp_path):
    fs = _stub_forensics()
    feat, labels = R.draws(12, 9)
    path = str(tmp_path / "full.pth")
    HT.HeadTrainer(fs, batch_size=4, epochs=1).fit(feat, labels, feat, labels, checkpoint_path=path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = fs.detector.state_dict()
    assert set(ck["model_state_dict"]) == set(sd)
    for k, v in sd.items():
        assert torch.equal(ck["model_state_dict"][k], v), k
    with pytest.raises(ValueError):
        HT.HeadTrainer(fs, head="fusion_layer")
    with pytest.raises(ValueError):
        HT.HeadTrainer(fs, batch_size=65)
    with pytest.raises(ValueError):
        HT.HeadTrainer(fs).fit(feat[:, :700], labels, feat, labels)
    with pytest.raises(ValueError):
        HT.HeadTrainer(fs).fit(feat, labels + 2, feat, labels)
    fs.engine.head_eval = lambda *a: (torch.tensor([float("nan")]), torch.zeros(12, 2))
    with pytest.raises(FloatingPointError):
        HT.HeadTrainer(fs, batch_size=4, epochs=1).fit(feat, labels, feat, labels)


def test_train_head_from_a_csv(tmp_path, capsys):
    import pandas as pd
    fs = _stub_forensics()
    fs._run_chunks = MisinfoForensics._run_chunks
    fs._fit_text = lambda n: None
    assert HT.train_head(str(tmp_path / "missing.csv"), forensics=fs) is None
    rows = [("a human wrote this sentence number %d" % i, 0) if i % 2 else ("machine text number %d" % i, 1)
            for i in range(30)]
    rows += [("   ", 1), (" \t ", 0)]  # stripped to nothing: dropped (train_ai_head.py:176-177)
    csv = str(tmp_path / "hc3.csv")
    pd.DataFrame(rows, columns=["text", "label"]).to_csv(csv, index=False)
    path = str(tmp_path / "ai_head_best.pth")
    hist = HT.train_head(csv, head="ai_head", checkpoint_path=path, batch_size=8, epochs=2, forensics=fs,
                         save_full_model=False)
    out = capsys.readouterr().out
    assert "Loaded 30 samples" in out and "Training: 24 samples" in out and "Confusion Matrix" in out
    assert len(hist) == 2 and sum(s[0] for s in fs.engine.pooled_shapes) == 30
    assert max(s[0] for s in fs.engine.pooled_shapes) <= fs.engine.max_batch
    assert torch.load(path, weights_only=True)["epoch"] in (1, 2)
    # each text once, truncated at max_length; the features are those of the truncated ids
    fs.engine.pooled_shapes.clear()
    long = "word " * 40
    a = HT.extract_text_features(fs, [long, "short one"], max_length=16)
    assert fs.engine.pooled_shapes == [(2, 16)]
    ids = fs.roberta_tokenizer(long)["input_ids"][:, :16].numpy()
    assert np.array_equal(a[0], fs.engine.text_pooled(ids, np.ones_like(ids))[0].numpy())
    assert np.array_equal(HT.confusion_matrix([0, 1, 1, 0, 1], [0, 1, 0, 0, 1]), [[2, 0], [1, 2]])
