"""CPU checks of the projection-head training pieces that need no GPU: the float64 restatement of
mmf_clip_train_epoch (tests/clip_train_refs.py) against a real torch training loop, the conditions the GPU tests
assert on the reference alone, the median-accuracy rule, the epoch plan, the checkpoint dict and
extract_features' dataset rules (mmf_amd/clip_training.py)."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import mmf_amd.clip_training as CT
from tests import clip_train_refs as R


class _TorchHeads(nn.Module):
    def __init__(self, p0):
        super().__init__()
        Wv, Wt, ls = R.unpack(p0.astype(np.float64))
        self.visual_projection = nn.Linear(768, 512, bias=False).double()
        self.text_projection = nn.Linear(512, 512, bias=False).double()
        self.logit_scale = nn.Parameter(torch.tensor(float(ls[0]), dtype=torch.float64))
        with torch.no_grad():
            self.visual_projection.weight.copy_(torch.from_numpy(Wv))
            self.text_projection.weight.copy_(torch.from_numpy(Wt))

    def flat(self, what=lambda p: p.detach()):
        return torch.cat([what(p).reshape(-1) for p in (self.visual_projection.weight, self.text_projection.weight,
                                                        self.logit_scale)]).numpy()

    def loss(self, pi, pt):
        """train_clip_detective.py:129-166 in the project's words: unit rows, exp(logit_scale) I T^T, the mean of
        the two cross-entropies against the diagonal."""
        ie, te = self.visual_projection(pi), self.text_projection(pt)
        ie, te = ie / ie.norm(dim=-1, keepdim=True), te / te.norm(dim=-1, keepdim=True)
        logits = self.logit_scale.exp() * ie @ te.t()
        target = torch.arange(pi.shape[0])
        return (nn.functional.cross_entropy(logits, target) + nn.functional.cross_entropy(logits.t(), target)) / 2


@pytest.mark.parametrize("N,batch,epochs,lr", [(37, 16, 2, 1e-4), (7, 3, 2, 1e-3)])
def test_restatement_equals_torch_loop(N, batch, epochs, lr):
    """Two bias-free nn.Linear + a logit_scale parameter, autograd, clip_grad_norm_, AdamW and CosineAnnealingLR in
    float64 against epoch(dtype=float64) on the plan's perm / lr: float64 round-off."""
    img, txt = R.draws(N, 4)
    p = R.initial_params(4).astype(np.float64)
    net = _TorchHeads(p)
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=R.WD)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr * 0.01)
    m, v = np.zeros_like(p), np.zeros_like(p)
    step0 = 0
    for perm, lr_e in CT.plan(N, epochs, lr, seed=3):
        assert lr_e == opt.param_groups[0]["lr"]
        ls, ns, g_last, _ = R.epoch(img, txt, perm, batch, lr_e, step0, p, m, v, np.float64)
        step0 += len(ls)
        for s in range(len(ls)):
            pos = np.arange(s * batch, min(N, (s + 1) * batch))
            opt.zero_grad()
            loss = net.loss(torch.from_numpy(img[perm[pos]]).double(), torch.from_numpy(txt[perm[pos]]).double())
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=R.MAX_NORM)
            if s == len(ls) - 1:
                np.testing.assert_allclose(g_last, net.flat(lambda q: q.grad), rtol=0, atol=1e-13)
            opt.step()
            assert abs(loss.item() - ls[s]) < 1e-13
            assert abs(norm.item() - ns[s]) < 1e-12
        sched.step()
    np.testing.assert_allclose(p, net.flat(), rtol=0, atol=1e-12)
    st = opt.state
    prm = (net.visual_projection.weight, net.text_projection.weight, net.logit_scale)
    np.testing.assert_allclose(m, np.concatenate([st[q]["exp_avg"].reshape(-1).numpy() for q in prm]), rtol=0,
                               atol=1e-13)
    np.testing.assert_allclose(v, np.concatenate([st[q]["exp_avg_sq"].reshape(-1).numpy() for q in prm]), rtol=0,
                               atol=1e-13)


def test_eval_restatement_equals_torch():
    img, txt = R.draws(21, 5)
    p0 = R.initial_params(5)
    net = _TorchHeads(p0)
    losses, cos = R.evaluate(img, txt, 8, p0)
    with torch.no_grad():
        for k, a in enumerate(range(0, 21, 8)):
            pi, pt = torch.from_numpy(img[a:a + 8]).double(), torch.from_numpy(txt[a:a + 8]).double()
            assert abs(net.loss(pi, pt).item() - losses[k]) < 1e-13
            ie, te = net.visual_projection(pi), net.text_projection(pt)
            sim = ((ie / ie.norm(dim=-1, keepdim=True)) * (te / te.norm(dim=-1, keepdim=True))).sum(-1).numpy()
            np.testing.assert_allclose(cos[a:a + 8], sim, rtol=0, atol=1e-14)


def test_float32_restatement_sits_inside_the_single_step_bounds():
    """The derived bounds are bounds of any fp32 evaluation, and the reference alone decides the clamp: norms above
    1.5 ("clip") or below 0.67 ("noclip")."""
    for B in R.SINGLE_BATCHES:
        for regime in ("clip", "noclip"):
            img, txt, p0 = R.single_case(B, regime)
            b = R.step_bounds(img, txt, p0.astype(np.float64))
            if B > 1:
                assert (b["norm"] > 1.5) if regime == "clip" else (b["norm"] < 0.67), (B, regime, b["norm"])
                assert (b["coef"] < 1) == (regime == "clip")
            Wv, Wt, ls = R.unpack(p0)
            r32 = R.forward_backward(img, txt, Wv, Wt, ls[0], np.float32)
            g32 = R.flat(r32["grads"])
            n32 = np.sqrt((g32 * g32).sum(dtype=np.float32))
            g32 = g32 * R.clip_coef(n32, R.MAX_NORM, np.float32)
            assert (np.abs(g32 - b["grad"]) <= b["grad_tol"]).all(), (B, regime)
            assert abs(float(r32["loss"]) - b["loss"]) <= b["loss_tol"]
            assert abs(float(n32) - b["norm"]) <= b["norm_tol"]
            assert (np.abs(r32["row_cos"] - b["r"]["row_cos"]) <= b["cos_tol"]).all()
            if B > 1:  # the bounds say something
                assert b["loss_tol"] < 1e-2 and b["norm_tol"] < 0.05 * b["norm"] and b["cos_tol"].max() < 1e-3
                assert np.median(b["grad_tol"]) < 0.05 * np.abs(b["grad"]).max()
            else:
                assert b["loss"] == 0 and b["norm"] == 0 and not b["grad"].any()


def test_multi_step_reference_conditioning():
    """Every multi-step case's conditioning number is below the floor of the GPU test's bound
    (clip_train_refs' docstring); float32 stays within the bound itself."""
    assert R.FLOOR == 2.0 ** -22
    for case in R.MULTI_CASES:
        p64, _, _, l64, _, _, cond = R.run_case(*case, np.float64)
        p32 = R.run_case(*case, np.float32)[0]
        steps = sum(len(l) for l in l64)
        assert steps == case[2] * -(-case[0] // case[1])
        assert cond <= R.FLOOR * steps, (case, cond)
        assert np.abs(p32 - p64).max() <= 8 * R.FLOOR * steps, case
        assert np.abs(p64[:-1]).max() < 0.25 and 2 <= p64[-1] < 4  # the magnitudes the floor is derived from


def test_median_accuracy_rule():
    """torch.median is the lower median; cos <= threshold predicts 1 (train_clip_detective.py:181-186)."""
    # even count: sorted 0.1 0.2 0.3 0.4 -> threshold 0.2 (not 0.25): predictions 1 1 0 0
    assert CT.batch_accuracy([0.3, 0.1, 0.4, 0.2], [0, 1, 0, 1]) == 1.0
    assert CT.batch_accuracy([0.3, 0.1, 0.4, 0.2], [1, 1, 0, 1]) == 0.75
    # odd count: threshold 0.3 -> predictions of (0.3, 0.1, 0.5) are 1 1 0
    assert CT.batch_accuracy([0.3, 0.1, 0.5], [1, 1, 0]) == 1.0
    # ties at the threshold are all predicted 1
    assert CT.batch_accuracy([0.2, 0.2, 0.2, 0.9], [1, 1, 1, 0]) == 1.0
    assert CT.batch_accuracy([0.2, 0.2, 0.2, 0.2], [0, 0, 1, 1]) == 0.5
    assert CT.batch_accuracy([0.7], [1]) == 1.0
    g = np.random.default_rng(0)
    for n in (1, 2, 5, 8, 16):
        cos = np.round(g.uniform(-1, 1, n), 1).astype(np.float32)  # rounded: ties happen
        lab = g.integers(0, 2, n)
        assert CT.batch_accuracy(cos, lab) == pytest.approx(R.lower_median_accuracy(cos, lab), abs=1e-7)


def test_plan_is_deterministic_and_follows_the_scheduler():
    a, b, c = CT.plan(37, 5, 1e-4, seed=11), CT.plan(37, 5, 1e-4, seed=11), CT.plan(37, 5, 1e-4, seed=12)
    assert len(a) == 5
    for (p1, l1), (p2, l2) in zip(a, b):
        assert np.array_equal(p1, p2) and l1 == l2 and p1.dtype == np.int32 and p1.shape == (37,)
        assert sorted(p1.tolist()) == list(range(37))
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, c))
    assert not np.array_equal(a[0][0], a[1][0])  # a fresh permutation per epoch
    opt = torch.optim.AdamW([nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5, eta_min=1e-6)
    for _, lr in a:
        assert lr == opt.param_groups[0]["lr"]
        opt.step()
        sched.step()
    assert a[0][1] == 1e-4 and a[-1][1] > 1e-6


# ---- the trainer on a CPU engine ----
class _CpuEngine:
    """Engine.clip_train_epoch / clip_contrastive_eval by the float32 restatement, on CPU tensors."""
    device = torch.device("cpu")
    max_batch = 4

    def __init__(self):
        self.projections = []

    def clip_train_epoch(self, ti, tt, perm, batch, lr, betas, eps, wd, max_norm, step0, params, m, v, grad_out=None):
        ls, ns, _, _ = R.epoch(ti.numpy(), tt.numpy(), perm.numpy(), batch, lr, step0, params.numpy(), m.numpy(),
                               v.numpy(), np.float32, wd=wd, max_norm=max_norm)
        return torch.from_numpy(ls.astype(np.float32)), torch.from_numpy(ns.astype(np.float32))

    def clip_contrastive_eval(self, vi, vt, batch, params):
        ls, cos = R.evaluate(vi.numpy(), vt.numpy(), batch, params.numpy(), np.float32)
        return torch.from_numpy(ls.astype(np.float32)), torch.from_numpy(cos.astype(np.float32))

    def set_clip_projections(self, visual=None, text=None):
        self.projections.append((visual.clone(), text.clone()))


def _clip_state(seed=0):
    """A CLIPModel-shaped state dict with the real trained tensors and small stand-ins for the frozen ones."""
    p = R.initial_params(seed)
    Wv, Wt, ls = R.unpack(p)
    return {"logit_scale": np.float32(ls[0]), "text_model.final_layer_norm.weight": np.ones(512, np.float32),
            "text_model.embeddings.position_ids": np.arange(77, dtype=np.int64)[None],
            "vision_model.post_layernorm.bias": np.zeros(768, np.float32),
            "visual_projection.weight": Wv.copy(), "text_projection.weight": Wt.copy()}


class _Detective(nn.Module):
    """CLIPDetective's shape: a CLIPModel-like child `clip` (frozen towers, then the projections; logit_scale is
    the model's own parameter), optimised as the reference does: the parameters that require grad."""

    def __init__(self):
        super().__init__()
        self.clip = nn.Module()
        self.clip.logit_scale = nn.Parameter(torch.zeros(()))
        self.clip.text_model = nn.Linear(4, 4)
        self.clip.vision_model = nn.Linear(4, 4)
        self.clip.visual_projection = nn.Linear(768, 512, bias=False)
        self.clip.text_projection = nn.Linear(512, 512, bias=False)
        for q in list(self.clip.text_model.parameters()) + list(self.clip.vision_model.parameters()):
            q.requires_grad = False


def test_fit_checkpoint_has_the_reference_layout(tmp_path):
    import mmf_amd.vault_builder as VB
    state = _clip_state()
    before = CT.flatten_heads(state).clone()
    vault_sets = []
    f = types.SimpleNamespace(engine=_CpuEngine(), clip_state=state, vault_loaded=True, vault_embeddings="E",
                              vault_metadata="M", _emb_cache=("k", "v"),
                              set_vault=lambda e, m: vault_sets.append((e, m)))
    ti, tt = R.draws(20, 2)
    vi, vt = R.draws(10, 3)
    labels = np.arange(10) % 2
    path = str(tmp_path / "clip_detective_best.pth")
    hist = CT.ClipProjectionTrainer(f, batch_size=8, epochs=3, lr=1e-4, seed=5).fit((ti, tt), (vi, vt), labels,
                                                                                  checkpoint_path=path)
    assert [h["epoch"] for h in hist] == [0, 1, 2]
    assert [h["lr"] for h in hist] == [lr for _, lr in CT.plan(20, 3, 1e-4, 5)]
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) and 0 <= h["val_accuracy"] <= 1 for h in hist)
    # the restatement on the same plan: per-epoch parameters, train_loss = the plain mean of the step losses,
    # val_accuracy = the mean over batches of the per-batch accuracy
    p = before.numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    step0, per_epoch = 0, []
    for (perm, lr), h in zip(CT.plan(20, 3, 1e-4, 5), hist):
        ls, _, _, _ = R.epoch(ti, tt, perm, 8, lr, step0, p, m, v, np.float32)
        step0 += len(ls)
        assert h["train_loss"] == float(ls.astype(np.float32).astype(np.float64).mean())
        vl, cos = R.evaluate(vi, vt, 8, p, np.float32)
        accs = [R.lower_median_accuracy(cos[a:a + 8], labels[a:a + 8]) for a in (0, 8)]
        assert h["val_accuracy"] == pytest.approx(np.mean(accs), abs=1e-7)
        per_epoch.append((p.copy(), m.copy(), v.copy(), step0))
    best = max(hist, key=lambda h: (h["val_accuracy"], -h["epoch"]))  # the first epoch reaching the best accuracy
    bp, bm, bv, bsteps = per_epoch[best["epoch"]]
    # forensics holds the BEST epoch's heads, the engine got them, the loaded vault was set again
    assert np.array_equal(CT.flatten_heads(f.clip_state).numpy(), bp) and not np.array_equal(bp, before.numpy())
    assert isinstance(f.clip_state["visual_projection.weight"], np.ndarray)
    assert len(f.engine.projections) == 1 and np.array_equal(f.engine.projections[0][1].numpy().reshape(-1),
                                                              bp[R.NV:R.NV + R.NT])
    assert vault_sets == [("E", "M")] and f._emb_cache is None
    # the file
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "val_loss",
                       "val_accuracy", "train_loss"}
    assert ck["epoch"] == best["epoch"] and ck["val_accuracy"] == best["val_accuracy"]
    assert ck["val_loss"] == best["val_loss"] and ck["train_loss"] == best["train_loss"]
    assert set(ck["model_state_dict"]) == {"clip." + k for k in state}
    sd, meta = VB.load_clip_detective_checkpoint(path)
    assert set(sd) == set(state) and meta == {"epoch": best["epoch"], "val_accuracy": best["val_accuracy"]}
    assert np.array_equal(CT.flatten_heads(sd).numpy(), bp)
    assert np.array_equal(sd["text_model.final_layer_norm.weight"], state["text_model.final_layer_norm.weight"])
    # the optimizer state loads into the reference's optimizer over a CLIPDetective-shaped module
    det = _Detective()
    opt = torch.optim.AdamW([q for q in det.parameters() if q.requires_grad], lr=1e-4, weight_decay=0.01)
    opt.load_state_dict(ck["optimizer_state_dict"])
    want = {"visual": (det.clip.visual_projection.weight, slice(0, R.NV)),
            "text": (det.clip.text_projection.weight, slice(R.NV, R.NV + R.NT)),
            "scale": (det.clip.logit_scale, slice(R.NV + R.NT, None))}
    for q, sl in want.values():
        st = opt.state[q]
        assert float(st["step"]) == bsteps and st["exp_avg"].shape == q.shape
        assert np.array_equal(st["exp_avg"].reshape(-1).numpy(), bm[sl])
        assert np.array_equal(st["exp_avg_sq"].reshape(-1).numpy(), bv[sl])
    # saved after scheduler.step(), as the reference: epoch + 1 steps, the group holds the next learning rate
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3, eta_min=1e-6)
    sched.load_state_dict(ck["scheduler_state_dict"])
    assert sched.last_epoch == ck["epoch"] + 1
    assert opt.param_groups[0]["lr"] == sched.get_last_lr()[0] and opt.param_groups[0]["weight_decay"] == 0.01


def test_fit_validates_its_inputs_and_traps_a_non_finite_loss():
    f = types.SimpleNamespace(engine=_CpuEngine(), clip_state=_clip_state(), vault_loaded=False)
    tr = CT.ClipProjectionTrainer(f, batch_size=4, epochs=1)
    ti, tt = R.draws(8, 2)
    with pytest.raises(ValueError):
        tr.fit((ti[:, :512], tt), (ti, tt), np.zeros(8))
    bad = ti.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        tr.fit((bad, tt), (ti, tt), np.zeros(8))
    with pytest.raises(ValueError):
        tr.fit((ti, tt), (ti, tt), np.zeros(7))
    with pytest.raises(ValueError):
        CT.ClipProjectionTrainer(f, batch_size=65)
    zero = np.zeros_like(ti)  # a zero row has no direction: 0 / 0, as in the reference
    with pytest.raises(FloatingPointError), np.errstate(all="ignore"):
        tr.fit((zero, tt), (ti, tt), np.zeros(8))


# ---- extract_features' dataset rules, on a stub ----
class _Tok:
    """One token per word (+ BOS / EOS)."""

    def __call__(self, text=None, return_tensors="pt", padding=True, truncation=False, max_length=None):
        seqs = [[0] + [5 + len(w) for w in t.split()] + [2] for t in list(text)]
        if truncation:
            seqs = [s[:max_length or 77] for s in seqs]
        L = max(len(s) for s in seqs)
        return {"input_ids": [s + [1] * (L - len(s)) for s in seqs],
                "attention_mask": [[1] * len(s) + [0] * (L - len(s)) for s in seqs]}


class _StubForensics:
    """The attributes extract_features uses.  An image's features are its mean pixel value + 1, a caption's its
    token count; _stage_images raises for the whole chunk when one file does not open, as the real one does."""

    def __init__(self, max_batch=4):
        from mmf_amd.api import MisinfoForensics
        from PIL import Image
        self.Image = Image
        self.clip_processor, self.clip_eos_token_id = _Tok(), 2
        self.engine = _CpuEngine()
        self.engine.max_batch = max_batch
        self.engine.clip_pooled = self.clip_pooled
        self._run_chunks = MisinfoForensics._run_chunks
        self.clip_state = _clip_state()
        self.vault_loaded = False
        self.chunks, self.lengths = [], []

    def _ensure_jpeg_stager(self):
        pass

    def _stage_images(self, images):
        return ([np.asarray(x if isinstance(x, self.Image.Image) else self.Image.open(x).convert("RGB")) for x in images],)

    def _windows(self, arrs):
        assert all(a.shape == (224, 224, 3) for a in arrs)
        return None, np.stack(arrs)

    def clip_pooled(self, clp, cid, cm):
        assert clp.shape[0] == cid.shape[0] and cid.shape[1] <= 77
        self.chunks.append(clp.shape[0])
        self.lengths.append(cid.shape[1])
        means = torch.from_numpy(clp.reshape(len(clp), -1).mean(1).astype(np.float32)) + 1  # a black image: 1
        return means[:, None].expand(-1, 768).clone(), torch.from_numpy(cm.sum(1).astype(np.float32))[:, None].expand(-1, 512).clone()


def _images(tmp_path, n, Image):
    paths = []
    for i in range(n):
        p = str(tmp_path / f"img{i}.png")
        Image.new("RGB", (224, 224), (10 * (i + 1),) * 3).save(p)
        paths.append(p)
    return paths


def test_extract_features_dataset_rules(tmp_path):
    from PIL import Image
    paths = _images(tmp_path, 6, Image)
    paths[1] = str(tmp_path / "gone.png")  # missing: black
    open(paths[4], "wb").write(b"not an image")  # undecodable: black
    texts = [f"caption {i}" for i in range(6)]
    texts[2] = " ".join(["w"] * 90)  # 92 tokens: truncated at 77
    texts[5] = 12345  # str(text)
    f = _StubForensics(max_batch=4)
    img, txt = CT.extract_features(f, texts, paths)
    assert img.dtype == np.float32 and img.shape == (6, 768) and txt.dtype == np.float32 and txt.shape == (6, 512)
    assert img[:, 0].tolist() == [11, 1, 31, 41, 1, 61]
    assert txt[:, 0].tolist() == [4, 4, 77, 4, 4, 3]
    assert f.chunks == [4, 2] and f.lengths == [77, 4]
    with pytest.raises(ValueError):
        CT.extract_features(f, ["a", "b"], ["x"])
    f.clip_processor = None
    with pytest.raises(RuntimeError):
        CT.extract_features(f, ["a"], ["x"])
    a, b = CT.extract_features(_StubForensics(), [], [])
    assert a.shape == (0, 768) and b.shape == (0, 512)


def test_train_clip_detective_reads_the_csvs_and_trains(tmp_path, capsys):
    """train_clip_detective.py:276-424 from two CSVs: the matched rows train, every row validates."""
    import pandas as pd
    from PIL import Image
    paths = _images(tmp_path, 9, Image)
    tr_csv, va_csv = str(tmp_path / "clip_train.csv"), str(tmp_path / "clip_val.csv")
    pd.DataFrame({"text": [f"caption {'w ' * i}" for i in range(9)], "image_path": paths,
                  "label": [0, 0, 1, 0, 0, 1, 0, 0, 0]}).to_csv(tr_csv, index=False)
    pd.DataFrame({"text": [f"other {'v ' * i}" for i in range(5)], "image_path": paths[:4] + [str(tmp_path / "gone.png")],
                  "label": [0, 1, 0, 1, 1]}).to_csv(va_csv, index=False)
    f = _StubForensics(max_batch=4)
    ck = str(tmp_path / "out.pth")
    # (the stub's features are constant along a row, so the loss is fp noise; what is checked is the plumbing)
    hist = CT.train_clip_detective(tr_csv, va_csv, batch_size=4, epochs=2, lr=1e-4, forensics=f, checkpoint_path=ck,
                                   seed=2)
    assert len(hist) == 2 and f.chunks == [4, 3, 4, 1]  # 7 matched training rows, 5 validation rows
    out = capsys.readouterr().out
    assert "Filtered to 7 matched pairs (from 9 total)" in out and "Val samples: 5" in out
    assert torch.load(ck, weights_only=True)["epoch"] in (0, 1)
    assert len(f.engine.projections) == 1
    # a missing CSV: a message, nothing constructed (also through the command line)
    assert CT.train_clip_detective(str(tmp_path / "none.csv"), va_csv) is None
    CT.main(["--train-csv", tr_csv, "--val-csv", str(tmp_path / "none.csv"), "--epochs", "1"])
    assert capsys.readouterr().out.count("not found") == 2
