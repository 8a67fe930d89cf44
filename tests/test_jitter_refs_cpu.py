"""CPU checks of the ColorJitter pieces that need no GPU: the numpy restatement of the kernel's arithmetic
(tests/jitter_refs.py) against Pillow on all 2^24 RGB triples, the rounding of the contrast mean, the draws of
``jitter_params``, the epoch plan with views, and ``train_cifake(jitter_views=2)`` end to end on the stub engine of
tests/test_effcls_train_refs_cpu.py with a ``color_jitter`` that calls Pillow."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import mmf_amd.cifake_training as CT
import mmf_amd.hip as hip
from tests import jitter_refs as J
from tests import test_effcls_train_refs_cpu as E

FACTORS = (0.8, 1.0, 1.2) + tuple(float(x) for x in
                                  torch.empty(2).uniform_(0.8, 1.2, generator=torch.Generator().manual_seed(11)))


@pytest.fixture(scope="module")
def triples():
    x = J.all_triples()
    x.setflags(write=False)
    return x, Image.fromarray(x, "RGB")


def _same(got, pil_image):
    ref = np.asarray(pil_image)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"


def test_luma_and_hsv_both_ways_equal_pillow_on_every_triple(triples):
    x, im = triples
    _same(J.np_luma(x), im.convert("L"))
    _same(J.np_rgb_to_hsv(x), im.convert("HSV"))
    _same(J.np_hsv_to_rgb(x), Image.fromarray(x, "HSV").convert("RGB"))  # the same bytes read as (H, S, V)


@pytest.mark.parametrize("factor", FACTORS)
def test_brightness_and_saturation_equal_pillow_on_every_triple(triples, factor):
    x, im = triples
    _same(J.np_brightness(x, factor), J.pil_op(im, J.BRIGHTNESS, factor))
    _same(J.np_saturation(x, factor), J.pil_op(im, J.SATURATION, factor))


@pytest.mark.parametrize("factor", (0.8, 1.2))
def test_contrast_equals_pillow_on_every_triple(triples, factor):
    x, im = triples
    _same(J.np_contrast(x, factor), J.pil_op(im, J.CONTRAST, factor))


def test_hue_round_trip_equals_pillow_on_every_triple(triples):
    x, im = triples
    _same(J.np_hue(x, 239), J.pil_op(im, J.HUE, shift=239))
    assert not np.array_equal(J.np_hue(x[:64], 0), x[:64])  # the round trip is not the identity


def test_contrast_mean_rounds_half_up():
    """int(mean + 0.5) on two-pixel images: an L mean of exactly m + 0.5 gives m + 1, one step (half an L) below
    gives m.  A factor of 0.5 shows the mean in the result."""
    for pixels, mean in (((100, 101), 101), ((100, 100), 100), ((254, 255), 255), ((0, 1), 1), ((0, 0), 0)):
        x = np.array([[[v, v, v] for v in pixels]], np.uint8)
        assert J.np_contrast_mean(x) == mean
        _same(J.np_contrast(x, 0.5), J.pil_op(Image.fromarray(x, "RGB"), J.CONTRAST, 0.5))
        _same(J.np_chain(x[None], [[1, -1, -1, -1]], [[1, 0.5, 1]], [0])[0],
              Image.fromarray(J.pil_chain(x[None], [[1, -1, -1, -1]], [[1, 0.5, 1]], [0])[0]))


def test_chains_equal_pillow():
    """np_chain = pil_chain on every order of the four operations, the contrast mean taken of the image as it
    stands at that point of the chain."""
    rng = np.random.default_rng(5)
    orders = np.array(list(itertools.permutations(range(4))), np.int32)
    x = rng.integers(0, 256, (24, 16, 16, 3), dtype=np.uint8)
    fac = rng.uniform(0.8, 1.2, (24, 3)).astype(np.float32)
    shift = rng.integers(0, 256, 24).astype(np.int32)
    assert np.array_equal(J.np_chain(x, orders, fac, shift), J.pil_chain(x, orders, fac, shift))


# ---- jitter_params ----
def test_jitter_params_draws():
    N, views = 150, 3
    ops, fac, shift = CT.jitter_params(N, views, seed=4)
    again = CT.jitter_params(N, views, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip((ops, fac, shift), again))
    assert not np.array_equal(ops, CT.jitter_params(N, views, seed=5)[0])
    assert ops.shape == (views, N, 4) and ops.dtype == np.int32
    assert fac.shape == (views, N, 3) and fac.dtype == np.float32
    assert shift.shape == (views, N) and shift.dtype == np.int32
    assert (np.sort(ops, -1) == np.arange(4)).all()  # every chain a permutation of the four operations
    assert len({tuple(o) for o in ops.reshape(-1, 4).tolist()}) == 24  # all orders over 450 draws
    assert (fac >= np.float32(0.8)).all() and (fac <= np.float32(1.2)).all() and fac.std() > 0.05
    # |hue factor| <= 0.1: trunc(h * 255) in -25 .. 25, negative ones wrapped mod 256
    assert set(np.unique(shift)) <= set(range(0, 26)) | set(range(231, 256))
    assert (shift > 128).any() and (shift < 128).any()
    # a wider brightness range stops at 0
    wide = CT.jitter_params(N, 1, seed=4, brightness=1.5)[1][..., 0]
    assert wide.min() >= 0 and wide.max() <= 2.5 and wide.max() > 1.5


def test_jitter_params_zero_range_leaves_the_operation_out():
    full = CT.jitter_params(40, 2, seed=9)
    for k, name in enumerate(("brightness", "contrast", "saturation", "hue")):
        ops, fac, shift = CT.jitter_params(40, 2, seed=9, **{name: 0})
        assert not (ops == k).any() and np.array_equal(ops == -1, full[0] == k)
        assert np.array_equal(np.where(ops == -1, k, ops), full[0])  # the other draws are unchanged
        if k < 3:
            assert (fac[..., k] == 1).all()
            assert all(np.array_equal(fac[..., j], full[1][..., j]) for j in range(3) if j != k)
        assert np.array_equal(shift, full[2]) if k < 3 else not shift.any()


def test_hue_shift_rule_for_negative_factors():
    """adjust_hue: np.array(hue_factor * 255).astype(np.uint8) -- truncation toward zero, then mod 256; -0.07 gives
    239.  jitter_params applies the same rule to its float64 draws."""
    assert int(np.trunc(-0.07 * 255)) % 256 == 239
    g = torch.Generator().manual_seed(21)
    torch.rand(2, 30, 4, generator=g)
    for _ in range(3):
        torch.empty(2, 30, dtype=torch.float32).uniform_(0.8, 1.2, generator=g)
    h = torch.empty(2, 30, dtype=torch.float64).uniform_(-0.1, 0.1, generator=g).numpy()
    shift = CT.jitter_params(30, 2, seed=21)[2]
    want = np.array([[int(v * 255) % 256 for v in row] for row in h])  # int(): toward zero
    assert (h < 0).any() and np.array_equal(shift, want)
    assert np.array_equal(shift[h < 0], (256 - np.floor(-h[h < 0] * 255)) % 256)  # -0.0001 truncates to 0, not 255


# ---- the plan ----
@pytest.mark.parametrize("flip", [True, False])
def test_plan_with_views(flip):
    N, bs, epochs, K = 37, 8, 5, 3
    base = CT.plan(N, bs, epochs, seed=6, flip=flip)
    zero = CT.plan(N, bs, epochs, seed=6, flip=flip, views=0)
    g = torch.Generator().manual_seed(6)
    for (perm, keep, flipped), (p0, k0, f0) in zip(base, zero):
        assert np.array_equal(perm, p0) and np.array_equal(keep, k0) and np.array_equal(flipped, f0)
        order = torch.randperm(N, generator=g).numpy()  # views=0: today's draws in today's order
        fl = (torch.rand(N, generator=g) < 0.5).numpy() if flip else np.zeros(N, bool)
        torch.rand(N, CT.WIDTH, generator=g)
        assert np.array_equal(perm, order + N * fl[order]) and perm.dtype == np.int32
    for e, ((perm, keep, flipped), (p0, k0, f0)) in enumerate(zip(CT.plan(N, bs, epochs, 6, flip, views=K), base)):
        assert np.array_equal(keep, k0) and np.array_equal(flipped, f0) and perm.dtype == np.int32
        row = perm % N
        block = perm // N
        assert np.array_equal(row, p0 % N)  # no extra draw: the same order
        if flip:
            assert np.array_equal(block // 2, np.full(N, e % K)) and np.array_equal(block % 2, flipped[row])
        else:
            assert np.array_equal(block, np.full(N, e % K))


# ---- the header's constant ----
def test_binding_knows_the_workspace_size():
    text = open(os.path.join(os.path.dirname(E.__file__), "..", "include", "mmf_hip.h")).read()
    assert int(re.search(r"#define MMF_JITTER_CHUNKS (\d+)", text).group(1)) == hip.JITTER_CHUNKS
    assert "mmf_color_jitter_u8" in hip.SIGNATURES


# ---- train_cifake on the stub engine ----
class _JitterStubEngine(E._StubEngine):
    def __init__(self):
        super().__init__()
        self.jitter_calls, self.banks = [], []

    def effcls_train_epoch(self, feat, *args, **kwargs):
        self.banks.append(feat.clone())
        return super().effcls_train_epoch(feat, *args, **kwargs)

    def color_jitter(self, img, ops, factors, hue_shift):
        self.jitter_calls.append(int(img.shape[0]))
        return torch.from_numpy(J.pil_chain(img.numpy(), ops, factors, hue_shift))


def _stub_forensics():
    fs = E._stub_forensics()
    fs.engine = _JitterStubEngine()
    fs.detector.bind(fs.engine)
    return fs


def test_train_cifake_with_jitter_views_on_a_stub_engine(tmp_path, capsys):
    root = tmp_path / "cifake"
    E._cifake_tree(root, n_real=12, n_fake=(7, 6))
    fs = _stub_forensics()
    before = CT.flatten_classifier(fs.detector).clone()
    hist = CT.train_cifake(str(root), batch_size=4, lr=1e-3, epochs=3, forensics=fs, checkpoint_path=None,
                           jitter_views=2)
    assert "Loaded 19 training samples" in capsys.readouterr().out
    assert len(hist) == 3 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert sum(fs.engine.jitter_calls) == 2 * 19 and max(fs.engine.jitter_calls) <= fs.engine.max_batch
    assert sum(fs.engine.pooled_batches) == 2 * 2 * 19 + 5  # (2 views) x (plain, mirrored) of 19, one of the others
    assert fs.engine.train_calls == [(0, 4 * 19, 19), (5, 4 * 19, 19), (10, 4 * 19, 19)]  # the 4N-row bank
    assert not torch.equal(CT.flatten_classifier(fs.detector), before)

    # extract_image_features: the views' rows are the rows of the Pillow-jittered windows, in both flips
    tp, _, _, _ = CT.load_cifake_data(str(root))
    paths = tp[:5]
    jit = CT.jitter_params(len(paths), 2, seed=1)
    rows, mirrored, ok = CT.extract_image_features(fs, paths, flip=True, jitter=jit)
    assert rows.shape == mirrored.shape == (2, 5, 1280) and rows.dtype == np.float32 and ok.all()
    plain, plain_m, _ = CT.extract_image_features(fs, paths, flip=True)
    assert plain.shape == (5, 1280)
    win = np.stack([np.asarray(Image.open(p).convert("RGB").resize((224, 224), Image.BILINEAR)) for p in paths])
    for v in range(2):
        want = torch.from_numpy(J.pil_chain(win, jit[0][v], jit[1][v], jit[2][v]))
        assert np.array_equal(rows[v], E._StubEngine().effnet_pooled(want).numpy())
        assert np.array_equal(mirrored[v], E._StubEngine().effnet_pooled(torch.flip(want, dims=[2])).numpy())
    assert not np.array_equal(rows[0], plain) and not np.array_equal(rows[0], rows[1])
    with pytest.raises(ValueError):
        CT.extract_image_features(fs, paths, jitter=CT.jitter_params(4, 2, seed=1))  # draws for another N

    # fit: the bank's block order is the plan's
    K, N = 2, 5
    feats = np.arange(2 * K * N, dtype=np.float32)[:, None].repeat(1280, 1).reshape(K, 2, N, 1280)
    CT.ClassifierTrainer(fs, batch_size=4, epochs=1, jitter_views=K).fit(
        (feats[:, 0], feats[:, 1]), [0, 1, 0, 1, 1], plain, [0, 1, 0, 1, 1])
    assert fs.engine.banks[-1][:, 0].tolist() == list(range(2 * K * N))  # view 0 rows, view 0 mirrored, view 1 rows, ...
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, jitter_views=3).fit((feats[:, 0], feats[:, 1]), [0, 1, 0, 1, 1], plain, [0] * 5)
    with pytest.raises(ValueError):
        CT.ClassifierTrainer(fs, jitter_views=-1)
