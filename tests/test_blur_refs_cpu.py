"""CPU checks of the GaussianBlur pieces that need no GPU: ``gaussian_kernel2d`` against the independent restatement
of torchvision's weights (tests/blur_refs.py), the numpy restatement of the kernel's arithmetic against torch's
conv2d under the tie rule, the draws of ``blur_params``, the argument checks, and
``train_cifake(jitter_views=K, blur_views=K, jpeg_views=K)`` on a stub engine that records the order of its calls.

One statement of the issue did not hold and is tested as it is: at sigma 0.35 the outer weights of the 5 x 9
window are tiny (3.3e-36 in the corner) but still NORMAL float32 numbers; they are zero at 0.25 and zero or
subnormal at 0.3.
"""
import numpy as np
import pytest
import torch

import mmf_amd.cifake_training as CT
import mmf_amd.hip as hip
from tests import blur_refs as R
from tests import test_effcls_train_refs_cpu as E

SIGMAS = (0.1, 0.25, 0.3, 0.35, 1.0, 5.0)
TINY = float(np.finfo(np.float32).tiny)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the weights ----
@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_kernel2d_is_torchvisions_bit_for_bit(sigma):
    w = CT.gaussian_kernel2d(sigma)
    assert w.shape == (9, 5) and w.dtype == np.float32  # kernel_size = (5, 9): 5 wide, 9 high
    assert np.array_equal(_bits(w), _bits(R.tv_kernel2d(sigma).numpy()))
    assert abs(float(w.astype(np.float64).sum()) - 1) < 1e-6 and (w >= 0).all()
    assert np.array_equal(w, w[::-1, ::-1]) and w.argmax() == 4 * 5 + 2


def test_gaussian_kernel2d_other_sizes_and_errors():
    for size in ((1, 1), (3, 3), (9, 5), (15, 15), (5, 1)):
        w = CT.gaussian_kernel2d(0.8, size)
        assert w.shape == (size[1], size[0])
        assert np.array_equal(_bits(w), _bits(R.tv_kernel2d(0.8, size).numpy()))
    assert CT.gaussian_kernel2d(2.0, (1, 1)).tolist() == [[1.0]]
    for bad in (0, -1.0, float("nan"), float("inf"), [1.0, 0.0]):
        with pytest.raises(ValueError):
            CT.gaussian_kernel2d(bad)
    for bad in ((4, 9), (5, 17), (0, 3), (5,), 5, "ab"):
        with pytest.raises(ValueError):
            CT.gaussian_kernel2d(1.0, bad)


def test_an_array_of_sigmas_gives_the_bits_of_the_single_calls():
    s32 = np.float32(SIGMAS + (float(torch.empty(1).uniform_(0.1, 5.0, generator=torch.Generator().manual_seed(2))),))
    for arr in (s32, s32.astype(np.float64), s32.reshape(7, 1), list(map(float, s32))):
        w = CT.gaussian_kernel2d(arr)
        assert w.shape == np.shape(arr) + (9, 5) and w.dtype == np.float32
        flat = w.reshape(-1, 9, 5)
        for n, s in enumerate(s32):
            # float(s): the float32 draw as a Python float, what GaussianBlur.get_params' .item() hands on
            assert np.array_equal(_bits(flat[n]), _bits(CT.gaussian_kernel2d(float(s))))
            assert np.array_equal(_bits(flat[n]), _bits(R.tv_kernel2d(float(s)).numpy()))


def test_outer_weights_underflow_at_small_sigmas():
    """0.25: the outer rows are zero.  0.3: zero or subnormal, some of each.  0.35: normal numbers below 1e-27 (the
    issue expected subnormals here too).  0.1: a delta for every byte -- the centre exactly 1, its neighbours
    exp(-50) = 1.9e-22, twenty orders below a byte's rounding."""
    w = {s: CT.gaussian_kernel2d(s) for s in SIGMAS}
    outer = {s: np.concatenate([w[s][0], w[s][-1]]) for s in SIGMAS}
    assert (outer[0.25] == 0).all()
    assert (outer[0.3] < TINY).all() and (outer[0.3] == 0).any() and (outer[0.3] > 0).any()
    assert (outer[0.35] >= TINY).all() and (outer[0.35] < 1e-27).all()
    rest = w[0.1].copy()
    rest[4, 2] = 0
    assert w[0.1][4, 2] == 1 and rest.max() < 1e-21


# ---- the kernel's arithmetic against torch's ----
def _noise(seed, shape=(224, 224, 3)):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _ramp(h=96, w=128):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([np.rint(x * 255.0 / (w - 1)), np.rint(y * 255.0 / (h - 1)), (x + y) % 256], -1).astype(np.uint8)


def _two_level(seed, shape=(96, 128, 3)):
    return np.where(np.random.default_rng(seed).random(shape) < 0.5, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def against_torch():
    """Per case (name, sigma, bytes, bytes within DELTA of a tie, bytes that differ from torch): np_blur held to
    tv_blur under the tie rule, once for the whole module."""
    cases = [(f"noise sigma {s}", _noise(k), s) for k, s in enumerate(SIGMAS)]
    cases += [(f"two-level sigma {s}", _two_level(20 + k), s) for k, s in enumerate((0.3, 1.0, 5.0))]
    cases += [(f"ramp sigma {s}", _ramp(), s) for s in (0.35, 1.0, 5.0)]
    out = []
    for name, img, s in cases:
        got = R.np_blur(img[None], CT.gaussian_kernel2d(s)[None])[0]
        near, diff = R.check_against_authority(got, img, s)
        out.append((name, s, img.size, near, diff))
        if s == 0.1:
            assert np.array_equal(got, img) and np.array_equal(R.tv_blur(img, s), img)  # a delta: the input
    return out


def test_np_blur_equals_torch_away_from_ties(against_torch):
    for name, s, size, near, diff in against_torch:
        print(f"{name}: {near} of {size} bytes within {R.DELTA} of a tie ({100 * near / size:.3f} %), {diff} differ")
        assert diff <= near
    total = sum(c[2] for c in against_torch)
    share = sum(c[3] for c in against_torch) / total
    print(f"pooled: {100 * share:.3f} % of {total} bytes near a tie")
    assert share <= R.TIE_SHARE
    assert all(near == 0 and diff == 0 for _, s, _, near, diff in against_torch if s == 0.1)


@pytest.mark.parametrize("sigma", (0.25, 0.3, 0.35))
def test_zero_and_subnormal_weights_leave_torchs_bytes(sigma):
    img = _noise(40, (33, 41, 3))
    img[:9, :9] = 0     # a black corner: sums of subnormal products alone elsewhere in the window
    img[-5:, -7:] = 255
    got = R.np_blur(img[None], CT.gaussian_kernel2d(sigma)[None])[0]
    near, diff = R.check_against_authority(got, img, sigma)
    assert diff <= near <= 0.01 * img.size


def test_np_blur_shapes_apply_and_sizes():
    img = _noise(41, (3, 5, 7, 3))
    w = CT.gaussian_kernel2d(np.float32([0.7, 1.5, 5.0]))
    whole = R.np_blur(img, w)
    mixed = R.np_blur(img, w, apply=[True, False, True])
    assert np.array_equal(mixed[1], img[1]) and np.array_equal(mixed[[0, 2]], whole[[0, 2]])
    assert not np.array_equal(whole[1], img[1])
    small = _noise(42, (1, 5, 3, 3))  # the smallest legal image: every tap reflects
    R.check_against_authority(R.np_blur(small, CT.gaussian_kernel2d(1.5)[None])[0], small[0], 1.5)
    for size in ((1, 1), (3, 3), (9, 5), (15, 15)):
        x = _noise(43, (17, 19, 3))
        got = R.np_blur(x[None], CT.gaussian_kernel2d(1.2, size)[None])[0]
        R.check_against_authority(got, x, 1.2, size)
        assert size != (1, 1) or np.array_equal(got, x)
    # the float32 sum stays within 46 * 2^-24 * 255 of the real value, so the byte within that of its rounding
    real = np.stack([R.f64_blur(img[b], w[b]) for b in range(3)])
    assert np.abs(real - whole).max() <= 0.5 + 46 * 2.0 ** -24 * 255


# ---- blur_params ----
def test_blur_params_draws():
    N, views = 400, 3
    apply, sigma = CT.blur_params(N, views, seed=4)
    again = CT.blur_params(N, views, seed=4)
    assert np.array_equal(apply, again[0]) and np.array_equal(sigma, again[1])
    assert not np.array_equal(sigma, CT.blur_params(N, views, seed=5)[1])
    assert apply.shape == sigma.shape == (views, N) and apply.dtype == np.bool_ and sigma.dtype == np.float32
    assert 0.2 < apply.mean() < 0.4  # p = 0.3 over 1200 draws
    assert sigma.min() >= np.float32(0.1) and sigma.max() <= np.float32(5.0) and sigma.min() < 0.3 and sigma.max() > 4.8
    # the generator's draws, in order: rand <= p, then uniform_ in float32
    g = torch.Generator().manual_seed(4)
    assert np.array_equal(apply, (torch.rand(views, N, generator=g) <= 0.3).numpy())
    assert np.array_equal(sigma, torch.empty(views, N).uniform_(0.1, 5.0, generator=g).numpy())
    # p moves no sigma; its ends give none and all
    none, s0 = CT.blur_params(N, views, seed=4, p=0)
    every, s1 = CT.blur_params(N, views, seed=4, p=1)
    assert not none.any() and every.all() and np.array_equal(s0, sigma) and np.array_equal(s1, sigma)
    narrow = CT.blur_params(N, 1, seed=4, sigma=(1.5, 2.0))[1]
    assert narrow.min() >= 1.5 and narrow.max() <= 2.0 and narrow.std() > 0.05
    assert (CT.blur_params(9, 2, seed=0, sigma=(0.7, 0.7))[1] == np.float32(0.7)).all()
    assert CT.blur_params(0, 3, seed=0)[0].shape == (3, 0)


def test_blur_params_errors():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="p must be"):
            CT.blur_params(4, 2, seed=0, p=bad)
    for bad in ((0.0, 5.0), (-1.0, 2.0), (5.0, 0.1), (0.1, float("inf")), (0.1,), "ab", None, 1.0):
        with pytest.raises(ValueError, match="sigma must"):
            CT.blur_params(4, 2, seed=0, sigma=bad)


def test_blur_params_leaves_the_other_draws_alone():
    """Literals taken from jitter_params / jpeg_params before blur_params existed."""
    CT.blur_params(3, 2, seed=7)
    ops, fac, hue = CT.jitter_params(3, 2, seed=7)
    assert ops.tolist() == [[[1, 0, 3, 2], [2, 0, 1, 3], [0, 3, 1, 2]], [[1, 0, 3, 2], [1, 3, 0, 2], [1, 3, 2, 0]]]
    assert hue.tolist() == [[18, 8, 247], [20, 11, 22]]
    want = [[["0x1.0224acp+0", "0x1.2472d6p+0", "0x1.e936e0p-1"], ["0x1.098c00p+0", "0x1.119f18p+0", "0x1.c6f3c6p-1"],
             ["0x1.26e1b8p+0", "0x1.0cf812p+0", "0x1.e63c92p-1"]],
            [["0x1.0d2ae4p+0", "0x1.0712b4p+0", "0x1.c196c0p-1"], ["0x1.1b29fep+0", "0x1.18f550p+0", "0x1.18a132p+0"],
             ["0x1.b0c99ep-1", "0x1.2f0618p+0", "0x1.cd63ccp-1"]]]
    assert fac.dtype == np.float32 and fac.tolist() == [[[float.fromhex(x) for x in r] for r in v] for v in want]
    assert CT.jpeg_params(6, 2, seed=7).tolist() == [[78, 80, 54, 55, 74, 75], [76, 66, 43, 72, 62, 42]]


# ---- the checks that need no device ----
def test_extract_image_features_argument_checks():
    """Raised before the first use of the forensics object: None stands in for it."""
    paths = ["a.jpg", "b.jpg", "c.jpg"]
    good = CT.blur_params(3, 2, seed=0)
    for bad in ((good[0],), (good[0][:, :2], good[1][:, :2]), (good[0], good[1][:1]), (good[0].astype(int), good[1]),
                (good[0], np.zeros((2, 3), np.float32)), (good[0][0], good[1][0]), (good[0][:0], good[1][:0]),
                (good[0], good[1].astype(np.int32)), 5):
        with pytest.raises(ValueError, match="blur"):
            CT.extract_image_features(None, paths, blur=bad)
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(None, paths, jitter=CT.jitter_params(3, 3, seed=0), blur=good)
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(None, paths, blur=good, jpeg=np.full((3, 3), 50))
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(None, paths, jitter=CT.jitter_params(3, 2, seed=0), blur=good, jpeg=np.full((1, 3), 50))


def test_train_cifake_argument_checks(tmp_path):
    """Raised before the tree is read: the root does not exist."""
    root = str(tmp_path / "nowhere")
    for kw in (dict(jitter_views=2, blur_views=3), dict(blur_views=2, jpeg_views=3),
               dict(jitter_views=2, blur_views=2, jpeg_views=1)):
        with pytest.raises(ValueError, match="must be equal"):
            CT.train_cifake(root, **kw)
    with pytest.raises(ValueError, match=">= 0"):
        CT.train_cifake(root, blur_views=-1)
    with pytest.raises(ValueError, match="p must be"):
        CT.train_cifake(root, blur_views=2, blur_p=1.2)
    with pytest.raises(ValueError, match="sigma must"):
        CT.train_cifake(root, blur_views=2, blur_sigma=(0.0, 1.0))
    with pytest.raises(ValueError, match="Insufficient data"):  # the checks passed: the missing tree is next
        CT.train_cifake(root, jitter_views=2, blur_views=2, jpeg_views=2)
    with pytest.raises(ValueError, match="Insufficient data"):  # blur_p / blur_sigma are not looked at without views
        CT.train_cifake(root, blur_p=7)
    with pytest.raises(SystemExit):
        CT.main(["--root", root, "--blur-sigma", "0.1"])
    with pytest.raises(ValueError, match="Insufficient data"):
        CT.main(["--root", root, "--blur-views", "2", "--blur-p", "0.5", "--blur-sigma", "0.2", "3"])


def test_binding_knows_the_symbol():
    assert "mmf_gaussian_blur_u8" in hip.SIGNATURES
    assert len(hip.SIGNATURES["mmf_gaussian_blur_u8"][1]) == 10


# ---- train_cifake on a stub engine that records what each pooled window went through ----
class _ChainStubEngine(E._StubEngine):
    """Every augmentation is a cheap stand-in that changes the bytes; ``chains`` holds, per effnet_pooled call of a
    view, the names of the calls its window passed through, in order."""

    def __init__(self):
        super().__init__()
        self.history, self.keep, self.chains, self.blur_args = {}, [], [], []

    def _step(self, name, src, out):
        self.keep.append(out)  # alive, so no id is used twice
        self.history[id(out)] = self.history.get(id(src), ()) + (name,)
        return out

    def color_jitter(self, img, ops, factors, hue_shift):
        return self._step("jitter", img, img + 1)

    def hflip(self, img):
        return self._step("hflip", img, super().hflip(img))

    def gaussian_blur(self, img, sigma, apply=None, kernel_size=(5, 9)):
        self.blur_args.append((np.asarray(sigma).copy(), np.asarray(apply).copy(), tuple(kernel_size)))
        on = torch.from_numpy(np.asarray(apply))[:, None, None, None]
        return self._step("blur", img, torch.where(on, img // 2, img))

    def jpeg_compress(self, img, quality):
        return self._step("jpeg", img, img ^ 3)

    def effnet_pooled(self, img):
        if id(img) in self.history:
            self.chains.append(self.history[id(img)])
        return super().effnet_pooled(img)


def test_train_cifake_runs_jitter_blur_jpeg_in_the_composes_order(tmp_path, capsys):
    root = tmp_path / "cifake"
    E._cifake_tree(root, n_real=12, n_fake=(7, 6))
    fs = E._stub_forensics()
    fs.engine = _ChainStubEngine()
    fs.detector.bind(fs.engine)
    K = 2
    hist = CT.train_cifake(str(root), batch_size=4, lr=1e-3, epochs=2, forensics=fs, checkpoint_path=None, seed=3,
                           jitter_views=K, blur_views=K, jpeg_views=K, flip=True)
    assert "Loaded 19 training samples" in capsys.readouterr().out
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) for h in hist)
    eng = fs.engine
    straight, mirrored = ("jitter", "blur", "jpeg"), ("jitter", "hflip", "blur", "jpeg")
    chunks = -(-19 // eng.max_batch)
    assert eng.chains == [straight, mirrored] * (K * chunks)  # per chunk and view: the straight window, then its mirror
    assert eng.train_calls == [(0, 2 * K * 19, 19), (5, 2 * K * 19, 19)]  # the 2K N-row bank
    # the draws handed to the blur are blur_params' of the same seed, chunk by chunk, the same for both flips
    apply, sigma = CT.blur_params(19, K, seed=3)
    calls = iter(eng.blur_args)
    for a in range(0, 19, eng.max_batch):
        b = min(a + eng.max_batch, 19)
        for v in range(K):
            for _ in range(2):
                s, on, size = next(calls)
                assert np.array_equal(s, sigma[v, a:b]) and np.array_equal(on, apply[v, a:b]) and size == (5, 9)
    assert next(calls, None) is None

    # blur alone, no flip: one chain per view and chunk
    eng.chains.clear()
    tp = CT.load_cifake_data(str(root))[0][:5]
    rows, ok = CT.extract_image_features(fs, tp, blur=CT.blur_params(5, 3, seed=1, p=1.0))
    assert rows.shape == (3, 5, 1280) and ok.all() and eng.chains == [("blur",)] * (3 * 2)
    with pytest.raises(ValueError, match="must be equal"):
        CT.train_cifake(str(root), forensics=fs, checkpoint_path=None, jitter_views=2, blur_views=3, jpeg_views=2)
