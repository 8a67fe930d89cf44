"""tests/jpeg_encode_refs.py held to Pillow on the CPU: the numpy restatement of libjpeg's forward half gives the
quantised coefficients and the tables of the file Pillow writes, and, with oracle.jpeg_decode.reconstruct behind it,
the pixels Pillow loads back -- equal, no tolerance.  Also the draws and the argument checks of
mmf_amd/cifake_training.py's JPEG views that need no device."""
import numpy as np
import pytest

from oracle import jpeg_decode as JD
from tests import jpeg_encode_refs as R

SMALL = [s for s in R.SIZES if s != (224, 224)]


def _images(H, W):
    return dict(R.extremes(H, W), noise=R.noise(H, W, 100 * H + W))


def _check_coefs(img, q):
    want, tables, (info, full) = R.pil_coefs(img, q)
    got = R.np_coefs(img, q)
    for name, a, b in zip("Y Cb Cr".split(), got, want):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert int((a != b).sum()) == 0, f"{name}: {int((a != b).sum())} coefficients differ from Pillow's file"
    for a, b in zip(R.np_qtables(q), tables):
        assert np.array_equal(a, b)
    assert JD.in_exact_range(full, info) and R.np_in_exact_range(img, q)


def _check_pixels(img, q):
    want = R.pil_roundtrip(img, q)
    got = R.np_roundtrip(img, q)
    assert got.shape == want.shape and int((got != want).sum()) == 0, \
        f"{int((got != want).sum())} of {want.size} bytes differ from Pillow"


@pytest.mark.parametrize("q", R.QUALITIES)
@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(size, q):
    for name, img in _images(*size).items():
        _check_coefs(img, q)
        _check_pixels(img, q)


@pytest.mark.parametrize("q", R.QUALITIES)
def test_restatement_equals_pillow_224(q):
    """The trainer's window: the coefficients, the pixels and the range of all five images at every quality.  (The
    Python entropy decoder reads the noise image's file in about 2 s up to quality 80 and in about 20 s at 100: the
    case at 100 takes half a minute in all, the others seconds.)"""
    for name, img in _images(224, 224).items():
        _check_coefs(img, q)
        _check_pixels(img, q)


def test_gradient_and_edge_every_quality_band():
    img = R.gradient_with_edge(32, 32)
    for q in (1, 25, 49, 50, 51, 75, 99, 100):
        _check_coefs(img, q)
        _check_pixels(img, q)


def test_tables():
    for q in range(1, 101):
        for std in (R.STD_LUMA, R.STD_CHROMA):
            t = R.np_qtable(q, std)
            assert t.min() >= 1 and t.max() <= 255
    assert (R.np_qtable(100, R.STD_LUMA) == 1).all()
    assert np.array_equal(R.np_qtable(50, R.STD_CHROMA), R.STD_CHROMA)
    assert R.np_qtable(1, R.STD_LUMA).max() == 255  # force_baseline


def test_roundtrip_does_not_commute_with_the_mirror():
    """Why the trainer mirrors first and compresses after: the chroma biases alternate with the column's parity."""
    img = R.noise(32, 32, 3)
    a = R.pil_roundtrip(img[:, ::-1], 60)
    b = R.pil_roundtrip(img, 60)[:, ::-1]
    assert not np.array_equal(a, b)


def test_block_roundtrip_restatement_flags():
    """np_block_roundtrip's predicate is in_exact_range's three conditions; R.outside_blocks trips what blocks of
    samples up to +-1024 can trip (its docstring: the first condition is out of reach there, the second never fails
    alone)."""
    blocks, table, which = R.outside_blocks()
    coef, _, bad = R.np_block_roundtrip(blocks, table)
    fails = R.range_conditions(coef, table)
    assert [tuple(k + 1 for k in range(3) if fails[k][i]) for i in range(len(which))] == which
    assert bad.tolist() == [int(bool(w)) for w in which]
    worst = np.where(np.add.outer(np.arange(8), np.arange(8)).reshape(64) % 2, -1024, 1024)[None]
    rnd = np.random.default_rng(0).integers(-1024, 1025, (500, 64))
    for t in (1, 16, 255):
        tab = np.full(64, t, np.int64)
        for blk in (np.full((1, 64), 1024), np.full((1, 64), -1024), worst, rnd):
            cf = R.np_quantise(R.np_fdct(blk), tab)
            assert np.abs(cf * tab).max() <= 8192 + t // 2 + 1
            c1, c2, c3 = R.range_conditions(cf, tab)
            assert not c1.any() and not (c2 & ~c3).any()
    pix = R.np_sample_blocks(R.noise(16, 16, 1))[0].reshape(-1, 64)
    assert R.np_block_roundtrip(pix, R.np_qtable(40, R.STD_LUMA))[2].tolist() == [0] * 4


# ---- cifake_training: the draws and the checks that need no device ----
def test_jpeg_params():
    import mmf_amd.cifake_training as CT
    a = CT.jpeg_params(700, 5, seed=3)
    assert a.shape == (5, 700) and a.dtype == np.int32
    assert np.array_equal(a, CT.jpeg_params(700, 5, seed=3)) and not np.array_equal(a, CT.jpeg_params(700, 5, seed=4))
    assert a.min() == 40 and a.max() == 80  # the closed range, both ends reached over 3500 draws
    assert set(np.unique(a).tolist()) == set(range(40, 81))
    b = CT.jpeg_params(2000, 2, seed=0, quality_range=(1, 100))
    assert b.min() == 1 and b.max() == 100
    assert (CT.jpeg_params(9, 2, seed=0, quality_range=(57, 57)) == 57).all()
    assert CT.jpeg_params(0, 3, seed=0).shape == (3, 0)
    for bad in ((0, 80), (40, 101), (80, 40), (-1, 5), (40,), "ab", None):
        with pytest.raises(ValueError):
            CT.jpeg_params(4, 2, seed=0, quality_range=bad)


def test_jpeg_params_leaves_jitter_params_alone():
    import mmf_amd.cifake_training as CT
    before = CT.jitter_params(50, 3, seed=7)
    CT.jpeg_params(50, 3, seed=7)
    after = CT.jitter_params(50, 3, seed=7)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_extract_image_features_argument_checks():
    """Raised before the first use of the forensics object: None stands in for it."""
    import mmf_amd.cifake_training as CT
    paths = ["a.jpg", "b.jpg", "c.jpg"]
    jit = CT.jitter_params(3, 2, seed=0)
    for bad in (np.full((2, 4), 50), np.full((0, 3), 50), np.full(3, 50), np.full((2, 3), 50.0),
                np.full((2, 3), 0), np.full((2, 3), 101)):
        with pytest.raises(ValueError):
            CT.extract_image_features(None, paths, jpeg=bad)
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(None, paths, flip=True, jitter=jit, jpeg=np.full((3, 3), 50))


def test_train_cifake_argument_checks(tmp_path):
    """Raised before the tree is read: the root does not exist."""
    import mmf_amd.cifake_training as CT
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match="must be equal"):
        CT.train_cifake(root, jitter_views=2, jpeg_views=3)
    with pytest.raises(ValueError, match=">= 0"):
        CT.train_cifake(root, jpeg_views=-1)
    for bad in ((0, 80), (80, 40), (40, 101)):
        with pytest.raises(ValueError, match="quality_range"):
            CT.train_cifake(root, jpeg_views=2, jpeg_quality=bad)
    with pytest.raises(ValueError, match="Insufficient data"):  # the checks passed: the missing tree is next
        CT.train_cifake(root, jitter_views=2, jpeg_views=2)
    with pytest.raises(SystemExit):
        CT.main(["--root", root, "--jpeg-quality", "40"])
