"""mmf_gaussian_blur_u8 (csrc/blur.hip), Engine.gaussian_blur and the blurred views of mmf_amd/cifake_training.py on
the MI355X.

The kernel is held to tests/blur_refs.np_blur, the float32 numpy restatement of its arithmetic in its order, on
every byte and with no tolerance; Engine.gaussian_blur is held to the authority, torch's own pad / conv2d / round
(tests/blur_refs.tv_blur), under the tie rule stated there: equal wherever the float64 value is farther than 1e-3
from a half-integer, at most one apart elsewhere, and at most 0.5 % of the bytes that close to a tie.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import blur_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22
SENTINEL, GUARD = 0xA5, 4096
DRAW = float(torch.empty(1).uniform_(0.1, 5.0, generator=torch.Generator().manual_seed(11)))
SIGMAS = (0.1, 0.3, 0.7, 1.5, 5.0, DRAW)
# the kernel's tile (csrc/kernels.h kBlurTileRows, kBlurTileBytes): 32 rows of 256 row bytes (85 1/3 pixels)
TILE_ROWS, TILE_BYTES = 32, 256
SHAPES = [(2, 5, 3, 3),      # the smallest legal image: every tap reflects
          (3, 5, 7, 3),      # 105 bytes per image: images 1 and 2 do not start on a dword
          (2, 9, 224, 3),
          (2, 37, 53, 3),    # a multiple of no tile
          (1, TILE_ROWS + 1, TILE_BYTES // 3 + 1, 3),  # 33 x 86: one row and two bytes past a tile
          (4, 224, 224, 3)]  # the trainer's


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _weights(sigmas, size=(5, 9)):
    import mmf_amd.cifake_training as CT
    return CT.gaussian_kernel2d(np.asarray(sigmas, np.float32), size)


def blur(img, weights, apply, offset=0):
    """One mmf_gaussian_blur_u8 on a uint8 [B, H, W, 3] array -> the result on the host.  dst is filled with a
    sentinel and followed by a guard region that must come back untouched; ``offset`` moves the first byte of src
    and of dst off the dword."""
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    img = np.ascontiguousarray(img)
    B, H, W, _ = img.shape
    ky, kx = np.shape(weights)[1:]
    n = img.size
    s = torch.zeros(offset + n, dtype=torch.uint8, device=dev)
    s[offset:] = _t(img.reshape(-1), dev)
    d = torch.full((offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    w, a = _t(weights, dev, np.float32), _t(apply, dev, np.int32)
    assert w.shape == (B, ky, kx) and a.shape == (B,)
    rc = lib.mmf_gaussian_blur_u8(hip.ptr(s) + offset, hip.ptr(d) + offset, B, H, W, kx, ky, hip.ptr(w), hip.ptr(a),
                                  hip.stream_ptr())
    assert rc == 0, lib.mmf_last_error()
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert (out[:offset] == SENTINEL).all() and (out[offset + n:] == SENTINEL).all(), "a byte outside dst was written"
    assert np.array_equal(s[offset:].cpu().numpy(), img.reshape(-1)), "src was written"
    return out[offset:offset + n].reshape(img.shape)


def _same(got, want):
    diff = int((got != want).sum())
    assert diff == 0, f"{diff} of {want.size} bytes differ from np_blur, first at {np.argwhere(got != want)[:4].tolist()}"


def _case(shape, k):
    """Noise of the shape, per image a sigma (SIGMAS in turn, from the k + 1-th on) and a mixed apply."""
    B = shape[0]
    img = np.random.default_rng(100 + k).integers(0, 256, shape, dtype=np.uint8)
    sig = [SIGMAS[(k + 1 + b) % len(SIGMAS)] for b in range(B)]
    apply = np.array([1, 0, 1, 1][:B], np.int32) if B > 1 else np.ones(1, np.int32)
    return img, sig, apply


def test_the_tile_named_here_is_the_kernels():
    import mmf_amd.hip as hip
    text = open(os.path.join(hip.PKG_DIR, "csrc", "kernels.h")).read()
    assert int(re.search(r"kBlurTileRows = (\d+);", text).group(1)) == TILE_ROWS
    assert int(re.search(r"kBlurTileBytes = (\d+);", text).group(1)) == TILE_BYTES


# ---- (5, 9): byte equality with the restatement ----
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_shapes(k):
    img, sig, mixed = _case(SHAPES[k], k)
    w = _weights(sig)
    for apply in (mixed, 1 - mixed)[:2 if len(mixed) > 1 else 1]:  # every image blurred once and skipped once
        got = blur(img, w, apply)
        _same(got, R.np_blur(img, w, apply))
        for b in np.flatnonzero(apply == 0):
            assert np.array_equal(got[b], img[b])  # RandomApply did not fire: the image as it is
        for b in np.flatnonzero(apply):
            assert sig[b] == 0.1 or not np.array_equal(got[b], img[b])


def test_every_sigma_and_an_apply_that_is_not_one():
    """All six sigmas in one batch of 37 x 53 images; any non-zero apply blurs; all skipped is a copy."""
    img = np.random.default_rng(7).integers(0, 256, (6, 37, 53, 3), dtype=np.uint8)
    w = _weights(SIGMAS)
    apply = np.array([1, -1, 0, 7, 1 << 30, 0], np.int32)
    got = blur(img, w, apply)
    _same(got, R.np_blur(img, w, apply != 0))
    assert np.array_equal(got[0], img[0])  # sigma 0.1: a delta
    assert np.array_equal(blur(img, w, np.zeros(6, np.int32)), img)


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_src_and_dst_off_the_dword(offset):
    img, sig, apply = _case((3, 9, 13, 3), 3)  # 39 bytes per row, 351 per image: every alignment of a row occurs
    w = _weights(sig)
    _same(blur(img, w, apply, offset=offset), R.np_blur(img, w, apply))


def test_extreme_images_and_weights():
    """0 / 255 images (the sums reach 255 up to rounding and must not wrap), and weights no Gaussian gives: a sum
    above one clamps at 255, negative ones at 0."""
    img = np.stack([np.full((11, 9, 3), 255, np.uint8), np.zeros((11, 9, 3), np.uint8),
                    np.where(np.random.default_rng(9).random((11, 9, 3)) < 0.5, 0, 255).astype(np.uint8)])
    for sig in ((0.3, 1.5, 5.0), (5.0, 0.7, DRAW)):
        w = _weights(sig)
        got = blur(img, w, np.ones(3, np.int32))
        _same(got, R.np_blur(img, w))
        assert (got[0] == 255).all() and (got[1] == 0).all()
    w = np.stack([np.full((9, 5), 0.05, np.float32), np.full((9, 5), -0.01, np.float32), _weights([1.0])[0] * 1.5])
    noise = np.random.default_rng(10).integers(0, 256, (3, 11, 9, 3), dtype=np.uint8)
    got = blur(noise, w, np.ones(3, np.int32))
    _same(got, R.np_blur(noise, w))
    assert (got[1] == 0).all() and (got[0] == 255).any()


# ---- every other size: the instantiation with run-time tap counts ----
@pytest.mark.parametrize("size", [(1, 1), (3, 3), (9, 5), (15, 15), (1, 9), (5, 7)], ids=str)
def test_other_window_sizes(size):
    img = np.random.default_rng(sum(size)).integers(0, 256, (2, 17, 19, 3), dtype=np.uint8)
    w = _weights([1.2, 3.0], size)
    got = blur(img, w, np.ones(2, np.int32))
    _same(got, R.np_blur(img, w))
    assert size != (1, 1) or np.array_equal(got, img)  # one tap of weight 1: the identity


def test_other_window_sizes_past_one_tile():
    img, sig, apply = _case((3, TILE_ROWS + 9, TILE_BYTES // 3 + 4, 3), 2)
    for size in ((15, 15), (3, 11)):
        w = _weights(sig, size)
        _same(blur(img, w, apply), R.np_blur(img, w, apply))
    small = np.random.default_rng(3).integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)  # 15 taps reflect on both sides
    w = _weights([0.9, 4.0], (15, 15))
    _same(blur(small, w, np.ones(2, np.int32)), R.np_blur(small, w))


# ---- bad arguments ----
def test_einval_launches_nothing():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    B, H, W = 2, 6, 4
    src = np.random.default_rng(6).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    s, d = _t(src, dev), torch.full((B, H, W, 3), 9, dtype=torch.uint8, device=dev)
    w, a = _t(_weights([1.0, 2.0]), dev), _t(np.ones(B, np.int32), dev)
    w3 = _t(_weights([1.0, 2.0], (3, 3)), dev)

    def call(src_=s, dst_=d, B_=B, H_=H, W_=W, KX=5, KY=9, w_=None, a_=None):
        wp = hip.ptr(w) if w_ is None else w_
        return lib.mmf_gaussian_blur_u8(hip.ptr(src_), hip.ptr(dst_), B_, H_, W_, KX, KY, wp,
                                        hip.ptr(a) if a_ is None else a_, hip.stream_ptr())
    bad = [dict(KX=4), dict(KX=0), dict(KY=17), dict(KY=-1), dict(KX=17, KY=3),
           dict(W_=2),                # W <= KX / 2: torch's reflection pad raises there too
           dict(H_=4),                # H <= KY / 2
           dict(dst_=s),              # dst == src
           dict(B_=0), dict(B_=-1), dict(B_=65536), dict(H_=0), dict(W_=0),
           dict(H_=1 << 16, W_=(1 << 14) + 1),  # H * W past 2^30: rejected on the shape alone
           dict(w_=hip.ptr(w) + 2), dict(a_=hip.ptr(a) + 1), dict(w_=0), dict(a_=0)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b"gaussian_blur_u8" in lib.mmf_last_error() or b"null" in lib.mmf_last_error()
    assert lib.mmf_gaussian_blur_u8(None, hip.ptr(d), B, H, W, 5, 9, hip.ptr(w), hip.ptr(a), hip.stream_ptr()) == EINVAL
    assert lib.mmf_gaussian_blur_u8(hip.ptr(s), None, B, H, W, 5, 9, hip.ptr(w), hip.ptr(a), hip.stream_ptr()) == EINVAL
    # dst overlapping src anywhere, not only dst == src: by one byte at either end, or almost wholly
    n = src.size
    buf = torch.full((3 * n,), 9, dtype=torch.uint8, device=dev)
    mid = buf[n:2 * n]
    for k in (1, n - 1, -1, -(n - 1)):
        assert call(src_=mid, dst_=buf[n + k:2 * n + k]) == EINVAL, k
        assert b"overlap" in lib.mmf_last_error()
    torch.cuda.synchronize()
    assert (d == 9).all() and (buf == 9).all() and np.array_equal(s.cpu().numpy(), src)
    assert call(src_=mid, dst_=buf[2 * n:]) == 0 and call(src_=mid, dst_=buf[:n]) == 0  # adjacent is not overlapping
    # the same W and H are legal for a window that fits them
    assert call(W_=2, H_=2, KX=3, KY=3, w_=hip.ptr(w3)) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), R.np_blur(src, _weights([1.0, 2.0])))


# ---- Engine.gaussian_blur against the authority ----
@pytest.fixture(scope="module")
def forensics(det_sd, clip_sd):
    _dev()
    from tests.test_gpu_effcls_train import _forensics
    f = _forensics(det_sd, clip_sd)
    yield f
    f.engine.close()


def test_engine_gaussian_blur_against_torch(forensics):
    eng = forensics.engine
    x = np.random.default_rng(12).integers(0, 256, (4, 224, 224, 3), dtype=np.uint8)
    sig = np.float32([0.3, 1.5, 5.0, DRAW])
    got = eng.gaussian_blur(x, sig)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == x.shape
    got = got.cpu().numpy()
    _same(got, R.np_blur(x, _weights(sig)))
    near = differ = 0
    for b in range(4):
        n, d = R.check_against_authority(got[b], x[b], float(sig[b]))
        print(f"sigma {float(sig[b]):.4f}: {n} of {x[b].size} bytes within {R.DELTA} of a tie, {d} differ from torch")
        near, differ = near + n, differ + d
    assert near <= R.TIE_SHARE * x.size and differ <= near
    # sigma 0.1 is exactly the input; one float serves the batch; apply=False copies
    assert np.array_equal(eng.gaussian_blur(x, 0.1).cpu().numpy(), x)
    one = eng.gaussian_blur(torch.from_numpy(x).to(eng.device), 2.0, apply=np.array([True, False, True, False]))
    one = one.cpu().numpy()
    assert np.array_equal(one[[1, 3]], x[[1, 3]])
    for b in (0, 2):
        R.check_against_authority(one[b], x[b], 2.0)
    # another window size, against the authority too
    small = eng.gaussian_blur(x[:1, :40, :50], 1.1, kernel_size=(3, 7)).cpu().numpy()
    R.check_against_authority(small[0], x[0, :40, :50], 1.1, (3, 7))


def test_engine_gaussian_blur_argument_checks(forensics):
    eng = forensics.engine
    x = np.zeros((2, 8, 8, 3), np.uint8)
    for args, kw in (((np.zeros((2, 8, 8, 4), np.uint8), 1.0), {}), ((x.astype(np.float32), 1.0), {}),
                     ((x, 0.0), {}), ((x, -1.0), {}), ((x, [1.0, float("nan")]), {}), ((x, [1.0, 2.0, 3.0]), {}),
                     ((x, np.ones((2, 1))), {}), ((x, 1.0), dict(apply=[True])), ((x, 1.0), dict(apply=[1, 0])),
                     ((x, 1.0), dict(kernel_size=(4, 9))), ((x, 1.0), dict(kernel_size=(5, 17))),
                     ((x, 1.0), dict(kernel_size=5)), ((x[:, :4], 1.0), {}), ((x[:, :, :2], 1.0), {})):
        with pytest.raises(ValueError, match="gaussian_blur"):
            eng.gaussian_blur(*args, **kw)


# ---- end to end: the blurred views of the trainer ----
K = 2


@pytest.fixture(scope="module")
def cifake(forensics, tmp_path_factory):
    """A handful of 32 x 32 JPEG files and the three steps' draws; every image blurred in view 0."""
    import mmf_amd.cifake_training as CT
    from PIL import Image
    root = tmp_path_factory.mktemp("blurviews")
    g = np.random.default_rng(22)
    paths = []
    for i in range(5):
        paths.append(str(root / f"img{i}.jpg"))
        Image.fromarray(g.integers(30, 220, (32, 32, 3), dtype=np.uint8)).save(paths[-1], quality=92)
    apply, sigma = CT.blur_params(len(paths), K, seed=4)
    apply[0] = True
    assert not apply[1].all()
    return paths, CT.jitter_params(len(paths), K, seed=4), (apply, sigma), CT.jpeg_params(len(paths), K, seed=4)


def test_views_are_the_rows_of_the_chain_composed_by_hand(forensics, cifake):
    import mmf_amd.cifake_training as CT
    f, eng = forensics, forensics.engine
    paths, jit, (apply, sigma), qual = cifake
    N = len(paths)
    plain = CT.extract_image_features(f, paths, flip=True)
    rows, mirrored, ok = CT.extract_image_features(f, paths, flip=True, jitter=jit, blur=(apply, sigma), jpeg=qual)
    assert ok.all() and rows.shape == mirrored.shape == (K, N, 1280) and rows.dtype == np.float32
    assert np.isfinite(rows).all()
    again = CT.extract_image_features(f, paths, flip=True)  # blur=None returns what it returned before
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    no_blur = CT.extract_image_features(f, paths, flip=True, jitter=jit, jpeg=qual)
    assert not np.array_equal(rows[0], no_blur[0][0])
    win = f._windows(*f._stage_images(paths))[0]
    for v in range(K):
        jittered = eng.color_jitter(win, jit[0][v], jit[1][v], jit[2][v])
        straight = eng.jpeg_compress(eng.gaussian_blur(jittered, sigma[v], apply[v]), qual[v])
        flipped = eng.jpeg_compress(eng.gaussian_blur(eng.hflip(jittered), sigma[v], apply[v]), qual[v])
        assert torch.equal(torch.from_numpy(rows[v]), eng.effnet_pooled(straight).cpu())
        assert torch.equal(torch.from_numpy(mirrored[v]), eng.effnet_pooled(flipped).cpu())
        # the blur in the chain is the kernel's: the restatement on the downloaded window gives the same bytes
        host = jittered.cpu().numpy()
        _same(eng.gaussian_blur(jittered, sigma[v], apply[v]).cpu().numpy(),
              R.np_blur(host, _weights(sigma[v]), apply[v]))
    # blur alone, and a K that disagrees
    only, ok1 = CT.extract_image_features(f, paths, blur=(apply, sigma))
    assert ok1.all() and only.shape == (K, N, 1280)
    want = eng.effnet_pooled(eng.gaussian_blur(win, sigma[1], apply[1])).cpu()
    assert torch.equal(torch.from_numpy(only[1]), want)
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(f, paths, jitter=jit, blur=(apply[:1], sigma[:1]), jpeg=qual)
