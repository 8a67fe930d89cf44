"""mmf_jpeg_roundtrip_u8 (csrc/jpeg_encode.hip), Engine.jpeg_compress and the JPEG views of
mmf_amd/cifake_training.py on the MI355X.

The reference is Pillow itself (tests/jpeg_encode_refs.pil_roundtrip: save as a JPEG at quality q, load back);
every comparison is a count of differing bytes, required to be 0, and the flags are all 0 unless said otherwise.
"""
import numpy as np
import pytest
import torch

from tests import jpeg_encode_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _ws(lib, B, H, W, dev):
    n = int(lib.mmf_jpeg_roundtrip_ws_bytes(H, W))
    assert n > 0 and n % 64 == 0
    return torch.full(((B * n) // 8,), -1, dtype=torch.int64, device=dev)  # contents on entry do not matter


def roundtrip(img, quality, fill=7):
    """One mmf_jpeg_roundtrip_u8 on a uint8 [B, H, W, 3] array -> (the result, the flags) on the host."""
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    s = _t(img, dev)
    B, H, W, _ = s.shape
    d = torch.full_like(s, fill)
    q = _t(np.broadcast_to(np.asarray(quality, np.int32), (B,)).copy(), dev)
    ws, flags = _ws(lib, B, H, W, dev), torch.full((B,), 5, dtype=torch.int32, device=dev)
    rc = lib.mmf_jpeg_roundtrip_u8(hip.ptr(s), hip.ptr(d), B, H, W, hip.ptr(q), hip.ptr(ws), hip.ptr(flags),
                                   hip.stream_ptr())
    assert rc == 0, lib.mmf_last_error()
    torch.cuda.synchronize()
    return d.cpu().numpy(), flags.cpu().numpy()


def _check(img, quality):
    img = np.asarray(img)
    quality = np.broadcast_to(np.asarray(quality, np.int32), (img.shape[0],))
    got, flags = roundtrip(img, quality)
    want = R.pil_roundtrip_batch(img, quality)
    per_image = (got != want).reshape(len(img), -1).sum(1)
    print(f"{img.shape} q {quality.min()}..{quality.max()}: {int(per_image.sum())} of {want.size} bytes differ, "
          f"flags {flags.sum()}")
    assert int(per_image.sum()) == 0, f"bytes differing from Pillow per image: {per_image.tolist()}"
    assert (flags == 0).all(), flags.tolist()
    return got


# ---- against Pillow ----
@pytest.mark.parametrize("kind", ("noise", "gradient"))
def test_every_quality(kind):
    one = R.noise(32, 32, 1) if kind == "noise" else R.gradient_with_edge(32, 32)
    _check(np.repeat(one[None], 100, 0), np.arange(1, 101))


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 7, 9), (2, 15, 16), (2, 16, 15), (2, 17, 33), (1, 1, 1025),
                                   (4, 224, 224), (2, 24, 40), (2, 20, 12), (1, 2, 2), (1, 40, 24)], ids=str)
def test_shapes(shape):
    """Edge replication in both directions, odd chroma extents, one row or one column of blocks, rows that do not
    start dword-aligned, several workgroups per image (224 x 224: 1176 blocks, 50176 pixels); even heights that are
    no multiple of 16, where the chroma rows below the image repeat the last downsampled row."""
    B, H, W = shape
    x = np.random.default_rng(sum(shape)).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    for q in (40, 80):
        _check(x, q)


def test_extremes():
    imgs = np.stack(list(R.extremes(24, 40).values()) + [R.noise(24, 40, 8)])
    for q in (1, 40, 100):
        _check(imgs, q)


def test_mixed_qualities_and_the_copy():
    x = np.random.default_rng(2).integers(0, 256, (6, 19, 21, 3), dtype=np.uint8)
    q = np.array([75, 0, 1, 100, 0, 42], np.int32)
    got = _check(x, q)
    assert np.array_equal(got[1], x[1]) and np.array_equal(got[4], x[4])
    assert not np.array_equal(got[0], x[0])
    # a value outside 0..100 in the device array is a copy too, and reaches no memory it should not
    got, flags = roundtrip(x, np.array([101, -1, 1 << 30, -(1 << 31), 255, 50], np.int64).astype(np.int32))
    assert np.array_equal(got[:5], x[:5]) and np.array_equal(got[5], R.pil_roundtrip(x[5], 50)) and not flags.any()


def test_batch_invariance():
    x = np.random.default_rng(3).integers(0, 256, (5, 33, 18, 3), dtype=np.uint8)
    q = np.array([40, 55, 0, 80, 93], np.int32)
    whole, _ = roundtrip(x, q)
    assert np.array_equal(whole, roundtrip(x, q, fill=200)[0])  # the same call twice
    for b in range(5):
        assert np.array_equal(whole[b:b + 1], roundtrip(x[b:b + 1], q[b:b + 1])[0])


def test_not_the_mirror_of_the_mirrored():
    """The round trip does not commute with the flip (the chroma biases alternate with the column's parity): the
    kernel follows Pillow on both sides of that inequality."""
    x = R.noise(32, 32, 3)[None]
    a = _check(x[:, :, ::-1], 60)
    b = _check(x, 60)[:, :, ::-1]
    assert not np.array_equal(a, b)


# ---- bad arguments ----
def test_einval_launches_nothing():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    B, H, W = 2, 5, 7
    src = np.random.default_rng(6).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    s, d = _t(src, dev), torch.full((B, H, W, 3), 9, dtype=torch.uint8, device=dev)
    q, ws = _t([50, 60], dev, np.int32), _ws(lib, B, H, W, dev)
    flags = torch.full((B + 1,), 5, dtype=torch.int32, device=dev)
    good = [hip.ptr(s), hip.ptr(d), B, H, W, hip.ptr(q), hip.ptr(ws), hip.ptr(flags)]
    bad = []
    for k in (0, 1, 5, 6, 7):  # each NULL pointer in turn
        bad.append(good[:k] + [None] + good[k + 1:])
    bad.append([good[0], good[0]] + good[2:])  # dst == src
    for k, v in ((2, 0), (3, 0), (4, 0), (2, -1), (3, -3), (4, -7), (2, 65536)):  # a dimension; B past the grid
        bad.append(good[:k] + [v] + good[k + 1:])
    bad.append(good[:5] + [good[5] + 2] + good[6:])  # quality not 4-byte aligned
    bad.append(good[:7] + [good[7] + 1])             # flags not 4-byte aligned
    bad.append(good[:6] + [good[6] + 4] + good[7:])  # ws not 8-byte aligned
    bad.append(good[:3] + [1 << 15, (1 << 15) + 1] + good[5:])  # H * W past 2^30: rejected on the shape alone
    for args in bad:
        assert lib.mmf_jpeg_roundtrip_u8(*args, hip.stream_ptr()) == EINVAL, args
    torch.cuda.synchronize()
    assert (d == 9).all() and (flags == 5).all() and np.array_equal(s.cpu().numpy(), src)
    assert lib.mmf_jpeg_roundtrip_ws_bytes(0, 5) == 0 and lib.mmf_jpeg_roundtrip_ws_bytes(1 << 15, (1 << 15) + 1) == 0
    assert lib.mmf_jpeg_roundtrip_ws_bytes(224, 224) == 64 * (28 * 28 + 2 * 14 * 14)
    assert lib.mmf_jpeg_roundtrip_ws_bytes(1, 1) == 64 * 3
    assert lib.mmf_jpeg_roundtrip_u8(*good, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), R.pil_roundtrip_batch(src, [50, 60]))
    assert flags.cpu().tolist() == [0, 0, 5]


# ---- the forward half on its own, and the flag ----
def block_roundtrip(blocks, table):
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    b, t = _t(blocks, dev, np.int16), _t(table, dev, np.uint8)
    n = b.shape[0]
    coefs = torch.full((n, 64), -7, dtype=torch.int16, device=dev)
    samples = torch.full((n, 64), 3, dtype=torch.uint8, device=dev)
    outside = torch.full((n,), 5, dtype=torch.int32, device=dev)
    rc = lib.mmf_jpeg_block_roundtrip_raw(hip.ptr(b), hip.ptr(t), n, hip.ptr(coefs), hip.ptr(samples),
                                          hip.ptr(outside), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, coefs.cpu().numpy(), samples.cpu().numpy(), outside.cpu().numpy()


def test_blocks_of_real_images_give_pillows_coefficients():
    for img, q in ((R.noise(24, 40, 5), 57), (R.gradient_with_edge(17, 33), 80), (R.primaries(16, 15), 1)):
        want, tables, _ = R.pil_coefs(img, q)
        for blocks, cf, tab in zip(R.np_sample_blocks(img), want, tables):
            rc, coefs, samples, outside = block_roundtrip(blocks.reshape(-1, 64), tab)
            assert rc == 0
            assert int((coefs != cf.reshape(-1, 64)).sum()) == 0
            assert int((samples.reshape(cf.shape[:2] + (8, 8)) != R.JD.idct_islow(cf, tab)).sum()) == 0
            assert not outside.any()


def test_blocks_outside_the_exact_range():
    """What sets flags.  R.outside_blocks trips the third condition alone and the second with the third (its
    docstring: within +-1024 the first is out of reach, and the second never fails alone); on random blocks up to
    +-1024 under three tables, the predicate is the numpy restatement's and the coefficients are too."""
    blocks, table, which = R.outside_blocks()
    rc, coefs, samples, outside = block_roundtrip(blocks, table)
    want_cf, want_s, want_bad = R.np_block_roundtrip(blocks, table)
    assert rc == 0 and outside.tolist() == want_bad.tolist() == [int(bool(w)) for w in which]
    assert np.array_equal(coefs, want_cf)
    assert np.array_equal(samples[want_bad == 0], want_s[want_bad == 0])
    rng = np.random.default_rng(9)
    amp = np.repeat([128, 400, 600, 1024], 64)[:, None]
    rnd = np.concatenate([rng.integers(-1024, 1025, (256, 64)) * amp // 1024,
                          np.where(rng.random((64, 64)) < 0.5, -1024, 1024), blocks]).astype(np.int16)
    seen = set()
    for tab in (np.ones(64, np.int64), R.np_qtable(40, R.STD_CHROMA), np.full(64, 255, np.int64)):
        rc, coefs, samples, outside = block_roundtrip(rnd, tab)
        want_cf, want_s, want_bad = R.np_block_roundtrip(rnd, tab)
        assert rc == 0 and np.array_equal(coefs, want_cf) and np.array_equal(outside, want_bad)
        assert np.array_equal(samples[want_bad == 0], want_s[want_bad == 0])
        seen.update(want_bad.tolist())
    assert seen == {0, 1}
    # the entry's own bound
    over = blocks.copy()
    over[3, 9] = 1025
    out = block_roundtrip(over, table)
    assert out[0] == EINVAL and (out[1] == -7).all() and (out[2] == 3).all() and (out[3] == 5).all()
    over[3, 9] = -1025
    assert block_roundtrip(over, table)[0] == EINVAL
    assert block_roundtrip(blocks, np.r_[np.ones(63), 0])[0] == EINVAL


# ---- Engine.jpeg_compress ----
@pytest.fixture(scope="module")
def forensics(det_sd, clip_sd):
    _dev()
    from tests.test_gpu_effcls_train import _forensics
    f = _forensics(det_sd, clip_sd)
    yield f
    f.engine.close()


def test_engine_jpeg_compress(forensics):
    eng = forensics.engine
    x = np.random.default_rng(12).integers(0, 256, (4, 30, 26, 3), dtype=np.uint8)
    q = np.array([40, 0, 66, 80])
    want = R.pil_roundtrip_batch(x, q)
    got = eng.jpeg_compress(x, q)
    assert got.device.type == "cuda" and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(eng.jpeg_compress(torch.from_numpy(x).to(eng.device), 57).cpu().numpy(),
                          R.pil_roundtrip_batch(x, [57] * 4))
    for bad_img, bad_q in ((x[..., :2], 50), (x.astype(np.int32), 50), (x, [50, 60]), (x, 101), (x, -1), (x, 50.0),
                           (x[:0], 50)):
        with pytest.raises(ValueError):
            eng.jpeg_compress(bad_img, bad_q)


def test_engine_redoes_a_flagged_image_on_the_host(forensics, monkeypatch):
    """No image made of pixels is flagged, so the read-back is replaced by one that reports image 1: the result is
    still Pillow's and the host path ran for exactly that image."""
    eng = forensics.engine
    x = np.random.default_rng(13).integers(0, 256, (3, 20, 20, 3), dtype=np.uint8)
    q = np.array([45, 70, 90])
    calls, host = [], eng._jpeg_host_roundtrip

    def flagged(flags):
        assert flags.cpu().tolist() == [0, 0, 0]
        return np.array([0, 1, 0], np.int32)

    def counted(rgb, quality):
        calls.append((rgb.copy(), quality))
        return host(rgb, quality)

    monkeypatch.setattr(eng, "_jpeg_flags", flagged)
    monkeypatch.setattr(eng, "_jpeg_host_roundtrip", counted)
    got = eng.jpeg_compress(x, q).cpu().numpy()
    assert np.array_equal(got, R.pil_roundtrip_batch(x, q))
    assert len(calls) == 1 and calls[0][1] == 70 and np.array_equal(calls[0][0], x[1])
    # and what the host path writes is what lands: a marker instead of Pillow's bytes
    monkeypatch.setattr(eng, "_jpeg_host_roundtrip", lambda rgb, quality: np.full_like(rgb, 77))
    got = eng.jpeg_compress(x, q).cpu().numpy()
    assert (got[1] == 77).all() and np.array_equal(got[[0, 2]], R.pil_roundtrip_batch(x, q)[[0, 2]])


# ---- end to end: the JPEG views of the trainer ----
K = 2


@pytest.fixture(scope="module")
def cifake(forensics, tmp_path_factory):
    """A handful of 32 x 32 JPEG files, their qualities and jitter draws."""
    import mmf_amd.cifake_training as CT
    from PIL import Image
    root = tmp_path_factory.mktemp("jpegviews")
    g = np.random.default_rng(21)
    paths = []
    for i in range(5):
        paths.append(str(root / f"img{i}.jpg"))
        Image.fromarray(g.integers(30, 220, (32, 32, 3), dtype=np.uint8)).save(paths[-1], quality=92)
    return paths, CT.jpeg_params(len(paths), K, seed=4), CT.jitter_params(len(paths), K, seed=4)


def test_jpeg_views_are_the_rows_of_pillows_windows(forensics, cifake):
    import mmf_amd.cifake_training as CT
    f, eng = forensics, forensics.engine
    paths, qual, _ = cifake
    N = len(paths)
    plain = CT.extract_image_features(f, paths, flip=True)
    rows, mirrored, ok = CT.extract_image_features(f, paths, flip=True, jpeg=qual)
    assert ok.all() and rows.shape == mirrored.shape == (K, N, 1280) and rows.dtype == np.float32
    assert np.isfinite(rows).all() and not np.array_equal(rows[0], plain[0])
    again = CT.extract_image_features(f, paths, flip=True)  # jpeg=None returns what it returned before
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    only, ok1 = CT.extract_image_features(f, paths, jpeg=qual)
    assert ok1.all() and np.array_equal(only, rows)
    win = f._windows(*f._stage_images(paths))[0]
    host = win.cpu().numpy()
    swapped = 0
    for v in range(K):
        want = R.pil_roundtrip_batch(host, qual[v])
        want_m = R.pil_roundtrip_batch(host[:, :, ::-1], qual[v])  # mirrored first, compressed after
        swapped += int((want_m != want[:, :, ::-1]).sum())
        assert torch.equal(eng.jpeg_compress(win, qual[v]).cpu(), torch.from_numpy(want))
        assert torch.equal(torch.from_numpy(rows[v]), eng.effnet_pooled(torch.from_numpy(want)).cpu())
        assert torch.equal(torch.from_numpy(mirrored[v]), eng.effnet_pooled(torch.from_numpy(want_m)).cpu())
        wrong = eng.effnet_pooled(torch.from_numpy(np.ascontiguousarray(want[:, :, ::-1]))).cpu()
        assert not torch.equal(torch.from_numpy(mirrored[v]), wrong)  # not the mirror of the compressed window
    assert swapped > 0


def test_jitter_then_jpeg(forensics, cifake):
    import mmf_amd.cifake_training as CT
    from tests import jitter_refs as J
    f, eng = forensics, forensics.engine
    paths, qual, jit = cifake
    rows, mirrored, ok = CT.extract_image_features(f, paths, flip=True, jitter=jit, jpeg=qual)
    assert ok.all() and rows.shape == (K, len(paths), 1280)
    host = f._windows(*f._stage_images(paths))[0].cpu().numpy()
    for v in range(K):
        jittered = J.pil_chain(host, jit[0][v], jit[1][v], jit[2][v])
        want = R.pil_roundtrip_batch(jittered, qual[v])
        want_m = R.pil_roundtrip_batch(jittered[:, :, ::-1], qual[v])
        assert torch.equal(torch.from_numpy(rows[v]), eng.effnet_pooled(torch.from_numpy(want)).cpu())
        assert torch.equal(torch.from_numpy(mirrored[v]), eng.effnet_pooled(torch.from_numpy(want_m)).cpu())
    with pytest.raises(ValueError, match="must agree"):
        CT.extract_image_features(f, paths, jitter=jit, jpeg=qual[:1])
