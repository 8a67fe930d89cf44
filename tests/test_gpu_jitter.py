"""mmf_color_jitter_u8 (csrc/jitter.hip), Engine.color_jitter and the jittered views of mmf_amd/cifake_training.py on
the MI355X.

The reference is Pillow, composed as torchvision's PIL backend composes it (tests/jitter_refs.pil_chain); every
comparison is byte or bit equality, so there is no tolerance anywhere.  The single-operation tests run on all 2^24
RGB triples: a contracted FMA or a float / double mix-up in the kernel shows there as differing bytes.
"""
import itertools

import numpy as np
import pytest
import torch

from tests import jitter_refs as J

pytestmark = pytest.mark.gpu
EINVAL = -22
DRAW = float(torch.empty(1).uniform_(0.8, 1.2, generator=torch.Generator().manual_seed(11)))
ORDERS = np.array(list(itertools.permutations(range(4))), np.int32)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def jitter(img, ops, factors, hue_shift, fill=7):
    """One mmf_color_jitter_u8 on a uint8 [B, H, W, 3] numpy array or device tensor -> the result on the host."""
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    s = img if torch.is_tensor(img) else _t(img, dev)
    B, H, W, _ = s.shape
    d = torch.full_like(s, fill)
    o, f, h = _t(ops, dev, np.int32), _t(factors, dev, np.float32), _t(hue_shift, dev, np.int32)
    assert o.shape == (B, 4) and f.shape == (B, 3) and h.shape == (B,)
    ws = torch.full((B, hip.JITTER_CHUNKS), -1, dtype=torch.int64, device=dev)  # contents on entry do not matter
    rc = lib.mmf_color_jitter_u8(hip.ptr(s), hip.ptr(d), B, H, W, hip.ptr(o), hip.ptr(f), hip.ptr(h), hip.ptr(ws),
                                 hip.stream_ptr())
    assert rc == 0, hip.load().mmf_last_error()
    torch.cuda.synchronize()
    return d.cpu().numpy()


def hflip(img):
    import mmf_amd.hip as hip
    s = _t(img, _dev())
    d = torch.empty_like(s)
    B, H, W, C = s.shape
    assert hip.load().mmf_hflip_u8(hip.ptr(s), hip.ptr(d), B, H, W, C, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _check(img, ops, factors, hue_shift):
    got = jitter(img, ops, factors, hue_shift)
    want = J.pil_chain(img, ops, factors, hue_shift)
    diff = int((got != want).sum())
    assert diff == 0, f"{diff} of {want.size} bytes differ from Pillow"
    return got


# ---- single operations on every RGB triple ----
@pytest.fixture(scope="module")
def triples():
    dev = _dev()
    x = J.all_triples()[None]
    return x, _t(x, dev)


def _single(triples, op, factor=1.0, shift=0):
    x, xd = triples
    fac = np.ones((1, 3), np.float32)
    if op < 3:
        fac[0, op] = factor
    got = jitter(xd, [[op, -1, -1, -1]], fac, [shift])
    want = np.asarray(J.pil_op(J.Image.fromarray(x[0], "RGB"), op, float(fac[0, min(op, 2)]), shift))
    diff = int((got[0] != want).sum())
    assert diff == 0, f"{diff} of {want.size} bytes differ from Pillow"


@pytest.mark.parametrize("factor", (0.8, 1.0, 1.2, DRAW))
@pytest.mark.parametrize("op", (J.BRIGHTNESS, J.SATURATION), ids=("brightness", "saturation"))
def test_brightness_and_saturation_on_every_triple(triples, op, factor):
    _single(triples, op, factor)


@pytest.mark.parametrize("factor", (0.8, 1.2))
def test_contrast_on_every_triple(triples, factor):
    _single(triples, J.CONTRAST, factor)


@pytest.mark.parametrize("shift", (0, 1, 26, 230, 255))
def test_hue_on_every_triple(triples, shift):
    _single(triples, J.HUE, shift=shift)


# ---- chains ----
def _draws(B, seed, lo=0.8, hi=1.2):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (B, 3)).astype(np.float32), rng.integers(0, 256, B).astype(np.int32)


def test_every_order_of_the_four_operations():
    x = np.random.default_rng(1).integers(0, 256, (24, 32, 32, 3), dtype=np.uint8)
    fac, shift = _draws(24, 2)
    _check(x, ORDERS, fac, shift)
    # the ends of the ranges: 1.2 clips, 0.8 truncates; the widest hue shifts of ColorJitter(hue=0.1)
    ends = np.where(np.random.default_rng(3).random((24, 3)) < 0.5, np.float32(0.8), np.float32(1.2))
    _check(x, ORDERS, ends, np.where(np.arange(24) % 2, 25, 231))
    # far outside: factors that clip most bytes at either end, and 0
    _check(x, ORDERS, np.tile(np.float32([[3.0, 0.0, 2.5], [0.0, 4.0, 0.0]]), (12, 1)), shift)


@pytest.mark.parametrize("shape", [(5, 224, 224, 3), (2, 5, 7, 3), (3, 1, 1, 3), (1, 1, 1025, 3), (2, 513, 1023, 3)],
                         ids=str)
def test_shapes(shape):
    """224 x 224 (the trainer's), sizes that are no multiple of the four-pixel group or of a block's 1024 pixels,
    images whose first byte is not dword-aligned (5 x 7: 105 bytes each), and more chunks than one block sweep
    (513 x 1023 pixels > 256 chunks x 1024)."""
    B = shape[0]
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    fac, shift = _draws(B, 7)
    _check(x, ORDERS[[5, 9, 14, 20, 23][:B]], fac, shift)


def test_constant_images():
    x = np.stack([np.full((9, 11, 3), v, np.uint8) for v in (0, 255, 128)])
    for order in ORDERS[[0, 8, 17]]:
        _check(x, np.tile(order, (3, 1)), [[1.2, 0.8, 1.2], [1.2, 1.2, 0.8], [0.8, 1.2, 1.13]], [17, 239, 0])


def test_contrast_mean_half_way():
    """L means of exactly m + 0.5 and m on two-pixel images, contrast first; and the mean of the image as it stands
    after a brightness that clips: 212 -> 254 and 250 -> 255 at 1.2, mean 254.5 -> 255 (the source's would be 231)."""
    two = np.array([[[[v, v, v] for v in px]] for px in ((100, 101), (100, 100), (254, 255))], np.uint8)
    _check(two, [[1, -1, -1, -1]] * 3, [[1, 0.5, 1]] * 3, [0] * 3)
    _check(two, [[1, 0, 2, 3]] * 3, [[1.2, 0.8, 1.1]] * 3, [3] * 3)
    bright = np.array([[[[212, 212, 212], [250, 250, 250]]]], np.uint8)
    got = _check(bright, [[0, 1, -1, -1]], [[1.2, 0.5, 1]], [0])
    assert got[0, 0].tolist() == [[254, 254, 254], [255, 255, 255]]  # 255 + 0.5 (254 - 255) = 254.5 -> 254
    _check(bright, [[0, 1, 2, 3]], [[1.2, 1.2, 0.9]], [250])


# ---- invariance ----
def test_invariance():
    x = np.random.default_rng(4).integers(0, 256, (6, 37, 41, 3), dtype=np.uint8)
    ops = ORDERS[[3, 7, 11, 13, 19, 22]]
    fac, shift = _draws(6, 5)
    whole = jitter(x, ops, fac, shift)
    assert np.array_equal(whole, jitter(x, ops, fac, shift, fill=200))  # the same call twice
    for b in range(6):  # an image alone and inside a batch
        assert np.array_equal(whole[b:b + 1], jitter(x[b:b + 1], ops[b:b + 1], fac[b:b + 1], shift[b:b + 1]))
    # a -1 entry and the chain without it
    for k in range(4):
        gap = np.insert(np.delete(ORDERS[10], k), 0, -1)[None]     # the k-th operation dropped, a skip in front
        tail = np.append(np.delete(ORDERS[10], k), -1)[None]       # ... and a skip at the end
        mid = np.insert(np.delete(ORDERS[10], k), 2, -1)[None]
        a = jitter(x[:1], gap, fac[:1], shift[:1])
        assert np.array_equal(a, jitter(x[:1], tail, fac[:1], shift[:1]))
        assert np.array_equal(a, jitter(x[:1], mid, fac[:1], shift[:1]))
        assert np.array_equal(a, J.pil_chain(x[:1], tail, fac[:1], shift[:1]))
    assert np.array_equal(jitter(x, np.full((6, 4), -1), fac, shift), x)  # nothing to do: a copy
    # jitter and flip commute: every operation is per pixel or a whole-image mean
    assert np.array_equal(hflip(whole), jitter(hflip(x), ops, fac, shift))


# ---- bad arguments ----
def test_einval_launches_nothing():
    import mmf_amd.hip as hip
    dev = _dev()
    lib = hip.load()
    B, H, W = 2, 5, 7
    src = np.random.default_rng(6).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    s, d = _t(src, dev), torch.full((B, H, W, 3), 9, dtype=torch.uint8, device=dev)
    o, f, h = _t(ORDERS[:B], dev), _t(np.ones((B, 3), np.float32), dev), _t(np.zeros(B, np.int32), dev)
    ws = torch.zeros((B, hip.JITTER_CHUNKS), dtype=torch.int64, device=dev)
    good = [hip.ptr(s), hip.ptr(d), B, H, W, hip.ptr(o), hip.ptr(f), hip.ptr(h), hip.ptr(ws)]
    bad = []
    for k in (0, 1, 5, 6, 7, 8):  # each NULL pointer in turn
        bad.append(good[:k] + [None] + good[k + 1:])
    bad.append([good[0], good[0]] + good[2:])  # dst == src
    for k, v in ((2, 0), (3, 0), (4, 0), (2, -1), (3, -3), (2, 65536)):  # a non-positive dimension; B past the grid
        bad.append(good[:k] + [v] + good[k + 1:])
    bad.append(good[:5] + [good[5] + 2] + good[6:])  # ops not 4-byte aligned
    bad.append(good[:8] + [good[8] + 4])             # ws not 8-byte aligned
    for args in bad:
        assert lib.mmf_color_jitter_u8(*args, hip.stream_ptr()) == EINVAL, args
    torch.cuda.synchronize()
    assert (d == 9).all() and np.array_equal(s.cpu().numpy(), src)
    # H * W past 2^40 pixels: rejected on the shape alone, before any pointer is followed
    assert lib.mmf_color_jitter_u8(*good[:3], 1 << 21, (1 << 19) + 1, *good[5:], hip.stream_ptr()) == EINVAL
    assert lib.mmf_color_jitter_u8(*good, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), J.pil_chain(src, ORDERS[:B], np.ones((B, 3)), np.zeros(B, int)))


def test_values_out_of_range_in_the_device_arrays():
    """An op code outside -1..3 is a skip, a second contrast is a skip, the shift is taken & 255 -- and none of them
    reaches memory it should not."""
    x = np.random.default_rng(8).integers(0, 256, (4, 13, 9, 3), dtype=np.uint8)
    fac, _ = _draws(4, 9)
    ops = np.array([[7, 0, -5, 3], [1, 2, 1, 1], [1 << 30, -(1 << 31), 4, -2], [3, 1, 0, 1]], np.int32)
    shift = np.array([256 + 26, -17, 1 << 20, (1 << 31) - 1], np.int64).astype(np.int32)
    got = jitter(x, ops, fac, shift)
    clean = np.array([[-1, 0, -1, 3], [1, 2, -1, -1], [-1, -1, -1, -1], [3, 1, 0, -1]], np.int32)
    assert np.array_equal(got, J.pil_chain(x, clean, fac, [26, 239, 0, 255]))
    assert np.array_equal(got, J.np_chain(x, ops, fac, shift))
    assert np.array_equal(got[2], x[2])


# ---- end to end: the jittered views of the trainer ----
K = 2


@pytest.fixture(scope="module")
def cifake(det_sd, clip_sd, tmp_path_factory):
    """A CIFAKE tree of 24 files of 32 x 32, every other one a JPEG (19 to train on, 5 to validate), and the
    detector."""
    _dev()
    import mmf_amd.cifake_training as CT
    from tests.test_gpu_effcls_train import _forensics, _tree
    root = tmp_path_factory.mktemp("jitter") / "cifake"
    _tree(root)
    tp, ty, vp, vy = CT.load_cifake_data(str(root))
    assert len(tp) == 19 and len(vp) == 5
    f = _forensics(det_sd, clip_sd)
    yield f, tp, np.asarray(ty, np.int32), vp, np.asarray(vy, np.int32), CT.jitter_params(len(tp), K, seed=1)
    f.engine.close()


@pytest.fixture(scope="module")
def views(cifake):
    """(what extract_image_features returned before any call with jitter, what it returns with jitter)."""
    import mmf_amd.cifake_training as CT
    f, tp, _, _, _, jit = cifake
    plain = CT.extract_image_features(f, tp, flip=True)
    return plain, CT.extract_image_features(f, tp, flip=True, jitter=jit)


def test_jittered_views_are_the_rows_of_pillows_windows(cifake, views):
    import mmf_amd.cifake_training as CT
    f, tp, _, _, _, jit = cifake
    eng, N = f.engine, len(tp)
    plain, (rows, mirrored, ok) = views
    assert ok.all() and rows.shape == mirrored.shape == (K, N, 1280) and rows.dtype == np.float32
    assert np.isfinite(rows).all() and not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0], plain[0])
    # jitter=None returns what it returned before the call with jitter
    again = CT.extract_image_features(f, tp, flip=True)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    # the staged windows, jittered by Pillow on the host, through effnet_pooled in the same chunk shape
    cap = eng.max_batch
    for a in range(0, N, cap):
        b = min(a + cap, N)
        win = f._windows(*f._stage_images(tp[a:b]))[0]
        host = win.cpu().numpy()
        for v in range(K):
            want = torch.from_numpy(J.pil_chain(host, jit[0][v, a:b], jit[1][v, a:b], jit[2][v, a:b]))
            assert torch.equal(eng.color_jitter(win, jit[0][v, a:b], jit[1][v, a:b], jit[2][v, a:b]).cpu(), want)
            assert torch.equal(torch.from_numpy(rows[v, a:b]), eng.effnet_pooled(want).cpu())
            assert torch.equal(torch.from_numpy(mirrored[v, a:b]),
                               eng.effnet_pooled(torch.flip(want, dims=[2]).contiguous()).cpu())
    with pytest.raises(ValueError):
        eng.color_jitter(np.zeros((2, 4, 4, 3), np.uint8), np.zeros((1, 4), np.int32), np.ones((2, 3)), [0, 0])
    with pytest.raises(ValueError):
        eng.color_jitter(np.zeros((2, 4, 4, 4), np.uint8), np.zeros((2, 4), np.int32), np.ones((2, 3)), [0, 0])


def test_fit_on_the_jittered_bank(cifake, views):
    import mmf_amd.cifake_training as CT
    from tests import effcls_train_refs as R
    f, _, ty, vp, vy, _ = cifake
    rows, mirrored, _ = views[1]
    xv, okv = CT.extract_image_features(f, vp)
    assert okv.all()
    before = CT.flatten_classifier(f.detector).cpu().numpy()
    hist = CT.ClassifierTrainer(f, batch_size=8, epochs=2, seed=1, flip=True, jitter_views=K).fit(
        (rows, mirrored), ty, xv, vy)
    after = CT.flatten_classifier(f.detector).cpu().numpy()
    assert [h["epoch"] for h in hist] == [1, 2] and all(np.isfinite(h["train_loss"]) for h in hist)
    bank = np.concatenate([rows[0], mirrored[0], rows[1], mirrored[1]])  # the 4N-row bank, in the plan's order
    bl = np.concatenate([ty] * 4)
    loss0 = R.evaluate(bank, bl, len(bl), before.astype(np.float64))[0][0]
    loss1 = R.evaluate(bank, bl, len(bl), after.astype(np.float64))[0][0]
    print(f"fit on {len(bl)} cached rows: float64 eval loss {loss0:.6f} -> {loss1:.6f}; history {hist}")
    assert loss1 < loss0
