"""Device resampling of decoded images (mmf_resize_pil) against Pillow and the
oracle restatement: bit-exact EfficientNet squash and CLIP shortest-edge + crop windows for up- and
down-scaling, odd and extreme sizes; the API's analyze_pairs (host decode + device resample)
equals the all-host path."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Image = pytest.importorskip("PIL.Image")

SIZES = [(640, 480), (480, 640), (224, 224), (225, 224), (224, 300), (37, 500), (3, 2), (1500, 224),
         (2000, 1500), (800, 800), (1, 1), (4000, 3000)]


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    return Engine(0, None, None, max_batch=8)


def test_resize_matches_pillow(engine):
    from mmf_amd import io_utils
    g = np.random.default_rng(1)
    imgs = [g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for w, h in SIZES]
    eff, clp = engine.resize_images(imgs)
    eff, clp = eff.cpu().numpy(), clp.cpu().numpy()
    for i, a in enumerate(imgs):
        pil = Image.fromarray(a)
        np.testing.assert_array_equal(eff[i], io_utils.effnet_pixels(pil), err_msg=f"effnet {SIZES[i]}")
        np.testing.assert_array_equal(clp[i], io_utils.clip_pixels(pil), err_msg=f"clip {SIZES[i]}")
    # RGBX sources (Pillow's in-memory layout, 4 bytes per pixel) give the same windows
    e4, c4 = engine.resize_images([np.concatenate([a, np.full(a.shape[:2] + (1,), 7, np.uint8)], -1) for a in imgs])
    np.testing.assert_array_equal(e4.cpu().numpy(), eff)
    np.testing.assert_array_equal(c4.cpu().numpy(), clp)


def test_decoded_views_through_the_device(engine):
    """io_utils.decode_rgb (zero-copy RGBX views when Pillow exports Arrow) -> resize_images equals
    the all-host decode_batch on JPEG bytes, PNG paths and non-RGB modes."""
    from mmf_amd import io_utils
    g = np.random.default_rng(2)
    items = []
    for k, (w, h) in enumerate([(640, 480), (300, 500), (224, 224), (50, 80)]):
        im = Image.fromarray(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        if k == 1:
            im = im.convert("L")
        b = io.BytesIO()
        im.save(b, format="JPEG" if k % 2 == 0 else "PNG")
        items.append(b.getvalue())
    eff, clp = engine.resize_images(io_utils.decode_rgb(items))
    he, hc = io_utils.decode_batch(items)
    np.testing.assert_array_equal(eff.cpu().numpy(), he)
    np.testing.assert_array_equal(clp.cpu().numpy(), hc)


def test_resize_single_output_and_structured_images(engine):
    from oracle import pil_resample as R
    yy, xx = np.mgrid[0:333, 0:517]
    a = np.stack([(xx * 3 + yy) % 256, (xx * yy) % 256, (255 - xx) % 256], -1).astype(np.uint8)
    eff, clp = engine.resize_images([a], clip=False)
    assert clp is None
    np.testing.assert_array_equal(eff.cpu().numpy()[0], R.effnet_window(a))
    _, clp = engine.resize_images([a], effnet=False)
    np.testing.assert_array_equal(clp.cpu().numpy()[0], R.clip_window(a))


def test_resize_rejects_beyond_tap_limit(engine):
    from mmf_amd.hip import MMFError
    with pytest.raises(MMFError):
        engine.resize_images([np.zeros((224, 20000, 3), np.uint8)])


# ------------------------------------------------------------------------------------------------------------------
# Per coefficient and at the edges: the coefficient kernel alone (mmf_resize_coef_raw) against
# tests/resize_refs.window_coeffs, the windows on every geometry branch, at the tap budget's last sizes and around
# Image.resize's vertical-first order against Pillow, batch mechanics, RGBX and the rejects.  All exact.
from tests import resize_refs as RR  # noqa: E402

MMF_EINVAL, MMF_ERANGE = -22, -34
CANARY = 0x5A5A5A5A


def _pillow(a):
    from mmf_amd import io_utils
    pil = Image.fromarray(a)
    return io_utils.effnet_pixels(pil), io_utils.clip_pixels(pil)


_REFS = {}


def _ref(content, w, h):
    """(image, Pillow's EfficientNet window, Pillow's CLIP window), computed once per case and left unchanged."""
    key = (content, w, h)
    if key not in _REFS:
        a = RR.CONTENT[content](w, h)
        a.setflags(write=False)
        _REFS[key] = (a,) + _pillow(a)
    return _REFS[key]


def _check_windows(engine, cases, batch=48):
    for i in range(0, len(cases), batch):
        part = [_ref(*c) for c in cases[i:i + batch]]
        eff, clp = engine.resize_images([p[0] for p in part])
        eff, clp = eff.cpu().numpy(), clp.cpu().numpy()
        for j, (c, p) in enumerate(zip(cases[i:i + batch], part)):
            np.testing.assert_array_equal(eff[j], p[1], err_msg=f"effnet {c}")
            np.testing.assert_array_equal(clp[j], p[2], err_msg=f"clip {c}")
    return 2 * len(cases)


def _raw(engine, imgs, eff, clp, ps=None, wh=None, null=(), B=None):
    """mmf_resize_pil on caller-owned outputs: its return code."""
    import ctypes
    from mmf_amd.hip import ptr, stream_ptr
    ps = imgs[0].shape[2] if ps is None else ps
    flat = np.concatenate([a.reshape(-1) for a in imgs])
    offs = np.zeros(len(imgs), np.int64)
    offs[1:] = np.cumsum([a.nbytes for a in imgs])[:-1]
    wh = np.array([[a.shape[1], a.shape[0]] for a in imgs] if wh is None else wh, np.int32).reshape(-1)
    src = torch.from_numpy(flat).to(engine.device)
    rc = engine.lib.mmf_resize_pil(engine.h, None if "src" in null else ptr(src),
                                   None if "offsets" in null else offs.ctypes.data_as(ctypes.c_void_p),
                                   None if "wh" in null else wh.ctypes.data_as(ctypes.c_void_p), len(imgs) if B is None else B, ps,
                                   ptr(eff), ptr(clp), stream_ptr())
    torch.cuda.synchronize()
    return rc


def _a5(engine, n):
    return (torch.full((n, 224, 224, 3), 0xA5, dtype=torch.uint8, device=engine.device),
            torch.full((n, 224, 224, 3), 0xA5, dtype=torch.uint8, device=engine.device))


def test_coefficients_and_bounds_exact(engine):
    """resize_coef_kernel alone on the 4123 jobs of COEF_SIDES (8206 axes whose pass runs; the list is not thinned):
    every fixed-point weight and every (xmin, n) equals the vectorised restatement of Pillow's precompute_coeffs +
    normalize_coeffs_8bpc, taps at and past n are 0 up to ks, and the canaries behind both buffers stay.  The host
    planner's rows y0 .. y1 (and columns x0 .. x1 where the vertical pass runs first) equal the ends of the bounds
    the device computed: what the passes' tmp indexing relies on.  An axis whose pass does not run has ks = 1 and
    values no pass reads: only its canary is checked."""
    from mmf_amd.hip import ptr, stream_ptr
    lib, dev = engine.lib, engine.device
    coef = torch.empty(224 * 2 * RR.KMAX + 64, dtype=torch.int32, device=dev)
    bounds = torch.empty(2 * 224 * 2 + 64, dtype=torch.int32, device=dev)
    axes = 0
    for w, h, geom in RR.COEF_SIDES:
        p = np.zeros(12, np.int32)
        assert lib.mmf_resize_plan(w, h, geom, p.ctypes.data) == 0, (w, h, geom)
        ow, oh, cx, cy, need_h, need_v, y0, y1, ksh, ksv, x0, x1 = (int(v) for v in p)
        assert tuple(int(v) for v in p) == RR.plan(w, h, geom), (w, h, geom)
        used = 224 * (ksh + ksv)
        coef.fill_(CANARY)
        bounds.fill_(CANARY)
        assert lib.mmf_resize_coef_raw(w, h, geom, ptr(coef), ptr(bounds), stream_ptr()) == 0, (w, h, geom)
        c = coef[:used + 64].cpu().numpy()
        b = bounds.cpu().numpy()
        assert (c[used:] == CANARY).all() and (b[896:] == CANARY).all(), (w, h, geom)
        b = b[:896].reshape(2, 224, 2)
        name = RR.FILTERS[geom]
        for axis, need, size, out, first, ks, k in ((0, need_h, w, ow, cx, ksh, c[:224 * ksh]),
                                                   (1, need_v, h, oh, cy, ksv, c[224 * ksh:used])):
            if not need:
                continue
            rb, rk = RR.window_coeffs(size, out, first, name)
            assert rk.shape[1] == ks, (w, h, geom, axis)
            np.testing.assert_array_equal(b[axis], rb, err_msg=f"bounds {w}x{h} geom {geom} axis {axis}")
            np.testing.assert_array_equal(k.reshape(224, ks), rk, err_msg=f"coef {w}x{h} geom {geom} axis {axis}")
            axes += 1
        if need_v:
            assert (b[1, 0, 0], b[1, 223, 0] + b[1, 223, 1]) == (y0, y1), (w, h, geom)
        if x1 > 0:
            assert (b[0, 0, 0], b[0, 223, 0] + b[0, 223, 1]) == (x0, x1), (w, h, geom)
    assert len(RR.COEF_SIDES) == 4123 and axes == 8206


def test_windows_on_the_sweep(engine):
    """The 144 (w, h) pairs of SWEEP with random content, in batches of 48: every geometry branch (one pass, both,
    none, crop only, odd and even crops, sources narrower than the taps, 1-pixel sides, the vertical-first order of
    the narrow tall ones).  288 windows against Pillow itself, the extreme aspect ratios included (Pillow's
    224 x 150752 intermediates cost 2 to 3 s in all)."""
    assert _check_windows(engine, [("random", w, h) for w, h in RR.SWEEP_PAIRS]) == 288


def test_windows_on_the_ties_structured(engine):
    """The 18 TIES pairs (tap boundaries that are integers exactly) with each structured content -- checkerboards
    that drive both passes into both clamps, impulses, steps: 180 windows against Pillow."""
    assert _check_windows(engine, [(c, w, h) for w, h in RR.TIES_PAIRS for c in RR.STRUCTURED]) == 180


def test_windows_at_the_tap_budget_and_tall(engine):
    """The last supported sizes (95 taps on each axis and filter) and the sizes around Image.resize's vertical-first
    order, random and checker content, against Pillow.  The 22500-row sizes are past the squash's budget: CLIP
    only."""
    from mmf_amd import io_utils
    _check_windows(engine, [("random", w, h) for w, h in RR.BUDGET], batch=1)
    both = [(w, h) for w, h in RR.TALL if RR.plan(w, h, 0) is not None]
    _check_windows(engine, [(c, w, h) for w, h in both for c in ("random", "checker2")])
    for w, h in [s for s in RR.TALL if s not in both]:
        assert not engine.resize_supported(w, h)
        a = RR.random_image(w, h)
        _, clp = engine.resize_images([a], effnet=False)
        np.testing.assert_array_equal(clp.cpu().numpy()[0], io_utils.clip_pixels(Image.fromarray(a)), err_msg=f"clip {w}x{h}")


def test_over_budget_rejects_and_leaves_outputs(engine):
    """The first rejected sizes: MMFError with MMF_ERANGE through the engine, and through the ABI alone or as the
    middle image of three with both outputs, pre-filled with 0xA5, untouched."""
    from mmf_amd.hip import MMFError
    small = RR.random_image(50, 40)
    for w, h in RR.OVER:
        big = np.zeros((h, w, 3), np.uint8)
        assert not engine.resize_supported(w, h)
        for imgs in ([big], [small, big, small]):
            with pytest.raises(MMFError, match=rf"\({MMF_ERANGE}\)"):
                engine.resize_images(imgs)
            eff, clp = _a5(engine, len(imgs))
            assert _raw(engine, imgs, eff, clp) == MMF_ERANGE
            assert (eff == 0xA5).all() and (clp == 0xA5).all(), (w, h, len(imgs))


def test_batch_mechanics_bit_identical(engine):
    sizes = [(288, 288), (7, 449), (225, 224), (640, 480), (2, 448), (224, 224), (100, 100)]
    imgs = [RR.random_image(w, h, seed=5) for w, h in sizes]
    eff, clp = (t.cpu().numpy() for t in engine.resize_images(imgs))
    for i, a in enumerate(imgs):  # alone = inside the mixed batch, wherever it stands
        e1, c1 = (t.cpu().numpy() for t in engine.resize_images([a]))
        np.testing.assert_array_equal(e1[0], eff[i])
        np.testing.assert_array_equal(c1[0], clp[i])
    a, rest = imgs[0], imgs[1:4]
    for pos in (0, 1, 3):
        e, c = (t.cpu().numpy() for t in engine.resize_images(rest[:pos] + [a] + rest[pos:]))
        np.testing.assert_array_equal(e[pos], eff[0])
        np.testing.assert_array_equal(c[pos], clp[0])
    er, cr = (t.cpu().numpy() for t in engine.resize_images(imgs[::-1]))
    np.testing.assert_array_equal(er, eff[::-1])
    np.testing.assert_array_equal(cr, clp[::-1])
    e, none = engine.resize_images(imgs, clip=False)
    assert none is None
    np.testing.assert_array_equal(e.cpu().numpy(), eff)
    none, c = engine.resize_images(imgs, effnet=False)
    assert none is None
    np.testing.assert_array_equal(c.cpu().numpy(), clp)


def test_workspace_grows_once_and_serves_smaller_calls(engine):
    imgs = [RR.random_image(w, h, seed=6) for w, h in [(300, 200), (96, 352), (5, 501)]]
    first = [t.cpu().numpy() for t in engine.resize_images(imgs)]
    big = _ref("random", *RR.BUDGET[0])
    eff, clp = engine.resize_images([big[0]])
    np.testing.assert_array_equal(eff.cpu().numpy()[0], big[1])
    np.testing.assert_array_equal(clp.cpu().numpy()[0], big[2])
    grown = engine.device_bytes
    again = [t.cpu().numpy() for t in engine.resize_images(imgs)]
    assert engine.device_bytes == grown
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])
    for a, e, c in zip(imgs, again[0], again[1]):
        pe, pc = _pillow(a)
        np.testing.assert_array_equal(e, pe)
        np.testing.assert_array_equal(c, pc)


def test_empty_batch(engine):
    """resize_images([]) gives two empty [0, 224, 224, 3] uint8 device tensors (None for an output not asked for)."""
    eff, clp = engine.resize_images([])
    for t in (eff, clp):
        assert tuple(t.shape) == (0, 224, 224, 3) and t.dtype == torch.uint8 and t.is_cuda
    eff, clp = engine.resize_images([], clip=False)
    assert tuple(eff.shape) == (0, 224, 224, 3) and clp is None
    eff, clp = _a5(engine, 1)  # the ABI with B = 0: success, nothing written
    assert _raw(engine, [RR.random_image(3, 3)], eff, clp, B=0) == 0
    assert (eff == 0xA5).all() and (clp == 0xA5).all()


def test_rgbx_with_a_random_fourth_byte(engine):
    """Every content family as RGBX with a random fourth byte equals its RGB run (and Pillow)."""
    cases = [(c, w, h) for c in RR.CONTENT for w, h in [(288, 352), (7, 449), (225, 224), (2, 448)]]
    refs = [_ref(*c) for c in cases]
    e4, c4 = (t.cpu().numpy() for t in engine.resize_images([RR.rgbx(r[0], seed=i) for i, r in enumerate(refs)]))
    e3, c3 = (t.cpu().numpy() for t in engine.resize_images([r[0] for r in refs]))
    np.testing.assert_array_equal(e4, e3)
    np.testing.assert_array_equal(c4, c3)
    for i, r in enumerate(refs):
        np.testing.assert_array_equal(e3[i], r[1], err_msg=str(cases[i]))
        np.testing.assert_array_equal(c3[i], r[2], err_msg=str(cases[i]))


def test_raw_abi_rejects(engine):
    """MMF_EINVAL with nothing written: mmf_resize_pil for a zero or negative side, pixel_bytes 2 and 5 and a NULL
    src, offsets or wh; mmf_resize_coef_raw for the same sizes, another geom and NULL buffers, and MMF_ERANGE past
    the budget."""
    from mmf_amd.hip import ptr, stream_ptr
    imgs = [RR.random_image(30, 20), RR.random_image(20, 30)]
    bad = [dict(wh=[[30, 20], [0, 30]]), dict(wh=[[30, 20], [20, 0]]), dict(wh=[[-30, 20], [20, 30]]),
           dict(wh=[[30, 20], [20, -1]]), dict(ps=2), dict(ps=5), dict(null=("src",)), dict(null=("offsets",)),
           dict(null=("wh",))]
    for kw in bad:
        eff, clp = _a5(engine, 2)
        assert _raw(engine, imgs, eff, clp, **kw) == MMF_EINVAL, kw
        assert (eff == 0xA5).all() and (clp == 0xA5).all(), kw
    eff, clp = _a5(engine, 2)
    assert _raw(engine, imgs, eff, clp) == 0
    assert not (eff == 0xA5).all() and not (clp == 0xA5).all()
    coef = torch.full((224 * 2 * RR.KMAX,), CANARY, dtype=torch.int32, device=engine.device)
    bounds = torch.full((896,), CANARY, dtype=torch.int32, device=engine.device)
    calls = [((0, 5, 0), coef, bounds, MMF_EINVAL), ((5, 0, 1), coef, bounds, MMF_EINVAL),
             ((-3, 5, 0), coef, bounds, MMF_EINVAL), ((5, -3, 1), coef, bounds, MMF_EINVAL),
             ((5, 5, 2), coef, bounds, MMF_EINVAL), ((5, 5, -1), coef, bounds, MMF_EINVAL),
             ((5, 5, 0), None, bounds, MMF_EINVAL), ((5, 5, 0), coef, None, MMF_EINVAL),
             ((5265, 5265, 1), coef, bounds, MMF_ERANGE), ((10529, 200, 0), coef, bounds, MMF_ERANGE),
             ((200, 10529, 0), coef, bounds, MMF_ERANGE)]
    for (w, h, geom), c, b, want in calls:
        assert engine.lib.mmf_resize_coef_raw(w, h, geom, ptr(c), ptr(b), stream_ptr()) == want, (w, h, geom)
        torch.cuda.synchronize()
        assert (coef == CANARY).all() and (bounds == CANARY).all(), (w, h, geom)
