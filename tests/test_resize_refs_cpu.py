"""Pins tests/resize_refs.py -- the plan, the vectorised window coefficients and the window-only restatement the
device resampler's tests compare against -- to the host planner of libmmf_hip.so (mmf_resize_plan: host code, no
GPU needed), to oracle/pil_resample.py's scalar coefficients and to Pillow's pixels, all with equality; and
checks that the case lists reach what they are there for: tap boundaries decided in the last place, every
geometry branch, the tap budget's last sizes and both clamps of both passes."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import pil_resample as R
from tests import resize_refs as RR

MMF_EINVAL, MMF_ERANGE = -22, -34


def lib():
    from mmf_amd import hip
    try:
        return hip.load()
    except hip.MMFError as e:
        pytest.skip(f"libmmf_hip.so not built: {e}")


def c_plan(L, w, h, geom):
    out = np.full(12, -7, np.int32)
    rc = L.mmf_resize_plan(w, h, geom, out.ctypes.data)
    return rc, out


def test_plan_equals_host_planner():
    L = lib()
    pairs = [(w, h) for w in range(1, 257) for h in range(1, 257)]
    pairs += RR.SWEEP_PAIRS + RR.TIES_PAIRS + RR.BUDGET + RR.OVER
    for w, h in dict.fromkeys(pairs):
        ok = []
        for geom in (0, 1):
            ref = RR.plan(w, h, geom)
            rc, got = c_plan(L, w, h, geom)
            if ref is None:
                assert rc == MMF_ERANGE, (w, h, geom, rc)
                assert (got == -7).all(), (w, h, geom)
            else:
                assert rc == 0, (w, h, geom, rc)
                assert tuple(got) == ref, (w, h, geom, tuple(got), ref)
            ok.append(ref is not None)
        assert L.mmf_resize_supported(w, h) == int(all(ok)), (w, h)
    for w, h in RR.SWEEP_PAIRS + RR.TIES_PAIRS + RR.BUDGET:  # the plan's rows are the vertical bounds' ends
        for geom in (0, 1):
            p = RR.plan(w, h, geom)
            if p[5]:
                bv, _ = RR.window_coeffs(h, p[1], p[3], RR.FILTERS[geom])
                assert (p[6], p[7]) == (bv[0][0], bv[223][0] + bv[223][1]), (w, h, geom)
    # each OVER size is one pixel past the budget of one geometry: bicubic for the square, bilinear for the others
    assert [[RR.plan(w, h, g) is None for g in (0, 1)] for w, h in RR.OVER] == [[False, True], [True, False], [True, False]]
    for w, h in RR.BUDGET:
        assert RR.plan(w, h, 0) is not None and RR.plan(w, h, 1) is not None


def test_plan_rejects():
    L = lib()
    for w, h, geom in [(0, 5, 0), (5, 0, 1), (-1, 5, 0), (5, -224, 1), (5, 5, 2), (5, 5, -1)]:
        rc, got = c_plan(L, w, h, geom)
        assert rc == MMF_EINVAL and (got == -7).all(), (w, h, geom)
        assert L.mmf_resize_supported(w, h) == (1 if w > 0 and h > 0 else 0)
    assert L.mmf_resize_plan(5, 5, 0, None) == MMF_EINVAL


def _axes():
    """(in_size, out_size, first, filter) of every needed axis of the TIES and SWEEP pairs: the squash and CLIP's
    short axis (first 0) and CLIP's long axis (first = the crop offset, non-zero for most)."""
    axes = []
    for w, h in RR.TIES_PAIRS + RR.SWEEP_PAIRS:
        for geom in (0, 1):
            ow, oh, cx, cy = RR.geometry(w, h, geom)
            if ow != w:
                axes.append((w, ow, cx, RR.FILTERS[geom]))
            if oh != h:
                axes.append((h, oh, cy, RR.FILTERS[geom]))
    return list(dict.fromkeys(axes))


def test_window_coeffs_equal_scalar_oracle():
    axes = _axes()
    assert any(first > 0 for _, _, first, _ in axes) and {a[0] for a in axes} >= (set(RR.TIES) | set(RR.SWEEP)) - {224}
    # the scalar oracle costs out_size coordinates per call: the tallest outputs (a 1-pixel short side) are thinned
    axes = [a for a in axes if a[1] <= 20000]
    assert max(a[1] for a in axes) > 10000
    for in_size, out_size, first, name in axes:
        bounds, kk = R.coeffs(in_size, out_size, name)
        b, k = RR.window_coeffs(in_size, out_size, first, name)
        assert k.shape[1] == kk.shape[1] == RR.ksize(in_size, out_size, name)
        np.testing.assert_array_equal(b, np.array(bounds[first:first + 224]), err_msg=str((in_size, out_size, first, name)))
        np.testing.assert_array_equal(k, kk[first:first + 224], err_msg=str((in_size, out_size, first, name)))


Image = pytest.importorskip("PIL.Image")

WINDOW_CASES = [(w, h, c) for w, h in RR.TIES_PAIRS for c in ("random", "checker2")]
WINDOW_CASES += [(w, h, "random") for w, h in RR.SWEEP_PAIRS if w <= 227 and h <= 227]
WINDOW_CASES += [(w, h, c) for w, h in RR.TALL for c in ("random", "checker2")]


def test_windows_equal_pillow():
    from mmf_amd import io_utils
    for w, h, content in WINDOW_CASES:
        a = RR.CONTENT[content](w, h)
        pil = Image.fromarray(a)
        assert RR.plan(w, h, 1) is not None
        if RR.plan(w, h, 0) is not None:  # TALL's 22500-row sizes are past the squash's tap budget
            np.testing.assert_array_equal(RR.window(a, 0), io_utils.effnet_pixels(pil), err_msg=f"effnet {w}x{h} {content}")
        np.testing.assert_array_equal(RR.window(a, 1), io_utils.clip_pixels(pil), err_msg=f"clip {w}x{h} {content}")
        np.testing.assert_array_equal(RR.window(RR.rgbx(a), 1), RR.window(a, 1))


def _integer_boundaries(in_size, out_size, name):
    """Tap boundaries center -+ support + 0.5 of a resize whose exact (rational) value is an integer inside the
    source, and those of them whose double-precision value is not that integer."""
    scale = Fraction(in_size, out_size)
    fscale = float(in_size) / out_size
    sup, fsup = int(RR.SUPPORT[name]) * max(scale, 1), RR.SUPPORT[name] * max(fscale, 1.0)
    exact, inexact = 0, 0
    for xx in range(out_size):
        c, fc = (xx + Fraction(1, 2)) * scale, (xx + 0.5) * fscale
        for e, f in ((c - sup + Fraction(1, 2), fc - fsup + 0.5), (c + sup + Fraction(1, 2), fc + fsup + 0.5)):
            if e.denominator == 1 and 0 < e < in_size:
                exact += 1
                inexact += f != float(e)
    return exact, inexact


def test_ties_have_boundaries_decided_in_the_last_place():
    for name in RR.FILTERS:
        for s in (288, 352, 480):
            exact, inexact = _integer_boundaries(s, 224, name)
            assert exact >= 1 and inexact >= 1, (s, name, exact, inexact)
        for s in (96, 160):  # integer boundaries whose double value is the integer: the control
            exact, inexact = _integer_boundaries(s, 224, name)
            assert exact >= 1 and inexact == 0, (s, name, exact, inexact)


def test_sweep_reaches_every_branch():
    for geom in (0, 1):
        plans = {(w, h): RR.plan(w, h, geom) for w, h in RR.SWEEP_PAIRS}
        assert all(p is not None for p in plans.values())
        needs = {(p[4], p[5]) for p in plans.values()}
        # CLIP scales both axes by 224 / short: one pass alone cannot occur there (a short side of 224 leaves both
        # sizes unchanged, any other changes both); the squash reaches all four
        assert needs == ({(0, 0), (0, 1), (1, 0), (1, 1)} if geom == 0 else {(0, 0), (1, 1)}), (geom, needs)
        assert any(w < p[8] and p[4] for (w, h), p in plans.items()), geom  # a source narrower than the taps
        assert any(h < p[9] and p[5] for (w, h), p in plans.items()), geom
        if geom == 1:
            for axis in (0, 1):  # odd and even crop differences, in both orientations
                diffs = {(p[axis] - 224) % 2 for p in plans.values() if p[axis] > 224}
                assert diffs == {0, 1}, (axis, diffs)
                assert any(p[2 + axis] > 0 and p[4 + axis] == 0 for p in plans.values()), axis  # crop without a pass


def test_tall_reaches_the_vertical_first_order():
    """Image.resize's order of the passes: TALL holds, per geometry, sizes on both sides of each of its two
    conditions (height > 100 * width; the height shrinks), and SWEEP reaches the order in the squash."""
    first = {(w, h, g): RR.plan(w, h, g)[11] > 0 for w, h in RR.TALL for g in (0, 1) if RR.plan(w, h, g)}
    assert first[(5, 501, 0)] and not first[(5, 500, 0)] and not first[(2, 223, 0)] and first[(2, 225, 0)]
    assert first[(225, 22501, 1)] and not first[(225, 22500, 1)] and not first[(5, 501, 1)]
    assert RR.plan(224, 22500, 1)[4:6] == (0, 0) and not first[(224, 22500, 1)]  # no pass: the order is moot
    assert sum(RR.plan(w, h, 0)[11] > 0 for w, h in RR.SWEEP_PAIRS) >= 10
    for (w, h, g), f in first.items():
        p = RR.plan(w, h, g)
        assert f == (R.vertical_first(w, h, p[1]) and p[4] == 1), (w, h, g)
        if f:
            bh, _ = RR.window_coeffs(w, p[0], p[2], RR.FILTERS[g])
            assert (p[10], p[11]) == (bh[0][0], bh[223][0] + bh[223][1]), (w, h, g)


def test_budget_reaches_95_taps():
    assert RR.plan(5264, 5264, 1)[8:10] == (95, 95)     # bicubic, horizontal (and vertical)
    assert RR.plan(10528, 200, 0)[8] == 95              # bilinear, horizontal
    assert RR.plan(200, 10528, 0)[9] == 95              # bilinear, vertical
    assert RR.KMAX == 96 and math.ceil(2.0 * 5265 / 224) * 2 + 1 == 97 and math.ceil(10529 / 224) * 2 + 1 == 97


def test_checkers_reach_both_clamps_of_both_passes():
    for content, (w, h) in (("checker2", (100, 100)), ("checker1", (96, 96)), ("checker2", (288, 288))):
        accs = {}
        RR.window(RR.CONTENT[content](w, h), 1, accs)
        for k in ("h", "v"):
            v = accs[k] >> RR.PRECISION_BITS
            assert (v < 0).any() and (v > 255).any(), (content, w, h, k, int(v.min()), int(v.max()))
