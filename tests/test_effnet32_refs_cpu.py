"""The references, bounds and exactness claims of tests/effnet32_refs.py, checked without a GPU: for every
case of tests/test_gpu_effnet32_kernels.py a float32 emulation stays within HALF of each derived bound (or
equals the float64 reference where the case is exact), the dispatch tables reach every kernel instantiation,
and a planted defect puts more than half of the elements it affects outside the bound, or breaks equality
in an exact case."""
import numpy as np
import pytest
import torch

from tests import effnet_refs as R
from tests import effnet32_refs as R32


def _ratio(got, ref, tol):
    return (got.double() - ref).abs() / tol


def _half_of(got, ref, tol):
    return float(_ratio(got, ref, tol).max()) <= 0.5


def _half_tol(tol, e_res):
    """Half of a bound, except its final add's half-ulp (e_res), which one rounding can use up whole."""
    return 0.5 * (tol - e_res) + e_res


def _mostly_outside(got, ref, tol, affected=None):
    bad = (got.double() - ref).abs() > tol
    if affected is not None:
        bad = bad[affected]
    return float(bad.double().mean()) > 0.5


# ---- pw32 ----
def test_pw_tables_reach_every_instantiation():
    reached = set()
    for *_, expect in R32.PW_CASES + R32.PW_BIG:
        reached |= set(expect.values())
    assert (R32.VALU, 0, 0) in reached and (R32.MFMA, 2, 0) in reached and (R32.MFMA, 4, 0) in reached
    assert {(nf, d) for kind, d, nf in reached if kind == R32.ROWS} == {(nf, d) for nf in range(1, 17) for d in (2, 4)}
    # (a): both widths of every NF in both forms; N in (240, 256] is the 64 KB LDS launch
    a = [(N, K, e[4]) for M, N, K, form, e in R32.PW_CASES if M == 130 and K in (24, 72) and 4 in e and len(e) == 1]
    assert {(N, K) for N, K, _ in a} == {(N, K) for nf in range(1, 17) for N in (16 * nf - 12, 16 * nf) for K in (24, 72)}
    assert all(v == (R32.ROWS, 2 if K == 24 else 4, -(-N // 16)) for N, K, v in a)
    # every form meets every kernel family
    for kind in (R32.VALU, R32.MFMA, R32.ROWS):
        assert {form for *_, form, e in R32.PW_CASES if kind in {v[0] for v in e.values()}} >= {"expand", "project"}
    # the mode-5 thresholds: 512 and 1024 row blocks with a last block of one row, and 511
    assert [(-(-M // 64), M % 64) for M, *_ in R32.PW_BIG[1:]] == [(512, 1), (512, 1), (1024, 1), (511, 1)]
    assert -(-4096 // 64) * -(-1024 // 64) == 4 * 256


@pytest.mark.parametrize("K", [4, 24, 72, 1152])
@pytest.mark.parametrize("form", list(R32.FORMS))
def test_pw_dyadic_grid_is_exact_in_both_orders(K, form):
    """Ascending and descending k in float32 both equal the float64 reference (act none: bit for bit; SiLU: the
    pre-activation does, checked through act none on the same operands), and max |partial| 2^8 < 2^24."""
    M, N = 130, 40
    c = R32.pw_inputs(M, N, K, form, "dyadic")
    lin = dict(c, act=R32.ACT_NONE)
    ref, tol, _, _ = R32.pw_ref(**lin, kind="dyadic")
    assert float(tol.max()) == 0
    for order in ("asc", "desc"):
        got, big = R32.pw_emulate(**lin, order=order)
        assert big * 2 ** 8 < 2 ** 24
        assert torch.equal(got.double(), ref)
    if c["act"] == R32.ACT_SILU:
        ref, tol, pre, e_res = R32.pw_ref(**c, kind="dyadic")
        got, _ = R32.pw_emulate(**c)
        r = _ratio(got, ref, _half_tol(tol, e_res))
        print(f"K {K} {form}: |pre| up to {float(pre.abs().max()):.1f}, SiLU error / act_err = {float(r.max()):.2f}")
        assert float(r.max()) <= 1.0


@pytest.mark.parametrize("M,N,K,form", sorted({c[:4] for c in R32.PW_CASES}))
def test_pw_emulation_within_half_bound(M, N, K, form):
    for kind in ("dyadic", "real"):
        c = R32.pw_inputs(M, N, K, form, kind)
        ref, tol, _, e_res = R32.pw_ref(**c, kind=kind)
        got = R32.pw_emulate_fast(**c)
        if kind == "dyadic" and c["act"] == R32.ACT_NONE:
            assert torch.equal(got.double(), ref)
        else:
            assert float(_ratio(got, ref, _half_tol(tol, e_res)).max()) <= 1.0


def test_pw_big_cases_are_exact():
    M, N, K, form, _ = R32.PW_BIG[1]
    c = R32.pw_inputs(M, N, K, form, "dyadic")
    ref, tol, _, _ = R32.pw_ref(**c, kind="dyadic")
    assert float(tol.max()) == 0 and torch.equal(R32.pw_emulate_fast(**c).double(), ref)
    assert all(FORM == "project" for *_, FORM, _ in R32.PW_BIG)


@pytest.mark.parametrize("kind", ["dyadic", "real"])
@pytest.mark.parametrize("K,form", [(24, "expand"), (72, "project"), (64, "full")])
def test_pw_planted_defects(K, form, kind):
    M, N = 130, 52
    c = R32.pw_inputs(M, N, K, form, kind)
    ref, tol, _, e_res = R32.pw_ref(**c, kind=kind)
    exact = kind == "dyadic" and c["act"] == R32.ACT_NONE

    def caught(got, affected=None):
        if exact:
            ne = got.double() != ref
            return float((ne[affected] if affected is not None else ne).double().mean()) > 0.5
        return _mostly_outside(got, ref, tol, affected)

    good, _ = R32.pw_emulate(**c)
    assert torch.equal(good.double(), ref) if exact else float(_ratio(good, ref, _half_tol(tol, e_res)).max()) <= 1.0
    assert caught(R32.pw_emulate(**c, drop_last_quad=True)[0])
    if c["s"] is not None:
        rows = torch.arange(M)
        second = (rows // c["rpi"]) != ((rows // 64 * 64) // c["rpi"])
        assert 0 < int(second.sum()) < M
        assert caught(R32.pw_emulate(**c, neighbour_scale=True)[0], second)
    if form == "full":  # behind a SiLU the residual's place matters
        assert caught(R32.pw_emulate(**c, res_first=True)[0])


# ---- dw32 ----
@pytest.mark.parametrize("H,W", R32.DW32_HW)
@pytest.mark.parametrize("k,stride", R32.DW32_KS)
def test_dw32_emulation_and_defects(k, stride, H, W):
    for C in R32.DW32_C:
        for kind in ("dyadic", "real"):
            x, w, b = R32.dw32_inputs(R32.DW32_B, H, W, C, k, kind)
            ref, tol = R32.dw32_ref(x, w, b, k, stride, kind)
            assert ref.shape == (R32.DW32_B, R.out_size(H, stride), R.out_size(W, stride), C)
            assert _half_of(R32.dw32_emulate(x, w, b, k, stride), ref, tol)
            if (H, W) == (1, 1):
                continue  # one tap: no layout or edge to get wrong
            # [C][k*k] weights read as tap-major [k*k][C]
            mixed = w.contiguous().view(k * k, C).T.contiguous()
            assert _mostly_outside(R32.dw32_emulate(x, mixed, b, k, stride), ref, tol)
            # the tap on the image's last column dropped: the outputs whose window holds that column
            cut = x.clone()
            cut[:, :, -1] = 0
            wo = ref.shape[2]
            reach = torch.tensor([ox * stride + (k - 1) // 2 >= W - 1 for ox in range(wo)])
            assert bool(reach.any())
            assert _mostly_outside(R32.dw32_emulate(cut, w, b, k, stride), ref, tol, (slice(None), slice(None), reach))


def test_dw32_dyadic_preactivation_is_exact():
    """25 products (multiples of 2^-6 up to 2) and the bias: every partial sum < 2^12 units."""
    assert (25 * 2 + 2) * 2 ** 6 < 2 ** 24


# ---- sum32 ----
@pytest.mark.parametrize("HW,n", R32.SUM32_HW_N)
def test_sum32_emulation_and_defects(HW, n):
    slots = set()
    for C in R32.SUM32_C:
        x = R32.sum32_inputs(R32.SUM32_B, HW, C)
        ref, tol = R32.sum32_ref(x, n)
        emu = R32.sum32_emulate(x, n)
        assert _half_of(emu, ref, tol + 1e-300)
        slots.add((n * R32.sum32_lanes(C)) % 16)
        if HW // n >= 2:  # a chunk one pixel short, a lane stride of 3
            assert _mostly_outside(R32.sum32_emulate(x, n, short=1), ref, tol)
        if HW // n >= 8:
            assert _mostly_outside(R32.sum32_emulate(x, n, lane_stride=3), ref, tol)
            # the other pairing of the lane sums is within the bound and still not the documented result
            other = R32.sum32_emulate(x, n, order="02_13")
            assert _half_of(other, ref, tol)
            assert float((other != emu).double().mean()) > 0.1
    if n in (1, 3, 5, 23, 49):
        assert slots - {0}, "no case leaves idle chunk slots in the last block"


def test_sum32_lane_table():
    assert [R32.sum32_lanes(C) for C in R32.SUM32_C] == [4, 4, 8, 8, 16]


# ---- gap32 ----
@pytest.mark.parametrize("HW,C", R.GAP_SHAPES)
def test_gap32_emulation_within_half_bound(HW, C):
    x, w, b = R32.gap32_inputs(3, HW, C)
    logits, tol_l, score, tol_s = R.gap_ref(x, w, b)
    el, es = R.gap_emulate(x, w, b)
    assert _half_of(el, logits, tol_l) and _half_of(es, score, tol_s)
    # inv taken over HW + 1
    m = x.float().sum(1) * np.float32(1.0 / (HW + 1))
    assert _mostly_outside(m @ w.T + b, logits, tol_l)


def test_gap32_exact_case():
    HW, C = R32.GAP32_EXACT
    x, w, b = R32.gap32_inputs(3, HW, C, "dyadic")
    logits, _, score, tol_s = R.gap_ref(x, w, b)
    el, es = R.gap_emulate(x, w, b)
    assert torch.equal(el.double(), logits) and _half_of(es, score, tol_s)
    # any order: channels reversed
    m = x.flip(1).sum(1) * np.float32(1.0 / HW)
    acc = torch.zeros(3, 2)
    for c in reversed(range(C)):
        acc = acc + m[:, c:c + 1] * w[:, c]
    assert torch.equal((acc + b).double(), logits)


# ---- stem32 ----
@pytest.fixture(scope="module")
def stem_case():
    img = R.stem_images()
    return img, R.normalise_f32(img)


def test_stem32_f32_input(stem_case):
    _, xf = stem_case
    ws, bs, _, _ = R.stem_inputs()
    ref, e = R.stem_ref(None, xf, ws, bs)
    assert _half_of(R32.stem32_emulate(xf, ws, bs), ref, e)
    xd, wd, bd = R32.stem32_dyadic_inputs()
    ref, _ = R.stem_ref(None, xd, wd, bd)
    assert (27 * 2 + 2) * 2 ** 6 < 2 ** 24
    assert _half_of(R32.stem32_emulate(xd, wd, bd), ref, R.act_err(ref))


def test_stem32_u8_input_and_the_fma_form(stem_case):
    img, _ = stem_case
    ws, bs, _, _ = R.stem_inputs()
    ref, e = R32.stem32_u8_ref(img, ws, bs)
    v32 = R32.stem32_norm_f32(img)
    assert _half_of(R32.stem32_emulate(v32, ws, bs), ref, e)
    # the frame image keeps the padding check: padding taken as pixel value 0 (normalised -2.1) is far outside
    wrong = torch.nn.functional.conv2d(torch.nn.functional.pad(v32, (1, 1, 1, 1), value=float(v32.min())), ws, bs, 2, 0)
    wrong = torch.from_numpy(R32.silu32(wrong.permute(0, 2, 3, 1).contiguous().numpy()))
    edge = torch.zeros(112, dtype=torch.bool)
    edge[0] = True
    assert _mostly_outside(wrong, ref, e, (slice(None), edge))
    # pass-through weights: the elements that must match bit for bit tell the two normalisations apart
    wp, bp = R32.stem32_passthrough_weights()
    pre, exact = R32.stem32_passthrough_ref(v32, wp)
    emu = R32.stem32_emulate(v32, wp, bp)
    assert 0.2 < float(exact.double().mean()) < 1
    assert torch.equal(emu.double()[exact], pre[exact])
    assert _half_of(emu, torch.nn.functional.silu(pre), R.act_err(torch.nn.functional.silu(pre)))
    fma = R32.stem32_emulate(R32.stem32_norm_fma(img), wp, bp)
    differ = float((fma.double()[exact] != pre[exact]).double().mean())
    print(f"one-FMA normalisation: {differ:.3f} of the exact elements differ")
    assert differ > 0.02
