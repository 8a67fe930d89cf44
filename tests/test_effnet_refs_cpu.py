"""The float64 references and derived bounds of tests/effnet_refs.py, checked without a GPU: for every
case of tests/test_gpu_effnet_kernels.py a float32 torch emulation of the op stays within HALF of each
bound, and the stated caps hold for the chosen inputs.  The tolerances the GPU tests apply are thereby
facts about the references and the number formats, not about what a kernel returned."""
import pytest
import torch

from tests import effnet_refs as R

B = 2


def _half_of(err, tol):
    return float((err / tol).max()) <= 0.5


def _check_dw(x, w, b, k, stride):
    ref = R.dw_ref(x, w, b, k, stride)
    out, pool = R.dw_emulate(x, w, b, k, stride)
    assert out.shape == ref["out"].shape and pool.shape == ref["pool"].shape
    assert _half_of((out.double() - ref["out"]).abs(), ref["tol"])
    assert _half_of((pool.double() - ref["pool"]).abs(), ref["pool_tol"])
    return ref


@pytest.mark.parametrize("k,stride,H,W,C", [r[:5] for r in R.DW_ROWS] + R.DW_EDGES)
def test_dw_emulation_within_half_bound(k, stride, H, W, C):
    _check_dw(*R.dw_inputs(B, H, W, C, k), k, stride)


def test_dw_geometry_of_the_rows():
    """Each table row selects the compile-time kernel it is listed for (flags bit 0), the runtime-geometry
    kernel of the same tile without it, and has more than one tile and more than one channel group."""
    for k, s, H, W, C, bit3, key in R.DW_ROWS:
        assert R.dw_selected(H, W, C, k, s, 1 | bit3) == ("ct", key)
        assert R.dw_selected(H, W, C, k, s, bit3) == ("rt", key)
        T, cw, n = R.dw_geometry(H, W, C, s, bool(bit3))
        assert n > 1 and C // cw > 1
    assert {key for *_, key in R.DW_ROWS} == R.DW_CT
    for k, s, H, W, C in R.DW_EDGES:
        assert R.dw_selected(H, W, C, k, s, 0)[0] == "rt"
    assert R.dw_geometry(17, 17, 64, 1) == (1, 32, 289)
    for k, s, ks, T, cin, C, H in R.EDW_ROWS:
        assert (k, s, (cin + 31) // 32, R.tile_edge(R.out_size(H, s), s)) == (k, s, ks, T) and (k, s, ks, T) in R.EDW_CT
    assert {r[:4] for r in R.EDW_ROWS} == R.EDW_CT


def test_dw_pool_bound_sees_a_dropped_pixel():
    """A pool partial that misses its tile's largest output is far outside the bound."""
    k, s, H, W, C = 5, 1, 28, 28, 96
    x, w, b = R.dw_inputs(B, H, W, C, k)
    ref = R.dw_ref(x, w, b, k, s)
    T = ref["T"]
    biggest = ref["out"].abs().view(B, H // T, T, W // T, T, C).amax((2, 4)).reshape(B, -1, C)
    assert biggest.shape == ref["pool_tol"].shape
    assert float((biggest / ref["pool_tol"]).min()) > 100


@pytest.mark.parametrize("k,stride,ks,T,cin,C,H", R.EDW_ROWS)
def test_expand_dw_emulation_within_half_bound(k, stride, ks, T, cin, C, H):
    x, we, be, w, b = R.edw_inputs(B, H, cin, C, k)
    _check_dw(R.expand_emulate(x, we, be), w, b, k, stride)


def test_expand_dw_walk_case_emulation_within_half_bound():
    c = R.EDW_WALK
    x, we, be, w, b = R.edw_inputs(c["distinct"], c["H"], c["cin"], c["C"], c["k"])
    _check_dw(R.expand_emulate(x[list(c["checked"])], we, be), w, b, c["k"], c["stride"])


@pytest.mark.parametrize("C,Csq", R.SE_SHAPES)
def test_se_emulation_within_half_bound(C, Csq):
    for n in R.SE_NCHUNKS:
        args = R.se_inputs(3, n, C, Csq)
        ref, tol = R.se_ref(*args)
        assert float(args[0][-1].abs().max()) == 0  # the all-zero image
        assert _half_of((R.se_emulate(*args).double() - ref).abs(), tol)
        # the worst-case bound still separates a structural error from rounding: a dropped last chunk or a
        # dropped last squeeze channel (the unrolled loops' tails) moves the median scale by > 5 bounds
        part, inv_hw, w1, b1, w2t, b2 = args
        if n > 1:
            cut = part.clone()
            cut[:, -1] = 0
            assert float(((R.se_ref(cut, inv_hw, w1, b1, w2t, b2)[0] - ref).abs() / tol)[:-1].median()) > 5
        cut = w2t.clone()
        cut[-1] = 0
        assert float(((R.se_ref(part, inv_hw, w1, b1, cut, b2)[0] - ref).abs() / tol).median()) > 5


@pytest.mark.parametrize("HW,C", R.GAP_SHAPES)
def test_gap_classifier_emulation_within_half_bound(HW, C):
    x, w, b = R.gap_inputs(3, HW, C)
    logits, tol_l, score, tol_s = R.gap_ref(x, w, b)
    el, es = R.gap_emulate(x, w, b)
    assert _half_of((el.double() - logits).abs(), tol_l)
    assert _half_of((es.double() - score).abs(), tol_s)
    if HW > 1:  # a missed last pixel (the unrolled loop's tail) is far outside the worst-case bound
        cut = x.clone()
        cut[:, -1] = 0
        cl, _, cs, _ = R.gap_ref(cut, w, b)
        assert float(((cl - logits).abs() / tol_l).max()) > 20 and float(((cs - score).abs() / tol_s).max()) > 20


@pytest.fixture(scope="module")
def stem_case():
    img = R.stem_images()
    return img, R.normalise_f32(img), R.stem_inputs(), R.stem_inputs(tame=True)


@pytest.mark.parametrize("f32", [False, True])
def test_stem_emulation_within_half_bound(stem_case, f32):
    img, xf, (ws, bs, wd, bd), _ = stem_case
    a = (None, xf) if f32 else (img, None)
    ref, e = R.stem_ref(*a, ws, bs)
    emu = R.stem_emulate(*a, ws, bs)
    assert _half_of((emu.double() - ref).abs(), e)                           # before the fp16 store
    assert _half_of((emu.half().double() - ref).abs(), R.stem_tol(ref, e))   # the stored value


@pytest.mark.parametrize("f32", [False, True])
def test_stem_dw_emulation_and_ambiguity_cap(stem_case, f32):
    """The fused kernel's reference chain.  An ambiguous tap flips by a whole fp16 ulp or not at all, so the
    emulation is held to half of the depthwise bound plus the full allowance of its ambiguous taps."""
    img, xf, _, (ws, bs, wd, bd) = stem_case
    a = (None, xf) if f32 else (img, None)
    ref = R.stem_dw_ref(*a, ws, bs, wd, bd)
    print("ambiguous outputs: %.3f" % ref["ambiguous"])
    assert 0 < ref["ambiguous"] <= R.AMBIGUOUS_CAP
    s16 = R.stem_emulate(*a, ws, bs).half()
    out, pool = R.dw_emulate(s16, wd, bd, 3, 1)
    assert ref["T"] == 16 and pool.shape == ref["pool"].shape == (2, 49, 32)
    extra = ref["tol"] - (2.0 ** -10 * ref["out"].abs() + 2.0 ** -18 * ref["S"] + 2.0 ** -24)
    assert float(((out.double() - ref["out"]).abs() / (0.5 * (ref["tol"] - extra) + extra)).max()) <= 1.0
    pextra = R.tile_sums(extra, 16)
    assert float(((pool.double() - ref["pool"]).abs() / (0.5 * (ref["pool_tol"] - pextra) + pextra)).max()) <= 1.0
    # outputs without an ambiguous tap carry the plain depthwise bound
    clear = extra == 0
    assert float(((out.double() - ref["out"]).abs() / ref["tol"])[clear].max()) <= 0.5
