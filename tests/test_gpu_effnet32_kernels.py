"""Per-kernel numerics of the fp32 EfficientNet tower's kernels (csrc/effnet_f32.hip, stem_kernel<*, float>)
on a real MI355X, through the test-only entry points of include/mmf_hip.h, against the float64 references,
derived bounds and exact cases of tests/effnet32_refs.py (certified without a GPU by
tests/test_effnet32_refs_cpu.py).  Every output element of every case is compared.  Output buffers start
as NaN with a canary band behind them, and the input operands have NaN behind them: an element a kernel
does not write, a write past the end, or a read past an operand's end that reaches a result all fail."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import effnet_refs as R
from tests import effnet32_refs as R32

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 4096  # floats behind every buffer: canary (outputs, must stay NaN) or NaN guard (inputs)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    return hip.load()


def _g(t):
    """The tensor on the device with GUARD NaNs behind it (same dtype for floats; uint8 gets 255s)."""
    if t is None:
        return None
    flat = t.contiguous().view(-1)
    buf = torch.full((flat.numel() + GUARD,), float("nan") if t.dtype.is_floating_point else 255, dtype=t.dtype,
                     device="cuda")
    buf[:flat.numel()] = flat.cuda()
    return buf


def _p(buf):
    return None if buf is None else buf.data_ptr()


def _nan(n):
    return torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)


def _canary_ok(*bufs):
    return all(bool(torch.isnan(b[-GUARD:]).all()) for b in bufs)


def _close(got, ref, tol, what):
    """Every element within its bound (NaN fails); prints the worst error / bound ratio first."""
    err = (got.double().cpu() - ref).abs()
    ratio = (err / tol)[tol > 0]
    print(f"{what}: max err / bound = {float(ratio.max()) if ratio.numel() else 0:.3f}")
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {float((err / tol)[bad].nan_to_num(float('inf')).max()):.3g} x"


# ---- pw32 ----
def _variant(lib, M, N, K, mode):
    o = (ctypes.c_int32 * 3)()
    kind = lib.mmf_pw32_variant(M, N, K, mode, o)
    return (kind, o[0], o[1])


def _pw_run(lib, dev, M, N, K, act, rpi, mode):
    import mmf_amd.hip as hip
    C = _nan(M * N)
    hip.check(lib.mmf_pw32_f32(_p(dev["A"]), _p(dev["W"]), _p(dev["b"]), _p(dev["s"]), rpi, _p(dev["res"]), C.data_ptr(),
                               M, N, K, act, mode, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _canary_ok(C), f"mode {mode}: wrote past the end of C"
    return C[:-GUARD].view(M, N)


def _pw_case(lib, M, N, K, form, expect, kinds):
    for mode, want in expect.items():
        assert _variant(lib, M, N, K, mode) == want, f"mode {mode}"
    assert _variant(lib, M, N, K, 0) == (R32.VALU, 0, 0)
    for kind in kinds:
        c = R32.pw_inputs(M, N, K, form, kind)
        ref, tol, _, _ = R32.pw_ref(**c, kind=kind)
        dev = {n: _g(c[n]) for n in ("A", "W", "b", "s", "res")}
        base = _pw_run(lib, dev, M, N, K, c["act"], c["rpi"], 0)
        if kind == "dyadic" and c["act"] == R32.ACT_NONE:
            assert float(tol.max()) == 0
            assert torch.equal(base.cpu(), ref.float()) and torch.equal(ref.float().double(), ref), f"{kind}: not exact"
        else:
            _close(base, ref, tol, f"pw32 {form} {kind}")
        for mode in range(1, 6):
            got = _pw_run(lib, dev, M, N, K, c["act"], c["rpi"], mode)
            assert torch.equal(got, base), f"{kind}: mode {mode} {_variant(lib, M, N, K, mode)} differs from mode 0"


@pytest.mark.parametrize("M,N,K,form,expect", R32.PW_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_pw32_vs_fp64_and_modes_bit_identical(lib, M, N, K, form, expect):
    """Dyadic inputs: equal to the float64 reference (act none) or within the SiLU's evaluation error; real
    inputs within the derived bound; every pw32_mfma mode bit-identical to mode 0 (the documented claim, per
    element); the kernel each listed mode reaches is what the table says."""
    _pw_case(lib, M, N, K, form, expect, ("dyadic", "real"))


@pytest.mark.parametrize("M,N,K,form,expect", R32.PW_BIG, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_pw32_thresholds_large(lib, M, N, K, form, expect):
    """The mode-2 workgroup threshold and the mode-5 row-block thresholds, at the smallest shapes on each side."""
    _pw_case(lib, M, N, K, form, expect, ("dyadic",))


def test_pw32_rejects_unsupported(lib):
    M, N, K = 66, 40, 24
    c = R32.pw_inputs(M, N, K, "project", "dyadic")
    dev = {n: _g(c[n]) for n in ("A", "W", "b", "s", "res")}
    C = _nan(M * N)
    A, W, b, s, res = (_p(dev[n]) for n in ("A", "W", "b", "s", "res"))

    def call(A=A, W=W, b=b, s=s, rpi=R32.RPI, res=res, Cp=C.data_ptr(), M=M, N=N, K=K, act=0, mode=4):
        return lib.mmf_pw32_f32(A, W, b, s, rpi, res, Cp, M, N, K, act, mode, None)

    assert call(N=38) == EINVAL and lib.mmf_last_error()
    for kw in (dict(K=22), dict(act=1), dict(rpi=0), dict(M=0), dict(mode=6), dict(mode=-1), dict(A=None), dict(W=None),
               dict(b=None), dict(Cp=None), dict(A=A + 4), dict(Cp=C.data_ptr() + 8), dict(N=0), dict(K=0)):
        assert call(**kw) == EINVAL, kw
    for mode in range(6):
        assert lib.mmf_pw32_variant(M, 38, K, mode, None) == EINVAL
    assert lib.mmf_pw32_variant(M, N, K, 6, None) == EINVAL and lib.mmf_pw32_variant(0, N, K, 4, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all())
    assert call() == 0 and call(s=None) == 0 and call(res=None) == 0  # the optional operands
    torch.cuda.synchronize()


# ---- dw32 ----
def _dw32(lib, xd, wd, bd, B, H, W, C, k, stride):
    import mmf_amd.hip as hip
    ho, wo = R.out_size(H, stride), R.out_size(W, stride)
    out = _nan(B * ho * wo * C)
    hip.check(lib.mmf_dw32_f32(_p(xd), _p(wd), _p(bd), out.data_ptr(), B, H, W, C, k, stride, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _canary_ok(out), "wrote past the end"
    return out[:-GUARD].view(B, ho, wo, C)


@pytest.mark.parametrize("H,W", R32.DW32_HW)
@pytest.mark.parametrize("k,stride", R32.DW32_KS)
def test_dw32_vs_fp64(lib, k, stride, H, W):
    B = R32.DW32_B
    for C in R32.DW32_C:
        for kind in ("dyadic", "real"):
            x, w, b = R32.dw32_inputs(B, H, W, C, k, kind)
            ref, tol = R32.dw32_ref(x, w, b, k, stride, kind)
            out = _dw32(lib, _g(x), _g(R32.tap_major(w)), _g(b), B, H, W, C, k, stride)
            _close(out, ref, tol, f"dw32 {kind}")


def test_dw32_rejects_unsupported(lib):
    B, H, W, C, k = 2, 6, 6, 8, 3
    x, w, b = R32.dw32_inputs(B, H, W, C, k, "real")
    xd, wd, bd = _g(x), _g(R32.tap_major(w)), _g(b)
    out = _nan(B * H * W * C)
    o = out.data_ptr()
    args = lambda **kw: {**dict(x=_p(xd), w=_p(wd), b=_p(bd), o=o, B=B, H=H, W=W, C=C, k=k, s=1), **kw}
    for kw in (dict(C=6), dict(k=7), dict(s=3), dict(s=0), dict(x=None), dict(w=None), dict(b=None), dict(o=None),
               dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(o=o + 4), dict(B=65536, H=65536, W=4)):
        a = args(**kw)
        assert lib.mmf_dw32_f32(a["x"], a["w"], a["b"], a["o"], a["B"], a["H"], a["W"], a["C"], a["k"], a["s"], None) == EINVAL, kw
        assert lib.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- sum32 ----
@pytest.mark.parametrize("HW,n", R32.SUM32_HW_N)
def test_sum32_bit_exact_fixed_order(lib, HW, n):
    """The documented summation order, emulated in numpy float32: bit for bit."""
    import mmf_amd.hip as hip
    B = R32.SUM32_B
    for C in R32.SUM32_C:
        x = R32.sum32_inputs(B, HW, C)
        part, xd = _nan(B * n * C), _g(x)
        hip.check(lib.mmf_sum32_f32(_p(xd), B, HW, C, n, part.data_ptr(), hip.stream_ptr()))
        torch.cuda.synchronize()
        assert _canary_ok(part), "wrote past the end"
        got = part[:-GUARD].view(B, n, C).cpu()
        ref, tol = R32.sum32_ref(x, n)
        _close(got, ref, tol + 1e-300, "sum32 float64 bound")
        emu = R32.sum32_emulate(x, n)
        assert torch.equal(got.view(torch.int32), emu.view(torch.int32)), \
            f"C {C}: {int((got != emu).sum())} of {emu.numel()} partials differ from the documented order"


def test_sum32_rejects_unsupported(lib):
    B, HW, C = 2, 8, 16
    xd = _g(R32.sum32_inputs(B, HW, 32))
    part = _nan(B * HW * 32)
    for hw, c, n in ((HW, C, 0), (HW, C, -1), (HW, C, HW + 1), (HW, 24, 2), (HW, 0, 2), (0, C, 1)):
        assert lib.mmf_sum32_f32(_p(xd), B, hw, c, n, part.data_ptr(), None) == EINVAL, (hw, c, n)
        assert lib.mmf_last_error()
    assert lib.mmf_sum32_f32(None, B, HW, C, 2, part.data_ptr(), None) == EINVAL
    assert lib.mmf_sum32_f32(_p(xd), B, HW, C, 2, None, None) == EINVAL
    assert lib.mmf_sum32_f32(_p(xd), 0, HW, C, 2, part.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all())


# ---- gap32 ----
def _gap32(lib, xd, wd, bd, B, HW, C, want_l, want_s, stride):
    import mmf_amd.hip as hip
    gl, gs = _nan(B * 2), _nan(B * stride)
    hip.check(lib.mmf_gap32_f32(_p(xd), HW, C, _p(wd), _p(bd), gl.data_ptr() if want_l else None,
                                gs.data_ptr() if want_s else None, stride, B, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _canary_ok(gl, gs)
    if not want_l:
        assert bool(torch.isnan(gl).all())
    if not want_s:
        assert bool(torch.isnan(gs).all())
    got_s = gs[:-GUARD].view(B, stride)
    assert bool(torch.isnan(got_s[:, 1:]).all()), "wrote between the strided scores"
    return gl[:-GUARD].view(B, 2), got_s[:, 0]


@pytest.mark.parametrize("HW,C", R.GAP_SHAPES)
def test_gap32_vs_fp64(lib, HW, C):
    B = 3
    x, w, b = R32.gap32_inputs(B, HW, C)
    logits, tol_l, score, tol_s = R.gap_ref(x, w, b)
    xd, wd, bd = _g(x), _g(w), _g(b)
    for want_l, want_s, stride in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 5), (0, 1, 5)):
        gl, gs = _gap32(lib, xd, wd, bd, B, HW, C, want_l, want_s, stride)
        if want_l:
            _close(gl, logits, tol_l, "gap32 logits")
        if want_s:
            _close(gs, score, tol_s, "gap32 score")


def test_gap32_exact_case(lib):
    """Dyadic x and w at HW = 8, C = 64: every mean, product and partial sum is representable, so the logits
    equal the float64 reference whatever wave_sum's order is."""
    B = 3
    HW, C = R32.GAP32_EXACT
    x, w, b = R32.gap32_inputs(B, HW, C, "dyadic")
    logits, _, score, tol_s = R.gap_ref(x, w, b)
    gl, gs = _gap32(lib, _g(x), _g(w), _g(b), B, HW, C, 1, 1, 5)
    assert torch.equal(gl.cpu().double(), logits)
    _close(gs, score, tol_s, "gap32 exact-case score")


def test_gap32_rejects_unsupported(lib):
    B, HW, C = 2, 4, 16
    x, w, b = R32.gap32_inputs(B, HW, C)
    xd, wd, bd = _g(x), _g(w), _g(b)
    gl, gs = _nan(B * 2), _nan(B)
    L, S = gl.data_ptr(), gs.data_ptr()
    for a in ((_p(xd), HW, C, _p(wd), _p(bd), None, None, 1, B), (_p(xd), HW, C, _p(wd), _p(bd), L, S, 0, B),
              (_p(xd), HW, C, _p(wd), _p(bd), L, S, -1, B), (_p(xd), 0, C, _p(wd), _p(bd), L, S, 1, B),
              (_p(xd), HW, 0, _p(wd), _p(bd), L, S, 1, B), (_p(xd), HW, C, _p(wd), _p(bd), L, S, 1, 0),
              (None, HW, C, _p(wd), _p(bd), L, S, 1, B), (_p(xd), HW, C, None, _p(bd), L, S, 1, B),
              (_p(xd), HW, C, _p(wd), None, L, S, 1, B)):
        assert lib.mmf_gap32_f32(*a, None) == EINVAL, a
        assert lib.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(gl).all()) and bool(torch.isnan(gs).all())


# ---- stem32 ----
@pytest.fixture(scope="module")
def stem_case():
    img = R.stem_images()
    return img, R.normalise_f32(img)


def _stem32(lib, img, xf, ws, bs):
    import mmf_amd.hip as hip
    src, wd, bd = _g(xf if img is None else img), _g(ws), _g(bs)
    out = _nan(2 * 112 * 112 * 32)
    hip.check(lib.mmf_effnet_stem32_f32(None if img is None else _p(src), _p(src) if img is None else None, _p(wd),
                                        _p(bd), out.data_ptr(), 2, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _canary_ok(out)
    return out[:-GUARD].view(2, 112, 112, 32)


def test_stem32_f32_input_vs_fp64(lib, stem_case):
    """The bound is stem_ref's e (the value before the fp16 tower's store); on dyadic operands the
    pre-activation is exact and the SiLU's evaluation error is all there is."""
    _, xf = stem_case
    ws, bs, _, _ = R.stem_inputs()
    ref, e = R.stem_ref(None, xf, ws, bs)
    _close(_stem32(lib, None, xf, ws, bs), ref, e, "stem32 f32 input")
    xd, wd, bd = R32.stem32_dyadic_inputs()
    ref, _ = R.stem_ref(None, xd, wd, bd)
    _close(_stem32(lib, None, xd, wd, bd), ref, R.act_err(ref), "stem32 dyadic")


def test_stem32_u8_input_vs_fp64(lib, stem_case):
    """uint8 pixels: ((u / 255 - mean) / std) with two IEEE divisions, under the e_v derived for that form
    (effnet32_refs.stem32_u8_ref).  With the pass-through weights the output is PASS_GAIN v bit for bit
    wherever that is >= PASS_MIN (and 0 in the padding), v the fp32 value of exactly that expression: one ulp
    of the normalisation shows, which the one-FMA form of the fp16 tower would not match."""
    img, _ = stem_case
    ws, bs, _, _ = R.stem_inputs()
    ref, e = R32.stem32_u8_ref(img, ws, bs)
    _close(_stem32(lib, img, None, ws, bs), ref, e, "stem32 u8 input")
    wp, bp = R32.stem32_passthrough_weights()
    pre, exact = R32.stem32_passthrough_ref(R32.stem32_norm_f32(img), wp)
    got = _stem32(lib, img, None, wp, bp).cpu().double()
    assert torch.equal(got[exact], pre[exact]), f"{int((got[exact] != pre[exact]).sum())} of {int(exact.sum())} pass-through elements differ"
    _close(got, F.silu(pre), R.act_err(F.silu(pre)), "stem32 pass-through")


def test_stem32_rejects_unsupported(lib, stem_case):
    img, xf = stem_case
    ws, bs, _, _ = R.stem_inputs()
    a, b, wd, bd = _g(img), _g(xf), _g(ws), _g(bs)
    out = _nan(2 * 112 * 112 * 32)
    o = out.data_ptr()
    for args in ((None, None, _p(wd), _p(bd), o, 2), (_p(a), _p(b), _p(wd), _p(bd), o, 2), (_p(a), None, None, _p(bd), o, 2),
                 (_p(a), None, _p(wd), None, o, 2), (_p(a), None, _p(wd), _p(bd), None, 2), (_p(a), None, _p(wd), _p(bd), o, 0),
                 (_p(a), None, _p(wd), _p(bd), o + 4, 2)):
        assert lib.mmf_effnet_stem32_f32(*args, None) == EINVAL, args
        assert lib.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
