"""Every base (epilogue 0) fp16 GEMM instantiation on a real MI355X, per element against float64: the
register-staged tiles (configs 0 - 3), the LDS-DMA tiles (5, 10, 11), the persistent walk and its tile orders,
and the streaming 1x1 kernel pw_conv (9), through mmf_gemm_f16_raw (csrc/test_host.cpp).

Every comparison is |got - ref| <= e for an fp32 output and <= store16(ref, e) for an fp16 one, with
(ref, e) = gemm_ref(..., chain = K + 4) computed beside the reference in tests/gemm_refs.py from K and the operand
magnitudes (tests/test_gemm_refs_cpu.py holds a float32 emulation under half of it and planted defects outside it).
Operands sit in NaN-padded buffers with strides of their own (lda = K + 8, ldw = K + 16, ldr = N + 4, ldc = N + 8,
16 NaN rows behind A and W) and outputs start as NaN with a guard row: a read of padding that reaches a result, a
tile that is never written and a write outside [M][N] all fail.  Every forced case asserts the instantiation that
ran (config_out): a forced config that is silently replaced fails, it does not skip."""
import ctypes

import pytest
import torch

from tests import gemm_refs as G
from tests.test_gpu_transformer_kernels import _close, _untouched

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    return hip.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    """Device operands stay alive until the test ends; the process options go back to their defaults."""
    yield
    import mmf_amd.hip as hip
    torch.cuda.synchronize()
    _KEEP.clear()
    hip.set_process_option("gemm_config", -1)
    hip.set_process_option("gemm_group_m", 0)


def _d(t):
    if t is None:
        return None
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(rows, ld, dtype):
    return torch.full((rows + 1, ld), NAN, device="cuda", dtype=dtype)


class Dev:
    """The device operands of one case (uploaded once, shared by its launches)."""

    def __init__(self, c, ops):
        self.c, self.ops = c, ops
        self.A, self.W, self.bias, self.scale = _d(ops.Ap), _d(ops.Wp), _d(ops.biasp), _d(ops.scalep)
        self.res = None if c.inplace else _d(ops.resp)


def _launch(lib, dev, force=-1, group_m=0):
    """One mmf_gemm_f16_raw launch with process options gemm_config = force, gemm_group_m = group_m ->
    (c32 [M + 1][ldc] or None, c16 or None, config_out); the canaries of both outputs are checked."""
    import mmf_amd.hip as hip
    c, ops = dev.c, dev.ops
    c32 = _nan(c.M, ops.ldc, torch.float32) if c.outs in ("c32", "both") else None
    c16 = _nan(c.M, ops.ldc, torch.float16) if c.outs in ("c16", "both") else None
    r32 = r16 = None
    if c.inplace:
        c32[:c.M, :c.N] = ops.res.cuda()
        r32 = c32
    elif c.res == "res32":
        r32 = dev.res
    elif c.res == "res16":
        r16 = dev.res
    out = ctypes.c_int(-7)
    hip.set_process_option("gemm_config", force)
    hip.set_process_option("gemm_group_m", group_m)
    try:
        rc = lib.mmf_gemm_f16_raw(_p(dev.A), ops.lda, _p(dev.W), ops.ldw, _p(dev.bias), _p(r32), _p(r16), ops.ldr,
                                  _p(dev.scale), c.rpb, _p(c32), _p(c16), ops.ldc, c.M, c.N, c.K, c.act,
                                  ctypes.byref(out), hip.stream_ptr())
        hip.check(rc)
        torch.cuda.synchronize()
    finally:
        hip.set_process_option("gemm_config", -1)
        hip.set_process_option("gemm_group_m", 0)
    for buf, what in ((c32, "c32"), (c16, "c16")):
        if buf is not None:
            _untouched(buf, c.M, c.N, what)
    return c32, c16, out.value


def _check(c, ref, e, c32, c16, what):
    if c32 is not None:
        _close(c32[:c.M, :c.N], ref, e, what + " c32")
    if c16 is not None:
        _close(c16[:c.M, :c.N], ref, G.store16(ref, e), what + " c16")


def _same_bits(c, a, b, what):
    """Two launches' outputs bit for bit (fp32 and fp16, the written part; the canaries were checked)."""
    for x, y, bits in ((a[0], b[0], torch.int32), (a[1], b[1], torch.int16)):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x[:c.M, :c.N].contiguous().view(bits), y[:c.M, :c.N].contiguous().view(bits)), f"{what}: not bit-identical"


def _forced_vs_fp64(lib, c):
    ops = G.operands(c)
    ref, e = G.reference(c, ops)
    dev = Dev(c, ops)
    c32, c16, ran = _launch(lib, dev, force=c.cfg)
    assert ran == c.cfg, f"forced gemm_config {c.cfg}, ran {ran}"
    _check(c, ref, e, c32, c16, f"config {c.cfg}")
    return dev, ref, e, (c32, c16)


@pytest.mark.parametrize("c", G.reg_cases(), ids=G.case_id)
def test_register_staged_tiles_vs_fp64(lib, c):
    """Configs 0 - 3 (256x32, 256x64, 64x128, 128x128) around every tile edge, K-loop depths 1 - 4 with and without a
    K tail, every epilogue form, and the SE-scaled (ASC) instantiation."""
    _forced_vs_fp64(lib, c)


@pytest.mark.parametrize("c", G.glds_cases(), ids=G.case_id)
def test_lds_dma_tiles_vs_fp64(lib, c):
    """Configs 5, 10, 11 (256x128, 256x192 PIPE2, 256x256 PIPE2): K-loop depths 1 - 5, N % 8 == 4 (the full8 == false
    stores), a ragged row panel behind a full one, and the in-place fp32 residual as the towers use it."""
    _forced_vs_fp64(lib, c)


@pytest.mark.parametrize("c", G.walk_cases(), ids=G.case_id)
def test_persistent_walk_and_tile_orders(lib, c):
    """288 tiles for 256 workgroups with ragged last panels against float64 in row-major order; every grouped order
    (gemm_group_m, ragged last groups included) bit-identical to it: no tile twice, none skipped."""
    dev, ref, e, base = _forced_vs_fp64(lib, c)
    del ref, e
    for gm in G.WALK_GROUP_M:
        c32, c16, ran = _launch(lib, dev, force=c.cfg, group_m=gm)
        assert ran == c.cfg
        _same_bits(c, (c32, c16), base, f"gemm_group_m {gm}")


@pytest.mark.parametrize("c", G.pw_cases(), ids=G.case_id)
def test_pw_conv_vs_fp64_and_tiled(lib, c):
    """pw_conv (config 9) at every KS x CF template, over two row blocks per workgroup, with the SE scale and the
    fp16 residual: within the float64 bound, and bit-identical to the 128x128 tiled GEMM (config 3) -- the claim of
    pointwise.hip's header."""
    dev, ref, e, pw = _forced_vs_fp64(lib, c)
    c32, c16, ran = _launch(lib, dev, force=3)
    assert ran == 3
    _check(c, ref, e, c32, c16, "config 3")
    _same_bits(c, pw, (c32, c16), "pw_conv against the 128x128 tiles")


# ---- dispatch ----
def _auto(lib, c):
    ops = G.operands(c)
    ref, e = G.reference(c, ops)
    dev = Dev(c, ops)
    c32, c16, ran = _launch(lib, dev)
    _check(c, ref, e, c32, c16, f"automatic config {ran}")
    return dev, (c32, c16), ran


def test_removed_config_numbers_fall_back(lib):
    """Forcing a number whose instantiation was removed gives the automatic choice and its bits."""
    c = G.Case(-1, 300, 136, 72, 1, True, "res16", "both", 0, False)
    dev, base, auto = _auto(lib, c)
    assert auto == 2
    for n in G.REMOVED + (17, 40):
        c32, c16, ran = _launch(lib, dev, force=n)
        assert ran == auto, f"gemm_config {n} ran {ran}"
        _same_bits(c, (c32, c16), base, f"gemm_config {n}")


@pytest.mark.parametrize("c", [G.Case(-1, 600, 136, 72, 0, True, "none", "both", 0, False),      # K % 64 != 0
                               G.Case(-1, 600, 136, 64, 0, True, "none", "both", 49, False)],    # an SE scale
                         ids=G.case_id)
def test_forced_lds_dma_inapplicable(lib, c):
    dev, base, auto = _auto(lib, c)
    assert auto in G.REG_CONFIGS
    for n in G.GLDS_CONFIGS:
        c32, c16, ran = _launch(lib, dev, force=n)
        assert ran == auto, f"gemm_config {n} ran {ran}"
        _same_bits(c, (c32, c16), base, f"gemm_config {n}")


@pytest.mark.parametrize("c", [G.Case(-1, 2047, 40, 32, 3, True, "none", "c16", 0, False),       # M < 2048
                               G.Case(-1, 2048, 40, 32, 3, True, "none", "both", 0, False)],     # an fp32 output
                         ids=G.case_id)
def test_forced_pw_conv_inapplicable(lib, c):
    dev, base, auto = _auto(lib, c)
    assert auto == 1
    c32, c16, ran = _launch(lib, dev, force=G.PW_CONFIG)
    assert ran == auto
    _same_bits(c, (c32, c16), base, "gemm_config 9")


@pytest.mark.parametrize("c,want", G.ladder_cases(), ids=lambda v: G.case_id(v) if isinstance(v, G.Case) else str(v))
def test_automatic_choice_follows_the_ladder(lib, c, want):
    """gemm_config's documented order, one shape per rung (and each result against float64)."""
    _, _, ran = _auto(lib, c)
    assert ran == want


# ---- rejects ----
def test_raw_gemm_rejects(lib):
    """Every validation of mmf_gemm_f16_raw: MMF_EINVAL with nothing written.  The inputs are well-formed device
    buffers, larger than any of the refused shapes would touch."""
    M, N, K = 64, 136, 72
    A = torch.zeros(M + 16, K + 16, dtype=torch.float16, device="cuda")
    W = torch.zeros(N + 16, K + 16, dtype=torch.float16, device="cuda")
    bias = torch.zeros(N + 16, device="cuda")
    r32 = torch.zeros(M + 16, N + 16, device="cuda")
    r16 = torch.zeros(M + 16, N + 16, dtype=torch.float16, device="cuda")
    sc = torch.ones(M + 16, K + 16, device="cuda")
    c32 = _nan(M + 16, N + 16, torch.float32)
    c16 = _nan(M + 16, N + 16, torch.float16)
    good = dict(A=_p(A), lda=K + 8, W=_p(W), ldw=K + 16, bias=_p(bias), res32=None, res16=_p(r16), ldr=N + 4, ascale=None,
                rpb=0, c32=_p(c32), c16=_p(c16), ldc=N + 8, M=M, N=N, K=K, act=1)

    def call(**over):
        a = dict(good, **over)
        out = ctypes.c_int(-7)
        rc = lib.mmf_gemm_f16_raw(a["A"], a["lda"], a["W"], a["ldw"], a["bias"], a["res32"], a["res16"], a["ldr"], a["ascale"],
                                  a["rpb"], a["c32"], a["c16"], a["ldc"], a["M"], a["N"], a["K"], a["act"], ctypes.byref(out),
                                  None)
        return rc, out.value

    bad = [dict(A=None), dict(W=None), dict(c32=None, c16=None),
           dict(res32=_p(r32)),                                           # both residual kinds
           dict(ascale=_p(sc), rpb=0), dict(ascale=_p(sc), rpb=-49),
           dict(M=0), dict(N=0), dict(K=0), dict(M=-1),
           dict(lda=K - 8), dict(ldw=K - 8), dict(ldc=N - 4),
           dict(ldr=N - 4), dict(ldr=N + 2), dict(res16=None, res32=_p(r32), ldr=N + 6),
           dict(act=-1), dict(act=5),
           dict(A=_p(A) + 8), dict(W=_p(W) + 8), dict(bias=_p(bias) + 4), dict(res16=_p(r16) + 8),
           dict(res16=None, res32=_p(r32) + 8), dict(ascale=_p(sc) + 4, rpb=49), dict(c32=_p(c32) + 8), dict(c16=_p(c16) + 8),
           dict(K=K - 4), dict(N=N - 2), dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 6)]
    for over in bad:
        rc, out = call(**over)
        assert rc == EINVAL, f"{over}: returned {rc}"
        assert out == -7, f"{over}: config_out written by a refused call"
    torch.cuda.synchronize()
    assert bool(torch.isnan(c32).all()) and bool(torch.isnan(c16).all())
    # and the well-formed call is accepted
    rc, out = call()
    assert rc == 0 and out == 2
    torch.cuda.synchronize()
    for buf in (c32, c16):      # (rows of ldc = N + 8 elements in the flat buffer)
        assert not bool(torch.isnan(buf.view(-1)[:M * (N + 8)].view(M, N + 8)[:, :N]).any())
