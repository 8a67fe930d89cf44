"""Per-kernel numerics of the fp16 EfficientNet kernels (csrc/effnet.hip) on a real MI355X against the
float64 references of tests/effnet_refs.py, through the test-only entry points of include/mmf_hip.h.
Every output element is compared, with the bounds derived there (and checked against a float32
emulation in tests/test_effnet_refs_cpu.py).  Output buffers start as NaN with a guard band behind
them, so an element a kernel does not write, or a write past the end, fails too."""
import pytest
import torch

from tests import effnet_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 4096  # elements behind every output buffer that must stay untouched


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    return hip.load()


def _d(t):
    return t.contiguous().cuda()


def _nan(n, dtype):
    return torch.full((n + GUARD,), float("nan"), device="cuda", dtype=dtype)


def _guard_ok(*bufs):
    return all(bool(torch.isnan(b[-GUARD:]).all()) for b in bufs)


def _close(got, ref, tol, what):
    """Every element within its bound (NaN fails); prints the worst error / bound ratio first."""
    err = (got.double().cpu() - ref).abs()
    ratio = err / tol
    print(f"{what}: max err / bound = {float(ratio[~torch.isnan(ratio)].max()) if ratio.numel() else 0:.3f}")
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {float(ratio.nan_to_num(float('inf')).max()):.3g} x"


def _dwconv(lib, xd, wd, bd, B, H, W, C, k, stride, flags):
    """mmf_dwconv_f16 on device operands -> (out [B][Ho][Wo][C] fp16, pool [B][nchunks][C] fp32), device views."""
    import mmf_amd.hip as hip
    ho, wo = R.out_size(H, stride), R.out_size(W, stride)
    n = lib.mmf_dwconv_nchunks(H, W, C, stride)
    assert n == R.dw_geometry(H, W, C, stride, bool(flags & 8))[2]
    out, pool = _nan(B * ho * wo * C, torch.float16), _nan(B * n * C, torch.float32)
    hip.check(lib.mmf_dwconv_f16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), pool.data_ptr(), B, H, W,
                                 C, k, stride, flags, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(out, pool), "wrote past the end"
    return out[:-GUARD].view(B, ho, wo, C), pool[:-GUARD].view(B, n, C)


def _expand_dw(lib, xd, cin, wed, bed, wd, bd, B, H, C, k, stride, ct):
    import mmf_amd.hip as hip
    ho = R.out_size(H, stride)
    n = lib.mmf_dwconv_nchunks(H, H, C, stride)
    out, pool = _nan(B * ho * ho * C, torch.float16), _nan(B * n * C, torch.float32)
    hip.check(lib.mmf_expand_dw_f16(xd.data_ptr(), cin, wed.data_ptr(), bed.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                    out.data_ptr(), pool.data_ptr(), B, H, H, C, k, stride, ct, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(out, pool), "wrote past the end"
    return out[:-GUARD].view(B, ho, ho, C), pool[:-GUARD].view(B, n, C)


def _expand_gemm(lib, xd, wed, bed, rows, cin, C):
    """The 1x1 expand + SiLU as its own launch (mmf_gemm_f16_ex, act 3; tests/test_gpu_gemm_kernels.py covers it)."""
    import mmf_amd.hip as hip
    E = torch.empty(rows, C, device="cuda", dtype=torch.float16)
    hip.check(lib.mmf_gemm_f16_ex(xd.data_ptr(), cin, wed.data_ptr(), cin, bed.data_ptr(), None, None, 0, E.data_ptr(),
                                  C, rows, C, cin, 3, hip.stream_ptr()))
    torch.cuda.synchronize()
    return E


# ---- standalone depthwise conv ----
@pytest.mark.parametrize("k,stride,H,W,C,bit3,key", R.DW_ROWS)
def test_dwconv_vs_fp64(lib, k, stride, H, W, C, bit3, key):
    """Compile-time (flags bit 0) and runtime-geometry kernels of one table row against float64, and the
    code comments' claim that their outputs are bit-identical (the pool partials are summed in different
    orders: each against the reference only)."""
    B = 2
    assert R.dw_selected(H, W, C, k, stride, 1 | bit3) == ("ct", key)
    x, w, b = R.dw_inputs(B, H, W, C, k)
    ref = R.dw_ref(x, w, b, k, stride)
    xd, wd, bd = _d(x), _d(w), _d(b)
    outs = {}
    for flags in (1 | bit3, bit3):
        out, pool = _dwconv(lib, xd, wd, bd, B, H, W, C, k, stride, flags)
        _close(out, ref["out"], ref["tol"], f"out flags {flags}")
        _close(pool, ref["pool"], ref["pool_tol"], f"pool flags {flags}")
        outs[flags & 1] = out
    assert torch.equal(outs[0], outs[1]), "compile-time and runtime-geometry outputs differ"


@pytest.mark.parametrize("k,stride,H,W,C", R.DW_EDGES)
def test_dwconv_runtime_edges_vs_fp64(lib, k, stride, H, W, C):
    """Runtime-geometry kernels: a prime output edge (T = 1, 289 tiles), an image smaller than a halo."""
    B = 2
    x, w, b = R.dw_inputs(B, H, W, C, k)
    ref = R.dw_ref(x, w, b, k, stride)
    out, pool = _dwconv(lib, _d(x), _d(w), _d(b), B, H, W, C, k, stride, 0)
    _close(out, ref["out"], ref["tol"], "out")
    _close(pool, ref["pool"], ref["pool_tol"], "pool")


def test_dwconv_rejects_unsupported_channels(lib):
    """C = 40 is neither a multiple of 48 nor of 32: MMF_EINVAL from the host, nothing launched."""
    B, H, C, k = 2, 8, 40, 3
    x, w, b = R.dw_inputs(B, H, H, C, k)
    xd, wd, bd = _d(x), _d(w), _d(b)
    out, pool = _nan(B * H * H * C, torch.float16), _nan(B * C, torch.float32)
    for flags in (0, 1):
        assert lib.mmf_dwconv_f16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), pool.data_ptr(), B, H, H,
                                  C, k, 1, flags, None) == EINVAL
        assert lib.mmf_last_error()
    assert lib.mmf_dwconv_f16(None, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), pool.data_ptr(), B, H, H, 64, k, 1, 1,
                              None) == EINVAL
    assert lib.mmf_dwconv_f16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), pool.data_ptr(), B, H, H, 64,
                              4, 1, 1, None) == EINVAL
    assert lib.mmf_dwconv_nchunks(8, 8, 64, 0) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(pool).all())


# ---- fused expand + depthwise ----
@pytest.mark.parametrize("k,stride,ks,T,cin,C,H", R.EDW_ROWS)
def test_expand_dw_vs_fp64_and_separate_launches(lib, k, stride, ks, T, cin, C, H):
    """The fused front (compile-time and runtime geometry) against expand GEMM -> fp16 E -> float64 depthwise
    conv, and bit-identical in out and pool partials to the same GEMM followed by mmf_dwconv_f16 on
    48-channel groups (the claim checked so far on final logits only)."""
    B = 2
    x, we, be, w, b = R.edw_inputs(B, H, cin, C, k)
    xd, wed, bed, wd, bd = _d(x), _d(we), _d(be), _d(w), _d(b)
    E = _expand_gemm(lib, xd, wed, bed, B * H * H, cin, C)
    ref = R.dw_ref(E.cpu().view(B, H, H, C), w, b, k, stride)
    assert ref["T"] == T
    for ct in (1, 0):
        out, pool = _expand_dw(lib, xd, cin, wed, bed, wd, bd, B, H, C, k, stride, ct)
        _close(out, ref["out"], ref["tol"], f"out ct {ct}")
        _close(pool, ref["pool"], ref["pool_tol"], f"pool ct {ct}")
        assert R.dw_selected(H, H, C, k, stride, ct)[1][3] == 48
        sout, spool = _dwconv(lib, E, wd, bd, B, H, H, C, k, stride, ct)
        assert torch.equal(out, sout), f"ct {ct}: fused out differs from GEMM + depthwise"
        assert torch.equal(pool, spool), f"ct {ct}: fused pool partials differ from GEMM + depthwise"


@pytest.mark.parametrize("ct", [1, 0])
def test_expand_dw_block_walks_its_groups(lib, ct):
    """B = 2048 x 4 tiles = 8192 blocks: at the launcher's threshold each block walks both channel groups
    instead of one block per (tile, group).  64 distinct images repeated 32 x must give exactly what the
    same 64 give as B = 64 (the split layout); 4 of them are checked against float64."""
    c = R.EDW_WALK
    k, stride, cin, C, H, n64, rep = c["k"], c["stride"], c["cin"], c["C"], c["H"], c["distinct"], c["repeat"]
    x, we, be, w, b = R.edw_inputs(n64, H, cin, C, k)
    xd, wed, bed, wd, bd = _d(x), _d(we), _d(be), _d(w), _d(b)
    assert lib.mmf_dwconv_nchunks(H, H, C, stride) * n64 * rep == 8192
    out64, pool64 = _expand_dw(lib, xd, cin, wed, bed, wd, bd, n64, H, C, k, stride, ct)
    big, pbig = _expand_dw(lib, xd.repeat(rep, 1, 1, 1), cin, wed, bed, wd, bd, n64 * rep, H, C, k, stride, ct)
    assert torch.equal(big, out64.repeat(rep, 1, 1, 1)) and torch.equal(pbig, pool64.repeat(rep, 1, 1))
    sel = list(c["checked"])
    E = _expand_gemm(lib, _d(x[sel]), wed, bed, len(sel) * H * H, cin, C)
    ref = R.dw_ref(E.cpu().view(len(sel), H, H, C), w, b, k, stride)
    for r in (0, rep - 1):
        idx = [r * n64 + i for i in sel]
        _close(big[idx], ref["out"], ref["tol"], f"out repeat {r}")
        _close(pbig[idx], ref["pool"], ref["pool_tol"], f"pool repeat {r}")


def test_expand_dw_rejects_unsupported_shapes(lib):
    """cin = 112 with k = 5 (stages 5.1 - 6.1 keep their separate launches): MMF_EINVAL, nothing launched."""
    B, H, C = 2, 14, 96
    x, we, be, w, b = R.edw_inputs(B, H, 112, C, 5)
    xd, wed, bed, wd, bd = _d(x), _d(we), _d(be), _d(w), _d(b)
    out, pool = _nan(B * H * H * C, torch.float16), _nan(B * C, torch.float32)
    for cin, CC, k, s in ((112, C, 5, 1), (112, C, 5, 2), (20, C, 3, 1), (24, 64, 3, 1), (40, C, 5, 2)):
        for ct in (1, 0):
            assert lib.mmf_expand_dw_f16(xd.data_ptr(), cin, wed.data_ptr(), bed.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                         out.data_ptr(), pool.data_ptr(), B, H, H, CC, k, s, ct, None) == EINVAL, (cin, CC, k, s)
            assert lib.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(pool).all())


# ---- squeeze-excitation ----
@pytest.mark.parametrize("nchunks", R.SE_NCHUNKS)
@pytest.mark.parametrize("C,Csq", R.SE_SHAPES)
def test_se_vs_fp64(lib, C, Csq, nchunks):
    import mmf_amd.hip as hip
    B = 3
    args = R.se_inputs(B, nchunks, C, Csq)
    ref, tol = R.se_ref(*args)
    part, inv_hw, w1, b1, w2t, b2 = args
    dv = [_d(t) for t in (part, w1, b1, w2t, b2)]
    for precise in (0, 1):
        scale = _nan(B * C, torch.float32)
        hip.check(lib.mmf_se_f32(dv[0].data_ptr(), nchunks, inv_hw, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
                                 dv[4].data_ptr(), scale.data_ptr(), B, C, Csq, precise, hip.stream_ptr()))
        torch.cuda.synchronize()
        assert _guard_ok(scale)
        _close(scale[:-GUARD].view(B, C), ref, tol, f"scale precise {precise}")


def test_se_rejects_unsupported_shapes(lib):
    B, n = 2, 4
    part, inv_hw, w1, b1, w2t, b2 = R.se_inputs(B, n, 1288, 72)
    dv = [_d(t) for t in (part, w1, b1, w2t, b2)]
    scale = _nan(B * 1288, torch.float32)
    for C, Csq in ((1281, 64), (1280, 65)):
        for precise in (0, 1):
            assert lib.mmf_se_f32(dv[0].data_ptr(), n, inv_hw, dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
                                  dv[4].data_ptr(), scale.data_ptr(), B, C, Csq, precise, None) == EINVAL
            assert lib.mmf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(scale).all())


# ---- stem, and the stem fused into the stage-1 depthwise conv ----
@pytest.fixture(scope="module")
def stem_case():
    img = R.stem_images()
    return img, R.normalise_f32(img)


@pytest.mark.parametrize("f32", [False, True])
def test_stem_vs_fp64(lib, stem_case, f32):
    import mmf_amd.hip as hip
    img, xf = stem_case
    ws, bs, _, _ = R.stem_inputs()
    ref, e = R.stem_ref(None if f32 else img, xf if f32 else None, ws, bs)
    src = _d(xf) if f32 else _d(img)
    wsd, bsd = _d(ws), _d(bs)
    out = _nan(2 * 112 * 112 * 32, torch.float16)
    hip.check(lib.mmf_effnet_stem_f16(None if f32 else src.data_ptr(), src.data_ptr() if f32 else None, wsd.data_ptr(),
                                      bsd.data_ptr(), out.data_ptr(), 2, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(out)
    _close(out[:-GUARD].view(2, 112, 112, 32), ref, R.stem_tol(ref, e), "stem")
    # exactly one input
    for a, b in ((None, None), (src.data_ptr(), src.data_ptr())):
        assert lib.mmf_effnet_stem_f16(a, b, wsd.data_ptr(), bsd.data_ptr(), out.data_ptr(), 2, None) == EINVAL


@pytest.mark.parametrize("f32", [False, True])
def test_stem_dw_vs_fp64(lib, stem_case, f32):
    """The fused kernel keeps its stem tile in LDS and rounds it to fp16 from its own fp32 value; the reference
    chain and the allowance of taps near an fp16 rounding tie are those of effnet_refs.stem_dw_ref."""
    import mmf_amd.hip as hip
    img, xf = stem_case
    ws, bs, wd, bd = R.stem_inputs(tame=True)
    ref = R.stem_dw_ref(None if f32 else img, xf if f32 else None, ws, bs, wd, bd)
    assert ref["ambiguous"] <= R.AMBIGUOUS_CAP
    src = _d(xf) if f32 else _d(img)
    dv = [_d(t) for t in (ws, bs, wd, bd)]
    out, pool = _nan(2 * 112 * 112 * 32, torch.float16), _nan(2 * 49 * 32, torch.float32)
    hip.check(lib.mmf_effnet_stem_dw_f16(None if f32 else src.data_ptr(), src.data_ptr() if f32 else None,
                                         *[t.data_ptr() for t in dv], out.data_ptr(), pool.data_ptr(), 2,
                                         hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _guard_ok(out, pool)
    _close(out[:-GUARD].view(2, 112, 112, 32), ref["out"], ref["tol"], "stem_dw out")
    _close(pool[:-GUARD].view(2, 49, 32), ref["pool"], ref["pool_tol"], "stem_dw pool")
    for a, b in ((None, None), (src.data_ptr(), src.data_ptr())):
        assert lib.mmf_effnet_stem_dw_f16(a, b, *[t.data_ptr() for t in dv], out.data_ptr(), pool.data_ptr(), 2,
                                          None) == EINVAL


# ---- global average pool + classifier ----
@pytest.mark.parametrize("HW,C", R.GAP_SHAPES)
def test_gap_classifier_vs_fp64(lib, HW, C):
    """HW 50 and 8 leave a tail behind the 7-pixel unrolled loop; C = 2056 takes a second trip of the channel
    loop; logits only, score only, and scores at a stride of 5."""
    import mmf_amd.hip as hip
    B = 3
    x, w, b = R.gap_inputs(B, HW, C)
    logits, tol_l, score, tol_s = R.gap_ref(x, w, b)
    xd, wd, bd = _d(x), _d(w), _d(b)
    for want_l, want_s, stride in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 5)):
        gl, gs = _nan(B * 2, torch.float32), _nan(B * stride, torch.float32)
        hip.check(lib.mmf_gap_classifier_f16(xd.data_ptr(), HW, C, wd.data_ptr(), bd.data_ptr(),
                                             gl.data_ptr() if want_l else None, gs.data_ptr() if want_s else None,
                                             stride, B, hip.stream_ptr()))
        torch.cuda.synchronize()
        assert _guard_ok(gl, gs)
        if want_l:
            _close(gl[:-GUARD].view(B, 2), logits, tol_l, "logits")
        else:
            assert bool(torch.isnan(gl).all())
        if want_s:
            got = gs[:-GUARD].view(B, stride)
            _close(got[:, 0], score, tol_s, f"score stride {stride}")
            assert bool(torch.isnan(got[:, 1:]).all()), "wrote between the strided scores"
        else:
            assert bool(torch.isnan(gs).all())


def test_gap_classifier_rejects_unsupported_channels(lib):
    B, HW = 2, 4
    x, w, b = R.gap_inputs(B, HW, 16)
    xd, wd, bd = _d(x), _d(w), _d(b)
    gl, gs = _nan(B * 2, torch.float32), _nan(B, torch.float32)
    assert lib.mmf_gap_classifier_f16(xd.data_ptr(), HW, 12, wd.data_ptr(), bd.data_ptr(), gl.data_ptr(), gs.data_ptr(), 1,
                                      B, None) == EINVAL
    assert lib.mmf_last_error()
    assert lib.mmf_gap_classifier_f16(xd.data_ptr(), HW, 16, wd.data_ptr(), bd.data_ptr(), None, None, 1, B, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(gl).all()) and bool(torch.isnan(gs).all())
