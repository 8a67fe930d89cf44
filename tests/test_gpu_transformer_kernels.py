"""Per-kernel numerics of the transformer towers' kernels (csrc/norm.hip, csrc/precise.hip, attention.hip,
the split-K path of gemm.hip) on a real MI355X against the float64 references of
tests/transformer_refs.py, through the test-only entry points of csrc/test_host.cpp.  Every output
element is compared, with the bounds derived there (and certified against a float32 emulation in
tests/test_transformer_refs_cpu.py); hi / lo splits and integer results must be exact.  Output buffers
start as NaN (integers: a sentinel), with canary columns where a row stride exceeds the row and a guard
band behind: an element a kernel does not write, or a write it should not make, fails too."""
import pytest
import torch

from tests import transformer_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = 1024
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    return hip.load()


def _run(rc):
    import mmf_amd.hip as hip
    hip.check(rc)
    torch.cuda.synchronize()


def _sp():
    import mmf_amd.hip as hip
    return hip.stream_ptr()


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    """Device operands made inside a call's argument list stay alive until the test ends (a freed block could be
    handed to the next operand before the kernel has read it)."""
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _d(t):
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(rows, ld, dtype=torch.float32):
    """[rows + 1][ld] of NaN (the last row is a guard)."""
    return torch.full((rows + 1, ld), NAN, device="cuda", dtype=dtype)


def _strided(t, ld):
    """Device copy of host [rows][C] with row stride ld >= C; the padding columns hold NaN."""
    buf = torch.full((t.shape[0], ld), NAN, device="cuda", dtype=t.dtype)
    buf[:, :t.shape[1]] = t.cuda()
    _KEEP.append(buf)
    return buf


def _untouched(buf, rows, C, what):
    """The canary columns of the first `rows` rows and every later row are still NaN."""
    assert bool(torch.isnan(buf[:rows, C:]).all()), f"{what}: wrote into the row padding"
    assert bool(torch.isnan(buf[rows:]).all()), f"{what}: wrote past the last row"


def _close(got, ref, tol, what):
    """Every element within its bound (NaN fails); prints the worst error / bound ratio."""
    err = (got.double().cpu() - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    ok = err <= tol
    worst = float(ratio[ok].max()) if bool(ok.any()) else 0.0
    print(f"RATIO {what}: {worst:.3f}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst {float(ratio.nan_to_num(float('inf')).max()):.3g} x"


def _same_bits(got, want, what):
    assert torch.equal(R.bits16(got.cpu()), R.bits16(want)), f"{what}: not bit-identical"


def _check_hilo(hi, lo, ref, e, what):
    """hi within the fp16 store bound, hi + lo within the split's bound, |lo| at most half an ulp of hi."""
    _close(hi, ref, R.store16(ref, e), what + " hi")
    if lo is not None:
        s = hi.double().cpu() + lo.double().cpu()
        _close(s, ref, R.hilo_sum_tol(ref, e), what + " hi+lo")
        assert bool((lo.double().cpu().abs() <= R.half_ulp16(hi.double().cpu())).all()), f"{what}: |lo| above half an ulp of hi"


# ---- LayerNorm ----
@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("add,dominant", [(False, False), (True, False), (False, True)])
def test_layernorm_vs_fp64(lib, rows, C, add, dominant):
    x = R.rows_input(rows, C, dominant=dominant)
    a = R.rows_input(rows, C, 11) * 0.5 if add else None
    gam, bet = R.dominant_params(C) if dominant else R.ln_params(C)
    if add:
        s = x.double() + a.double()
        ref, e = R.ln_ref(s, gam, bet, e_x=R.U * s.abs())
    else:
        ref, e = R.ln_ref(x, gam, bet)
    xd, ad = _strided(x, C + 8), (_strided(a, C + 4) if add else None)
    y32, y16 = _nan(rows, C + 12), _nan(rows, C + 4, torch.float16)
    _run(lib.mmf_layernorm_f32(_p(xd), C + 8, _p(ad), C + 4, _p(_d(gam)), _p(_d(bet)), R.EPS, _p(y32), C + 12, _p(y16),
                               C + 4, rows, C, _sp()))
    _untouched(y32, rows, C, "y32")
    _untouched(y16, rows, C, "y16")
    _close(y32[:rows, :C], ref, e, "layernorm fp32")
    _close(y16[:rows, :C], ref, R.store16(ref, e), "layernorm fp16")


def test_layernorm_rejects(lib):
    rows, C = 4, 256
    x = _d(R.rows_input(rows, C))
    gam, bet = (_d(t) for t in R.ln_params(C))
    y32, y16 = _nan(rows, C), _nan(rows, C, torch.float16)
    assert lib.mmf_layernorm_f32(_p(x), C, None, 0, _p(gam), _p(bet), R.EPS, _p(y32), C, _p(y16), C, rows, C, None) == EINVAL
    assert lib.mmf_last_error()
    assert lib.mmf_layernorm_f32(_p(x), 510, None, 0, _p(gam), _p(bet), R.EPS, _p(y32), 512, None, 0, 2, 512, None) == EINVAL
    assert lib.mmf_layernorm_f32(None, C, None, 0, _p(gam), _p(bet), R.EPS, _p(y32), C, None, 0, rows, C, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(y32).all()) and bool(torch.isnan(y16).all())


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("form", ["pre_inplace", "post_inplace", "apart"])
def test_add_ln_f32_vs_fp64(lib, rows, C, form):
    """s32 over x (the pre-LN stream), o32 over x (the post-LN stream), or both apart from x."""
    x, y = R.rows_input(rows, C, 1), R.branch_input(rows, C)
    gam, bet = R.ln_params(C)
    s, e_s = R.add_ref(x, y)
    ref, e = R.ln_ref(s, gam, bet, e_x=e_s / 2)
    ldx, ldy, ldo = C + 4, C + 8, C + 4
    xd, yd = _strided(x, ldx), _strided(y, ldy)
    xd = torch.cat([xd, torch.full((1, ldx), NAN, device="cuda")])
    s32 = xd if form == "pre_inplace" else (_nan(rows, ldx) if form == "apart" else None)
    o32 = xd if form == "post_inplace" else (_nan(rows, ldx) if form == "apart" else None)
    o16 = _nan(rows, ldo, torch.float16)
    _run(lib.mmf_add_ln_f32(_p(xd), ldx, _p(yd), ldy, _p(_d(gam)), _p(_d(bet)), R.EPS, _p(s32), _p(o32), _p(o16), ldo,
                            rows, C, _sp()))
    _untouched(o16, rows, C, "o16")
    _close(o16[:rows, :C], ref, R.store16(ref, e), "add_ln o16")
    if s32 is not None:
        _untouched(s32, rows, C, "s32")
        _close(s32[:rows, :C], s, e_s, "add_ln s32")
    if o32 is not None:
        _untouched(o32, rows, C, "o32")
        _close(o32[:rows, :C], ref, e, "add_ln o32")
    if form == "apart":
        assert torch.equal(xd[:rows, :C].cpu(), x), "x changed"


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("form", ["inplace", "apart", "none"])
def test_add_ln_f16_vs_fp64(lib, rows, C, form):
    """The fp16 stream: s16 over x16, apart from it, or absent (then the LayerNorm sees the unrounded sum)."""
    x16, y = R.rows_input(rows, C, 1).half(), R.branch_input(rows, C)
    gam, bet = R.ln_params(C)
    s, e_s = R.add_ref(x16, y)
    ldx, ldy, ldo = C + 4, C + 8, C + 12
    xd, yd = _strided(x16, ldx), _strided(y, ldy)
    xd = torch.cat([xd, torch.full((1, ldx), NAN, device="cuda", dtype=torch.float16)])
    s16 = xd if form == "inplace" else (_nan(rows, ldx, torch.float16) if form == "apart" else None)
    o16 = _nan(rows, ldo, torch.float16)
    _run(lib.mmf_add_ln_f16(_p(xd), ldx, _p(yd), ldy, _p(_d(gam)), _p(_d(bet)), R.EPS, _p(s16), _p(o16), ldo, rows, C,
                            _sp()))
    _untouched(o16, rows, C, "o16")
    if s16 is not None:
        _untouched(s16, rows, C, "s16")
        _close(s16[:rows, :C], s, R.store16(s, e_s), "add_ln16 s16")
        ref, e = R.ln_ref(s16[:rows, :C].cpu(), gam, bet)    # the LayerNorm of the stored stream
    else:
        ref, e = R.ln_ref(s, gam, bet, e_x=e_s / 2)
    _close(o16[:rows, :C], ref, R.store16(ref, e), "add_ln16 o16")


def test_add_ln_rejects(lib):
    rows, C = 4, 1024
    x, y = _d(R.rows_input(rows, C)), _d(R.branch_input(rows, C))
    gam, bet = (_d(t) for t in R.ln_params(C))
    s32, o16 = _nan(rows, C), _nan(rows, C, torch.float16)
    assert lib.mmf_add_ln_f32(_p(x), C, _p(y), C, _p(gam), _p(bet), R.EPS, _p(s32), None, _p(o16), C, rows, C, None) == EINVAL
    assert lib.mmf_add_ln_f16(_p(_d(x.half().cpu())), C, _p(y), C, _p(gam), _p(bet), R.EPS, None, _p(o16), C, rows, C, None) == EINVAL
    assert lib.mmf_add_ln_f32(_p(x), C, _p(y), C, _p(gam), _p(bet), R.EPS, _p(s32), None, None, C, rows, 512, None) == EINVAL
    hi = _nan(rows, 512, torch.float16)
    assert lib.mmf_add_ln_hilo_f16(_p(hi), None, 512, _p(y), C, _p(gam), _p(bet), R.EPS, rows, 512, None, 0, None) == EINVAL
    s3 = _nan(rows, 3 * 512, torch.float16)
    assert lib.mmf_layernorm_split3_f32(_p(s32), _p(x), _p(gam), _p(bet), R.EPS, _p(s3), 1, rows, 512, None) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (s32, o16, hi, s3))


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("with_lo", [True, False])
def test_add_ln_hilo_vs_fp64(lib, rows, with_lo):
    C, ld, ldy = 768, 768 + 8, 768 + 4
    x, y = R.rows_input(rows, C, 2), R.branch_input(rows, C, 2)
    gam, bet = R.ln_params(C)
    hi, lo = R.split_hilo(x)
    a = hi.double() + (lo.double() if with_lo else 0)
    s = a + y.double()
    ref, e = R.ln_ref(s, gam, bet, e_x=R.U * (a.abs() + s.abs()))
    hd = torch.cat([_strided(hi, ld), torch.full((1, ld), NAN, device="cuda", dtype=torch.float16)])
    ldv = torch.cat([_strided(lo, ld), torch.full((1, ld), NAN, device="cuda", dtype=torch.float16)]) if with_lo else None
    _run(lib.mmf_add_ln_hilo_f16(_p(hd), _p(ldv), ld, _p(_strided(y, ldy)), ldy, _p(_d(gam)), _p(_d(bet)), R.EPS, rows, C,
                                 None, 0, _sp()))
    _untouched(hd, rows, C, "hi")
    if with_lo:
        _untouched(ldv, rows, C, "lo")
    _check_hilo(hd[:rows, :C], ldv[:rows, :C] if with_lo else None, ref, e, "add_ln_hilo")


def test_add_ln_hilo_overflow_flag(lib):
    """An fp16 inf in the branch output of row 5 (sequences of L = 2 rows) flags sequence 2 and no other."""
    rows, C, L = 9, 768, 2
    x, y = R.rows_input(rows, C, 2), R.branch_input(rows, C, 2)
    y[5, 100] = float("inf")
    gam, bet = R.ln_params(C)
    hi, lo = R.split_hilo(x)
    s = (hi.double() + lo.double()) + y.double()
    ref, e = R.ln_ref(s, gam, bet, e_x=R.U * ((hi.double() + lo.double()).abs() + s.abs()))
    hd, ldv = _d(hi), _d(lo)
    ovf = torch.zeros(5 + 4, device="cuda", dtype=torch.int32)
    _run(lib.mmf_add_ln_hilo_f16(_p(hd), _p(ldv), C, _p(_d(y)), C, _p(_d(gam)), _p(_d(bet)), R.EPS, rows, C, _p(ovf), L, _sp()))
    assert ovf.cpu().tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    keep = torch.arange(rows) != 5
    _check_hilo(hd[keep], ldv[keep], ref[keep], e[keep], "add_ln_hilo beside an overflow")
    assert not bool(torch.isfinite(hd[5].float()).any())


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("B", R.ROWS)
@pytest.mark.parametrize("with_lo", [True, False])
def test_hilo_rows_exact(lib, B, C, with_lo):
    """out = float(hi) + float(lo) of rows a stride apart: one exact-operand fp32 addition, bit for bit."""
    stride = 3 * C + 8
    hi, lo = R.split_hilo(R.rows_input(B, C, 4))
    out = _nan(B, C)
    _run(lib.mmf_hilo_rows_f32(_p(_strided(hi, stride)), _p(_strided(lo, stride)) if with_lo else None, stride, _p(out),
                               B, C, _sp()))
    _untouched(out, B, C, "out")
    want = hi.float() + lo.float() if with_lo else hi.float()
    assert torch.equal(out[:B].cpu(), want)
    assert lib.mmf_hilo_rows_f32(_p(_d(hi)), None, C + 2, _p(out), 1, C, None) == EINVAL


def _check_split3(s3, x32, C, with_lo, what):
    """[hi | lo | hi] thirds exact from the fp32 values x32; without lo the other two thirds stay NaN."""
    rows = x32.shape[0]
    hi, lo = R.split_hilo(x32)
    _same_bits(s3[:rows, :C], hi, what + " hi")
    if with_lo:
        _same_bits(s3[:rows, C:2 * C], lo, what + " lo")
        _same_bits(s3[:rows, 2 * C:3 * C], hi, what + " hi copy")
    else:
        assert bool(torch.isnan(s3[:rows, C:]).all()), f"{what}: wrote the lo / copy thirds"
    assert bool(torch.isnan(s3[rows:]).all()), f"{what}: wrote past the last row"


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("with_lo", [1, 0])
def test_layernorm_split3_vs_fp64(lib, rows, with_lo):
    C = 768
    x, a = R.rows_input(rows, C, 6), R.rows_input(rows, C, 8) * 0.5
    gam, bet = R.ln_params(C)
    s = x.double() + a.double()
    ref, e = R.ln_ref(s, gam, bet, e_x=R.U * s.abs())
    xd = torch.cat([_d(x), torch.full((1, C), NAN, device="cuda")])
    s3 = _nan(rows, 3 * C, torch.float16)
    _run(lib.mmf_layernorm_split3_f32(_p(xd), _p(_d(a)), _p(_d(gam)), _p(_d(bet)), R.EPS, _p(s3), with_lo, rows, C, _sp()))
    assert bool(torch.isnan(xd[rows:]).all())
    _close(xd[:rows], ref, e, "layernorm_split3 x")
    _check_split3(s3, xd[:rows].cpu(), C, with_lo, "layernorm_split3")


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("C", [512, 768, 3072])
@pytest.mark.parametrize("with_lo", [1, 0])
def test_split3_exact(lib, rows, C, with_lo):
    x = R.rows_input(rows, C, 9)
    x[0, :8] = torch.tensor([0.0, -0.0, 1e-8, -3e-6, 6.1e-5, 65504.0, -1.0009765625, 2.0 ** -24])
    s3 = _nan(rows, 3 * C, torch.float16)
    _run(lib.mmf_split3_f32(_p(_strided(x, C + 4)), C + 4, _p(s3), rows, C, with_lo, _sp()))
    _check_split3(s3, x, C, with_lo, "split3")
    assert lib.mmf_split3_f32(_p(_d(x)), C + 2, _p(s3), 1, C, 1, None) == EINVAL


# ---- embeddings ----
def _roberta(lib, ids, word, pos, type0, gam, bet, form, ovf=None):
    B, L = ids.shape
    n = B * L
    xb, xlo, x32 = _nan(n, 768, torch.float16), None, None
    if form == "hilo":
        xlo = _nan(n, 768, torch.float16)
    if form == "x32":
        x32 = _nan(n, 768)
    _run(lib.mmf_roberta_embed_f32(_p(_d(ids)), _p(_d(word)), _p(_d(pos)), _p(_d(type0)), _p(_d(gam)), _p(_d(bet)), R.EPS,
                                   _p(xlo), _p(xb), _p(x32), _p(ovf), B, L, 768, R.PAD, _sp()))
    for t in (xb, xlo, x32):
        if t is not None:
            assert bool(torch.isnan(t[n:]).all()), "wrote past the last row"
    return xb[:n], None if xlo is None else xlo[:n], None if x32 is None else x32[:n]


@pytest.mark.parametrize("L", R.ROBERTA_L)
@pytest.mark.parametrize("form", ["hilo", "hi", "x32"])
def test_roberta_embed_vs_fp64(lib, L, form):
    """The row added from `pos` is the position id: with well-separated table rows a wrong id, in any of the no-pad,
    leading-pad, interior-pad and all-pad sequences, puts the whole row far outside the bound."""
    ids = R.roberta_ids(L)
    word, pos, type0 = R.roberta_tables(L)
    gam, bet = R.ln_params(768)
    ref, e = R.roberta_ref(ids, word, pos, type0, gam, bet)
    ref, e = ref.view(-1, 768), e.view(-1, 768)
    xb, xlo, x32 = _roberta(lib, ids, word, pos, type0, gam, bet, form)
    if form == "x32":
        _close(x32, ref, e, "roberta_embed x32")
        assert bool(torch.isnan(xb).all()), "the fp32 form wrote the split stream"
    else:
        _check_hilo(xb, xlo, ref, e, "roberta_embed")


def test_roberta_embed_overflow_flag_and_reject(lib):
    L = 65
    ids = R.roberta_ids(L)
    word, pos, type0 = R.roberta_tables(L)
    gam, bet = R.ln_params(768)
    ref, e = R.roberta_ref(ids, word, pos, type0, gam, bet)
    word = word.clone()
    word[R.ROBERTA_VOCAB - 1, 5] = float("inf")     # a row no id of roberta_ids uses
    ids[2, 3] = R.ROBERTA_VOCAB - 1
    ovf = torch.zeros(4 + 4, device="cuda", dtype=torch.int32)
    xb, xlo, _ = _roberta(lib, ids, word, pos, type0, gam, bet, "hilo", ovf)
    assert ovf.cpu().tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    keep = torch.ones(4, L, dtype=torch.bool)
    keep[2, 3] = False
    keep = keep.view(-1)
    _check_hilo(xb[keep], xlo[keep], ref.view(-1, 768)[keep], e.view(-1, 768)[keep], "roberta_embed beside an overflow")
    # L = 513 and H != 768: MMF_EINVAL, nothing written
    big = torch.full((1, 513), 5, dtype=torch.int32)
    out = _nan(513, 768, torch.float16)
    args = (_p(_d(word)), _p(_d(pos)), _p(_d(type0)), _p(_d(gam)), _p(_d(bet)), R.EPS)
    assert lib.mmf_roberta_embed_f32(_p(_d(big)), *args, None, _p(out), None, None, 1, 513, 768, R.PAD, None) == EINVAL
    assert lib.mmf_roberta_embed_f32(_p(_d(big)), *args, None, _p(out), None, None, 1, 64, 512, R.PAD, None) == EINVAL
    assert lib.mmf_roberta_embed_f32(_p(_d(big)), *args, None, None, None, None, 1, 64, 768, R.PAD, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def _check_partials(st, stored, what):
    """st [rows] float2 = (mean, M2) of the stored rows `stored` (host tensor, the kernel's own output)."""
    mean, e_m, m2, e_m2 = R.partial_ref(stored)
    _close(st[:, 0], mean, e_m, what + " st mean")
    _close(st[:, 1], m2, e_m2, what + " st M2")


@pytest.mark.parametrize("L", R.CLIP_TEXT_L)
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("lazy", [False, True])
def test_clip_text_embed_vs_fp64(lib, L, x16, lazy):
    B, C = 2, 512
    n = B * L
    ids, tok, pos = R.clip_text_inputs(B, L)
    gam, bet = R.ln_params(C)
    x_ref, e_x = R.clip_text_x_ref(ids, tok, pos)
    x = _nan(n, C, torch.float16 if x16 else torch.float32)
    xb = _nan(n, C, torch.float16)
    st = _nan(n, 2) if lazy else None
    _run(lib.mmf_clip_text_embed_f32(_p(_d(ids)), _p(_d(tok)), _p(_d(pos)), _p(_d(gam)), _p(_d(bet)), R.EPS,
                                     None if x16 else _p(x), _p(x) if x16 else None, _p(xb), _p(st), B, L, C, _sp()))
    assert bool(torch.isnan(x[n:]).all()) and bool(torch.isnan(xb[n:]).all())
    _close(x[:n], x_ref, R.store16(x_ref, e_x) if x16 else e_x, "clip_text x")
    stored = x[:n].cpu()
    if lazy:
        assert bool(torch.isnan(st[n:]).all()) and bool(torch.isnan(xb).all()), "xb written in lazy-LN mode"
        _check_partials(st[:n], stored, "clip_text")
        return
    ref, e = R.ln_ref(stored, gam, bet) if x16 else R.ln_ref(x_ref, gam, bet, e_x=e_x / 2)
    _close(xb[:n], ref, R.store16(ref, e), "clip_text xb")


def test_clip_text_embed_rejects(lib):
    B, L, C = 2, 5, 512
    ids, tok, pos = R.clip_text_inputs(B, L)
    gam, bet = R.ln_params(C)
    x, x16, xb = _nan(B * L, C), _nan(B * L, C, torch.float16), _nan(B * L, C, torch.float16)
    a = (_p(_d(ids)), _p(_d(tok)), _p(_d(pos)), _p(_d(gam)), _p(_d(bet)), R.EPS)
    assert lib.mmf_clip_text_embed_f32(*a, None, None, _p(xb), None, B, L, C, None) == EINVAL
    assert lib.mmf_clip_text_embed_f32(*a, _p(x), _p(x16), _p(xb), None, B, L, C, None) == EINVAL
    assert lib.mmf_clip_text_embed_f32(*a, _p(x), None, _p(xb), None, B, L, 768, None) == EINVAL
    assert lib.mmf_clip_text_embed_f32(*a, _p(x), None, None, None, B, L, C, None) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (x, x16, xb))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("lazy", [False, True])
def test_clip_vision_assemble_vs_fp64(lib, B, x16, lazy):
    C, n = 768, B * 50
    patches, cls, pos = R.vision_inputs(B)
    pg, pb = R.ln_params(C, 2)
    g1, b1 = R.ln_params(C, 3)
    x_ref, e_x = R.vision_x_ref(patches, cls, pos, B, pg, pb)
    x = _nan(n, C, torch.float16 if x16 else torch.float32)
    xb = _nan(n, C, torch.float16)
    st = _nan(n, 2) if lazy else None
    _run(lib.mmf_clip_vision_assemble_f32(_p(_d(patches)), _p(_d(cls)), _p(_d(pos)), _p(_d(pg)), _p(_d(pb)), _p(_d(g1)),
                                          _p(_d(b1)), R.EPS, None if x16 else _p(x), _p(x) if x16 else None, _p(xb),
                                          _p(st), B, _sp()))
    assert bool(torch.isnan(x[n:]).all()) and bool(torch.isnan(xb[n:]).all())
    _close(x[:n], x_ref, R.store16(x_ref, e_x) if x16 else e_x, "clip_vision x")
    stored = x[:n].cpu()
    if lazy:
        assert bool(torch.isnan(st[n:]).all()) and bool(torch.isnan(xb).all()), "xb written in lazy-LN mode"
        _check_partials(st[:n], stored, "clip_vision")
        return
    ref, e = R.ln_ref(stored, g1, b1) if x16 else R.ln_ref(x_ref, g1, b1, e_x=e_x / 2)
    _close(xb[:n], ref, R.store16(ref, e), "clip_vision xb")


def test_clip_vision_assemble_rejects(lib):
    patches, cls, pos = R.vision_inputs(1)
    g, b = R.ln_params(768)
    x, x16, xb = _nan(50, 768), _nan(50, 768, torch.float16), _nan(50, 768, torch.float16)
    a = (_p(_d(patches)), _p(_d(cls)), _p(_d(pos)), _p(_d(g)), _p(_d(b)), _p(_d(g)), _p(_d(b)), R.EPS)
    assert lib.mmf_clip_vision_assemble_f32(*a, None, None, _p(xb), None, 1, None) == EINVAL
    assert lib.mmf_clip_vision_assemble_f32(*a, _p(x), _p(x16), _p(xb), None, 1, None) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (x, x16, xb))


@pytest.mark.parametrize("B", [1, 2])
def test_clip_im2col_vs_fp64(lib, B):
    img = torch.randint(0, 256, (B, 224, 224, 3), generator=R._gen(B, 73), dtype=torch.uint8)
    ref, e = R.im2col_ref(img)
    A = _nan(B * 49, 3072, torch.float16)
    _run(lib.mmf_clip_im2col_f16(_p(_d(img)), _p(A), B, _sp()))
    assert bool(torch.isnan(A[B * 49:]).all())
    _close(A[:B * 49], ref, R.store16(ref, e), "clip_im2col")
    pad = torch.zeros(224 * 224 * 3 + 8, dtype=torch.uint8, device="cuda")
    A = _nan(49, 3072, torch.float16)
    assert lib.mmf_clip_im2col_f16(pad.data_ptr() + 4, _p(A), 1, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(A).all())


# ---- pooling ----
@pytest.mark.parametrize("L", R.EOS_L)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("mode", ["eos", "argmax"])
def test_eos_index_exact(lib, B, L, mode):
    ids = R.eos_inputs(B, L, mode)
    eos = R.EOS_ID if mode == "eos" else 2
    out = torch.full((B + 8,), -77, device="cuda", dtype=torch.int32)
    _run(lib.mmf_eos_index_i32(_p(_d(ids)), _p(out), B, L, eos, _sp()))
    assert torch.equal(out[:B].cpu(), R.eos_ref(ids, eos))
    assert bool((out[B:] == -77).all())


def test_eos_index_rejects(lib):
    ids = torch.zeros(1, 1025, dtype=torch.int32, device="cuda")
    out = torch.full((4,), -77, device="cuda", dtype=torch.int32)
    assert lib.mmf_eos_index_i32(_p(ids), _p(out), 1, 1025, 2, None) == EINVAL
    assert lib.mmf_eos_index_i32(_p(ids), _p(out), 1, 1025, R.EOS_ID, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == -77).all())


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("B", [1, 5])
def test_l2norm_vs_fp64(lib, B, C):
    x = R.rows_input(B, C, 7)
    ref, e = R.l2norm_ref(x)
    xd = torch.cat([_d(x), torch.full((1, C), NAN, device="cuda")])
    _run(lib.mmf_l2norm_f32(_p(xd), B, C, _sp()))
    assert bool(torch.isnan(xd[B:]).all())
    _close(xd[:B], ref, e, "l2norm")
    before = xd.clone()
    assert lib.mmf_l2norm_f32(_p(xd), B, 100, None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(xd[:B], before[:B])


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("use_idx", [False, True])
def test_gather_ln_vs_fp64(lib, C, L, use_idx):
    """Rows are unlike each other (row-dependent scale and offset): the LayerNorm of any other row is far outside."""
    B = 5
    x = R.rows_input(B * L, C, 12)
    gam, bet = R.ln_params(C)
    idx = R.gather_idx(B, L) if use_idx else None
    sel = torch.arange(B) * L + (idx.long() if use_idx else 0)
    ref, e = R.ln_ref(x[sel], gam, bet)
    o16, o32 = _nan(B, C, torch.float16), _nan(B, C)
    _run(lib.mmf_gather_ln_f32(_p(_d(x)), _p(_d(idx)) if use_idx else None, L, _p(_d(gam)), _p(_d(bet)), R.EPS, _p(o16),
                               _p(o32), B, C, _sp()))
    assert bool(torch.isnan(o16[B:]).all()) and bool(torch.isnan(o32[B:]).all())
    _close(o32[:B], ref, e, "gather_ln fp32")
    _close(o16[:B], ref, R.store16(ref, e), "gather_ln fp16")
    c16 = _nan(B, 256, torch.float16)
    assert lib.mmf_gather_ln_f32(_p(_d(x)), None, L, _p(_d(gam)), _p(_d(bet)), R.EPS, _p(c16), None, 1, 256, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(c16).all())


@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("use_idx", [False, True])
@pytest.mark.parametrize("src", ["f32", "f16"])
@pytest.mark.parametrize("with_a16", [True, False])
def test_gather_rows2_exact(lib, L, use_idx, src, with_a16):
    B, C = 5, 768
    a32 = R.rows_input(B * L, C, 13)
    a16 = R.rows_input(B * L, C, 14).half()
    idx = R.gather_idx(B, L, 1) if use_idx else None
    sel = torch.arange(B) * L + (idx.long() if use_idx else 0)
    o16, o32 = _nan(B, C, torch.float16), _nan(B, C)
    s32 = _d(a32) if src == "f32" else None
    s16 = _d(a32.half()) if src == "f16" else None
    _run(lib.mmf_gather_rows2(_p(_d(a16)) if with_a16 else None, _p(s32), _p(s16), _p(_d(idx)) if use_idx else None, L, C,
                              _p(o16), _p(o32), B, _sp()))
    assert bool(torch.isnan(o16[B:]).all()) and bool(torch.isnan(o32[B:]).all())
    want = a32[sel] if src == "f32" else a32.half()[sel].float()
    assert torch.equal(o32[:B].cpu(), want)
    if with_a16:
        _same_bits(o16[:B], a16[sel], "o16")
    else:
        assert bool(torch.isnan(o16).all()), "o16 written without a16"
    # exactly one of the fp32 and the fp16 source; o16 with a16; C % 4 == 0: MMF_EINVAL, nothing written
    c16, c32 = _nan(B, C, torch.float16), _nan(B, C)
    assert lib.mmf_gather_rows2(None, _p(_d(a32)), _p(_d(a32.half())), None, L, C, _p(c16), _p(c32), B, None) == EINVAL
    assert lib.mmf_gather_rows2(None, None, None, None, L, C, _p(c16), _p(c32), B, None) == EINVAL
    assert lib.mmf_gather_rows2(_p(_d(a16)), _p(_d(a32)), None, None, L, C, None, _p(c32), B, None) == EINVAL
    assert lib.mmf_gather_rows2(_p(_d(a16)), _p(_d(a32)), None, None, L, C - 2, _p(c16), _p(c32), B, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(c16).all()) and bool(torch.isnan(c32).all())


# ---- attention ----
@pytest.mark.parametrize("L", R.Q1_L)
@pytest.mark.parametrize("B,H", R.Q1_BH)
def test_attention_q1_vs_fp64(lib, B, H, L):
    """One query per sequence: no mask and all keys; then a mask with holes (the last sequence fully masked when
    B > 1) with the query at position 0, mid and L - 1."""
    D = H * 64
    ld, koff, voff, ldq, ldo = 3 * D + 16, D + 8, 2 * D + 16, D + 4, D + 2
    g = R._gen(B, H, L, 79)
    kv = R.attn_inputs(B, L, H, 3)
    qkv = torch.zeros(B * L, ld, dtype=torch.float16)
    qkv[:, koff:koff + D] = kv[:, D:2 * D]
    qkv[:, voff:voff + D] = kv[:, 2 * D:]
    q = torch.randn(B, D, generator=g) * 0.7
    k, v = R.heads(qkv, B, L, H, koff), R.heads(qkv, B, L, H, voff)
    q4 = q.view(B, H, 1, 64)
    qkv_d, q_d = _d(qkv), _strided(q, ldq)
    mask = R.holes_mask(B, L, dead=B - 1 if B > 1 else None)
    for m, qp in ((None, None), (mask, 0), (mask, L // 2), (mask, L - 1)):
        qpos = None if qp is None else torch.full((B,), qp, dtype=torch.int32)
        valid = R.attn_valid(m, B, L, qpos=qpos if qpos is not None else torch.full((B,), L - 1))
        ref, e = R.attn_ref(q4, k, v, valid, p16=False)
        ref, e = ref.reshape(B, D), e.reshape(B, D)
        out = _nan(B, ldo, torch.float16)
        _run(lib.mmf_attention_q1_f16(_p(q_d), ldq, _p(qkv_d), ld, koff, voff, _p(_d(m)) if m is not None else None,
                                      _p(_d(qpos)) if qpos is not None else None, _p(out), ldo, B, L, H, _sp()))
        _untouched(out, B, D, "q1 out")
        _close(out[:B, :D], ref, R.store16(ref, e), "attention_q1")
        if m is not None and B > 1:
            assert bool((out[B - 1, :D] == 0).all()), "a fully masked sequence must give zeros"


def test_attention_q1_rejects(lib):
    B, H, L = 1, 1, 8
    qkv = torch.zeros(520 * 200, dtype=torch.float16, device="cuda")
    q = torch.zeros(64, device="cuda")
    out = _nan(1, 64, torch.float16)
    assert lib.mmf_attention_q1_f16(_p(q), 64, _p(qkv), 192, 64, 128, None, None, _p(out), 64, B, 513, H, None) == EINVAL
    assert lib.mmf_attention_q1_f16(_p(q), 64, _p(qkv), 196, 64, 128, None, None, _p(out), 64, B, L, H, None) == EINVAL
    assert lib.mmf_attention_q1_f16(_p(q), 64, _p(qkv), 200, 68, 128, None, None, _p(out), 64, B, L, H, None) == EINVAL
    assert lib.mmf_attention_q1_f16(_p(q), 66, _p(qkv), 192, 64, 128, None, None, _p(out), 64, B, L, H, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("L", R.ATTN32_L)
@pytest.mark.parametrize("masking", ["none", "first_chunk_masked", "dead_sequence"])
def test_attention32_vs_fp64(lib, L, masking):
    """fp32 attention in 32-key chunks; out3 (with and without lo) is the exact split of the `out` run."""
    B, H = 2, 2
    D = H * 64
    ld, koff, voff, ldo = 3 * D + 8, D + 4, 2 * D + 8, D + 4
    g = R._gen(L, 83)
    src = R.attn_inputs(B, L, H, 5).float() * (1 + 1e-3 * torch.randn(B * L, 3 * D, generator=g))   # not fp16 values
    qkv = torch.zeros(B * L, ld)
    qkv[:, :D], qkv[:, koff:koff + D], qkv[:, voff:voff + D] = src[:, :D], src[:, D:2 * D], src[:, 2 * D:]
    mask = None
    if masking == "first_chunk_masked":
        mask = R.holes_mask(B, L)
        if L > 32:
            mask[0, :32] = 0    # every key of the first chunk masked, valid ones after: m stays -inf through it
    elif masking == "dead_sequence":
        mask = R.holes_mask(B, L, dead=1)
    valid = R.attn_valid(mask, B, L)
    ref, e = R.attn_ref(R.heads(qkv, B, L, H, 0), R.heads(qkv, B, L, H, koff), R.heads(qkv, B, L, H, voff), valid,
                        p16=False, chunks=-(-L // 32))
    ref, e = (t.permute(0, 2, 1, 3).reshape(B * L, D) for t in (ref, e))
    qd, md = _d(qkv), (_d(mask) if mask is not None else None)
    out = _nan(B * L, ldo)
    _run(lib.mmf_attention32_f32(_p(qd), ld, koff, voff, _p(md), _p(out), ldo, None, 1, B, L, H, _sp()))
    _untouched(out, B * L, D, "out")
    _close(out[:B * L, :D], ref, e, "attention32")
    if masking == "dead_sequence":
        assert bool((out[L:2 * L, :D] == 0).all()), "a fully masked sequence must give zeros"
    for with_lo in (1, 0):
        out3 = _nan(B * L, 3 * D, torch.float16)
        _run(lib.mmf_attention32_f32(_p(qd), ld, koff, voff, _p(md), None, 0, _p(out3), with_lo, B, L, H, _sp()))
        _check_split3(out3, out[:B * L, :D].cpu().contiguous(), D, with_lo, "attention32 out3")


def test_attention32_rejects(lib):
    qkv = torch.zeros(8 * 400, device="cuda")
    out = _nan(8, 128)
    assert lib.mmf_attention32_f32(_p(qkv), 386, 128, 256, None, _p(out), 128, None, 1, 1, 8, 2, None) == EINVAL
    assert lib.mmf_attention32_f32(_p(qkv), 388, 130, 256, None, _p(out), 128, None, 1, 1, 8, 2, None) == EINVAL
    assert lib.mmf_attention32_f32(_p(qkv), 384, 128, 256, None, None, 128, None, 1, 1, 8, 2, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("L", R.ATTN_SHORT_L + R.ATTN_LONG_L)
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("causal", [0, 1])
def test_attention_f16_vs_fp64(lib, L, H, causal):
    """attention_kernel<LK> (L <= 128, every LK at and around its edge) and attention_long_kernel, each element of
    every unpadded query row against float64 with the derived bound (P rounded to fp16 before P V)."""
    B, D = 2, H * 64
    qkv = R.attn_inputs(B, L, H)
    mask = R.holes_mask(B, L)
    valid = R.attn_valid(mask, B, L, bool(causal))
    ref, e = R.attn_ref(R.heads(qkv, B, L, H, 0), R.heads(qkv, B, L, H, D), R.heads(qkv, B, L, H, 2 * D), valid, p16=True,
                        chunks=R.long_chunks(L) if L > 128 else 1)
    ref, e = (t.permute(0, 2, 1, 3).reshape(B * L, D) for t in (ref, e))
    out = _nan(B * L, D, torch.float16)
    _run(lib.mmf_attention_f16(_p(_d(qkv)), _p(_d(mask)), _p(out), B, L, H, causal, _sp()))
    assert bool(torch.isnan(out[B * L:]).all())
    rows = (mask != 0).view(-1)     # padded query rows are don't-care
    _close(out[:B * L][rows.cuda()], ref[rows], R.store16(ref, e)[rows], "attention_f16 long" if L > 128 else "attention_f16")


# ---- split-K ----
def _splitk(lib, A, W, b, res, M, N, K, act, res_kind, outs, ws_elems):
    """One mmf_gemm_f16_splitk launch -> (c32 [M + 1][ldc] or None, c16 or None, ws with GUARD canaries behind)."""
    ldc = N + 4
    c32 = _nan(M, ldc) if outs in ("c32", "both") else None
    c16 = _nan(M, ldc, torch.float16) if outs in ("c16", "both") else None
    r32 = r16 = None
    if res_kind == "res32":
        if c32 is not None:
            c32[:M, :N] = res.cuda()      # in place: the residual aliases the fp32 output
            r32 = c32
        else:
            r32 = _strided(res, ldc)
    elif res_kind == "res16":
        r16 = _strided(res.half(), ldc)
    ws = torch.full((ws_elems + GUARD,), NAN, device="cuda")
    _run(lib.mmf_gemm_f16_splitk(_p(A), K, _p(W), K, _p(b), _p(r32), _p(r16), _p(c32), _p(c16), ldc, M, N, K, act, _p(ws),
                                 ws_elems, _sp()))
    assert bool(torch.isnan(ws[ws_elems:]).all()), "wrote past the workspace"
    for c in (c32, c16):
        if c is not None:
            _untouched(c, M, N, "c")
    return c32, c16, ws


@pytest.mark.parametrize("M,N,K,act,bias,res,outs", R.splitk_cases())
def test_gemm_splitk_vs_fp64(lib, M, N, K, act, bias, res, outs):
    """S = K / 256 slices reduced in order (N > 64: the skinny-M tile; N = 4 takes another tile, unsplit, and must
    leave the workspace alone).  A workspace one float short gives the unsplit kernel: bit-identical to process
    option gemm_splitk = 0, and not a partial write."""
    import mmf_amd.hip as hip
    A, W, bv, rv = R.gemm_inputs(M, N, K)
    S = lib.mmf_gemm_splitk_factor(M, N, K, N + 4)
    assert S == K // 256
    split = N > 64
    b = bv if bias else None
    r = None if res == "none" else (rv if res == "res32" else rv.half())
    ref, e = R.gemm_ref(A, W, b, r, act, (K // S + S + 4) if split else K + 4)
    Ad, Wd, bd = _d(A), _d(W), (_d(bv) if bias else None)
    c32, c16, ws = _splitk(lib, Ad, Wd, bd, rv, M, N, K, act, res, outs, S * M * N)
    assert bool(torch.isnan(ws[:S * M * N]).any()) != split, "split-K ran" if not split else "split-K did not fill its planes"
    if c32 is not None:
        _close(c32[:M, :N], ref, e, "gemm split-K c32")
    if c16 is not None:
        _close(c16[:M, :N], ref, R.store16(ref, e), "gemm split-K c16")
    if not split:
        return
    # one float short: the fallback, whole
    f32, f16, ws = _splitk(lib, Ad, Wd, bd, rv, M, N, K, act, res, outs, S * M * N - 1)
    assert bool(torch.isnan(ws).all()), "a short workspace was written"
    hip.set_process_option("gemm_splitk", 0)
    try:
        assert lib.mmf_gemm_splitk_factor(M, N, K, N + 4) == 1
        n32, n16, ws = _splitk(lib, Ad, Wd, bd, rv, M, N, K, act, res, outs, S * M * N)
    finally:
        hip.set_process_option("gemm_splitk", 1)
    assert bool(torch.isnan(ws).all())
    ref1, e1 = R.gemm_ref(A, W, b, r, act, K + 4)
    for f, n, tol in ((f32, n32, e1), (f16, n16, R.store16(ref1, e1))):
        if f is not None:
            assert torch.equal(f[:M, :N], n[:M, :N]), "short workspace and gemm_splitk = 0 differ"
            _close(f[:M, :N], ref1, tol, "gemm unsplit")


def test_gemm_splitk_rejects(lib):
    A, W = torch.zeros(64 * 512, dtype=torch.float16, device="cuda"), torch.zeros(136 * 512, dtype=torch.float16, device="cuda")
    c = _nan(64, 136)
    r = torch.zeros(64 * 136, device="cuda")
    assert lib.mmf_gemm_f16_splitk(_p(A), 512, _p(W), 512, None, _p(r), _p(_d(r.half().cpu())), _p(c), None, 136, 64, 136, 512, 0,
                                   None, 0, None) == EINVAL
    assert lib.mmf_gemm_f16_splitk(_p(A), 512, _p(W), 512, None, None, None, None, None, 136, 64, 136, 512, 0, None, 0,
                                   None) == EINVAL
    assert lib.mmf_gemm_f16_splitk(_p(A), 512, _p(W), 512, None, None, None, _p(c), None, 136, 64, 136, 512, 7, None, 0,
                                   None) == EINVAL
    assert lib.mmf_gemm_f16_splitk(_p(A), 508, _p(W), 508, None, None, None, _p(c), None, 136, 64, 136, 508, 0, None, 0,
                                   None) == EINVAL
    assert lib.mmf_gemm_splitk_factor(0, 136, 512, 136) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


# ---- the QKV GEMM's attention epilogue (gemm.hip epi 3) ----
@pytest.mark.parametrize("M", [128, 256, 384])     # one, two and three sequences: the last tile holds one
@pytest.mark.parametrize("N", [192, 384])          # one and two heads
@pytest.mark.parametrize("K", [192, 768])
def test_gemm_attention_epilogue(lib, M, N, K):
    """ctx bit-identical to the plain 256 x 192 GEMM (forced gemm_config 10) on the same head-interleaved weights,
    de-interleaved, followed by mmf_attention_f16 -- and within the attention bound of float64 on the fp16 qkv
    that GEMM stored (itself within the GEMM bound).  Key masks with holes and padded tails."""
    import mmf_amd.hip as hip
    B, H, D = M // 128, N // 192, N // 3
    A, W, bias, _ = R.gemm_inputs(M, N, K, 5)
    A = (A.float() * 0.7).half()
    mask = R.holes_mask(B, 128)
    Ad, Wd, bd, md = _d(A), _d(W), _d(bias), _d(mask)
    ctx = _nan(M, D + 4, torch.float16)
    _run(lib.mmf_gemm_f16_attn(_p(Ad), K, _p(Wd), K, _p(bd), _p(md), _p(ctx), D + 4, M, N, K, _sp()))
    _untouched(ctx, M, D, "ctx")
    qkv_il = _nan(M, N, torch.float16)
    hip.set_process_option("gemm_config", 10)
    try:
        _run(lib.mmf_gemm_f16(_p(Ad), K, _p(Wd), K, _p(bd), None, None, _p(qkv_il), N, M, N, K, 0, _sp()))
    finally:
        hip.set_process_option("gemm_config", -1)
    ref, e = R.gemm_ref(A, W, bias, None, 0, K + 4)
    _close(qkv_il[:M], ref, R.store16(ref, e), "qkv GEMM")
    # column h * 192 + part * 64 + d  ->  part * D + h * 64 + d
    qkv = qkv_il[:M].view(M, H, 3, 64).permute(0, 2, 1, 3).reshape(M, 3 * D).contiguous()
    out = _nan(M, D, torch.float16)
    _run(lib.mmf_attention_f16(_p(qkv), _p(md), _p(out), B, 128, H, 0, _sp()))
    assert torch.equal(R.bits16(ctx[:M, :D].cpu()), R.bits16(out[:M].cpu())), "epilogue and GEMM + attention differ"
    qh = qkv.cpu()
    ref, e = R.attn_ref(R.heads(qh, B, 128, H, 0), R.heads(qh, B, 128, H, D), R.heads(qh, B, 128, H, 2 * D),
                        R.attn_valid(mask, B, 128), p16=True)
    ref, e = (t.permute(0, 2, 1, 3).reshape(M, D) for t in (ref, e))
    rows = (mask != 0).view(-1)
    _close(ctx[:M, :D][rows.cuda()], ref[rows], R.store16(ref, e)[rows], "attention epilogue")


def test_gemm_attention_epilogue_rejects(lib):
    A, W = _d(torch.zeros(256, 192, dtype=torch.float16)), _d(torch.zeros(384, 192, dtype=torch.float16))
    bias = _d(torch.zeros(384))
    ctx = _nan(256, 128, torch.float16)
    assert lib.mmf_gemm_f16_attn(_p(A), 192, _p(W), 192, _p(bias), None, _p(ctx), 128, 200, 192, 192, None) == EINVAL
    assert lib.mmf_gemm_f16_attn(_p(A), 192, _p(W), 192, _p(bias), None, _p(ctx), 128, 128, 200, 192, None) == EINVAL
    assert lib.mmf_gemm_f16_attn(_p(A), 128, _p(W), 128, _p(bias), None, _p(ctx), 128, 128, 192, 128, None) == EINVAL
    assert lib.mmf_gemm_f16_attn(_p(A), 192, _p(W), 192, _p(bias), None, _p(ctx), 32, 128, 192, 192, None) == EINVAL
    assert lib.mmf_gemm_f16_attn(_p(A), 192, _p(W), 192, None, None, _p(ctx), 128, 128, 192, 192, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all())


# ---- the lazy-LN producer epilogue (gemm.hip epi 2) ----
@pytest.mark.parametrize("M", R.PRODUCER_M)
@pytest.mark.parametrize("N", R.PRODUCER_N)
@pytest.mark.parametrize("K", R.PRODUCER_K)
def test_gemm_ln_producer_vs_fp64(lib, M, N, K):
    """In place over the fp16 stream: the stored values against float64, and every (mean, M2) partial against the
    float64 statistics of the values the kernel stored over that 96-column block (the last block covers 4, 32 or
    96 columns).  Stream and partial rows at or above M, and the stream's padding columns, stay NaN."""
    A, W, bias, res = R.gemm_inputs(M, N, K, 7)
    res = res.half()
    ref, e = R.gemm_ref(A, W, bias, res, 0, K + 4)
    tn = lib.mmf_gemm_ln_tn(M, N, K)
    assert tn == R.LN_TN
    P, ldc = -(-N // tn), N + 4
    stream = torch.full((M + 8, ldc), NAN, device="cuda", dtype=torch.float16)
    stream[:M, :N] = res.cuda()
    st = torch.full((M + 8, P, 2), NAN, device="cuda")
    _run(lib.mmf_gemm_f16_ln_producer(_p(_d(A)), K, _p(_d(W)), K, _p(_d(bias)), _p(stream), _p(stream), ldc, _p(st), M, N,
                                      K, _sp()))
    _untouched(stream, M, N, "stream")
    assert bool(torch.isnan(st[M:]).all()), "partials written at or above M"
    _close(stream[:M, :N], ref, R.store16(ref, e), "ln producer stream")
    mean, e_m, m2, e_m2 = R.block_partials_ref(stream[:M, :N].cpu())
    _close(st[:M, :, 0], mean, e_m, "ln producer mean")
    _close(st[:M, :, 1], m2, e_m2, "ln producer M2")


def test_gemm_ln_producer_rejects(lib):
    A, W = _d(torch.zeros(100, 192, dtype=torch.float16)), _d(torch.zeros(960, 192, dtype=torch.float16))
    stream = _nan(100, 960, torch.float16)
    st = _nan(100, 20)
    assert lib.mmf_gemm_f16_ln_producer(_p(A), 128, _p(W), 128, None, _p(stream), _p(stream), 100, _p(st), 100, 100, 128,
                                        None) == EINVAL      # K < 192
    assert lib.mmf_gemm_f16_ln_producer(_p(A), 192, _p(W), 192, None, _p(stream), _p(stream), 960, _p(st), 100, 960, 192,
                                        None) == EINVAL      # 10 partials per row
    assert lib.mmf_gemm_f16_ln_producer(_p(A), 192, _p(W), 192, None, None, _p(stream), 100, _p(st), 100, 100, 192,
                                        None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(stream).all()) and bool(torch.isnan(st).all())


# ---- the lazy-LN consumer epilogue (gemm.hip epi 1) ----
def _consumer(lib, sd, lda, Wp, u, c, act, pm, pq, tn, M, N, K):
    """One mmf_gemm_f16_ln_consumer launch with every padding the launcher requires filled with NaN: partial rows up
    to the next multiple of 256 (and the slots behind the last row), the 256 extra entries of u and of the bias."""
    P = pm.shape[1]
    rows = -(-M // 256) * 256
    st = torch.full((rows * P + 64, 2), NAN, device="cuda")
    st[:M * P, 0], st[:M * P, 1] = pm.reshape(-1).cuda(), pq.reshape(-1).cuda()
    ud, cd = torch.full((N + 256,), NAN, device="cuda"), torch.full((N + 256,), NAN, device="cuda")
    ud[:N], cd[:N] = u.cuda(), c.cuda()
    out = _nan(M, N + 4, torch.float16)
    _KEEP.extend([st, ud, cd])
    _run(lib.mmf_gemm_f16_ln_consumer(_p(sd), lda, _p(_d(Wp)), K, _p(cd), _p(st), P, tn, _p(ud), R.EPS, _p(out), N + 4, M,
                                      N, K, act, _sp()))
    _untouched(out, M, N, "consumer out")
    return out[:M, :N]


@pytest.mark.parametrize("M", R.CONSUMER_M)
@pytest.mark.parametrize("N", R.CONSUMER_N)
@pytest.mark.parametrize("K", R.CONSUMER_K)
@pytest.mark.parametrize("form", ["one", "blocks"])
def test_gemm_ln_consumer_vs_fp64(lib, M, N, K, form):
    """Partials from float64 statistics as (P = 1, tn = K) or (P = ceil(K / 96), tn = 96); NaN in every padding (the
    kernel selects padding out, it never weights it by 0); 256 x 192 and 256 x 256 tiles (forced gemm_config 10 and
    11) bit-identical: a row's result does not depend on the tile its batch size selects."""
    import mmf_amd.hip as hip
    act = R.CONSUMER_ACT[K]
    tn = K if form == "one" else R.LN_TN
    s, Wp, u, c = R.consumer_inputs(M, N, K)
    pm, pq, e_pm, e_pq = R.supplied_partials(s, tn)
    ref, e = R.consumer_ref(s, Wp, u, c, act, tn, e_pm, e_pq)
    sd = _d(s)
    outs = []
    for cfg in (10, 11):
        hip.set_process_option("gemm_config", cfg)
        try:
            outs.append(_consumer(lib, sd, K, Wp, u, c, act, pm, pq, tn, M, N, K))
        finally:
            hip.set_process_option("gemm_config", -1)
        _close(outs[-1], ref, R.store16(ref, e), f"ln consumer cfg {cfg}")
    assert torch.equal(R.bits16(outs[0].cpu()), R.bits16(outs[1].cpu())), "256 x 192 and 256 x 256 tiles differ"


@pytest.mark.parametrize("M", [100, 300])
@pytest.mark.parametrize("C", [512, 768])
def test_gemm_ln_producer_feeds_consumer(lib, M, C):
    """The producer's stored stream and the partials it wrote (rows padded with NaN to 256) straight into the
    consumer, against the float64 LayerNorm of that stored stream."""
    Kp, N = 192, 200
    A, W, bias, res = R.gemm_inputs(M, C, Kp, 7)
    P, ldc = -(-C // R.LN_TN), C + 8
    rows = -(-M // 256) * 256
    stream = torch.full((M + 8, ldc), NAN, device="cuda", dtype=torch.float16)
    stream[:M, :C] = res.half().cuda()
    st = torch.full((rows * P + 64, 2), NAN, device="cuda")
    _run(lib.mmf_gemm_f16_ln_producer(_p(_d(A)), Kp, _p(_d(W)), Kp, _p(_d(bias)), _p(stream), _p(stream), ldc, _p(st), M, C,
                                      Kp, _sp()))
    assert bool(torch.isnan(st[M * P:]).all())
    stored = stream[:M, :C].cpu()
    _, e_pm, _, e_pq = R.block_partials_ref(stored)
    _, Wp, u, c = R.consumer_inputs(M, N, C)
    ref, e = R.consumer_ref(stored, Wp, u, c, 1, R.LN_TN, e_pm, e_pq)
    ud, cd = torch.full((N + 256,), NAN, device="cuda"), torch.full((N + 256,), NAN, device="cuda")
    ud[:N], cd[:N] = u.cuda(), c.cuda()
    out = _nan(M, N + 4, torch.float16)
    _run(lib.mmf_gemm_f16_ln_consumer(_p(stream), ldc, _p(_d(Wp)), C, _p(cd), _p(st), P, R.LN_TN, _p(ud), R.EPS, _p(out),
                                      N + 4, M, N, C, 1, _sp()))
    _untouched(out, M, N, "chain out")
    _close(out[:M, :N], ref, R.store16(ref, e), "ln producer -> consumer")


def test_gemm_ln_consumer_rejects(lib):
    A, W = _d(torch.zeros(256, 192, dtype=torch.float16)), _d(torch.zeros(200, 192, dtype=torch.float16))
    v = _d(torch.zeros(200 + 256))
    st = _d(torch.zeros(256 * 8, 2))
    out = _nan(256, 200, torch.float16)
    a = (_p(A), 192, _p(W), 192, _p(v), _p(st))
    assert lib.mmf_gemm_f16_ln_consumer(*a, 1, 96, _p(v), R.EPS, _p(out), 200, 100, 200, 192, 0, None) == EINVAL   # P tn < K
    assert lib.mmf_gemm_f16_ln_consumer(*a, 9, 96, _p(v), R.EPS, _p(out), 200, 100, 200, 192, 0, None) == EINVAL   # P > 8
    assert lib.mmf_gemm_f16_ln_consumer(*a, 2, 96, _p(v), R.EPS, _p(out), 200, 100, 200, 128, 0, None) == EINVAL   # K < 192
    assert lib.mmf_gemm_f16_ln_consumer(*a, 2, 96, _p(v), R.EPS, _p(out), 200, 100, 200, 192, 3, None) == EINVAL   # SiLU
    assert lib.mmf_gemm_f16_ln_consumer(*a, 2, 96, None, R.EPS, _p(out), 200, 100, 200, 192, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
