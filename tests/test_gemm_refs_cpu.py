"""The bounds and case tables of tests/gemm_refs.py, certified without a GPU: for every case of
tests/test_gpu_gemm_kernels.py a float32 emulation of the GEMM (tile by tile, on the kernels' rounding points)
stays within half of gemm_ref's bound (an fp16 store: half of it plus the store's half-ulp), and each planted
defect puts at least one element outside the whole bound in every case where gemm_refs.shows says it can -- the
tables are checked to hold such a case for every instantiation.  The defects that are smaller than an fp16 store's
rounding (gemm_refs.SHOWS_IN_C32) are paired with fp32 outputs.  Seeds are fixed in the reference modules."""
import numpy as np
import pytest
import torch

from tests import gemm_refs as G


def _outside(got, ref, tol):
    """Elements outside the bound (NaN -- never written -- counts)."""
    return ~((got.double() - ref).abs() <= tol)


@pytest.mark.parametrize("c", G.all_cases(), ids=G.case_id)
def test_emulation_under_half_and_defects_outside(c):
    ops = G.operands(c)
    ref, e = G.reference(c, ops)
    bm, bn = G.emulate_tile(c)
    emu = G.gemm_emulate(c, ops, bm, bn)
    err = (emu.double() - ref).abs()
    assert bool((err <= e / 2).all()), f"emulation at {float((err / e.clamp_min(1e-300)).max()):.3f} of the bound"
    if c.outs != "c32":
        assert not bool(_outside(emu.half(), ref, G.store16(ref, e / 2)).any()), "stored emulation outside e / 2 + half-ulp"
    for d in G.DEFECTS:
        if not G.shows(d, c):
            continue
        bad = G.gemm_emulate(c, ops, bm, bn, defect=d)
        # the tightest comparison the GPU test makes of this case: the fp32 output where there is one
        out = _outside(bad.half(), ref, G.store16(ref, e)) if c.outs == "c16" else _outside(bad, ref, e)
        assert bool(out.any()), f"{d}: every element within the bound"


@pytest.mark.parametrize("c", G.walk_cases(), ids=G.case_id)
def test_walk_orders(c):
    """The grouped orders the GPU test sets: 4 and 5 leave a ragged last group (18 = 4 * 4 + 2 = 3 * 5 + 3) and differ
    from row-major; 18 and 64 are one group (column-major); 1 is row-major.  Every order is a permutation of the
    tiles, so the emulation gives the same values in every one of them."""
    bm, bn = G.TILES[c.cfg]
    tm, tn = (c.M + bm - 1) // bm, (c.N + bn - 1) // bn
    assert (tm, tn) == G.WALK_TILES and tm * tn > 256 and c.M % bm and c.N % bn
    rowmajor = G.tile_order(tm, tn, 0)
    assert G.tile_order(tm, tn, 1) == rowmajor
    for gm in (4, 5):
        assert tm % gm and G.tile_order(tm, tn, gm) != rowmajor
    assert G.tile_order(tm, tn, 18) == G.tile_order(tm, tn, 64) == [(m, n) for n in range(tn) for m in range(tm)]
    for gm in G.WALK_GROUP_M:
        assert sorted(G.tile_order(tm, tn, gm)) == rowmajor


@pytest.mark.parametrize("gm", [0, 1, 3, 4, 5, 8, 64])
def test_tile_coords_is_a_bijection(gm):
    for tm in range(1, 21):
        for tn in range(1, 18):
            assert sorted(G.tile_order(tm, tn, gm)) == [(m, n) for m in range(tm) for n in range(tn)], (tm, tn, gm)


def test_scaled_operand_is_the_fp32_product_rounded():
    """fp16(fp32(a) * s) is what the kernels form; it differs from one rounding of the exact product in some
    elements (double rounding), which is why the reference is not built from the float64 product."""
    c = G.Case(3, 2049, 4, 200, 0, True, "none", "c32", 49, False)      # (about one element in 2^13 differs)
    ops = G.operands(c)
    got = G.scaled_operand(ops.A, ops.scale, c.rpb)
    rows = torch.arange(c.M) // c.rpb
    assert torch.equal(got, (ops.A.float() * ops.scale[rows]).half())
    once = torch.from_numpy((ops.A.double() * ops.scale.double()[rows]).numpy().astype(np.float16))   # correctly rounded
    assert got.dtype == torch.float16 and int((got != once).sum()) > 0


def test_operands_are_poisoned():
    c = G.Case(5, 257, 132, 128, 0, True, "res16", "both", 49, False)
    o = G.operands(c)
    assert (o.lda, o.ldw, o.ldr, o.ldc) == (c.K + 8, c.K + 16, c.N + 4, c.N + 8)
    assert o.Ap.shape == (c.M + 16, o.lda) and o.Wp.shape == (c.N + 16, o.ldw) and o.resp.shape == (c.M, o.ldr)
    for clean, buf in ((o.A, o.Ap), (o.W, o.Wp), (o.res, o.resp), (o.scale, o.scalep), (o.bias[None], o.biasp[None])):
        r, k = clean.shape
        assert torch.equal(buf[:r, :k], clean) and not bool(torch.isnan(clean.float()).any())
        assert bool(torch.isnan(buf[:, k:].float()).all()) and bool(torch.isnan(buf[r:].float()).all())
        assert buf[:, k:].numel() + buf[r:].numel() > 0
    assert G.operands(c._replace(inplace=True, res="res32")).ldr == c.N + 8


def _by_cfg(cases):
    d = {}
    for c in cases:
        d.setdefault(c.cfg, []).append(c)
    return d


def _forms_meet(cs):
    assert {c.act for c in cs} == {0, 1, 2, 3, 4} and {c.bias for c in cs} == {True, False}
    assert {c.res for c in cs} == set(G.RES_KINDS) and {c.outs for c in cs} == set(G.OUT_KINDS)


def test_reg_cases_cover_the_grid():
    by = _by_cfg(G.reg_cases())
    assert set(by) == set(G.REG_CONFIGS)
    for cfg, cs in by.items():
        BM, BN = G.TILES[cfg]
        plain = [c for c in cs if not c.rpb]
        assert {c.M for c in plain} == {1, BM - 1, BM + 1, 2 * BM + 17}
        assert {(c.N, c.K) for c in plain} == {(N, K) for N in (4, BN - 4, BN + 4, 2 * BN + 12) for K in G.REG_K}
        assert {(c.K + 63) // 64 for c in plain} == {1, 2, 3, 4} and {c.K % 64 == 0 for c in plain} == {True, False}
        _forms_meet(plain)
        asc = [c for c in cs if c.rpb]
        assert {c.rpb for c in asc} == set(G.ASC_RPB) and all(c.M % c.rpb and c.M > c.rpb for c in asc)
        for d in G.DEFECTS:
            assert any(G.shows(d, c) for c in cs), f"config {cfg}: no case shows {d}"
        for d in G.SHOWS_IN_C32:
            assert all(c.outs != "c16" for c in cs if G.shows(d, c))


def test_glds_cases_cover_the_grid():
    by = _by_cfg(G.glds_cases())
    assert set(by) == set(G.GLDS_CONFIGS)
    for cfg, cs in by.items():
        BN = G.TILES[cfg][1]
        plain = [c for c in cs if not c.inplace]
        assert {c.M for c in plain} == set(G.GLDS_M)
        assert {(c.N, c.K) for c in plain} == {(N, K) for N in (4, BN - 4, BN, BN + 4, 2 * BN + 12) for K in G.GLDS_K}
        assert {c.K // 64 for c in plain} == {1, 2, 3, 4, 5}
        _forms_meet(plain)
        # the paired fp16 stores (no residual, fp16 only) with a 4-column last group and without one
        assert {c.N % 8 for c in plain if c.res == "none" and c.outs == "c16"} == {0, 4}
        # a ragged last row panel behind a full one: the next tile's prefetch takes the clamped fill
        assert any(c.M > 256 and c.M % 256 for c in plain)
        inpl = [c for c in cs if c.inplace]
        assert {c.bias for c in inpl} == {True, False} and all(c.res == "res32" and c.outs == "c32" for c in inpl)
        for d in G.DEFECTS:
            if d != "scale_unrounded":      # (no SE scale on the LDS-DMA tiles: glds_ok)
                assert any(G.shows(d, c) for c in cs), f"config {cfg}: no case shows {d}"
        assert all(c.outs != "c16" for c in cs if G.shows("gelu_tanh", c))


def test_pw_cases_cover_the_templates():
    cs = G.pw_cases()
    grid, walk = cs[:-3], cs[-3:]
    cf = lambda N: 2 if N <= 32 else (4 if N <= 64 else 8)
    assert {c.K for c in grid} == set(G.PW_K) and {G.pw_ks(c.K) for c in grid} == {1, 2, 3, 4, 5, 6, 8}
    assert {c.N for c in grid} == {n for ns in G.PW_N for n in ns}
    assert {(G.pw_ks(c.K), cf(c.N), c.act) for c in grid} == {(k, f, a) for k in (1, 2, 3, 4, 5, 6, 8) for f in (2, 4, 8) for a in (0, 3)}
    assert {(c.N + 127) // 128 for c in grid if c.N > 64} == {1, 2, 3}
    assert {c.M for c in grid} == set(G.PW_M) and {c.rpb for c in grid} == {0, 49, 196}
    assert {c.res for c in grid} == {"none", "res16"} and {c.bias for c in grid} == {True, False}
    for c in cs:
        assert c.outs == "c16" and c.M >= 2048 and c.N % 8 == 0 and c.K % 8 == 0 and (c.K <= 128 or c.N <= 256)
    assert [G.pw_rows(c.K) for c in walk] == [256, 128, 64]
    for c in walk:
        rows = G.pw_rows(c.K)
        nrb = (c.M + rows - 1) // rows
        assert nrb > G.pw_grid_x(c.N, c.M, c.K) and nrb < 2 * G.pw_grid_x(c.N, c.M, c.K) and c.M % rows
    for d in ("drop_last_k8", "skip_tile", "bias_clamped_col", "res_before_act"):
        assert any(G.shows(d, c) for c in cs)


def test_ladder_has_every_rung():
    assert [cfg for _, cfg in G.ladder_cases()] == [9, 0, 1, 2, 5, 10, 11, 2, 3]
    assert set(G.EXISTING) | set(G.REMOVED) == set(range(17))
