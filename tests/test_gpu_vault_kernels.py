"""The vault's stages (csrc/vault.hip) one by one on a real MI355X, through the test-only entry points of
csrc/test_host.cpp: the similarity matrix element by element against float64 (both kernels, which must also agree
bit for bit), the register and LDS-sort top-k on a caller-supplied matrix, the final ranking of per-chunk
candidates and the fused search, all against the numpy ranking of tests/vault_refs.py -- an expectation that shares
none of the kernels' ranking code -- compared on bit patterns, and the top-1 epilogue (discrepancy, caption-title
cosine).  Output buffers start as NaN (integers: a sentinel) with canary columns and a guard row."""
import numpy as np
import pytest
import torch

from tests import misc_refs as M
from tests import vault_refs as V
from tests.test_gpu_misc_kernels import _close
from tests.test_gpu_transformer_kernels import (EINVAL, _d, _nan, _p, _release, _run, _sp,  # noqa: F401
                                                _untouched, lib)

pytestmark = pytest.mark.gpu
SENTINEL = -77
THRESH = 0.85


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _dn(a):
    return None if a is None else _d(_t(a))


def _same(got, want, what):
    got = got.contiguous().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.contiguous().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(V.bits(got), V.bits(want)), f"{what}: not bit-identical"


class _Out:
    """sims / idx [B][k], disc with stride ds, tsim [B]: NaN / sentinel, one guard row each."""

    def __init__(self, B, k, ds=1):
        self.B, self.k, self.ds = B, k, ds
        self.sims, self.disc, self.tsim = _nan(B, k), _nan(B, ds), _nan(B, 1)
        self.idx = torch.full((B + 1, k), SENTINEL, device="cuda", dtype=torch.int32)

    def args(self, temb=None, title=None, D=0, thresh=THRESH):
        return [float(thresh), _p(self.sims), _p(self.idx), _p(self.disc), self.ds, _p(temb), _p(title), D, _p(self.tsim)]

    def check(self, want_v, want_i, what, thresh=THRESH, tsim_zero=True):
        B = self.B
        _same(self.sims[:B], want_v, what + " sims")
        _same(self.idx[:B], want_i, what + " idx")
        hit, disc = zip(*(V.top1_ref(want_v[b, 0], want_i[b, 0], thresh) for b in range(B)))
        _same(self.disc[:B, 0], np.array(disc, np.float32), what + " disc")
        _untouched(self.sims, B, self.k, what + " sims")
        _untouched(self.disc, B, 1, what + " disc")
        _untouched(self.tsim, B, 1, what + " tsim")
        assert bool((self.idx[B] == SENTINEL).all()), f"{what}: idx written past the last row"
        if tsim_zero:
            assert bool((self.tsim[:B] == 0).all()), f"{what}: tsim must be exactly 0 without a caption / title bank"
        return np.array(hit)


# ---- the similarity matrix ----
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_vault_sims_vs_fp64(lib, B, N):
    for D in (512, 64):          # D = 64: the staged loop runs once, with no next load
        for unit in (True, False):
            q, v = V.sims_inputs(B, N, D, unit)
            ref, e = V.sims_ref(q, v)
            qd, vd = _dn(q), _dn(v)
            S = []
            for r in (0, 1):
                s = _nan(B, N)
                _run(lib.mmf_vault_sims_f32(_p(qd), _p(vd), _p(s), B, N, D, r, _sp()))
                _close(s[:B], _t(ref), _t(e), f"vault_sims ref={r} D={D} unit={unit}")
                _untouched(s, B, N, "S")
                S.append(s)
            _same(S[0], S[1], f"MFMA vs VALU similarities D={D} unit={unit}")


def test_vault_sims_rejects(lib):
    q, v = (_dn(t) for t in V.sims_inputs(4, 8, 128, True))
    S = _nan(4, 8)
    f = lib.mmf_vault_sims_f32
    for D in (32, 96, 100):
        assert f(_p(q), _p(v), _p(S), 4, 8, D, 0, None) == EINVAL
    assert lib.mmf_last_error()
    assert f(None, _p(v), _p(S), 4, 8, 128, 0, None) == EINVAL
    assert f(_p(q), None, _p(S), 4, 8, 128, 0, None) == EINVAL
    assert f(_p(q), _p(v), None, 4, 8, 128, 0, None) == EINVAL
    assert f(_p(q), _p(v), _p(S), 0, 8, 128, 0, None) == EINVAL
    assert f(_p(q), _p(v), _p(S), 4, 0, 128, 0, None) == EINVAL
    assert f(_p(q) + 4, _p(v), _p(S), 3, 8, 128, 0, None) == EINVAL
    assert f(_p(q), _p(v), _p(S) + 4, 3, 8, 128, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(S).all())


# ---- top-k on a supplied matrix ----
def _topk(lib, Sd, B, N, k, ref, ds=1, **kw):
    o = _Out(B, k, ds)
    _run(lib.mmf_vault_topk_f32(_p(Sd), B, N, k, *o.args(**kw), ref, _sp()))
    return o


@pytest.mark.parametrize("kinds", V.ROW_SETS, ids=lambda ks: "+".join(ks))
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097])
def test_vault_topk_register_kernels(lib, N, kinds):
    """Every register k on one wave's worth of columns, the four-wave split and the 2048-column stride; k > N pads
    with (-inf, -1)."""
    S = V.topk_matrix(kinds, N)
    Sd, B = _dn(S), len(kinds)
    hits = []
    for k in range(1, 9):
        want_v, want_i = V.topk_ref(S, k)
        if k > N:
            assert bool((want_i[:, N:] == -1).all()) and bool(np.isneginf(want_v[:, N:]).all())
        o = _topk(lib, Sd, B, N, k, 0, ds=(1, 5)[k % 2])
        hits.append(o.check(want_v, want_i, f"topk<{k}> N={N}"))
    if "equal" in kinds:      # 1.25 is a hit; a NaN or zero top-1 is not
        assert hits[0].tolist() == [N < 8, False, True]


def _sort_p(n):
    return next(p for p in (2048, 4096, 8192, 16384) if n <= p)


SORT_N = [700, 2048, 2049, 4097, 8193, 16384]


@pytest.mark.parametrize("kinds", V.ROW_SETS, ids=lambda ks: "+".join(ks))
@pytest.mark.parametrize("N", SORT_N)
def test_vault_topk_sort_kernel(lib, N, kinds):
    """The LDS sort, reached by k > 8 and by ref = 1 with k <= 8, at every padded size P; where the register kernels
    apply too they must return the same bits."""
    assert {_sort_p(n) for n in SORT_N} == {2048, 4096, 8192, 16384}
    S = V.topk_matrix(kinds, N)
    Sd, B = _dn(S), len(kinds)
    for k in (9, 64):
        _topk(lib, Sd, B, N, k, 0, ds=5).check(*V.topk_ref(S, k), f"sort<{_sort_p(N)}> k={k} N={N}")
    for k in (1, 5, 8):
        want = V.topk_ref(S, k)
        srt, reg = _topk(lib, Sd, B, N, k, 1), _topk(lib, Sd, B, N, k, 0)
        srt.check(*want, f"sort<{_sort_p(N)}> ref=1 k={k} N={N}")
        _same(reg.sims, srt.sims, f"register vs sort sims k={k} N={N}")
        _same(reg.idx, srt.idx, f"register vs sort idx k={k} N={N}")
        _same(reg.disc, srt.disc, f"register vs sort disc k={k} N={N}")


def test_vault_topk_sort_k_equals_n(lib):
    S = V.topk_matrix(V.ROW_SETS[1], 700)
    _topk(lib, _dn(S), 3, 700, 700, 0).check(*V.topk_ref(S, 700), "sort k = N = 700")


@pytest.mark.parametrize("k,ref", [(1, 0), (5, 0), (5, 1), (9, 0)])
@pytest.mark.parametrize("ds", [1, 5])
def test_vault_topk_epilogue(lib, k, ref, ds):
    """The top-1 epilogue on a top-1 exactly on the threshold, one float32 above it, a NaN and a clean hit: disc, and
    the caption-title cosine within the rowdot bound and with rowdot_kernel's bits; 0 on a miss and without a bank."""
    B, N, D = 4, 130, 512
    g = np.random.default_rng(5)
    S = g.uniform(0, 0.5, (B, N)).astype(np.float32)
    _, at, above = M.around(THRESH)
    top = [17, 64, 3, 129]
    for b, val in enumerate((at, above, np.float32(np.nan), np.float32(0.93))):
        S[b, top[b]] = val
    temb = M.rowdot_inputs(B, D, 3)[0]
    title = M.rowdot_inputs(N, D, 4)[1]
    Sd, td, bd = _dn(S), _dn(temb), _dn(title)
    want = V.topk_ref(S, k)
    assert want[1][:, 0].tolist() == top
    o = _Out(B, k, ds)
    _run(lib.mmf_vault_topk_f32(_p(Sd), B, N, k, *o.args(td, bd, D, at), ref, _sp()))
    hit = o.check(*want, "epilogue", thresh=at, tsim_zero=False)
    assert hit.tolist() == [False, True, False, True]          # both sides of the threshold, the NaN, the hit
    ts_ref, ts_e = M.rowdot_ref(temb, title[top])
    ts_ref, ts_e = np.where(hit, ts_ref, 0.0), np.where(hit, ts_e, 0.0)
    _close(o.tsim[:B, 0], _t(ts_ref), _t(ts_e), "vault tsim")
    rd = _nan(B, 1)
    _run(lib.mmf_rowdot_f32(_p(td), _p(_dn(title[top])), _p(rd), 1, B, D, _sp()))
    _same(o.tsim[:B, 0].cpu()[_t(hit)], rd[:B, 0].cpu()[_t(hit)], "tsim vs rowdot")
    for kw in (dict(temb=td), dict(title=bd)):                 # either pointer null: exactly 0
        o = _Out(B, k, ds)
        _run(lib.mmf_vault_topk_f32(_p(Sd), B, N, k, *o.args(D=D, thresh=at, **kw), ref, _sp()))
        o.check(*want, "epilogue without a bank", thresh=at)


def test_vault_topk_rejects(lib):
    Sd = _dn(V.topk_matrix(V.ROW_SETS[0], 64))
    o = _Out(1, 5)
    f = lib.mmf_vault_topk_f32
    assert f(None, 1, 64, 5, *o.args(), 0, None) == EINVAL
    assert f(_p(Sd), 0, 64, 5, *o.args(), 0, None) == EINVAL
    assert f(_p(Sd), 1, 0, 5, *o.args(), 0, None) == EINVAL
    assert f(_p(Sd), 1, 64, 0, *o.args(), 0, None) == EINVAL
    assert f(_p(Sd), 1, 64, 16385, *o.args(), 0, None) == EINVAL            # past the largest sort
    assert f(_p(Sd), 1, 64, 5, THRESH, None, None, None, 1, None, None, 0, None, 0, None) == EINVAL   # no output
    assert f(_p(Sd), 1, 64, 5, THRESH, _p(o.sims), _p(o.idx), _p(o.disc), 0, None, None, 0, None, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.sims).all()) and bool((o.idx == SENTINEL).all()) and bool(torch.isnan(o.disc).all())


# ---- the final ranking of per-chunk candidates ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("chunk_rows", [16384, 100])
@pytest.mark.parametrize("chunks,k", [(2, 12), (32, 64), (33, 64), (256, 64)])
def test_vault_sort_cand(lib, chunks, k, chunk_rows, B):
    """24 and 2048 candidates through P = 2048, 2112 and 16384 through P = 16384: -1 padding of a short last chunk,
    global indices, NaN candidates, ties across chunks; with small chunks also the caption-title cosine."""
    cs, cidx = V.cand_inputs(chunks, k, chunk_rows, B)
    want = V.cand_ref(cs, cidx, chunk_rows, k)
    o = _Out(B, k, 5)
    D = 64
    small = chunk_rows == 100
    # a threshold below the best finite candidate of the rows that have no NaN, so hits occur
    td = _dn(M.rowdot_inputs(B, D, 6)[0]) if small else None
    title = M.rowdot_inputs(chunks * chunk_rows, D, 7)[1] if small else None
    _run(lib.mmf_vault_sort_cand_f32(_p(_dn(cs)), _p(_dn(cidx)), chunks, chunk_rows, B, k,
                                     *o.args(td, _dn(title), D if small else 0), _sp()))
    hit = o.check(*want, f"sort_cand {chunks}x{k} rows={chunk_rows}", tsim_zero=not small)
    if small:
        ts_ref, ts_e = M.rowdot_ref(M.rowdot_inputs(B, D, 6)[0], title[np.maximum(want[1][:, 0], 0)])
        _close(o.tsim[:B, 0], _t(np.where(hit, ts_ref, 0.0)), _t(np.where(hit, ts_e, 0.0)), "sort_cand tsim")


@pytest.mark.parametrize("ds", [1, 5])
def test_vault_sort_cand_epilogue(lib, ds):
    """test_vault_topk_epilogue's checks behind the candidate sort: the best candidate exactly on the threshold, one
    float32 above it, a NaN and a clean hit, each in another chunk; disc, and the caption-title cosine of the
    GLOBAL top-1 row within the rowdot bound and with rowdot_kernel's bits, 0 on a miss and without a bank."""
    chunks, k, chunk_rows, B, D = 3, 12, 100, 4, 512
    g = np.random.default_rng(8)
    cs = np.sort(g.uniform(0, 0.5, (chunks, B, k)).astype(np.float32), axis=2)[:, :, ::-1].copy()
    cidx = np.stack([np.stack([g.choice(chunk_rows, k, replace=False) for _ in range(B)]) for _ in range(chunks)])
    cidx = cidx.astype(np.int32)
    _, at, above = M.around(THRESH)
    where = [2, 0, 1, 2]                                       # the chunk that holds row b's best candidate
    for b, val in enumerate((at, above, np.float32(np.nan), np.float32(0.93))):
        cs[where[b], b, 0] = val
    top = [where[b] * chunk_rows + int(cidx[where[b], b, 0]) for b in range(B)]
    want = V.cand_ref(cs, cidx, chunk_rows, k)
    assert want[1][:, 0].tolist() == top
    temb = M.rowdot_inputs(B, D, 12)[0]
    title = M.rowdot_inputs(chunks * chunk_rows, D, 13)[1]
    csd, cid, td, bd = _dn(cs), _dn(cidx), _dn(temb), _dn(title)
    o = _Out(B, k, ds)
    _run(lib.mmf_vault_sort_cand_f32(_p(csd), _p(cid), chunks, chunk_rows, B, k, *o.args(td, bd, D, at), _sp()))
    hit = o.check(*want, "sort_cand epilogue", thresh=at, tsim_zero=False)
    assert hit.tolist() == [False, True, False, True]          # both sides of the threshold, the NaN, the hit
    ts_ref, ts_e = M.rowdot_ref(temb, title[top])
    _close(o.tsim[:B, 0], _t(np.where(hit, ts_ref, 0.0)), _t(np.where(hit, ts_e, 0.0)), "sort_cand epilogue tsim")
    rd = _nan(B, 1)
    _run(lib.mmf_rowdot_f32(_p(td), _p(_dn(title[top])), _p(rd), 1, B, D, _sp()))
    _same(o.tsim[:B, 0].cpu()[_t(hit)], rd[:B, 0].cpu()[_t(hit)], "sort_cand tsim vs rowdot")
    for kw in (dict(temb=td), dict(title=bd)):                 # either pointer null: exactly 0
        o = _Out(B, k, ds)
        _run(lib.mmf_vault_sort_cand_f32(_p(csd), _p(cid), chunks, chunk_rows, B, k,
                                         *o.args(D=D, thresh=at, **kw), _sp()))
        o.check(*want, "sort_cand epilogue without a bank", thresh=at)


def test_vault_sort_cand_hits_and_rejects(lib):
    """Candidates without NaN: the shared top value 4.5 is a hit; and chunks * k > 16384 is MMF_EINVAL."""
    cs, cidx = V.cand_inputs(4, 12, 100, 3)
    cs[np.isnan(cs)] = np.float32(-3)
    want = V.cand_ref(cs, cidx, 100, 12)
    o = _Out(3, 12)
    csd, cid = _dn(cs), _dn(cidx)
    _run(lib.mmf_vault_sort_cand_f32(_p(csd), _p(cid), 4, 100, 3, 12, *o.args(), _sp()))
    assert o.check(*want, "sort_cand hits").all() and bool((o.disc[:3, 0] == 4.5).all())
    o = _Out(3, 64)
    f = lib.mmf_vault_sort_cand_f32
    assert f(_p(csd), _p(cid), 257, 100, 3, 64, *o.args(), None) == EINVAL
    assert lib.mmf_last_error()
    assert f(None, _p(cid), 4, 100, 3, 12, *o.args(), None) == EINVAL
    assert f(_p(csd), None, 4, 100, 3, 12, *o.args(), None) == EINVAL
    assert f(_p(csd), _p(cid), 0, 100, 3, 12, *o.args(), None) == EINVAL
    assert f(_p(csd), _p(cid), 4, 0, 3, 12, *o.args(), None) == EINVAL
    assert f(_p(csd), _p(cid), 4, 100, 0, 12, *o.args(), None) == EINVAL
    assert f(_p(csd), _p(cid), 4, 100, 3, 0, *o.args(), None) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.sims).all()) and bool((o.idx == SENTINEL).all())


# ---- the fused search against the ranking of the similarity kernel's own matrix ----
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("N", [65, 1001])
def test_fused_search_vs_numpy_ranking(lib, N, B):
    """mmf_vault_search_rows against vault_refs.rank applied to the S that mmf_vault_sims_f32 returned for the same
    operands, bit for bit: an expectation that shares none of the fused path's ranking code.  The bank holds
    bit-equal rows (exact ties), planted hits, and at N = 65 a NaN row (which tops every query)."""
    q, v = V.sims_inputs(B, N, 512, True, seed=9)
    v[N // 2] = v[1]
    v[N - 1] = v[1]
    q[0], q[1] = v[1], v[7]
    if N == 65:
        v[40] = np.float32(np.nan)
    qd, vd = _dn(q), _dn(v)
    S = _nan(B, N)
    _run(lib.mmf_vault_sims_f32(_p(qd), _p(vd), _p(S), B, N, 512, 0, _sp()))
    Sn = S[:B].cpu().numpy()
    any_hit = False
    for k in (1, 5, 8):
        want = V.topk_ref(Sn, k)
        for nblocks in (1, 3, 0):
            o = _Out(B, k, 5)
            ws = torch.empty(int(lib.mmf_vault_search_ws_bytes(B, k, nblocks)), dtype=torch.uint8, device="cuda")
            a = o.args()
            del a[7]    # (the fused entry takes D before k, not among the outputs)
            _run(lib.mmf_vault_search_rows(_p(qd), _p(vd), B, N, 512, k, *a, _p(ws), ws.numel(), nblocks, _sp()))
            any_hit |= bool(o.check(*want, f"fused search N={N} B={B} k={k} nblocks={nblocks}").any())
    assert any_hit == (N != 65)
    if N != 65:     # query 0 ties on the three bit-equal rows: descending index
        assert V.topk_ref(Sn, 5)[1][0, :3].tolist() == [N - 1, N // 2, 1]
