"""tests/vault_refs.py certified without a GPU: the similarity bound against a float32 emulation of the kernels'
ascending-k fmaf chain (under half of the bound; planted defects outside it), and the numpy ranking against planted
ranking defects on the very inputs tests/test_gpu_vault_kernels.py uses (each defect must break the exact
comparison, so a kernel with that defect fails there)."""
import numpy as np
import pytest

from tests import vault_refs as V


def _same(a, b):
    return all(np.array_equal(V.bits(x), V.bits(y)) for x, y in zip(a, b))


# ---- similarities ----
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("B,N,D", [(1, 1, 64), (17, 65, 64), (33, 130, 512), (16, 63, 512)])
def test_sims_bound(B, N, D, unit):
    q, v = V.sims_inputs(B, N, D, unit)
    ref, e = V.sims_ref(q, v)
    err = np.abs(V.sims_emulate(q, v).astype(np.float64) - ref)
    ratio = float((err / np.maximum(e, 1e-300)).max())
    print(f"RATIO emu vault_sims D={D} unit={unit}: {ratio:.3g}")
    assert bool((err <= e / 2).all()), ratio
    if N >= 63:
        for defect in ("drop_last_chunk", "swap_rows"):
            bad = np.abs(V.sims_emulate(q, v, defect).astype(np.float64) - ref) > e
            if defect == "swap_rows":   # the affected columns: the first two of every group of four
                n = np.arange(0, N - 1, 4)
                bad = bad[:, np.concatenate([n, n + 1])]
            assert float(bad.mean()) > 0.5, (defect, float(bad.mean()))


# ---- the ranking ----
def test_rank_on_a_hand_made_row():
    nan = np.float32(np.nan)
    s = np.array([1.0, nan, 3.0, 3.0, -0.0, 0.0, nan, -2.0], np.float32)
    v, i = V.rank(s, 8)
    assert i.tolist() == [6, 1, 3, 2, 0, 5, 4, 7]
    assert np.array_equal(V.bits(v), V.bits(s[[6, 1, 3, 2, 0, 5, 4, 7]]))
    pv, pi = V.rank_padded(s[:3], 5)
    assert pi.tolist() == [1, 2, 0, -1, -1] and bool(np.isneginf(pv[3:]).all())
    assert V.top1_ref(np.float32(0.9), 3, 0.85) == (True, np.float32(0.9))
    assert V.top1_ref(np.float32(0.85), 3, 0.85)[0] is False
    assert V.top1_ref(np.nextafter(np.float32(0.85), np.float32(1)), 3, 0.85)[0] is True
    assert V.top1_ref(nan, 3, 0.85) == (False, np.float32(0)) and V.top1_ref(V.NEG_INF, -1, 0.85)[0] is False


@pytest.mark.parametrize("N", [65, 257, 2049, 4097])
def test_ranking_defects_break_the_comparison(N):
    """On the `mixed` row (ties across the partitions, NaNs) every planted ranking defect changes the first k."""
    s = V.topk_row("mixed", N)
    for k in (5, 8):
        want = V.rank_padded(s, k)
        assert bool(np.isnan(want[0][:3]).all()) and want[1][0] > want[1][1] > want[1][2]   # NaN first, index descending
        assert bool((want[0][3:5] == 5.0).all()) and want[1][3] > want[1][4]                 # then the planted tie
        for defect in ("ties_ascending", "nan_last", "no_unkey"):
            assert not _same(V.rank_defective(s, k, defect), want), defect
    z = V.topk_row("zeros", N)
    want = V.rank_padded(z, 3)
    assert bool((want[0] == 0).all()) and want[1].tolist() == sorted(want[1].tolist(), reverse=True)
    assert len({int(b) for b in V.bits(want[0])}) == 2     # zeros of both signs among the top three
    assert not _same(V.rank_defective(z, 3, "ties_ascending"), want)


def test_k_above_n_pads():
    s = V.topk_row("mixed", 3)
    v, i = V.rank_padded(s, 8)
    assert bool((i[3:] == -1).all()) and bool(np.isneginf(v[3:]).all()) and sorted(i[:3].tolist()) == [0, 1, 2]


@pytest.mark.parametrize("chunks,k", [(2, 12), (33, 64)])
@pytest.mark.parametrize("chunk_rows", [16384, 100])
def test_cand_defects_break_the_comparison(chunks, k, chunk_rows):
    cs, cidx = V.cand_inputs(chunks, k, chunk_rows, 3)
    assert bool((cidx[-1, :, -1] == -1).all()) and bool(np.isnan(cs).any())
    want = V.cand_ref(cs, cidx, chunk_rows, k)
    assert bool((want[1] >= 0).all()) and int(want[1].max()) >= chunk_rows       # global indices past chunk 0
    assert bool(np.isnan(want[0][:, 0]).any())
    for defect in ("no_offset",):
        assert not _same(V.cand_ref(cs, cidx, chunk_rows, k, defect), want), defect
    # a -1 candidate ranked / padding that is not (-inf, -1): visible where the valid candidates do not fill k
    few_cs, few_idx = cs[-1:, :, :], cidx[-1:, :, :]
    want = V.cand_ref(few_cs, few_idx, chunk_rows, k)
    assert bool((want[1][:, -1] == -1).all())
    bad = V.cand_ref(few_cs, few_idx, chunk_rows, k, "pad_zero")
    assert not _same(bad, want)
    neg = few_cs.copy()
    neg[few_idx < 0] = np.float32(9.0)      # an empty slot that carries a large value must still not rank
    assert _same(V.cand_ref(neg, few_idx, chunk_rows, k), want)
    assert not _same(V.cand_ref(neg, few_idx, chunk_rows, k, "rank_empty"), want)
