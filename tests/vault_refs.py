"""Inputs, references and the derived similarity bound of the vault's stages (csrc/vault.hip: the similarity
matrix, the register and LDS-sort top-k, the final ranking of per-chunk candidates, the top-1 epilogue), shared by
tests/test_vault_refs_cpu.py (no GPU) and tests/test_gpu_vault_kernels.py.

The conventions are those of tests/transformer_refs.py.  The similarity reference is float64 numpy with a bound
derived from the kernel's one chain of D fmaf per output at U = 2^-24, times MARGIN = 2.  The ranking kernels
select and copy values, so everything they return is exact: the expectation is the numpy ranking `rank` below,
which shares no code with the kernels' `better`, insert, wave selection or sort network, and results are compared
on their bit patterns (NaN and the sign of zero included)."""
import numpy as np

U = 2.0 ** -24
MARGIN = 2.0
F32 = np.float32
NEG_INF = F32(-np.inf)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def bits(a):
    """The bit patterns of a float32 array (int32); other dtypes unchanged."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------
# The ranking
# ---------------------------------------------------------------------------------------------
def rank(s, k, idx=None):
    """The project's ranking of one row of similarities: value descending, NaN first, exact ties (+0.0 and -0.0 are
    one) by descending index (what np.argsort(s)[::-1] gives with a stable sort) -> (values, indices) of the first
    k.  idx: the candidates' own (global) indices instead of their positions."""
    s = np.asarray(s)
    idx = np.arange(len(s)) if idx is None else np.asarray(idx)
    key = np.where(np.isnan(s), np.inf, s)
    order = np.lexsort((-idx.astype(np.int64), -key))[:k]
    return s[order], idx[order]


def rank_padded(s, k, idx=None):
    """rank for a fixed k: slots past the candidates hold (-inf, -1) -> (float32 [k], int32 [k])."""
    v, i = rank(s, k, idx)
    pv, pi = np.full(k, NEG_INF, F32), np.full(k, -1, np.int32)
    pv[:len(v)], pi[:len(i)] = v, i
    return pv, pi


def rank_defective(s, k, defect, idx=None):
    """rank with a planted defect: "ties_ascending" -- exact ties by ascending index; "nan_last" -- NaN ranked
    after every number; "no_unkey" -- the NaN key +inf returned as it is."""
    s = np.asarray(s)
    idx = np.arange(len(s)) if idx is None else np.asarray(idx)
    key = np.where(np.isnan(s), -np.inf if defect == "nan_last" else np.inf, s)
    tie = idx.astype(np.int64) if defect == "ties_ascending" else -idx.astype(np.int64)
    order = np.lexsort((tie, -key))[:k]
    v = s[order]
    if defect == "no_unkey":
        v = np.where(np.isnan(v), F32(np.inf), v).astype(F32)
    pv, pi = np.full(k, NEG_INF, F32), np.full(k, -1, np.int32)
    pv[:len(v)], pi[:len(order)] = v, idx[order]
    return pv, pi


def top1_ref(v0, i0, thresh):
    """The epilogue's decision on the best candidate: a hit is a top-1 above the threshold that is neither NaN nor
    an empty slot -> (hit, disc = the top-1 of a hit, else 0)."""
    hit = bool(i0 >= 0 and not np.isnan(v0) and v0 > F32(thresh))
    return hit, (F32(v0) if hit else F32(0))


def cand_ref(cs, cidx, chunk_rows, k, defect=None):
    """The final ranking of cs / cidx [chunks][B][k] per-chunk results: the valid candidates (local index >= 0)
    with their global index chunk * chunk_rows + local, ranked -> (float32 [B][k], int32 [B][k]).  defects:
    "no_offset" -- the chunk's row offset dropped; "rank_empty" -- the -1 candidates ranked with their value;
    "pad_zero" -- slots past the candidates hold (0, 0)."""
    chunks, B, _ = cs.shape
    out_v, out_i = np.zeros((B, k), F32), np.zeros((B, k), np.int32)
    for b in range(B):
        v, li = cs[:, b, :].reshape(-1), cidx[:, b, :].reshape(-1).astype(np.int64)
        gi = li if defect == "no_offset" else np.repeat(np.arange(chunks, dtype=np.int64), cs.shape[2]) * chunk_rows + li
        ok = np.ones_like(li, bool) if defect == "rank_empty" else li >= 0
        out_v[b], out_i[b] = rank_padded(v[ok], k, gi[ok])
        if defect == "pad_zero":
            empty = out_i[b] < 0
            out_v[b][empty], out_i[b][empty] = 0, 0
    return out_v, out_i


# ---------------------------------------------------------------------------------------------
# Contents of a similarity matrix for the top-k kernels (finite or NaN only: the kernels document that +inf
# cannot occur)
# ---------------------------------------------------------------------------------------------
ROW_KINDS = ("mixed", "zeros", "equal", "all_nan", "ascending", "descending")
ROW_SETS = (("mixed",), ("mixed", "zeros", "equal"), ("all_nan", "ascending", "descending"))  # B = 1, 3, 3


def topk_row(kind, N, seed=0):
    """One row of N similarities.
      mixed     : seeded normals; the largest value 5.0 planted at j, j + 64, j + 256 and j + 2048 (the lane, wave
                  and stride partitions of the register kernel), as far as they exist, and at N - 1; three NaNs
                  (N >= 8), which rank first by descending index
      zeros     : negative numbers with +0.0, -0.0, +0.0 planted: the top is a tie of zeros of both signs
      equal / all_nan : one value everywhere
      ascending / descending : 0, 1, 2, ... and its reverse."""
    g = _rng(N, ROW_KINDS.index(kind), seed, 23)
    if kind == "mixed":
        s = g.standard_normal(N).astype(F32)
        j = int(g.integers(0, min(N, 64)))
        for o in (0, 64, 256, 2048):
            if j + o < N:
                s[j + o] = F32(5.0)
        s[N - 1] = F32(5.0)
        if N >= 8:
            s[g.choice(N - 1, 3, replace=False)] = F32(np.nan)
        return s
    if kind == "zeros":
        s = (-1 - np.abs(g.standard_normal(N))).astype(F32)
        for p, z in zip(g.choice(N, min(N, 3), replace=False), (F32(0.0), F32(-0.0), F32(0.0))):
            s[p] = z
        return s
    if kind == "equal":
        return np.full(N, F32(1.25))
    if kind == "all_nan":
        return np.full(N, F32(np.nan))
    s = np.arange(N, dtype=F32)
    return s if kind == "ascending" else s[::-1].copy()


def topk_matrix(kinds, N, seed=0):
    return np.stack([topk_row(kd, N, seed) for kd in kinds])


def topk_ref(S, k):
    """rank_padded of every row -> (float32 [B][k], int32 [B][k])."""
    out = [rank_padded(row, k) for row in S]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def cand_inputs(chunks, k, chunk_rows, B, seed=0):
    """cs / cidx [chunks][B][k] as the per-chunk top-k leaves them: distinct chunk-local indices, values descending
    within a chunk; NaN candidates (first in their chunk), one value shared by several chunks (ties across chunks,
    at the top of the ranking), and a short last chunk: only k / 3 candidates, the rest (-inf, -1)."""
    g = _rng(chunks, k, chunk_rows, B, seed, 29)
    cs = np.zeros((chunks, B, k), F32)
    cidx = np.zeros((chunks, B, k), np.int32)
    for c in range(chunks):
        for b in range(B):
            v = g.standard_normal(k).astype(F32)
            if c % 3 == 0:
                v[0] = F32(4.5)                     # the same top value in every third chunk
            if (c + 2 * b) % 5 == 1:
                v[0] = F32(np.nan)
            li = g.choice(chunk_rows, k, replace=False).astype(np.int32)
            order = np.lexsort((-li.astype(np.int64), -np.where(np.isnan(v), np.inf, v)))
            cs[c, b], cidx[c, b] = v[order], li[order]
    keep = max(1, k // 3)
    cs[-1, :, keep:], cidx[-1, :, keep:] = NEG_INF, -1
    return cs, cidx


# ---------------------------------------------------------------------------------------------
# The similarity matrix (vault_sims_kernel, vault_sims_mfma_kernel)
# ---------------------------------------------------------------------------------------------
def sims_inputs(B, N, D, unit, seed=0):
    """q [B][D], v [N][D]: unit rows, or unnormalised rows of mixed magnitude (row scales 2^-6 .. 2^6)."""
    g = _rng(B, N, D, int(unit), seed, 31)
    q, v = g.standard_normal((B, D)), g.standard_normal((N, D))
    if unit:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    else:
        q *= 2.0 ** g.integers(-6, 7, (B, 1))
        v *= 2.0 ** g.integers(-6, 7, (N, 1))
    return q.astype(F32), v.astype(F32)


def sims_ref(q, v):
    """S = q v^T in float64, and the bound of the kernels' value: every output is one chain of D fmaf over
    k = 0 .. D - 1 from 0, so e = D U sum_k |q_k v_k|, times MARGIN."""
    q, v = q.astype(np.float64), v.astype(np.float64)
    return q @ v.T, MARGIN * q.shape[1] * U * (np.abs(q) @ np.abs(v).T)


def sims_emulate(q, v, defect=None):
    """float32 emulation: the ascending-k fmaf chain of every output.  defects: "drop_last_chunk" -- the last
    16-deep K chunk left out; "swap_rows" -- vault rows n and n + 1 exchanged inside each group of four rows that
    a lane of the MFMA kernel stores (n % 4 == 0)."""
    B, D = q.shape
    acc = np.zeros((B, v.shape[0]), F32)
    for k in range(D - 16 if defect == "drop_last_chunk" else D):
        acc = (q[:, k].astype(np.float64)[:, None] * v[:, k].astype(np.float64)[None, :] + acc).astype(F32)
    if defect == "swap_rows":
        n = np.arange(0, v.shape[0] - 1, 4)
        acc[:, np.concatenate([n, n + 1])] = acc[:, np.concatenate([n + 1, n])]
    return acc
