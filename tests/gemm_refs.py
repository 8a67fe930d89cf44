"""Cases, poisoned operands, float64 references and a float32 emulation of the plain (epilogue 0) fp16 GEMM:
every instantiation of csrc/gemm.hip (register-staged tiles 0 - 3, LDS-DMA tiles 5 / 10 / 11 with
csrc/gemm_glds_body.inc) and the streaming 1x1 kernel of csrc/pointwise.hip (config 9), shared by
tests/test_gemm_refs_cpu.py (no GPU: the emulation under half of the bound, planted defects outside it) and
tests/test_gpu_gemm_kernels.py (the kernels, through mmf_gemm_f16_raw).

The reference and its bound are transformer_refs.gemm_ref with chain = K + 4, computed from K and the operand
magnitudes beside the reference -- never from what a kernel returned.  An fp16 output adds store16's half-ulp.
With an SE scale the reference starts from the operand the kernels form: fp16(float(A) * s), an fp32 product
rounded to nearest even -- not one rounding of the float64 product."""
import collections
import itertools

import numpy as np
import torch

from tests.transformer_refs import (OUT_KINDS, RES_KINDS, U, _gen, act32, act64, act_err, gemm_inputs, gemm_ref,  # noqa: F401
                                    half_ulp16, store16)

NAN = float("nan")
PAD_ROWS = 16                 # poisoned rows behind A and W
LDA_PAD, LDW_PAD = 8, 16      # lda = K + 8, ldw = K + 16
LDR_PAD, LDC_PAD = 4, 8       # ldr = N + 4 != ldc = N + 8

# BM x BN of the tiled instantiations (gemm.hip launch_gemm)
TILES = {0: (256, 32), 1: (256, 64), 2: (64, 128), 3: (128, 128), 5: (256, 128), 10: (256, 192), 11: (256, 256)}
REG_CONFIGS = (0, 1, 2, 3)
GLDS_CONFIGS = (5, 10, 11)
PW_CONFIG = 9
EXISTING = (0, 1, 2, 3, 5, 9, 10, 11)
REMOVED = (4, 6, 7, 8, 12, 13, 14, 15, 16)      # (15 / 16 exist in measurement builds only)

# cfg: forced instantiation (-1: automatic); rpb: rows_per_batch of the SE scale (0: none); inplace: res32 is c32
Case = collections.namedtuple("Case", "cfg M N K act bias res outs rpb inplace")


def case_id(c):
    return (f"cfg{c.cfg}-M{c.M}-N{c.N}-K{c.K}-act{c.act}-{'b' if c.bias else 'nb'}-{c.res}-{c.outs}"
            + (f"-rpb{c.rpb}" if c.rpb else "") + ("-inplace" if c.inplace else ""))


def _rot(j):
    """(act, bias, residual kind, outputs) of rotation step j: as transformer_refs.splitk_cases rotates them."""
    return j % 5, j % 2 == 0, RES_KINDS[(j + j // 3) % 3], OUT_KINDS[(j + j // 9) % 3]


# ---------------------------------------------------------------------------------------------
# The case tables
# ---------------------------------------------------------------------------------------------
REG_K = (8, 56, 64, 72, 136, 200)      # nk = 1 .. 4 K-steps of 64, with and without a K tail
ASC_RPB = (49, 196)


def reg_cases():
    """Register-staged tiles.  Per config every (N, K) pair of N in {4, BN - 4, BN + 4, 2 BN + 12} and REG_K, M
    rotating through {1, BM - 1, BM + 1, 2 BM + 17} and the epilogue forms rotating (offset per config, so that the
    configs do not all see the same combinations); then the ASC instantiation: an SE scale with rows_per_batch
    49 and 196 over an M that is no multiple of it, with an fp32 output (see SHOWS_IN_C32)."""
    cases = []
    for ci, cfg in enumerate(REG_CONFIGS):
        BM, BN = TILES[cfg]
        Ms = (1, BM - 1, BM + 1, 2 * BM + 17)
        Ns = (4, BN - 4, BN + 4, 2 * BN + 12)
        for i, (N, K) in enumerate(itertools.product(Ns, REG_K)):
            act, bias, res, outs = _rot(i + 7 * ci)
            cases.append(Case(cfg, Ms[(i + i // 4 + ci) % 4], N, K, act, bias, res, outs, 0, False))
        cases.append(Case(cfg, BM + 1, BN + 4, 72, 3, True, "res16", "both", 49, False))
        cases.append(Case(cfg, max(2 * BM + 17, 209), 2 * BN + 12, 136, 0, True, "none", "c32", 196, False))
    return cases


GLDS_M = (1, 255, 256, 257, 513)
GLDS_K = (64, 128, 192, 256, 320)      # nk = 1 .. 5: every depth of the two-stage PIPE2 pipeline's start-up and drain


def glds_cases():
    """LDS-DMA tiles.  Per config every (N, K) pair of N in {4, BN - 4, BN, BN + 4, 2 BN + 12} (N % 8 == 4: the
    full8 == false stores) and GLDS_K, M rotating through GLDS_M; then the in-place residual exactly as
    text_host.cpp / clip_host.cpp use it on the plain epilogue: res32 == c32, fp32 output only, ldr == ldc, with a
    bias (the out-projections and FFN-2 of the compact last layers) and without one (the lo-word query GEMM)."""
    cases = []
    for ci, cfg in enumerate(GLDS_CONFIGS):
        BN = TILES[cfg][1]
        Ns = (4, BN - 4, BN, BN + 4, 2 * BN + 12)
        for i, (N, K) in enumerate(itertools.product(Ns, GLDS_K)):
            act, bias, res, outs = _rot(i + 4 * ci)
            cases.append(Case(cfg, GLDS_M[(i + i // 5 + ci) % 5], N, K, act, bias, res, outs, 0, False))
        cases.append(Case(cfg, 257, BN, 128, 2, True, "none", "c16", 0, False))      # the paired fp16 stores, N % 8 == 0
        cases.append(Case(cfg, 255, BN - 4, 64, 1, True, "none", "c32", 0, False))      # GELU where its form shows (SHOWS_IN_C32)
        cases.append(Case(cfg, 257, BN + 4, 128, 0, True, "res32", "c32", 0, True))
        cases.append(Case(cfg, 513, 2 * BN + 12, 192, 0, False, "res32", "c32", 0, True))
    return cases


WALK_GROUP_M = (1, 4, 5, 18, 64)
WALK_TILES = (18, 16)


def walk_cases():
    """Persistent walk: 18 x 16 = 288 tiles for 256 workgroups, ragged last row and column panels, K = 128 (two
    K-steps: the next tile's first slab is prefetched during the second).  One epilogue form per config: the paired
    fp16 stores with N % 8 == 4, the fp16 residual, the fp32 residual with both outputs."""
    forms = {5: (1, True, "none", "c16"), 10: (0, True, "res16", "c32"), 11: (3, True, "res32", "both")}
    return [Case(cfg, 17 * 256 + 3, 15 * TILES[cfg][1] + 4, 128, *forms[cfg], 0, False) for cfg in GLDS_CONFIGS]


PW_K = (8, 32, 40, 64, 72, 96, 104, 128, 136, 160, 168, 192, 200, 256)     # KS = 1 1 2 2 3 3 4 4 5 5 6 6 8 8 (7 -> 8)
PW_N = ((8, 24, 32), (40, 64), (72, 128, 136, 264))                        # CF = 2, 4, 8 (nbn = 1, 2, 3)
PW_M = (2048, 2049, 2048 + 63)


def pw_ks(K):
    ks = (K + 31) // 32
    return 8 if ks == 7 else ks


def pw_rows(K):
    """Rows of a row block of pw_kernel (pointwise.hip pw_rpw)."""
    ks = pw_ks(K)
    return 4 * (4 if ks <= 2 else (2 if ks <= 4 else 1)) * 16


def pw_grid_x(N, M, K):
    """run_pw's persistent grid width."""
    nbn = 1 if N <= 64 else (N + 127) // 128
    gx = (1024 + nbn - 1) // nbn
    if nbn > 1:
        gx = gx // 8 * 8
    return min(gx, (M + pw_rows(K) - 1) // pw_rows(K))


def pw_cases():
    """pw_conv: every K of PW_K with one N of every column-fragment count (so every KS x CF template, with SiLU and
    without: the two K of a KS take the two activations, swapped from one CF to the next), N = 264 only with
    K <= 128 (pw_applicable); the SE scale with rows_per_batch 49 / 196, the fp16 residual (ldr != ldc) and the
    bias rotating.  Then one case per row-block height (256, 128, 64 rows) whose M is derived from run_pw's grid:
    four row blocks more than workgroups in x and a ragged last block, so the first four workgroups walk two."""
    cases = []
    j = 0
    for ki, K in enumerate(PW_K):
        for cf, Ns in enumerate(PW_N):
            N = Ns[(ki + cf) % len(Ns)]
            if N == 264 and K > 128:
                N = 136
            act = 3 if (ki + cf) % 2 else 0
            rpb = (0, 49, 196)[(j + j // 3) % 3]
            cases.append(Case(PW_CONFIG, PW_M[j % 3], N, K, act, j % 4 != 3, ("none", "res16")[(j // 2) % 2], "c16", rpb, False))
            j += 1
    for K, N, act, res, rpb in ((8, 8, 3, "res16", 196), (72, 24, 0, "none", 49), (136, 136, 3, "res16", 0)):
        gx = pw_grid_x(N, 1 << 30, K)
        cases.append(Case(PW_CONFIG, (gx + 3) * pw_rows(K) + 37, N, K, act, True, res, "c16", rpb, False))
    return cases


def all_cases():
    return reg_cases() + glds_cases() + walk_cases() + pw_cases()


# Defects of gemm_emulate and the cases of the tables in which each can show
DEFECTS = ("drop_last_k8", "skip_tile", "bias_clamped_col", "res_before_act", "gelu_tanh", "scale_unrounded",
           "group_dup_tile")
# Defects smaller than the rounding of an fp16 store, which therefore need an fp32 output:
#  * gelu_tanh: the tanh form is within about 5e-4 of the erf form, largest near |x| = 2, where half an fp16 ulp
#    is 2^-11 = 4.9e-4;
#  * scale_unrounded: the missing rounding of A * s is 2^-12 relative per term on average, and so is half an
#    fp16 ulp of the result.
# The fp32 bound grows with K (2.4 (K + 4) U sum |a| |w|, about 1.5e-7 K^1.5 for these operands): it passes the
# tanh gap near K = 200, so gelu_tanh is held to K <= 136.
SHOWS_IN_C32 = ("gelu_tanh", "scale_unrounded")
GELU_TANH_MAX_K = 136


def shows(defect, c):
    """Whether `defect` changes the result of case c by more than its bound somewhere."""
    if defect in SHOWS_IN_C32 and c.outs == "c16":
        return False
    if defect == "bias_clamped_col":
        return c.bias
    if defect == "res_before_act":
        return c.res != "none" and c.act != 0
    if defect == "gelu_tanh":
        return c.act == 1 and c.K <= GELU_TANH_MAX_K
    if defect == "scale_unrounded":
        return c.rpb > 0
    if defect == "group_dup_tile":      # (with one tile the walk's first tile is its last)
        bm, bn = emulate_tile(c)
        return (c.M + bm - 1) // bm * ((c.N + bn - 1) // bn) > 1
    return True


# ---------------------------------------------------------------------------------------------
# tile_coords (gemm.hip) in Python: which tile the persistent kernel's t-th step computes
# ---------------------------------------------------------------------------------------------
def tile_coords(t, tilesM, tilesN, gm):
    if gm <= 0:
        return t // tilesN, t % tilesN
    per_group = gm * tilesN
    group = t // per_group
    first_m = group * gm
    gsz = min(tilesM - first_m, gm)
    r = t - group * per_group
    return first_m + r % gsz, r // gsz


def tile_order(tilesM, tilesN, gm):
    return [tile_coords(t, tilesM, tilesN, gm) for t in range(tilesM * tilesN)]


# ---------------------------------------------------------------------------------------------
# Operands
# ---------------------------------------------------------------------------------------------
def _poisoned(t, rows, ld):
    buf = torch.full((rows, ld), NAN, dtype=t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf


def scale_rows(c, seed=0):
    """The SE excitation fp32 [ceil(M / rpb)][K] in (0.05, 1) (a sigmoid's range), or None."""
    if not c.rpb:
        return None
    nb = (c.M + c.rpb - 1) // c.rpb
    return 0.05 + 0.95 * torch.rand(nb, c.K, generator=_gen(c.M, c.K, c.rpb, seed, 73))


def scaled_operand(A, s, rpb):
    """fp16(float(A) * s[m / rpb]): the A operand exactly as gemm_f16_kernel<ASC> and pw_kernel form it."""
    rows = torch.arange(A.shape[0]) // rpb
    return (A.float() * s.float()[rows]).half()


Operands = collections.namedtuple("Operands", "A W bias res scale Ap Wp biasp resp scalep lda ldw ldr ldc")


def operands(c, seed=0):
    """Clean operands (A fp16 [M][K], W fp16 [N][K], bias fp32 or None, the residual in its kind's precision or None,
    scale) and the buffers a launch gets: A in [M + 16][lda], W in [N + 16][ldw], the residual in [M][ldr], bias
    and scale with 16 entries / one row behind them -- every element that is not an operand is NaN, so a read of
    padding that reaches a result fails the per-element comparison."""
    A, W, bv, rv = gemm_inputs(c.M, c.N, c.K, seed)
    bias = bv if c.bias else None
    res = None if c.res == "none" else (rv if c.res == "res32" else rv.half())
    s = scale_rows(c, seed)
    lda, ldw = c.K + LDA_PAD, c.K + LDW_PAD
    ldc = c.N + LDC_PAD
    ldr = ldc if c.inplace else c.N + LDR_PAD
    Ap = _poisoned(A, c.M + PAD_ROWS, lda)
    Wp = _poisoned(W, c.N + PAD_ROWS, ldw)
    biasp = None if bias is None else _poisoned(bias[None], 1, c.N + 16)[0]
    resp = None if res is None else _poisoned(res, c.M, ldr)
    sp = None if s is None else _poisoned(s, s.shape[0] + 1, c.K)
    return Operands(A, W, bias, res, s, Ap, Wp, biasp, resp, sp, lda, ldw, ldr, ldc)


def reference(c, ops):
    """(ref, e) of case c in float64: gemm_ref with chain = K + 4 from the operand the kernels multiply."""
    A = ops.A if ops.scale is None else scaled_operand(ops.A, ops.scale, c.rpb)
    return gemm_ref(A, ops.W, ops.bias, ops.res, c.act, c.K + 4)


# ---------------------------------------------------------------------------------------------
# float32 emulation
# ---------------------------------------------------------------------------------------------
def _gelu_tanh32(x):
    return 0.5 * x * (1 + torch.tanh(np.float32(0.7978845608028654) * (x + np.float32(0.044715) * x * x * x)))


def gemm_emulate(c, ops, bm, bn, gm=0, defect=None):
    """The GEMM of case c in float32, one bm x bn tile at a time in tile_coords' order (gm: gemm_group_m), on the
    kernels' rounding points: fp16(A * s), fp32 accumulation, + bias, the activation, + residual.  Returns the fp32
    values [M][N]; an fp16 store is .half() of them.  Elements no tile wrote stay NaN.  Defects:
      drop_last_k8      the last 8-wide K chunk is not accumulated
      skip_tile         the last tile of the walk is not computed
      bias_clamped_col  a column takes bias[min(n, N - 4)]: the clamp of the N-tail's vector load applied to
                        in-range columns
      res_before_act    the residual is added before the activation
      gelu_tanh         GELU in its tanh form
      scale_unrounded   A * s enters the product without its fp16 rounding
      group_dup_tile    the walk computes its first tile again instead of its last one"""
    M, N, K = c.M, c.N, c.K
    a = ops.A.float()
    if ops.scale is not None:
        rows = torch.arange(M) // c.rpb
        a = a * ops.scale[rows]
        if defect != "scale_unrounded":
            a = a.half().float()
    w = ops.W.float()
    if defect == "drop_last_k8":
        a, w = a[:, :K - 8], w[:, :K - 8]
    bias = ops.bias
    if bias is not None and defect == "bias_clamped_col":
        bias = bias[torch.arange(N).clamp_max(N - 4)]
    tilesM, tilesN = (M + bm - 1) // bm, (N + bn - 1) // bn
    order = tile_order(tilesM, tilesN, gm)
    if defect == "skip_tile":
        order = order[:-1]
    if defect == "group_dup_tile":
        order = order[:-1] + order[:1]
    out = torch.full((M, N), NAN)
    for tm, tn in order:
        ms, ns = slice(tm * bm, min(M, (tm + 1) * bm)), slice(tn * bn, min(N, (tn + 1) * bn))
        v = a[ms] @ w[ns].T
        if bias is not None:
            v = v + bias[ns]
        r = None if ops.res is None else ops.res[ms, ns].float()
        if r is not None and defect == "res_before_act":
            v = v + r
        v = _gelu_tanh32(v) if (defect == "gelu_tanh" and c.act == 1) else act32(v, c.act)
        if r is not None and defect != "res_before_act":
            v = v + r
        out[ms, ns] = v
    return out


def emulate_tile(c):
    """The tile gemm_emulate walks for case c: the instantiation's, pw_conv as its row block x 128 columns."""
    return TILES[c.cfg] if c.cfg in TILES else (pw_rows(c.K), 128)


# ---------------------------------------------------------------------------------------------
# gemm_config's ladder (gemm.hip), for the unforced dispatch cases
# ---------------------------------------------------------------------------------------------
def glds_pick(M, N, with_128=True):
    tm = (M + 255) // 256
    best, bc = 11, 1e30
    for bn, cfg, eff in ((256, 11, 1.0), (192, 10, 0.88), (128, 5, 0.80))[:3 if with_128 else 2]:
        tiles = tm * ((N + bn - 1) // bn)
        cost = float((tiles + 255) // 256) * bn / eff
        if cost < bc:
            bc, best = cost, cfg
    return best


def ladder_cases():
    """(case, expected config) at one shape per rung of gemm_config's automatic choice, in its order: pw_conv; N <= 32;
    N <= 64; M <= 512; the LDS-DMA tiles (K % 64 == 0, N >= 128: glds_pick); and, without them (K % 64 != 0), 64 x 128
    tiles while 128 x 128 ones would number fewer than 384, 128 x 128 from there.  The last four write fp32, which
    pw_conv does not."""
    t = []
    t.append((Case(-1, 2048, 32, 32, 0, True, "none", "c16", 0, False), 9))
    t.append((Case(-1, 2047, 32, 32, 0, True, "none", "c16", 0, False), 0))
    t.append((Case(-1, 2047, 64, 32, 0, True, "none", "c16", 0, False), 1))
    t.append((Case(-1, 512, 136, 64, 0, True, "none", "c32", 0, False), 2))
    for N in (136, 11008, 16512):       # three row panels: 256 x 128 tiles; 258 of them, so 256 x 192; 261 of those, so 256 x 256
        t.append((Case(-1, 513, N, 64, 0, True, "none", "c32", 0, False), glds_pick(513, N)))
    t.append((Case(-1, 47 * 128, 1024, 72, 0, True, "none", "c32", 0, False), 2))
    t.append((Case(-1, 47 * 128 + 1, 1024, 72, 0, True, "none", "c32", 0, False), 3))
    return t
