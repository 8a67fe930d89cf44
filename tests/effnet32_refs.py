"""Inputs, float64 references, derived bounds and float32 emulations of the fp32 EfficientNet tower's
kernels (csrc/effnet_f32.hip, stem_kernel<*, float> of csrc/effnet.hip), shared by
tests/test_effnet32_refs_cpu.py (no GPU) and tests/test_gpu_effnet32_kernels.py.

Every reference is plain torch float64, computed from the operands the kernel receives.  Every bound is
computed beside its reference from the number formats and the kernel's chain lengths (first-order worst
case times 2) -- never from what a kernel returned.  U = 2^-24 is the fp32 unit roundoff.

Worst-case bounds over long fp32 chains are blunt (results sit at 0.002 of them), so two
sharper instruments stand beside them:

  exact cases   inputs on a dyadic grid (multiples of 2^-3: activations, biases, residuals in [-2, 2],
                weights in [-1, 1], SE scales in {1/4, 1/2, 1, 2}).  A scaled activation is a multiple of
                2^-5 of at most 4, a product a multiple of 2^-8 of at most 4, and with K <= 1152 terms and
                the bias every partial sum is below (4 * 1152 + 2) * 2^8 < 2^21 units of 2^-8: all of them
                are fp32 numbers.  The pre-activation then has no rounding in ANY summation order; the
                kernel must equal the float64 reference bit for bit (act none) or within the evaluation
                error of the SiLU alone, act_err (effnet_refs).
  fixed orders  sum32's documented order is emulated in numpy float32 and compared bit for bit; the
                pw32_mfma modes are compared bit for bit with mode 0.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.effnet_refs import MEAN, STD, U, _gen, act_err

VALU, MFMA, ROWS = 0, 1, 2  # mmf_pw32_variant's kinds
ACT_NONE, ACT_SILU = 0, 3


def dyadic(shape, lim, g):
    """Multiples of 2^-3 in [-lim, lim], float32."""
    return torch.randint(-8 * lim, 8 * lim + 1, shape, generator=g).float() / 8


def silu32(x):
    """x / (1 + expf(-x)) in float32 (numpy): the kernels' silu_precise."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return x / (np.float32(1) + np.exp(-x))


# ---- pw32: C = act((A .* ascale[image]) W^T + bias) (+ res) ----
# form -> (act, ascale?, residual?).  expand / project are the tower's two uses; full has the residual
# behind a SiLU, where adding it before the activation is a different result.
FORMS = {"expand": (ACT_SILU, False, False), "project": (ACT_NONE, True, True), "full": (ACT_SILU, True, True)}
RPI = 49  # rows per image with ascale: a 64-row tile spans two images


def _pw_cases():
    """Each case: (M, N, K, form, {mode: (kind, D, NF)}) -- the variant mmf_pw32_variant must report under
    each listed pw32_mfma mode.  The GPU test runs every case under every mode 0..5."""
    cases = []
    # (a) every pw32r<NF, D>, mode 4, M = 130 (two full 64-row blocks and one of 2 rows); N = 16 NF - 12: the
    # last fragment is one float4 wide; K = 24: chunks 16 + 8, D = 2; K = 72: five chunks, the last 8 wide, D = 4
    for nf in range(1, 17):
        for N in (16 * nf - 12, 16 * nf):
            cases.append((130, N, 24, "expand", {4: (ROWS, 2, nf)}))
            cases.append((130, N, 72, "project", {4: (ROWS, 4, nf)}))
    for N, nf in ((40, 3), (256, 16)):
        for K in (4, 12, 16, 64):
            cases.append((130, N, K, "full", {4: (ROWS, 4 if K >= 64 else 2, nf)}))
    # (b) the VALU kernel (mode 0), pw32m<2> (mode 1), pw32m<4> (mode 2 from K = 64 on)
    forms = ("expand", "project", "full")
    for i, M in enumerate((1, 64, 130)):
        for j, N in enumerate((64, 100, 480)):
            for l, K in enumerate((4, 16, 40, 64, 200)):
                cases.append((M, N, K, forms[(i + j + l) % 3],
                              {0: (VALU, 0, 0), 1: (MFMA, 2, 0), 2: (MFMA, 4 if K >= 64 else 2, 0)}))
    # (c) mode 3: whole-row tiles up to K = 64 only
    cases.append((130, 96, 64, "project", {3: (ROWS, 4, 6), 4: (ROWS, 4, 6)}))
    cases.append((130, 96, 72, "project", {3: (MFMA, 4, 0), 4: (ROWS, 4, 6)}))
    return cases


PW_CASES = _pw_cases()
# the large cases (dyadic inputs only, act none: compared for equality).  Mode 2 with exactly 1024 workgroups
# stays on pw32m<2> (the "< 4 * 256" comparison); mode 5 at the smallest M on each side of its thresholds,
# K = 68: 512 row blocks (the last of one row), 1024 row blocks, 511 row blocks.
PW_BIG = [
    (4096, 1024, 64, "project", {2: (MFMA, 2, 0)}),
    (32705, 80, 68, "project", {5: (ROWS, 4, 5)}),
    (32705, 96, 68, "project", {5: (MFMA, 2, 0)}),   # 512 x 2 = 1024 workgroups: D = 2
    (65473, 96, 68, "project", {5: (ROWS, 4, 6)}),
    (32641, 80, 68, "project", {5: (MFMA, 4, 0)}),   # 511 x 2 workgroups: D = 4
]


def pw_inputs(M, N, K, form, kind):
    """kind "dyadic": the grid of the module docstring.  "real": A = randn, W = randn sqrt(2 / K), bias =
    randn / 2, ascale = rand, res = randn.  Returns dict(A [M][K], W [N][K], b [N], s [images][K] | None,
    res [M][N] | None, act, rpi)."""
    act, has_s, has_r = FORMS[form]
    g = _gen(M, N, K, list(FORMS).index(form), kind == "dyadic", 31)
    nimg = -(-M // RPI)
    if kind == "dyadic":
        A, W, b = dyadic((M, K), 2, g), dyadic((N, K), 1, g), dyadic((N,), 2, g)
        s = 2.0 ** torch.randint(-2, 2, (nimg, K), generator=g).float() if has_s else None
        res = dyadic((M, N), 2, g) if has_r else None
    else:
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) * math.sqrt(2.0 / K)
        b = torch.randn(N, generator=g) * 0.5
        s = torch.rand(nimg, K, generator=g) if has_s else None
        res = torch.randn(M, N, generator=g) if has_r else None
    return dict(A=A, W=W, b=b, s=s, res=res, act=act, rpi=RPI)


def _rows_scale(s, M, rpi):
    return s[torch.arange(M) // rpi]


def pw_ref(A, W, b, s, res, act, rpi, kind):
    """(out [M][N] float64, its bound tol, the pre-activation, e_res = the final add's half-ulp inside tol).
      pre = b + sum_k (a_k s_k) w_k      K FMAs from zero, the scaling and the bias add: K + 2 roundings of
                                         at most U S each, S = |b| + sum |a s| |w|
      y = act(pre)                       SiLU: 1.1 e_pre + act_err(y) (1.1 = SiLU's Lipschitz constant)
      out = y + res                      one more rounding: U |out|, where there is a residual
    real:   tol = 2 (1.1 U (K + 2) S + act_err(y)) + U |out|  (act_err only behind a SiLU)
    dyadic: pre is exact (module docstring) and so is y + res (multiples of 2^-8 below 2^10):
            act none -> tol = 0, the GPU test uses torch.equal; SiLU -> tol = act_err(y) (+ U |out|)."""
    Ad = A.double() * (_rows_scale(s, A.shape[0], rpi).double() if s is not None else 1.0)
    Wd, bd = W.double(), b.double()
    K = A.shape[1]
    pre = Ad @ Wd.T + bd
    S = Ad.abs() @ Wd.abs().T + bd.abs()
    y = F.silu(pre) if act == ACT_SILU else pre
    out = y + res.double() if res is not None else y
    e_act = act_err(y) if act == ACT_SILU else torch.zeros_like(y)
    e_res = U * out.abs() if res is not None else torch.zeros_like(y)
    if kind == "dyadic":
        tol = (e_act + e_res) if act == ACT_SILU else torch.zeros_like(y)
    else:
        tol = 2 * (1.1 * U * (K + 2) * S + e_act) + e_res
    return out, tol, pre, e_res


def pw_emulate(A, W, b, s, res, act, rpi, order="asc", drop_last_quad=False, neighbour_scale=False,
               res_first=False):
    """float32 numpy emulation: the scaled activation rounded to fp32, products added one k at a time in
    ascending ("asc") or descending ("desc") k from zero, + bias, SiLU, + residual.  Returns (out, the largest
    |partial sum|).  The keyword defects: the last k quad left out; rows of a 64-row tile that belong to the
    tile's second image scaled with the first image's row; the residual added before the activation."""
    f = np.float32
    M, K = A.shape
    a = A.numpy().astype(f)
    if s is not None:
        img = np.arange(M) // rpi
        if neighbour_scale:
            img = (np.arange(M) // 64 * 64) // rpi
        a = a * s.numpy().astype(f)[img]
    w = W.numpy().astype(f)
    ks = range(K - 4 if drop_last_quad else K)
    acc = np.zeros((M, W.shape[0]), f)
    big = 0.0
    for k in (ks if order == "asc" else reversed(ks)):
        acc = acc + a[:, k:k + 1] * w[None, :, k]
        big = max(big, float(np.abs(acc).max()))
    acc = acc + b.numpy().astype(f)
    big = max(big, float(np.abs(acc).max()))
    if res is not None and res_first:
        acc = acc + res.numpy().astype(f)
    y = silu32(acc) if act == ACT_SILU else acc
    if res is not None and not res_first:
        y = y + res.numpy().astype(f)
    return torch.from_numpy(y), big


def pw_emulate_fast(A, W, b, s, res, act, rpi):
    """The same by one float32 matmul (any order: enough to hold an emulation to half of a bound)."""
    a = A * _rows_scale(s, A.shape[0], rpi) if s is not None else A
    pre = a @ W.T + b
    y = torch.from_numpy(silu32(pre.numpy())) if act == ACT_SILU else pre
    return y + res if res is not None else y


# ---- dw32: depthwise k x k + SiLU, weights tap-major ----
DW32_KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
# 14 x 14: whole groups of 7 outputs (Wo 14 or 7); 9 x 10: a partial group, non-square; 5 x 3: narrower than
# one group and than the k = 5 halo; 1 x 1
DW32_HW = [(14, 14), (9, 10), (5, 3), (1, 1)]
DW32_C = [4, 20, 64]  # 20: no multiple of 16
DW32_B = 2


def dw32_inputs(B, H, W, C, k, kind):
    """x [B][H][W][C], w [C][k*k] (torch's layout; the kernel takes w.T = [k*k][C]), bias [C], fp32."""
    g = _gen(B, H, W, C, k, kind == "dyadic", 37)
    if kind == "dyadic":
        return dyadic((B, H, W, C), 2, g), dyadic((C, k * k), 1, g), dyadic((C,), 2, g)
    return torch.randn(B, H, W, C, generator=g) * 2, torch.randn(C, k * k, generator=g) * 0.3, torch.randn(C, generator=g)


def tap_major(w):
    return w.T.contiguous()


def dw32_ref(x, w, b, k, stride, kind):
    """out [B][Ho][Wo][C] float64 and tol: real 2 (1.1 U (k^2 + 2) S + act_err(out)) -- k^2 FMAs on the bias,
    S = |b| + sum |x| |w|; dyadic: at most 25 products (multiples of 2^-6 of at most 2) and the bias are exact
    in any order, tol = act_err(out)."""
    C = x.shape[-1]
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().view(C, 1, k, k)
    pad = (k - 1) // 2
    out = F.silu(F.conv2d(xd, wd, b.double(), stride, pad, groups=C)).permute(0, 2, 3, 1).contiguous()
    S = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), stride, pad, groups=C).permute(0, 2, 3, 1).contiguous()
    tol = act_err(out) if kind == "dyadic" else 2 * (1.1 * U * (k * k + 2) * S + act_err(out))
    return out, tol


def dw32_emulate(x, w, b, k, stride):
    """float32: conv2d, x / (1 + expf(-x))."""
    C = x.shape[-1]
    pre = F.conv2d(x.permute(0, 3, 1, 2), w.view(C, 1, k, k), b, stride, (k - 1) // 2, groups=C)
    return torch.from_numpy(silu32(pre.permute(0, 2, 3, 1).contiguous().numpy()))


# ---- sum32: SE pool partials in a fixed order ----
SUM32_C = [16, 144, 32, 96, 64]  # L = 4 (144: 9 channel groups), 8, 8, 16
# (49, 1): the 4-deep unrolled loop and its tail; (49, 49): one pixel per chunk, three empty lanes
SUM32_HW_N = [(49, 1), (49, 49), (49, 4), (196, 23), (50, 3), (7, 5), (1, 1)]
SUM32_B = 3


def sum32_inputs(B, HW, C):
    return torch.randn(B, HW, C, generator=_gen(B, HW, C, 41))


def sum32_lanes(C):
    c4 = C // 4
    return 16 if c4 % 16 == 0 else 8 if c4 % 8 == 0 else 4


def sum32_emulate(x, nchunks, short=0, lane_stride=4, order="01_23"):
    """numpy float32, the order csrc/effnet_f32.hip documents: chunk j covers [j HW / n, (j + 1) HW / n);
    lane r of 4 adds pixels p0 + r, p0 + r + 4, ... in order from zero; the lane sums are combined as
    (r0 + r1) + (r2 + r3).  These are additions only and the library is built without fast-math, so the
    order is the result: the kernel must match bit for bit.  Defects: short = pixels missing at each chunk's
    end, lane_stride = 3, order "02_13" = (r0 + r2) + (r1 + r3)."""
    f = np.float32
    xn = x.numpy().astype(f)
    B, HW, C = xn.shape
    part = np.zeros((B, nchunks, C), f)
    for j in range(nchunks):
        p0, p1 = j * HW // nchunks, (j + 1) * HW // nchunks - short
        lanes = []
        for r in range(4):
            a = np.zeros((B, C), f)
            for p in range(p0 + r, p1, lane_stride):
                a = a + xn[:, p]
            lanes.append(a)
        part[:, j] = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3]) if order == "01_23" else \
            (lanes[0] + lanes[2]) + (lanes[1] + lanes[3])
    return torch.from_numpy(part)


def sum32_ref(x, nchunks):
    """part [B][n][C] in float64 and the bound U (ceil(n_j / 4) + 3) sum |x| (a lane's adds, two joining
    adds, margin) -- stated for the record and used on the planted defects; the kernel test is the exact one."""
    B, HW, C = x.shape
    xd = x.double()
    part, tol = torch.zeros(B, nchunks, C, dtype=torch.float64), torch.zeros(B, nchunks, C, dtype=torch.float64)
    for j in range(nchunks):
        p0, p1 = j * HW // nchunks, (j + 1) * HW // nchunks
        part[:, j] = xd[:, p0:p1].sum(1)
        tol[:, j] = U * (-(-(p1 - p0) // 4) + 3) * xd[:, p0:p1].abs().sum(1)
    return part, tol


# ---- gap32 ----
GAP32_EXACT = (8, 64)


def gap32_inputs(B, HW, C, kind="real"):
    """x fp32 [B][HW][C], w [2][C], b [2].  dyadic (HW = 8, C = 64): a channel sum is a multiple of 2^-3 of at
    most 16, the mean (times the exact 1 / 8) a multiple of 2^-6, a product a multiple of 2^-9 of at most 2 and
    every partial sum of the 64 products and the bias below 2^17 units: logits exact in any order."""
    g = _gen(B, HW, C, kind == "dyadic", 43)
    if kind == "dyadic":
        return dyadic((B, HW, C), 2, g), dyadic((2, C), 1, g), dyadic((2,), 2, g)
    return torch.randn(B, HW, C, generator=g), torch.randn(2, C, generator=g) * (3 / math.sqrt(C)), torch.randn(2, generator=g)


# ---- stem32 ----
def stem32_dyadic_inputs():
    """x_f32_nchw [2][3][224][224], w [32][3][3][3], bias [32] on the dyadic grid: 27 products and the bias."""
    g = _gen(47)
    return dyadic((2, 3, 224, 224), 2, g), dyadic((32, 3, 3, 3), 1, g), dyadic((32,), 2, g)


def stem32_norm_f32(img):
    """The fp32 kernel's normalisation of uint8 pixels, ((u / 255 - mean) / std) with fp32 constants and two
    IEEE divisions, in numpy float32 -> [B][3][224][224]: bit for bit what the kernel feeds its FMAs."""
    f = np.float32
    u = img.numpy().astype(f).transpose(0, 3, 1, 2)
    mean, std = np.array(MEAN, f).reshape(1, 3, 1, 1), np.array(STD, f).reshape(1, 3, 1, 1)
    return torch.from_numpy((u / f(255) - mean) / std)


def stem32_norm_fma(img):
    """The fp16 tower's form, u sc + of as one fp32 FMA (float64 product, one rounding): the planted defect."""
    f = np.float32
    std, mean = np.array(STD, f), np.array(MEAN, f)
    sc = (f(1) / (f(255) * std)).reshape(1, 3, 1, 1)
    of = (-mean / std).reshape(1, 3, 1, 1)
    u = img.numpy().astype(np.float64).transpose(0, 3, 1, 2)
    return torch.from_numpy((u * sc.astype(np.float64) + of.astype(np.float64)).astype(f))


def stem32_u8_ref(img, ws, bs):
    """The stem from uint8 pixels in float64 -> out [B][112][112][32] and its bound e.  Unlike the fp16 tower's
    single FMA (effnet_refs.stem_ref's e_v), the fp32 output form evaluates v = ((u / 255 - mean) / std) with two
    IEEE divisions and fp32 constants mean32, std32:
      t1 = fl(u / 255)          U |u / 255|
      t2 = fl(t1 - mean32)      U |u / 255 - mean| + |mean32 - mean|, and t1's error carried
      v  = fl(t2 / std32)       U |v| + |v| |std32 - std| / std, and t2's error / std
      e_v = (U |u / 255| + U |u / 255 - mean| + |mean32 - mean|) / std + U |v| + |v| |std32 - std| / std
    (three roundings of v, plus the errors of the two constants carried through; first order).  Then, as in
    stem_ref: e_acc = 28 U (|b| + sum |w| |v|) + sum |w| e_v, e = 2 (1.1 e_acc + act_err(out))."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).view(1, 3, 1, 1)
    mean, std = t(MEAN), t(STD)
    d_mean = t(np.abs(np.array(MEAN, np.float32).astype(np.float64) - np.array(MEAN)))
    d_std = t(np.abs(np.array(STD, np.float32).astype(np.float64) - np.array(STD)))
    u = img.double().permute(0, 3, 1, 2) / 255.0
    v = (u - mean) / std
    e_v = (U * u + U * (u - mean).abs() + d_mean) / std + U * v.abs() + v.abs() * d_std / std
    W, Bv = ws.double(), bs.double()
    acc = F.conv2d(v, W, Bv, 2, 1)
    Mw = F.conv2d(v.abs(), W.abs(), None, 2, 1)
    e_acc = U * 28 * (Mw + Bv.abs().view(1, 32, 1, 1)) + F.conv2d(e_v, W.abs(), None, 2, 1)
    out = F.silu(acc)
    e = 2 * (1.1 * e_acc + act_err(out))
    return out.permute(0, 2, 3, 1).contiguous(), e.permute(0, 2, 3, 1).contiguous()


PASS_GAIN = 64.0
PASS_MIN = 18.0


def stem32_passthrough_weights():
    """One-hot stem weights that pass the normalised pixel through: output channel j = PASS_GAIN (a power of two)
    times input channel j % 3 at tap j % 9, bias 0.  Every other FMA adds an exact zero, so the pre-activation is
    PASS_GAIN v exactly, v the kernel's own fp32 normalised value (stem32_norm_f32).  From x >= PASS_MIN on,
    expf(-x) < 2^-25, 1 + expf(-x) rounds to 1 and x / 1 = x: the output is PASS_GAIN v bit for bit, and it is
    0 / 2 = 0 where the tap lies in the zero padding.  These elements see one ulp of v: the two-division form
    and the one-FMA form of the normalisation give different bits there."""
    w = torch.zeros(32, 3, 3, 3)
    for j in range(32):
        w[j, j % 3, (j % 9) // 3, (j % 9) % 3] = PASS_GAIN
    return w, torch.zeros(32)


def stem32_passthrough_ref(v32, ws):
    """(pre float64 [B][112][112][32] = the exact pre-activation from the fp32 normalised v32, mask of the
    elements that must equal it bit for bit: pre >= PASS_MIN, or pre == 0)."""
    pre = F.conv2d(v32.double(), ws.double(), None, 2, 1).permute(0, 2, 3, 1).contiguous()
    return pre, (pre >= PASS_MIN) | (pre == 0)


def stem32_emulate(v32, ws, bs):
    """float32: conv2d of the normalised input, x / (1 + expf(-x)) -> [B][112][112][32]."""
    pre = F.conv2d(v32, ws, bs, 2, 1).permute(0, 2, 3, 1).contiguous()
    return torch.from_numpy(silu32(pre.numpy()))
