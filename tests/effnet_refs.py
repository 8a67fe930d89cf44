"""Inputs, float64 references and derived error bounds of the fp16 EfficientNet kernels
(csrc/effnet.hip), shared by tests/test_effnet_refs_cpu.py (which checks the bounds against a
float32 emulation, no GPU) and tests/test_gpu_effnet_kernels.py (which checks the kernels).

Every reference is plain torch in float64, computed from the operands the kernel receives
(fp16-rounded activations, fp32 weights).  Every bound is computed in float64 beside its
reference, from the number formats and the length of the accumulation chains -- never from what a
kernel returned.  U = 2^-24 is the fp32 unit roundoff throughout.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def out_size(h, stride):
    return (h - 1) // stride + 1


def tile_edge(ho, stride):
    """The launchers' tile edge: the largest divisor of the output height up to 16 (stride 1) / 8 (stride 2)."""
    for t in range(16 if stride == 1 else 8, 0, -1):
        if ho % t == 0:
            return t
    return 1


def dw_geometry(H, W, C, stride, narrow=False):
    """(T, CW, nchunks) as launch_dwconv chooses them; narrow = flag bit 3."""
    ho, wo = out_size(H, stride), out_size(W, stride)
    T = tile_edge(ho, stride)
    cw = 48 if (C % 48 == 0 and not (narrow and C % 32 == 0)) else 32
    return T, cw, -(-ho // T) * -(-wo // T)


# compile-time geometries (k, stride, T, CW) of launch_dwconv / (k, stride, KS, T) of launch_expand_dw
DW_CT = {(3, 1, 16, 32), (3, 1, 14, 32), (5, 1, 14, 32), (5, 1, 7, 32), (3, 1, 7, 32), (5, 2, 7, 32), (3, 1, 14, 48),
         (5, 1, 14, 48), (3, 2, 8, 48), (5, 1, 7, 48), (3, 1, 7, 48), (5, 2, 7, 48), (3, 2, 7, 48)}
EDW_CT = {(3, 2, 1, 8), (3, 1, 1, 14), (5, 1, 2, 14), (5, 2, 1, 7), (3, 2, 2, 7), (3, 1, 3, 14)}


def dw_selected(H, W, C, k, stride, flags):
    """The kernel launch_dwconv runs: ("ct" | "rt", (k, stride, T, CW))."""
    T, cw, _ = dw_geometry(H, W, C, stride, bool(flags & 8))
    key = (k, stride, T, cw)
    return ("ct" if (flags & 1) and key in DW_CT else "rt"), key


# ---- cases (tests/test_gpu_effnet_kernels.py runs them, tests/test_effnet_refs_cpu.py emulates them) ----
# standalone depthwise: (k, stride, H, W, C, flag bit 3, the compile-time geometry the row selects or None)
DW_ROWS = [
    (3, 1, 32, 32, 64, 0, (3, 1, 16, 32)),
    (3, 1, 28, 28, 64, 0, (3, 1, 14, 32)), (5, 1, 28, 28, 64, 0, (5, 1, 14, 32)),
    (3, 1, 28, 28, 96, 8, (3, 1, 14, 32)), (5, 1, 28, 28, 96, 8, (5, 1, 14, 32)),
    (3, 1, 21, 21, 64, 0, (3, 1, 7, 32)), (5, 1, 21, 21, 64, 0, (5, 1, 7, 32)),
    (5, 2, 28, 28, 64, 0, (5, 2, 7, 32)), (5, 2, 27, 27, 64, 0, (5, 2, 7, 32)),
    (3, 1, 28, 28, 96, 0, (3, 1, 14, 48)), (5, 1, 28, 28, 96, 0, (5, 1, 14, 48)),
    (3, 2, 32, 32, 96, 0, (3, 2, 8, 48)), (3, 2, 31, 31, 96, 0, (3, 2, 8, 48)),
    (3, 1, 21, 21, 96, 0, (3, 1, 7, 48)), (5, 1, 21, 21, 96, 0, (5, 1, 7, 48)),
    (3, 2, 28, 28, 96, 0, (3, 2, 7, 48)), (5, 2, 28, 28, 96, 0, (5, 2, 7, 48)),
    (3, 2, 27, 27, 96, 0, (3, 2, 7, 48)), (5, 2, 27, 27, 96, 0, (5, 2, 7, 48)),
    # non-square: the second tile column is partial (the ox0 + ox + o < Wo guards)
    (3, 1, 28, 19, 64, 0, (3, 1, 14, 32)), (5, 1, 28, 19, 64, 0, (5, 1, 14, 32)),
    (3, 1, 28, 19, 96, 0, (3, 1, 14, 48)), (5, 1, 28, 19, 96, 0, (5, 1, 14, 48)),
]
# runtime-geometry edges (flags 0): Ho prime -> T = 1, 289 tiles; an image smaller than a halo
DW_EDGES = [
    (3, 1, 17, 17, 64), (5, 1, 17, 17, 96),
    (3, 1, 5, 5, 64), (5, 1, 5, 5, 96), (3, 2, 5, 5, 96), (5, 2, 5, 5, 64),
]
# fused expand + depthwise: (k, stride, KS, T, cin, C, H)
EDW_ROWS = [
    (3, 2, 1, 8, 16, 96, 32), (3, 1, 1, 14, 24, 144, 28), (5, 1, 2, 14, 40, 96, 28),
    (5, 2, 1, 7, 24, 96, 28), (3, 2, 2, 7, 40, 96, 28), (3, 1, 3, 14, 80, 96, 28),
]
EDW_WALK = dict(k=5, stride=2, cin=24, C=96, H=28, distinct=64, repeat=32, checked=(0, 21, 42, 63))
SE_SHAPES = [(32, 8), (96, 4), (144, 6), (240, 10), (672, 28), (1152, 48), (1280, 64)]
SE_NCHUNKS = [1, 3, 4, 16, 23, 49]
GAP_SHAPES = [(49, 1280), (1, 8), (8, 64), (50, 1280), (49, 2056)]
AMBIGUOUS_CAP = 0.25


# ---- depthwise conv ----
def dw_inputs(B, H, W, C, k, seed=0):
    """x fp16 NHWC = randn * 2, w fp32 [C][k*k] = randn * 0.3, bias fp32 [C] = randn."""
    g = _gen(B, H, W, C, k, seed)
    x = (torch.randn(B, H, W, C, generator=g) * 2).half()
    w = torch.randn(C, k * k, generator=g) * 0.3
    b = torch.randn(C, generator=g)
    return x, w, b


def tile_sums(a, T):
    """Sums of a [B][Ho][Wo][C] over T x T tiles, row-major tiles -> [B][ntiles][C] (partial tiles allowed)."""
    B, ho, wo, C = a.shape
    ty, tx = -(-ho // T), -(-wo // T)
    a = F.pad(a, (0, 0, 0, tx * T - wo, 0, ty * T - ho))
    return a.view(B, ty, T, tx, T, C).sum((2, 4)).reshape(B, ty * tx, C)


def dw_ref(x, w, b, k, stride, extra=None):
    """Depthwise k x k conv (pad (k - 1) / 2) + SiLU of x fp16 NHWC in float64.

    Returns a dict: out [B][Ho][Wo][C]; S = |b| + sum |x| |w| per output (the same conv on absolute
    values); tol = the fp16 output bound 2^-10 |out| + 2^-18 S + 2^-24 (+ extra); pool = per-tile sums
    of out (tile edge T of the launcher, row-major tiles); pool_tol = 2^-24 (n_tile + 2) sum_tile |out| +
    2^-18 sum_tile S (+ sum_tile extra), n_tile = the tile's number of outputs (<= 256 additions).
    extra (optional, [B][Ho][Wo][C]): a further per-output allowance (fused stem: ambiguous taps)."""
    C = x.shape[-1]
    xd = x.double().permute(0, 3, 1, 2)
    wd = w.double().view(C, 1, k, k)
    pad = (k - 1) // 2
    out = F.silu(F.conv2d(xd, wd, b.double(), stride, pad, groups=C)).permute(0, 2, 3, 1).contiguous()
    S = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), stride, pad, groups=C).permute(0, 2, 3, 1).contiguous()
    ex = torch.zeros_like(out) if extra is None else extra
    T = tile_edge(out.shape[1], stride)
    n_tile = tile_sums(torch.ones(1, out.shape[1], out.shape[2], 1, dtype=torch.float64), T)
    return dict(out=out, S=S, T=T, tol=2.0 ** -10 * out.abs() + 2.0 ** -18 * S + 2.0 ** -24 + ex,
                pool=tile_sums(out, T),
                pool_tol=U * (n_tile + 2) * tile_sums(out.abs(), T) + 2.0 ** -18 * tile_sums(S, T) + tile_sums(ex, T))


def dw_emulate(x, w, b, k, stride):
    """float32 emulation of the kernel: fp32 conv2d, x * sigmoid(x), fp16 store; pool partials from the
    unrounded fp32 activations."""
    C = x.shape[-1]
    pre = F.conv2d(x.float().permute(0, 3, 1, 2), w.view(C, 1, k, k), b, stride, (k - 1) // 2, groups=C)
    act = (pre * torch.sigmoid(pre)).permute(0, 2, 3, 1).contiguous()
    return act.half(), tile_sums(act, tile_edge(act.shape[1], stride))


# ---- fused expand + depthwise ----
def edw_inputs(B, H, cin, C, k, seed=0):
    """x fp16 [B][H][H][cin] = randn; we fp16 [C][cin] = randn * 1.5 / sqrt(cin); be = randn * 0.5;
    depthwise w = randn * 0.3, bias = randn (fp32)."""
    g = _gen(B, H, cin, C, k, seed, 7)
    x = torch.randn(B, H, H, cin, generator=g).half()
    we = (torch.randn(C, cin, generator=g) * (1.5 / math.sqrt(cin))).half()
    be = torch.randn(C, generator=g) * 0.5
    w = torch.randn(C, k * k, generator=g) * 0.3
    b = torch.randn(C, generator=g)
    return x, we, be, w, b


def expand_emulate(x, we, be):
    """float32 emulation of the 1x1 expand + SiLU, stored fp16 (on the GPU the tested GEMM provides it)."""
    pre = x.float() @ we.float().T + be
    return (pre * torch.sigmoid(pre)).half()


# ---- squeeze-excitation ----
def se_inputs(B, nchunks, C, Csq, seed=0):
    """partials = randn [B][nchunks][C], the last image's all zero; inv_hw = fp32(nchunks^-1/2);
    w1 [Csq][C] = randn / sqrt(C), b1 = randn * 0.5, w2t [Csq][C] = randn * 2 / sqrt(Csq), b2 = randn."""
    g = _gen(B, nchunks, C, Csq, seed, 11)
    part = torch.randn(B, nchunks, C, generator=g)
    part[-1] = 0
    inv_hw = float(np.float32(nchunks ** -0.5))
    w1 = torch.randn(Csq, C, generator=g) / math.sqrt(C)
    b1 = torch.randn(Csq, generator=g) * 0.5
    w2t = torch.randn(Csq, C, generator=g) * (2 / math.sqrt(Csq))
    b2 = torch.randn(C, generator=g)
    return part, inv_hw, w1, b1, w2t, b2


def act_err(y):
    """Error of an fp32 SiLU / sigmoid evaluation with value y: 8 U |y| + U.  v_exp_f32 and v_rcp_f32 are
    1 ulp each, the argument scaling and the 1 + e add half an ulp each; the scaled argument's rounding
    moves exp(-x) by |x| U relative, which reaches the result times |x| sigmoid(-x) -- under 8 units
    in all for |x| <= 5 and under U / 3 absolute beyond (|SiLU(x)| < 0.034 there).  expf and a division
    (<= 2 + 2.5 ulp) stay under the same 8 units."""
    return 8 * U * y.abs() + U


def se_ref(part, inv_hw, w1, b1, w2t, b2):
    """scale [B][C] in float64 and its first-order running error bound, with a factor 2 margin:
      pooled = inv_hw sum_j p_j           e_p = U Lp |inv_hw| sum_j |p_j|
      z = b1 + w1 pooled                  e_z = U L1 (|b1| + |w1| |pooled|) + |w1| e_p
      s1 = SiLU(z)                        e_s = 1.1 e_z + act_err(s1)
      a = b2 + w2t^T s1                   e_a = U L2 (|b2| + |w2t|^T |s1|) + |w2t|^T e_s
      scale = sigmoid(a)                  tol = 2 (0.25 e_a + act_err(scale))
    The chain lengths are the kernel's, one rounding per operation on the longest path to a result:
      Lp = ceil(nchunks / 4) + 3   four accumulators over the chunks, two joining adds, the multiply
      L1 = ceil(C / 64) + 7        a lane's FMAs over its channels, six wave-reduction adds, the bias
      L2 = ceil(Csq / 4) + 3       four accumulators (the bias starts one), two joining adds"""
    p, W1, B1, W2, B2 = part.double(), w1.double(), b1.double(), w2t.double(), b2.double()
    n, C = p.shape[1], p.shape[2]
    csq = W1.shape[0]
    pooled = p.sum(1) * inv_hw
    e_p = U * (-(-n // 4) + 3) * abs(inv_hw) * p.abs().sum(1)
    z = pooled @ W1.T + B1
    e_z = U * (-(-C // 64) + 7) * (pooled.abs() @ W1.abs().T + B1.abs()) + e_p @ W1.abs().T
    s1 = F.silu(z)
    e_s = 1.1 * e_z + act_err(s1)
    a = s1 @ W2 + B2
    e_a = U * (-(-csq // 4) + 3) * (s1.abs() @ W2.abs() + B2.abs()) + e_s @ W2.abs()
    scale = torch.sigmoid(a)
    return scale, 2 * (0.25 * e_a + act_err(scale))


def se_emulate(part, inv_hw, w1, b1, w2t, b2):
    pooled = part.sum(1) * np.float32(inv_hw)
    z = pooled @ w1.T + b1
    s1 = z * torch.sigmoid(z)
    return torch.sigmoid(s1 @ w2t + b2)


# ---- global average pool + classifier ----
def gap_inputs(B, HW, C, seed=0):
    """x fp16 [B][HW][C] = randn, w [2][C] = randn * 3 / sqrt(C), b [2] = randn."""
    g = _gen(B, HW, C, seed, 13)
    x = torch.randn(B, HW, C, generator=g).half()
    w = torch.randn(2, C, generator=g) * (3 / math.sqrt(C))
    b = torch.randn(2, generator=g)
    return x, w, b


def gap_ref(x, w, b):
    """(logits [B][2], score [B] = softmax(logits)[:, 1]) in float64 and their bounds, factor 2 margin:
      m = (sum_p x_p) / HW                e_m = U (HW + 2) sum_p |x_p| / HW   (HW - 1 adds, fp32(1 / HW), a multiply)
      l = b + w m                         e_l = U L (|b| + |w| |m|) + |w| e_m,  L = 8 ceil(C / 2048) + 11
                                          (a thread's FMAs, 6 wave-reduction adds, 4 wave partials + bias)
      score = sigmoid(l1 - l0)            e_score = 0.25 (e_l0 + e_l1 + U |l1 - l0|) + act_err(score)
    tol_logits = 2 e_l, tol_score = 2 e_score."""
    X, W, Bv = x.double(), w.double(), b.double()
    hw, C = X.shape[1], X.shape[2]
    m = X.sum(1) / hw
    e_m = U * (hw + 2) * X.abs().sum(1) / hw
    logits = m @ W.T + Bv
    L = 8 * -(-C // 2048) + 11
    e_l = U * L * (m.abs() @ W.abs().T + Bv.abs()) + e_m @ W.abs().T
    d = logits[:, 1] - logits[:, 0]
    score = torch.sigmoid(d)
    e_score = 0.25 * (e_l.sum(1) + U * d.abs()) + act_err(score)
    return logits, 2 * e_l, score, 2 * e_score


def gap_emulate(x, w, b):
    m = x.float().sum(1) * np.float32(1.0 / x.shape[1])
    logits = m @ w.T + b
    return logits, torch.softmax(logits, 1)[:, 1]


# ---- stem, and the stem fused into the stage-1 depthwise conv ----
def stem_images():
    """uint8 [2][224][224][3]: a structured synthetic image, and an all-0 image with a 3-pixel frame of 255
    (the zero padding, which is 0 in normalised space and far from both pixel values, dominates a padding error)."""
    import mmf_amd.synthetic as syn
    img = np.zeros((2, 224, 224, 3), np.uint8)
    img[0] = syn.images(1, 5)[0]
    img[1, :3] = img[1, -3:] = 255
    img[1, :, :3] = img[1, :, -3:] = 255
    return torch.from_numpy(img)


def normalise_f32(img):
    """ToTensor + Normalize in float64, rounded once to fp32 NCHW (the second entry point's input)."""
    x = img.double().permute(0, 3, 1, 2) / 255.0
    return ((x - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1))
            / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)).float()


WILD_CHANNELS = (5, 14, 23, 31)


def stem_inputs(seed=0, tame=False):
    """stem w [32][3][3][3] = randn * 0.25, bias = randn * 0.5; depthwise wd [32][9] = randn * 0.3, bd = randn.
    tame = True (the fused stem + depthwise test): all but WILD_CHANNELS have w = randn * 0.04 and bias =
    4 + randn * 0.5.  Their stem values sit near 4, where the worst-case fp32 bound (proportional to |b| +
    sum |w| |v|) is a small fraction of an fp16 ulp of the value, so few taps are ambiguous (stem_dw_ref);
    with the wide weights cancellation makes most taps ambiguous and the comparison would say little."""
    g = _gen(seed, 17)
    ws = torch.randn(32, 3, 3, 3, generator=g) * 0.25
    bs = torch.randn(32, generator=g) * 0.5
    wd = torch.randn(32, 9, generator=g) * 0.3
    bd = torch.randn(32, generator=g)
    if tame:
        keep = torch.zeros(32, dtype=torch.bool)
        keep[list(WILD_CHANNELS)] = True
        ws = torch.where(keep.view(32, 1, 1, 1), ws, ws * (0.04 / 0.25))
        bs = torch.where(keep, bs, bs + 4)
    return ws, bs, wd, bd


def _norm_consts():
    """sc = 1 / (255 std), of = -mean / std in float64 [1][3][1][1], and the errors of the kernels' fp32
    constants 1.0f / (255.0f * std_f), -mean_f / std_f (IEEE fp32 arithmetic, reproduced with numpy)."""
    std, mean = np.array(STD), np.array(MEAN)
    sc, of = 1.0 / (255.0 * std), -mean / std
    f = np.float32
    sc32 = (f(1) / (f(255) * std.astype(f))).astype(np.float64)
    of32 = (-mean.astype(f) / std.astype(f)).astype(np.float64)
    t = lambda a: torch.tensor(a, dtype=torch.float64).view(1, 3, 1, 1)
    return t(sc), t(of), t(np.abs(sc32 - sc)), t(np.abs(of32 - of))


def stem_ref(img, xf32, ws, bs, split=False):
    """Stem (ToTensor, Normalize, conv 3x3 stride 2 pad 1, SiLU) in float64 -> out [B][112][112][32], and the
    fp32 error bound e of the value before its fp16 store, factor 2 margin included:
      v = u sc + of (one FMA), sc = 1 / (255 std), of = -mean / std held as fp32 constants:
          e_v = u |sc32 - sc| + |of32 - of| + U |v|; e_v = 0 when the input is the fp32 tensor xf32 itself
      acc = b + sum_27 w v                e_acc = U n (|b| + sum |w| |v|) + sum |w| e_v,  n = 28 (27 FMAs on the bias)
          split = True: the fused kernel's stem on the MFMA, operands split as fp16 hi + lo, products
          w_lo x_hi, w_hi x_lo, w_hi x_hi accumulated in fp32 in that order.  The first two sums are 2^-11 of
          the third, so their 54 roundings count as 0.03; the third adds 27 terms and the bias: n = 28.03.
          The dropped w_lo x_lo (2^-22 relative) and the fp16 rounding of each lo part (2^-22 of its operand,
          or 2^-25 absolute in fp16's subnormal range) add 12 U sum |w| |v| + 2^-25 (sum |w| + sum |v|).
      out = SiLU(acc)                     e = 2 (1.1 e_acc + act_err(out))
    The fp16 output bound of the separate stem kernel is e + 2^-10 |out| (stem_tol)."""
    W, Bv = ws.double(), bs.double()
    if xf32 is not None:
        v = xf32.double()
        e_v = torch.zeros_like(v)
    else:
        u = img.double().permute(0, 3, 1, 2)
        sc, of, d_sc, d_of = _norm_consts()
        v = u * sc + of
        e_v = u * d_sc + d_of + U * v.abs()
    acc = F.conv2d(v, W, Bv, 2, 1)
    Mw = F.conv2d(v.abs(), W.abs(), None, 2, 1)
    e_acc = U * (28.03 if split else 28) * (Mw + Bv.abs().view(1, 32, 1, 1)) + F.conv2d(e_v, W.abs(), None, 2, 1)
    if split:
        ones = torch.ones(1, 3, 3, 3, dtype=torch.float64)
        e_acc = e_acc + 12 * U * Mw + 2.0 ** -25 * (W.abs().sum((1, 2, 3)).view(1, 32, 1, 1)
                                                    + F.conv2d(v.abs(), ones, None, 2, 1))
    out = F.silu(acc)
    e = 2 * (1.1 * e_acc + act_err(out))
    return out.permute(0, 2, 3, 1).contiguous(), e.permute(0, 2, 3, 1).contiguous()


def stem_tol(out, e):
    return e + 2.0 ** -10 * out.abs()


def stem_emulate(img, xf32, ws, bs):
    """float32 emulation of the stem before its fp16 store [B][112][112][32]."""
    if xf32 is not None:
        v = xf32
    else:
        sc = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32).view(1, 3, 1, 1)
        of = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32).view(1, 3, 1, 1)
        v = img.float().permute(0, 3, 1, 2) * sc + of
    pre = F.conv2d(v, ws, bs, 2, 1)
    return (pre * torch.sigmoid(pre)).permute(0, 2, 3, 1).contiguous()


def ulp16(x):
    """Spacing of fp16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 10), 2^-24 in the subnormal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -30))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-14) - 10)


def tie_distance16(x):
    """Distance of |x| (float64) to the nearest fp16 rounding tie (the midpoint of two neighbouring fp16 values)."""
    a = x.abs()
    h = a.half()
    bits = h.view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(torch.float16).double()
    dn = (bits - 1).clamp_min(0).to(torch.int16).view(torch.float16).double()
    hd = h.double()
    return torch.minimum((a - (hd + up) / 2).abs(), (a - (hd + dn) / 2).abs())


def stem_dw_ref(img, xf32, ws, bs, wd, bd):
    """The fused stem + depthwise kernel's reference: float64 stem -> fp16 -> float64 depthwise conv (dw_ref).
    The kernel's own stem value differs from the float64 one by up to e (stem_ref, split = True), so a tap
    within e of an fp16 rounding tie may round the other way: such a tap is ambiguous, an output with an
    ambiguous tap is ambiguous and is allowed 1.1 sum |wd| ulp16(s_tap) over its ambiguous taps on top of the
    depthwise bound (1.1: SiLU's Lipschitz constant).  Adds "ambiguous" = the fraction of such outputs."""
    s, e = stem_ref(img, xf32, ws, bs, split=True)
    amb = (tie_distance16(s) <= e).double() * ulp16(s)
    extra = 1.1 * F.conv2d(amb.permute(0, 3, 1, 2), wd.double().abs().view(32, 1, 3, 3), None, 1, 1, groups=32)
    extra = extra.permute(0, 2, 3, 1).contiguous()
    r = dw_ref(s.half(), wd, bd, 3, 1, extra=extra)
    r["ambiguous"] = float((extra > 0).double().mean())
    return r
