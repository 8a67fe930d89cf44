"""Inputs, float64 references and derived error bounds of the transformer towers' kernels
(csrc/norm.hip, csrc/precise.hip, csrc/attention.hip, the split-K path of csrc/gemm.hip), shared by
tests/test_transformer_refs_cpu.py (which checks the bounds against a float32 emulation and against
planted defects, no GPU) and tests/test_gpu_transformer_kernels.py (which checks the kernels).

Every reference is plain torch / numpy in float64, computed from the operands the kernel receives
(fp16-rounded activations, fp16 weights as passed, fp32 parameters).  Every bound is computed in
float64 beside its reference from the number formats and the kernel's chain lengths -- never from
what a kernel returned.  U = 2^-24 is the fp32 unit roundoff; an fp16 store adds half an fp16 ulp
(2^-25 in fp16's subnormal range).  The bounds are first-order worst-case ones: every rounding on the
longest path to a result counted once at full size."""
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-5
# MARGIN: every arithmetic bound below is the first-order worst case times 2 (as tests/effnet_refs.py does): the
# second-order terms, and room for tests/test_transformer_refs_cpu.py to require a float32 emulation under half
# of it.  The half-ulp of an fp16 store is not doubled: the emulation's stored value is held to half of the
# arithmetic bound plus that half-ulp.


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def half_ulp16(x):
    """Half the spacing of fp16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 11), 2^-25 in the subnormal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -30))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-14) - 11)


def store16(ref, e):
    """Bound of an fp16 store of a value within e of ref: e + half an ulp at the largest magnitude it can have."""
    return e + half_ulp16(ref.abs() + e)


def bits16(t):
    return t.contiguous().view(torch.int16)


def split_hilo(x32):
    """hi = fp16(x), lo = fp16(x - hi) of an fp32 tensor: exact functions of x (x - hi is exact in fp32)."""
    hi = x32.half()
    return hi, (x32 - hi.float()).half()


def hilo_sum_tol(ref, e):
    """Bound of float(hi) + float(lo) against ref when the split value is within e of ref: lo's own fp16
    rounding is half an ulp of a number below half an fp16 ulp of the value."""
    return e + half_ulp16(half_ulp16(ref.abs() + e))


# ---------------------------------------------------------------------------------------------
# LayerNorm family (norm.hip ln_row): one wave per row, C / 64 values per lane
# ---------------------------------------------------------------------------------------------
ROWS = (1, 4, 5, 9)     # one wave per row, four rows per block: a lone row, a full block, one and five more
WIDTHS = (512, 768)


def ln_ref(x, g, b, eps=EPS, e_x=None):
    """y = (x - mean) rstd g + b over the last axis in float64, and the bound e of the kernel's fp32 value:
      mean = (sum x) / C: a lane adds its C / 64 values, six tree additions join the lanes, one division
                         e_m = U (C / 64 + 6) mean|x| + mean(e_x)
      d = x - mean       e_d = e_x + e_m + U |d|
      var = (sum d^2) / C: a product and the same chain of additions
                         e_v = mean(2 |d| e_d) + U (C / 64 + 8) var
      r = rsqrtf(var + eps) (the addition, <= 2 ulp of the root)
                         rel_r = e_v / (2 (var + eps)) + 4 U
      y = d r g + b      e = 2 (|g| r e_d + |d r g| (rel_r + 2 U) + U |y|)   (factor 2: margin, see MARGIN)
    e_x (optional) = the bound of the kernel's own input row against x (an embedding sum, a stored stream).
    The cancellation in x - mean is in e_d: with one dominant channel e_m is U-relative to that channel and is
    amplified by r |g| on every other one."""
    x, g, b = x.double(), g.double(), b.double()
    C = x.shape[-1]
    e_x = torch.zeros_like(x) if e_x is None else e_x
    n = C // 64
    mean = x.mean(-1, keepdim=True)
    e_m = U * (n + 6) * x.abs().mean(-1, keepdim=True) + e_x.mean(-1, keepdim=True)
    d = x - mean
    e_d = e_x + e_m + U * d.abs()
    var = (d * d).mean(-1, keepdim=True)
    e_v = (2 * d.abs() * e_d).mean(-1, keepdim=True) + U * (n + 8) * var
    r = (var + eps).rsqrt()
    rel_r = e_v / (2 * (var + eps)) + 4 * U
    y = d * r * g + b
    e = g.abs() * r * e_d + (d * r * g).abs() * (rel_r + 2 * U) + U * y.abs()
    return y, 2 * e


def ln_emulate(x, g, b, eps=EPS, defect=None):
    """float32 emulation of ln_row.  defect "gamma_first": gamma applied before the mean is subtracted."""
    C = x.shape[-1]
    if defect == "gamma_first":
        x = x * g
        g = torch.ones_like(g)
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    r = torch.rsqrt((d * d).sum(-1, keepdim=True) / C + np.float32(eps))
    return d * r * g + b


def partial_ref(x, chain=None):
    """(mean, M2 = sum (x - mean)^2) of stored rows in float64 and their bounds (norm.hip row_partial: the chains
    of ln_ref without the division of M2).  chain: the number of additions counted instead of C / 64 + 6 (the
    GEMM producer's column blocks: one per column, an upper bound of its 6 + 2 + 2 deep tree)."""
    x = x.double()
    C = x.shape[-1]
    n = C // 64 if chain is None else chain - 6
    mean = x.mean(-1)
    e_m = U * (n + 6) * x.abs().mean(-1)
    d = x - mean[..., None]
    m2 = (d * d).sum(-1)
    e_m2 = (2 * d.abs() * (e_m[..., None] + U * d.abs())).sum(-1) + U * (n + 8) * m2
    return mean, 2 * e_m, m2, 2 * e_m2


def partial_emulate(x, defect=None):
    """defect "uncentred": M2 taken about 0."""
    C = x.shape[-1]
    mean = x.sum(-1) / C
    d = x if defect == "uncentred" else x - mean[..., None]
    return mean, (d * d).sum(-1)


def ln_params(C, seed=0):
    """gamma = 1 + 0.5 randn, beta = 0.5 randn (fp32)."""
    g = _gen(C, seed, 23)
    return 1 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)


def rows_input(rows, C, seed=0, dominant=False):
    """fp32 rows = randn * (1 + row / 4) + row (row-dependent scale and offset).  dominant:
    channel 77 of every row is about 100 times the rest and its gamma about 7."""
    g = _gen(rows, C, seed, 29)
    x = torch.randn(rows, C, generator=g) * (1 + torch.arange(rows)[:, None] / 4) + torch.arange(rows)[:, None]
    if dominant:
        x[:, 77] = 100 + 10 * torch.randn(rows, generator=g)
    return x


def dominant_params(C):
    gam, bet = ln_params(C, 1)
    gam[77] = 7.0
    return gam, bet


def branch_input(rows, C, seed=0):
    """an fp16 GEMM output y = randn * 0.7."""
    return (torch.randn(rows, C, generator=_gen(rows, C, seed, 31)) * 0.7).half()


def add_ref(x, y):
    """s = x + y (one fp32 addition of exactly converted operands) and its bound 2 U |s| (MARGIN)."""
    s = x.double() + y.double()
    return s, 2 * U * s.abs()


# ---------------------------------------------------------------------------------------------
# Embeddings
# ---------------------------------------------------------------------------------------------
ROBERTA_L = (1, 64, 65, 130, 512)
ROBERTA_VOCAB = 40
PAD = 1


def roberta_ids(L, seed=0):
    """int32 [4][L], ids in [2, ROBERTA_VOCAB - 1) besides the pad: no pad; leading pads; interior pads; all pad.
    (Four rows: one of each kind.)"""
    g = _gen(L, seed, 37)
    ids = torch.randint(2, ROBERTA_VOCAB - 1, (4, L), generator=g, dtype=torch.int32)
    ids[1, : max(1, L // 3)] = PAD
    if L > 2:
        ids[2, 1:L - 1:3] = PAD
        ids[2, L // 2] = PAD
    ids[3] = PAD
    return ids


def roberta_pos_ids(ids, pad=PAD):
    """cumsum(ids != pad) * (ids != pad) + pad."""
    keep = (ids != pad).to(torch.int64)
    return torch.cumsum(keep, 1) * keep + pad


def roberta_tables(L, seed=0):
    """word [ROBERTA_VOCAB][768], pos [L + 2][768] = independent randn * 0.5 rows, type0 = randn * 0.1: any two rows
    differ by about 0.7 in every column, some 10^5 bounds of the LayerNorm output."""
    g = _gen(L, seed, 41)
    return (torch.randn(ROBERTA_VOCAB, 768, generator=g) * 0.5, torch.randn(L + 2, 768, generator=g) * 0.5,
            torch.randn(768, generator=g) * 0.1)


def roberta_ref(ids, word, pos, type0, gam, bet, pid=None):
    """LN((word[id] + type0) + pos[pid]) in float64 [B][L][768] and the fp32 bound (two additions before the LN)."""
    pid = roberta_pos_ids(ids) if pid is None else pid
    a = word.double()[ids.long()] + type0.double()
    s = a + pos.double()[pid]
    return ln_ref(s, gam, bet, EPS, U * (a.abs() + s.abs()))   # (ln_ref doubles e_x with the rest)


def roberta_emulate(ids, word, pos, type0, gam, bet, defect=None):
    """defect "pos_off_by_one": the position id of every non-pad token one too small."""
    pid = roberta_pos_ids(ids)
    if defect == "pos_off_by_one":
        pid = torch.where(ids != PAD, pid - 1, pid)
    return ln_emulate((word[ids.long()] + type0) + pos[pid], gam, bet, EPS)


CLIP_TEXT_L = (5, 77)
CLIP_VOCAB = 48


def clip_text_inputs(B, L, seed=0):
    g = _gen(B, L, seed, 43)
    ids = torch.randint(0, CLIP_VOCAB, (B, L), generator=g, dtype=torch.int32)
    return ids, torch.randn(CLIP_VOCAB, 512, generator=g) * 0.5, torch.randn(L, 512, generator=g) * 0.5


def clip_text_x_ref(ids, tok, pos):
    """x = tok[id] + pos[t] in float64 [B * L][512] and the bound of its fp32 value."""
    x = (tok.double()[ids.long()] + pos.double()[None]).reshape(-1, 512)
    return x, 2 * U * x.abs()


def clip_text_x_emulate(ids, tok, pos, defect=None):
    """defect "pos_off_by_one": position t + 1 added (the last position wraps)."""
    p = torch.roll(pos, -1, 0) if defect == "pos_off_by_one" else pos
    return (tok[ids.long()] + p[None]).reshape(-1, 512)


def vision_inputs(B, seed=0):
    """patches [B * 49][768] = randn, cls = 3 randn (a CLS row unlike any patch row), pos [50][768] = 0.5 randn."""
    g = _gen(B, seed, 47)
    return (torch.randn(B * 49, 768, generator=g), 3 * torch.randn(768, generator=g),
            torch.randn(50, 768, generator=g) * 0.5)


def vision_e(patches, cls, pos, B, defect=None):
    """cat(cls, patches) + pos as [B * 50][768] in the operands' dtype.  defect "cls_is_patch": row 0 takes
    a patch row."""
    p = patches.view(B, 49, 768)
    first = p[:, :1] if defect == "cls_is_patch" else cls.expand(B, 1, 768)
    return (torch.cat([first, p], 1) + pos[None]).reshape(B * 50, 768)


def vision_x_ref(patches, cls, pos, B, pg, pb):
    e = vision_e(patches.double(), cls.double(), pos.double(), B)
    return ln_ref(e, pg, pb, EPS, U * e.abs())


MEAN_CLIP = (0.48145466, 0.4578275, 0.40821073)
STD_CLIP = (0.26862954, 0.26130258, 0.27577711)


def im2col_gather(v):
    """[B][224][224][3] -> [B * 49][3072]: patch p = 7 py + px, column c * 1024 + ky * 32 + kx."""
    B = v.shape[0]
    return v.view(B, 7, 32, 7, 32, 3).permute(0, 1, 3, 5, 2, 4).reshape(B * 49, 3072)


def im2col_ref(img):
    """v = (u / 255 - mean) / std in float64 and the fp32 bound.  The kernel evaluates (u c - m) s with fp32
    constants c = 1 / 255, m, s = 1 / std (each within U relative, s within 2 U: a rounded reciprocal of a rounded
    constant); a = u c carries 2 U |a|, the subtraction U |m| + U |a - m| (one rounding fewer if the compiler
    contracts the two into an fma), the product by s 3 U |v|:  e = (2 U |a| + U |m| + U |a - m|) / std + 3 U |v|."""
    u = img.double()
    m = torch.tensor(MEAN_CLIP, dtype=torch.float64)
    sd = torch.tensor(STD_CLIP, dtype=torch.float64)
    a = u / 255.0
    v = (a - m) / sd
    e = (2 * U * a + U * m + U * (a - m).abs()) / sd + 3 * U * v.abs()
    return im2col_gather(v), 2 * im2col_gather(e)


def im2col_emulate(img, defect=None):
    """defect "swap_xy": ky and kx exchanged within a patch."""
    m = torch.tensor(MEAN_CLIP, dtype=torch.float32)
    istd = np.float32(1.0) / torch.tensor(STD_CLIP, dtype=torch.float32)
    v = (img.float() * np.float32(1.0 / 255.0) - m) * istd
    if defect == "swap_xy":
        v = v.transpose(1, 2)
    return im2col_gather(v.contiguous())


# ---------------------------------------------------------------------------------------------
# Pooling
# ---------------------------------------------------------------------------------------------
EOS_L = (1, 5, 64, 65, 77, 1024)
EOS_ID = 49407


def eos_inputs(B, L, mode, seed=0):
    """mode "eos": ids below EOS_ID with EOS_ID planted (row 0: none; others: several, the first at a row-dependent
    place).  mode "argmax": eos_id == 2 convention, the maximum tied at several positions; row 0's first maximum
    at position 0, row 1's only maximum at L - 1."""
    g = _gen(B, L, seed, 53 if mode == "eos" else 59)
    ids = torch.randint(3, 1000, (B, L), generator=g, dtype=torch.int32)
    for r in range(B):
        if mode == "eos":
            if r == 0 and B > 1:
                continue
            first = (r * 37 + L // 2) % L
            ids[r, first::7] = EOS_ID
        else:
            if r == 0:
                ids[r, 0::5] = EOS_ID
            elif r == 1:
                ids[r, L - 1] = EOS_ID
            else:
                ids[r, (r * 29) % L::3] = EOS_ID
    return ids


def eos_ref(ids, eos_id):
    a = ids.numpy().astype(np.int64)
    if eos_id == 2:
        return torch.from_numpy(np.argmax(a, 1).astype(np.int32))
    hit = a == eos_id
    return torch.from_numpy(np.where(hit.any(1), hit.argmax(1), 0).astype(np.int32))


def eos_emulate(ids, eos_id, defect=None):
    """The kernel's keyed reduction in integers.  defect "last": ties resolved to the last position."""
    a = ids.numpy().astype(np.int64)
    L = a.shape[1]
    t = np.arange(L)[None]
    if eos_id == 2:
        key = a * 1024 + (t if defect == "last" else 1023 - t)
        k = key.max(1) & 1023
        return torch.from_numpy((k if defect == "last" else 1023 - k).astype(np.int32))
    key = np.where(a == eos_id, t, -1 if defect == "last" else 0x7fffffff)
    k = key.max(1) if defect == "last" else key.min(1)
    return torch.from_numpy(np.where((k == 0x7fffffff) | (k < 0), 0, k).astype(np.int32))


def l2norm_ref(x):
    """x / |x| in float64; the kernel's sum of C squares (a lane's C / 64 fmas, six tree additions) is within
    (C / 64 + 6) U relative, its root half of that, then sqrtf, a division and a product:
    e = 2 ((C / 64 + 6) / 2 + 4) U |y| (MARGIN)."""
    x = x.double()
    C = x.shape[-1]
    y = x / x.norm(dim=-1, keepdim=True)
    return y, 2 * ((C // 64 + 6) / 2 + 4) * U * y.abs()


def l2norm_emulate(x, defect=None):
    """defect "mean_square": the sum of squares divided by C."""
    s = (x * x).sum(-1, keepdim=True)
    if defect == "mean_square":
        s = s / x.shape[-1]
    return x * (np.float32(1.0) / torch.sqrt(s))


def gather_idx(B, L, seed=0):
    return torch.randint(0, L, (B,), generator=_gen(B, L, seed, 61), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------
# Attention: softmax(q k^T / 8 + mask) v per head of 64 dims
# ---------------------------------------------------------------------------------------------
def attn_inputs(B, L, H, seed=0, extra=0):
    """qkv fp16 [B * L][3 H 64 + extra]: q, k = randn * 0.7 (scores of about +-0.5: every valid key keeps a weight
    within a small factor of 1 / n, so none hides), v = +-3 with random signs + randn / 2 (a key's value is about
    3 away from the output in every dimension: a dropped key moves the output by about 3 times its weight)."""
    g = _gen(B, L, H, seed, 67)
    D = H * 64
    t = torch.randn(B * L, 3 * D + extra, generator=g)
    t[:, :2 * D] *= 0.7
    sign = torch.randint(0, 2, (B * L, D), generator=g).float() * 2 - 1
    t[:, 2 * D:3 * D] = 3 * sign + 0.5 * t[:, 2 * D:3 * D]
    return t.half()


def holes_mask(B, L, seed=0, dead=None):
    """int32 [B][L] key mask with interior holes (every third position from a batch-dependent start is masked,
    position L - 1 stays valid for b = 0); dead = a batch index that is fully masked."""
    m = torch.ones(B, L, dtype=torch.int32)
    for b in range(B):
        m[b, (b + 1) % 3::3] = 0
        if b > 0 and L > 4:
            m[b, L - max(1, L // 5):] = 0   # and a padded tail
    m[0, L - 1] = 1
    m[0, 0] = 1
    if dead is not None:
        m[dead] = 0
    return m


def attn_valid(mask, B, L, causal=False, qpos=None):
    """bool [B][Lq][L]: key j is visible to query i.  qpos (int [B]): one query per sequence at that position."""
    v = torch.ones(B, 1, L, dtype=torch.bool) if mask is None else (mask != 0)[:, None, :]
    j = torch.arange(L)
    if qpos is not None:
        return v & (j[None, None, :] <= qpos.long()[:, None, None])
    v = v.expand(B, L, L)
    if causal:
        v = v & (j[None, None, :] <= j[None, :, None])
    return v


def attn_ref(q, k, v, valid, p16, chunks=1):
    """softmax(q k^T / 8 over the valid keys) v in float64, q [B][H][Lq][64], k / v [B][H][L][64], valid
    [B][Lq][L] -> (out [B][H][Lq][64], bound); a query with no valid key gives 0 with bound 0.
      s_j = q . k_j / 8: 64 products accumulated in fp32, the scale and the mask's fma
                         ds_j = 68 U (|q| . |k_j|) / 8
      p_j = exp(s_j - m): both scores' errors, the subtraction and the exponential's argument scaling
                         (4 U (m - s_j)), exp itself, the running-maximum rescaling of an online softmax
                         over `chunks` key chunks (its arguments sum to at most m - s_j: 4 U (m - s_j) + 4 U
                         per chunk), and, where the kernel rounds P to fp16 (p16), 2^-11 relative + 2^-25:
                         rel_j = ds_j + max ds + 8 U (m - s_j) + (8 + 4 chunks) U [+ 2^-11]
      out = sum p_j v_j / sum p_j: with w_j = p_j / sum p and n valid keys (the P V and row-sum chains, the division)
                         e = sum_j w_j (rel_j + sum_i w_i rel_i + (n + 6) U) |v_j| [+ 2^-25 sum_j |v_j| / sum p]
    (the row sum is taken before P is rounded: its term carries no 2^-11), times 2 (MARGIN).  The bound is that
    of the fp32 value: an fp16 store adds store16."""
    q, k, v = q.double(), k.double(), v.double()
    vm = valid[:, None]                                                  # [B][1][Lq][L]
    s = (q @ k.transpose(-1, -2)) / 8
    ds = 68 * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8
    neg = torch.full_like(s, -float("inf"))
    sm = torch.where(vm, s, neg)
    m = sm.amax(-1, keepdim=True)
    alive = torch.isfinite(m)
    m = torch.where(alive, m, torch.zeros_like(m))
    p = torch.where(vm, (s - m).exp(), torch.zeros_like(s))
    l = p.sum(-1, keepdim=True)
    w = p / l.clamp_min(1e-300)
    out = w @ v
    ds_max = torch.where(vm, ds, torch.zeros_like(ds)).amax(-1, keepdim=True)
    rel_den = ds + ds_max + 8 * U * (m - s).abs() + (8 + 4 * chunks) * U
    rel_num = rel_den + (2.0 ** -11 if p16 else 0.0)
    n = vm.sum(-1, keepdim=True).double()
    den = (w * rel_den).sum(-1, keepdim=True)
    e = (w * (rel_num + den + (n + 6) * U)) @ v.abs()
    if p16:
        e = e + 2.0 ** -25 * (vm.double().expand_as(s) @ v.abs()) / l.clamp_min(1.0)
    e = torch.where(alive, 2 * e, torch.zeros_like(e))
    return out, e


def attn_emulate(q, k, v, valid, p16, defect=None):
    """float32 emulation before the store (fp16 P where the kernel rounds it).  defects: "drop_last_key" -- the last valid key of
    every query left out; "v_tail" -- the keys of the last partial 32-key chunk left out of P V (not of the sum)."""
    q, k, v = q.float(), k.float(), v.float()
    vm = valid[:, None].expand(q.shape[0], q.shape[1], valid.shape[1], valid.shape[2]).clone()
    L = vm.shape[-1]
    if defect == "drop_last_key":
        last = (vm.long() * torch.arange(1, L + 1)).amax(-1, keepdim=True) - 1
        vm &= torch.arange(L) != last
    s = (q @ k.transpose(-1, -2)) * np.float32(0.125)
    s = torch.where(vm, s, torch.full_like(s, -float("inf")))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pv = p.half().float() if p16 else p.clone()
    if defect == "v_tail" and L % 32:
        pv[..., L - L % 32:] = 0
    return (pv @ v) * torch.where(l > 0, 1 / l, torch.zeros_like(l))


def heads(t, B, L, H, off, ld=None):
    """[B * L][ld] -> [B][H][L][64] starting at column off."""
    return t.view(B, L, -1)[:, :, off:off + H * 64].view(B, L, H, 64).permute(0, 2, 1, 3)


ATTN_SHORT_L = (1, 31, 32, 33, 64, 96, 97, 128)     # every LK instantiation at and around its edge
ATTN_LONG_L = (129, 256, 257, 512)
ATTN32_L = (1, 31, 32, 33, 128, 129, 160)
Q1_L = (1, 5, 64, 65, 128, 129, 200, 512)
Q1_BH = ((3, 1), (1, 8), (2, 12))


def long_chunks(L):
    return -(-L // 128)


# ---------------------------------------------------------------------------------------------
# Split-K skinny GEMM (gemm.hip run_splitk + splitk_reduce_kernel)
# ---------------------------------------------------------------------------------------------
SPLITK_M = (1, 3, 64, 65, 512)
SPLITK_N = (4, 136, 512)
SPLITK_K = (512, 768, 1280, 1536, 3072)    # S = 2, 3, 5, 6, 12: 0, 1 and 3 slices left over by the groups of four
RES_KINDS = ("none", "res32", "res16")
OUT_KINDS = ("c32", "c16", "both")


def splitk_cases():
    """Every (N, K) pair, with M, the activation, the bias, the residual kind and the outputs rotating so that
    every value of each appears with every K: (M, N, K, act, bias, res, outs)."""
    cases = []
    for i, (K, N) in enumerate(itertools.product(SPLITK_K, SPLITK_N)):
        cases.append((SPLITK_M[(2 * i + i // 5) % 5], N, K, i % 5, i % 2 == 0, RES_KINDS[(i + i // 3) % 3],
                      OUT_KINDS[(i + i // 9) % 3]))
    cases.append((512, 512, 3072, 1, True, "res32", "both"))
    cases.append((65, 136, 1280, 0, False, "res16", "c16"))
    return cases


def gemm_inputs(M, N, K, seed=0):
    """A fp16 [M][K] = randn, W fp16 [N][K] = randn / sqrt(K) * 2, bias = randn, res = randn (fp32; its fp16
    rounding for res16)."""
    g = _gen(M, N, K, seed, 71)
    return (torch.randn(M, K, generator=g).half(), (torch.randn(N, K, generator=g) * (2 / math.sqrt(K))).half(),
            torch.randn(N, generator=g), torch.randn(M, N, generator=g))


def act64(x, act):
    if act == 1:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    if act == 2:
        return x * torch.sigmoid(1.702 * x)
    if act == 3:
        return x * torch.sigmoid(x)
    if act == 4:
        return x.clamp_min(0)
    return x


def act_err(x, y, act):
    """Error of the kernels' fp32 activations at pre-activation x with value y.  SiLU / quick-GELU: 8 U |y| + U
    (exp and rcp 1 ulp each, the argument scaling, the 1 + e addition, the product).  GELU (common.h gelu_erf:
    relu(x) - |x| erfc(|x| / sqrt 2) / 2 with Abramowitz & Stegun 7.1.26, |erfc error| <= 1.5e-7): 7.5e-8 |x|
    for the formula + 8 U |x| for its dozen fp32 operations on a term below |x| / 2, + 2 U."""
    if act == 1:
        return 7.5e-8 * x.abs() + 8 * U * x.abs() + 2 * U
    if act in (2, 3):
        return 8 * U * y.abs() + U
    return torch.zeros_like(x)


def gemm_ref(A, W, bias, res, act, chain):
    """act(A W^T + bias) + res in float64 and the bound of its fp32 value: chain = the number of roundings on the
    longest accumulation path (K + 4 for one pass over K; K / S + S + 4 for S slices of K / S added in order),
      e_pre = chain U (sum |a| |w| + |bias|);  e = 1.2 e_pre + act_err  (1.2 > every activation's slope)
      + U |out| for the residual addition; times 2 (MARGIN)."""
    a, w = A.double(), W.double()
    pre = a @ w.T
    mag = a.abs() @ w.abs().T
    if bias is not None:
        pre = pre + bias.double()
        mag = mag + bias.double().abs()
    y = act64(pre, act)
    e = 1.2 * chain * U * mag + act_err(pre, y, act)
    if res is not None:
        y = y + res.double()
        e = e + U * y.abs()
    return y, 2 * e


def act32(x, act):
    if act == 1:
        return 0.5 * x * (1 + torch.erf(x * np.float32(1 / math.sqrt(2))))
    if act == 2:
        return x * torch.sigmoid(np.float32(1.702) * x)
    if act == 3:
        return x * torch.sigmoid(x)
    if act == 4:
        return x.clamp_min(0)
    return x


def splitk_emulate(A, W, bias, res, act, S, defect=None):
    """float32 emulation: S slices of K / S multiplied apart and added in slice order.  defect "skip_last_slice"."""
    K = A.shape[1]
    ks = K // S
    a, w = A.float(), W.float()
    acc = None
    for z in range(S - 1 if defect == "skip_last_slice" else S):
        p = a[:, z * ks:(z + 1) * ks] @ w[:, z * ks:(z + 1) * ks].T
        acc = p if acc is None else acc + p
    if bias is not None:
        acc = acc + bias
    y = act32(acc, act)
    return y + res.float() if res is not None else y


# ---------------------------------------------------------------------------------------------
# Lazy-LayerNorm producer (gemm.hip epi 2): the stored stream and its per-block partials
# ---------------------------------------------------------------------------------------------
PRODUCER_M = (100, 256, 300)
PRODUCER_K = (192, 512)
PRODUCER_N = (100, 512, 768)     # the last 96-column partial covers 4, 32 or 96 columns
LN_TN = 96


def block_partials_ref(stored, tn=LN_TN):
    """Per row and block of tn columns (mean, M2) of the stored values in float64 with their bounds (an fp32 chain
    over the block's columns): four [M][P] tensors."""
    N = stored.shape[1]
    cols = [partial_ref(stored[:, c:c + tn], chain=min(tn, N - c) + 2) for c in range(0, N, tn)]
    return tuple(torch.stack([c[i] for c in cols], 1) for i in range(4))


def block_partials_emulate(stored, tn=LN_TN, defect=None):
    """defect "tail_as_full": the last, partial block's sum divided by tn."""
    N = stored.shape[1]
    means, m2s = [], []
    for c in range(0, N, tn):
        blk = stored[:, c:c + tn]
        n = tn if defect == "tail_as_full" else blk.shape[1]
        mean = blk.sum(-1) / n
        means.append(mean)
        m2s.append(((blk - mean[:, None]) ** 2).sum(-1))
    return torch.stack(means, 1), torch.stack(m2s, 1)


# ---------------------------------------------------------------------------------------------
# Lazy-LayerNorm consumer (gemm.hip epi 1): act(r (s W'^T - mean u) + c), mean / r from partials
# ---------------------------------------------------------------------------------------------
CONSUMER_M = (100, 256, 300)
CONSUMER_K = (192, 512, 768)      # P = ceil(K / 96) = 2, 6 (the last block 32 columns), 8
CONSUMER_N = (200, 512)
CONSUMER_ACT = {192: 0, 512: 1, 768: 2}


def consumer_inputs(M, N, K, seed=0):
    """s fp16 [M][K] = randn * (1 + (m % 5) / 4) + (m % 7 - 3) / 2 (row means from -1.5 to 1.5: mean u matters);
    W' = fp16(W diag(gamma)) with W = randn * 2 / sqrt(K); u = fp32(sum_k W'); c = fp32(b + W beta)."""
    g = _gen(M, N, K, seed, 89)
    m = torch.arange(M)[:, None]
    s = (torch.randn(M, K, generator=g) * (1 + (m % 5) / 4) + ((m % 7) - 3) * 0.5).half()
    W = torch.randn(N, K, generator=g) * (2 / math.sqrt(K))
    gam, bet = ln_params(K, 5)
    b = torch.randn(N, generator=g)
    Wp = (W * gam).half()
    return s, Wp, Wp.double().sum(1).float(), (b.double() + W.double() @ bet.double()).float()


def block_sizes(K, tn):
    return torch.tensor([min(K - c, tn) for c in range(0, K, tn)], dtype=torch.float64)


def supplied_partials(s, tn):
    """The float64 statistics of s over blocks of tn columns, rounded to fp32: (mean [M][P], M2 [M][P], and the
    bounds U |.| of that rounding)."""
    mean, _, m2, _ = block_partials_ref(s, tn)
    return mean.float(), m2.float(), U * mean.abs(), U * m2.abs()


def consumer_ref(s, Wp, u, c, act, tn, e_pm, e_pq, eps=EPS):
    """act(r (s W'^T - mean u) + c) in float64 with mean / r the float64 statistics of the rows of s, and the
    bound of the kernel's fp32 value given partials within e_pm / e_pq [M][P] of the true block statistics
    (m_p, q_p over n_p columns):
      mean = (sum_p n_p m_p) / K          e_mean = (sum n_p e_pm + (P + 1) U sum n_p |m_p|) / K   (P fmas, a division)
      s2 = sum_p (n_p d_p^2 + q_p), d_p = m_p - mean
                                          e_d = e_pm + e_mean + U |d_p|
                                          e_s2 = sum (2 n_p |d_p| e_d + e_pq) + (P + 4) U s2
      r = rsqrtf(s2 / K + eps)            rel_r = e_s2 / (2 K (var + eps)) + 4 U
      t = acc - mean u                    e_t = (K + 4) U sum |s| |w'| + |u| e_mean + 2 U |mean u| + U |t|
                                          (the cancellation: through |acc| and |mean| |u|, not through |t|)
      pre = r t + c                       e_pre = r e_t + |r t| (rel_r + 2 U) + U |pre|
      out = act(pre)                      e = 2 (1.2 e_pre + act_err)   (MARGIN)"""
    S, W, u, c = s.double(), Wp.double(), u.double(), c.double()
    K = S.shape[1]
    n = block_sizes(K, tn)
    P = n.numel()
    bm, _, bq, _ = block_partials_ref(s, tn)
    mean = S.mean(1, keepdim=True)
    var = ((S - mean) ** 2).mean(1, keepdim=True)
    r = (var + eps).rsqrt()
    e_mean = ((n * e_pm).sum(1, keepdim=True) + (P + 1) * U * (n * bm.abs()).sum(1, keepdim=True)) / K
    d = bm - mean
    e_d = e_pm + e_mean + U * d.abs()
    e_s2 = (2 * n * d.abs() * e_d + e_pq).sum(1, keepdim=True) + (P + 4) * U * K * var
    rel_r = e_s2 / (2 * K * (var + eps)) + 4 * U
    acc = S @ W.T
    mu = mean * u
    t = acc - mu
    e_t = (K + 4) * U * (S.abs() @ W.abs().T) + u.abs() * e_mean + 2 * U * mu.abs() + U * t.abs()
    pre = r * t + c
    e_pre = r * e_t + (r * t).abs() * (rel_r + 2 * U) + U * pre.abs()
    y = act64(pre, act)
    return y, 2 * (1.2 * e_pre + act_err(pre, y, act))


def consumer_emulate(s, Wp, u, c, act, pm, pq, tn, eps=EPS, defect=None):
    """float32 emulation with the kernel's combination of the partials.  defects: "tail_as_full" -- every block
    weighted as tn columns; "no_mean" -- the mean u term left out."""
    K = s.shape[1]
    n = block_sizes(K, tn).float()
    if defect == "tail_as_full":
        n = torch.full_like(n, float(tn))
    mean = (n * pm).sum(1, keepdim=True) / K
    d = pm - mean
    r = torch.rsqrt((n * d * d + pq).sum(1, keepdim=True) / K + np.float32(eps))
    acc = s.float() @ Wp.float().T
    t = acc if defect == "no_mean" else acc - mean * u
    return act32(r * t + c, act)
