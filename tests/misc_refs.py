"""Inputs, float64 references and derived error bounds of the closing fp32 kernels (csrc/misc.hip: the RoBERTa
dual heads, the CLS copy, the FusionJudge MLP with verdict / confidence / rule, the cosine rows and the finish
of mmf_analyze_mixed), shared by tests/test_misc_refs_cpu.py (which certifies the bounds against a float32
emulation of the kernels' own operation order and against planted defects, no GPU) and
tests/test_gpu_misc_kernels.py (which checks the kernels).

The conventions are those of tests/transformer_refs.py: every reference is plain numpy in float64, computed
from exactly the operands the kernel receives; every bound is computed in float64 beside its reference from the
kernel's chain lengths at U = 2^-24 -- never from what a kernel returned -- and is the first-order worst case
(every rounding on the path to a result counted once at full size) times MARGIN = 2.  A chain of n fmaf into one
accumulator is within n U of the sum of the magnitudes of its terms (the accumulator's start included)."""
import numpy as np

U = 2.0 ** -24
MARGIN = 2.0
TINY = 2.0 ** -126   # the smallest normal float32
ROWS = (1, 4, 5, 9)  # four rows per block: a lone row, a full block, one and five rows into the next
F32 = np.float32
T07, T03, T05, T085 = F32(0.7), F32(0.3), F32(0.5), F32(0.85)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def around(t):
    """(the largest float32 below t, t, the smallest float32 above t)."""
    t = F32(t)
    return np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))


# ---------------------------------------------------------------------------------------------
# float32 emulation pieces (the kernels' operation order)
# ---------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product of two float32 is exact in float64, so the only roundings are
    the float64 addition (2^-53 relative, far below U) and the rounding to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def wave_sum32(v):
    """common.h wave_sum over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1; lane 0's value."""
    lanes = np.arange(64)
    v = v.astype(F32)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(F32)
    return v[..., 0]


def softmax2_32(l0, l1):
    """The kernels' two-way softmax in float32 (exp of the difference to the larger logit) -> (p0, p1)."""
    m = np.maximum(l0, l1)
    e0 = np.exp((l0 - m).astype(F32)).astype(F32)
    e1 = np.exp((l1 - m).astype(F32)).astype(F32)
    s = (e0 + e1).astype(F32)
    return (e0 / s).astype(F32), (e1 / s).astype(F32)


def softmax2_ref(l0, l1, e0, e1):
    """(p0, p1) = softmax of two float64 logits known within e0 / e1 (first-order, not yet times MARGIN), and the
    first-order bounds of the kernel's float32 probabilities.  With d = l1 - l0 the kernel forms exp(-|d|) for
    the smaller logit and exp(0) = 1 exactly for the larger; p_o has sensitivity p0 p1 per unit of d, so
      the logits' errors and the subtraction's rounding         p0 p1 (e0 + e1 + U |d|)
      expf: its argument scaling (4 U |d|) and the function itself (4 U, as the attention exponentials of
        transformer_refs.attn_ref), relative on the smaller exponential     p0 p1 (4 U |d| + 4 U)
      the sum e0 + e1 and the division, one rounding each, relative on p_o  2 U p_o
      float32's range: below the smallest normal 2^-126 a result is rounded to the subnormal grid or flushed to
        zero, an absolute error of at most 2^-126 (it matters only for gaps beyond 87, where p_o < 1e-37)."""
    d = l1 - l0
    p1 = 1.0 / (1.0 + np.exp(-d))
    p0 = 1.0 / (1.0 + np.exp(d))
    common = p0 * p1 * (e0 + e1 + 5 * U * np.abs(d) + 4 * U) + TINY
    return p0, p1, common + 2 * U * p0, common + 2 * U * p1


# ---------------------------------------------------------------------------------------------
# RoBERTa dual heads (text_heads_kernel): Linear(768, 256) - ReLU - Linear(256, 2) twice, softmax[:, 1]
# ---------------------------------------------------------------------------------------------
HEAD_REGIMES = ("default", "trained", "halfneg")


def heads_inputs(B, regime, seed=0):
    """x [B][768] ~ N(0, 1) (CLS rows behind a LayerNorm) and the two heads' tensors, DIFFERENT per head (a crossed
    blockIdx.y fails): dict head -> (w1t [768][256] = the first layer transposed, as the kernel reads it, b1 [256],
    w2 [2][256], b2 [2]).
      default : PyTorch's Linear init, uniform +-1 / sqrt(fan_in)
      trained : the second layer 8 times that, and output biases (-10, +10) for ai, (+10, -10) for misinfo: the
                logit gaps reach +-20, so ai scores saturate to exactly 1 and misinfo scores fall to about 2e-9
      halfneg : b1 = 0.5 randn over zero-mean rows: about half of the hidden pre-activations are negative, and
                the bias decides the sign of many of them."""
    g = _rng(B, HEAD_REGIMES.index(regime), seed, 7)
    x = g.standard_normal((B, 768)).astype(F32)
    heads = {}
    for h in ("ai", "mi"):
        a1, a2 = 1 / np.sqrt(768.0), 1 / 16.0
        w1t = g.uniform(-a1, a1, (768, 256)).astype(F32)
        b1 = g.uniform(-a1, a1, 256).astype(F32)
        w2 = g.uniform(-a2, a2, (2, 256)).astype(F32)
        b2 = g.uniform(-a2, a2, 2).astype(F32)
        if regime == "trained":
            w2 = (w2 * F32(8)).astype(F32)
            b2 = (b2 + (np.array([-10, 10], F32) if h == "ai" else np.array([10, -10], F32))).astype(F32)
        if regime == "halfneg":
            b1 = (0.5 * g.standard_normal(256)).astype(F32)
        heads[h] = (w1t, b1, w2, b2)
    return x, heads


def heads_ref(x, w1t, b1, w2, b2):
    """One head in float64 -> (pre [B][256] hidden pre-activations, logits [B][2], e_logits, score [B], e_score).
      hidden: four K-slices of 192 fmaf each from 0 (192 U on the slice's magnitudes), three additions that join
        the slices in fixed order (3 U), the bias addition (U on the magnitudes and the bias); with
        A = sum_k |x_k w1t[k][h]|:                       e_h = U (195 A + (A + |b1|))
      ReLU: 1-Lipschitz, the hidden error passes at most unchanged.
      logits: one product per hidden unit (U), the six-level wave_sum tree (6 U), three additions across the
        waves (3 U), the output bias (U); the hidden errors enter weighted by |w2|; with P = sum_h |h w2[o][h]|:
                                                         e_l = sum_h |w2[o][h]| e_h + 11 U P + U |b2[o]|
      score = softmax(logits)[1]: softmax2_ref.
    Both bounds are returned times MARGIN."""
    x, w1t, b1, w2, b2 = (t.astype(np.float64) for t in (x, w1t, b1, w2, b2))
    pre = x @ w1t + b1
    A = np.abs(x) @ np.abs(w1t)
    e_h = U * (195 * A + A + np.abs(b1))
    h = np.maximum(pre, 0.0)
    logits = h @ w2.T + b2
    e_l = e_h @ np.abs(w2).T + 11 * U * (h @ np.abs(w2).T) + U * np.abs(b2)
    _, p1, _, e_p1 = softmax2_ref(logits[:, 0], logits[:, 1], e_l[:, 0], e_l[:, 1])
    return pre, logits, MARGIN * e_l, p1, MARGIN * e_p1


def heads_emulate(x, w1t, b1, w2, b2, defect=None):
    """float32 emulation of text_heads_kernel for one head -> (logits [B][2], score [B]).  defects: "drop_slice" --
    the last K-slice left out; "bias_after_relu"; "untransposed" -- the first layer's [256][768] image read as
    [768][256]; "softmax0" -- score = softmax[:, 0]."""
    B = x.shape[0]
    if defect == "untransposed":
        w1t = np.ascontiguousarray(w1t.T).reshape(768, 256)
    hp = np.zeros((4, B, 256), F32)
    for k in range(192):
        for ks in range(4):
            kk = ks * 192 + k
            hp[ks] = fma32(w1t[kk][None, :], x[:, kk][:, None], hp[ks])
    hs = hp[0]
    for q in range(1, 3 if defect == "drop_slice" else 4):
        hs = (hs + hp[q]).astype(F32)
    if defect == "bias_after_relu":
        hv = (np.maximum(hs, F32(0)) + b1).astype(F32)
    else:
        hv = np.maximum((hs + b1).astype(F32), F32(0))
    logits = np.zeros((B, 2), F32)
    for o in range(2):
        part = (hv * w2[o]).astype(F32).reshape(B, 4, 64)          # wave = hidden / 64, lane = hidden % 64
        red = wave_sum32(part)                                       # [B][4]
        l = (((red[:, 0] + red[:, 1]).astype(F32) + red[:, 2]).astype(F32) + red[:, 3]).astype(F32)
        logits[:, o] = (l + b2[o]).astype(F32)
    p0, p1 = softmax2_32(logits[:, 0], logits[:, 1])
    return logits, (p0 if defect == "softmax0" else p1)


# ---------------------------------------------------------------------------------------------
# FusionJudge (fusion_kernel): Linear(5, 64) - ReLU - Linear(64, 32) - ReLU - Linear(32, 2), softmax; verdict,
# confidence and the explanation rule
# ---------------------------------------------------------------------------------------------
def fusion_weights(scale=1.0, seed=0):
    """(w0 [64][5], b0, w3 [32][64], b3, w5 [2][32], b5): PyTorch's Linear init, times `scale`."""
    g = _rng(seed, 11)
    out = []
    for n, k in ((64, 5), (32, 64), (2, 32)):
        a = 1 / np.sqrt(float(k))
        out.append((g.uniform(-a, a, (n, k)) * scale).astype(F32))
        out.append((g.uniform(-a, a, n) * scale).astype(F32))
    return tuple(out)


def fusion_inputs(B, seed=0):
    """x5 [B][5] uniform in [0, 1]."""
    return _rng(B, seed, 13).uniform(0, 1, (B, 5)).astype(F32)


def threshold_rows():
    """Rows that put a single score exactly on, one float32 below and one above a threshold of the cascade, over a
    base row whose rule is the fall-through 5, then rows in which several levels fire at once (the first one in
    the cascade's order x[4], x[2], x[0], x[1] decides), so every level decides at least once."""
    base = np.array([0.1, 0.1, 0.1, 0.5, 0.1], F32)
    rows = [base.copy()]
    for slot in (4, 2, 0, 1):
        for v in around(T07):
            r = base.copy()
            r[slot] = v
            rows.append(r)
    for v in around(T03):
        r = base.copy()
        r[3] = v
        rows.append(r)
    for hot in ((0, 1, 2, 4), (0, 1, 2), (0, 1), (1,), ()):
        r = np.array([0.1, 0.1, 0.1, 0.1, 0.1], F32)
        r[list(hot)] = F32(0.9)
        rows.append(r)
    return np.stack(rows)


def rule_ref(x, defect=None):
    """The cascade of explanation_rule in exact float32 comparisons on x [B][5] -> int32 [B].  defects: "x2_first"
    -- x[2] tested before x[4]; "ge07" -- >= for > at 0.7; "le03" -- <= for < at 0.3."""
    x = x.astype(F32)
    gt = (lambda a: a >= T07) if defect == "ge07" else (lambda a: a > T07)
    lt = (lambda a: a <= T03) if defect == "le03" else (lambda a: a < T03)
    order = [(2, 1), (4, 0), (0, 2), (1, 3)] if defect == "x2_first" else [(4, 0), (2, 1), (0, 2), (1, 3)]
    rule = np.where(lt(x[:, 3]), 4, 5)
    for slot, r in reversed(order):
        rule = np.where(gt(x[:, slot]), r, rule)
    return rule.astype(np.int32)


def fusion_ref(x5, w0, b0, w3, b3, w5, b5):
    """The MLP in float64 -> (probs [B][2], e_probs).  Every layer is a chain of fmaf that starts from the bias:
      a1 = b0 + 5 fmaf      e1 = 5 U (|b0| + sum |w0 x|)
      a2 = b3 + 64 fmaf     e2 = sum |w3| e1 + 64 U (|b3| + sum |w3 h1|)          (ReLU: 1-Lipschitz)
      l  = b5 + 32 fmaf     e_l = sum |w5| e2 + 32 U (|b5| + sum |w5 h2|)
      probs = softmax(l): softmax2_ref.  The bound is returned times MARGIN."""
    x5, w0, b0, w3, b3, w5, b5 = (t.astype(np.float64) for t in (x5, w0, b0, w3, b3, w5, b5))
    h1 = np.maximum(x5 @ w0.T + b0, 0.0)
    e1 = 5 * U * (np.abs(b0) + np.abs(x5) @ np.abs(w0).T)
    h2 = np.maximum(h1 @ w3.T + b3, 0.0)
    e2 = e1 @ np.abs(w3).T + 64 * U * (np.abs(b3) + h1 @ np.abs(w3).T)
    l = h2 @ w5.T + b5
    e_l = e2 @ np.abs(w5).T + 32 * U * (np.abs(b5) + h2 @ np.abs(w5).T)
    p0, p1, e_p0, e_p1 = softmax2_ref(l[:, 0], l[:, 1], e_l[:, 0], e_l[:, 1])
    return np.stack([p0, p1], 1), MARGIN * np.stack([e_p0, e_p1], 1)


def verdict_band(probs, e):
    """Rows whose reference p1 is within the bound of 0.5: the kernel's verdict may differ from the reference's."""
    return np.abs(probs[:, 1] - 0.5) <= e[:, 1]


def fusion_emulate(x5, w0, b0, w3, b3, w5, b5, defect=None):
    """float32 emulation of fusion_mlp + write_verdict -> (probs [B][2], verdict, conf).  defects: "w3_stride64" --
    the padded-65 LDS image of w3 read with row stride 64 (padding slots hold 0); "no_relu2"; "conf_p1"."""
    B = x5.shape[0]
    if defect == "w3_stride64":
        img = np.zeros(32 * 65, F32)
        i = np.arange(2048)
        img[(i >> 6) * 65 + (i & 63)] = w3.reshape(-1)
        w3 = img[:2048].reshape(32, 64)
    a = np.broadcast_to(b0, (B, 64)).astype(F32)
    for i in range(5):
        a = fma32(w0[:, i][None, :], x5[:, i][:, None], a)
    h1 = np.maximum(a, F32(0))
    a = np.broadcast_to(b3, (B, 32)).astype(F32)
    for i in range(64):
        a = fma32(w3[:, i][None, :], h1[:, i][:, None], a)
    h2 = a if defect == "no_relu2" else np.maximum(a, F32(0))
    l = np.broadcast_to(b5, (B, 2)).astype(F32)
    for o in range(32):
        l = fma32(w5[:, o][None, :], h2[:, o][:, None], l)
    p0, p1 = softmax2_32(l[:, 0], l[:, 1])
    verdict = (p1 > T05).astype(np.int32)
    conf = p1 if defect == "conf_p1" else np.where(verdict == 1, p1, p0)
    return np.stack([p0, p1], 1), verdict, conf.astype(F32)


# ---------------------------------------------------------------------------------------------
# Cosine rows (common.h wave_rowdot: rowdot_kernel, the x[3] and text_sim of the finish, the vault's tsim)
# ---------------------------------------------------------------------------------------------
ROWDOT_WIDTHS = (512, 8, 520)  # the production width, fewer columns than lanes, a ragged second pass


def rowdot_inputs(B, C, seed=0):
    """Two sets of unit rows [B][C] with a common component, so the cosines are spread over (-1, 1)."""
    g = _rng(B, C, seed, 17)
    a = g.standard_normal((B, C))
    c = g.standard_normal((B, C)) + a * g.uniform(-1.5, 1.5, (B, 1))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return a.astype(F32), c.astype(F32)


def rowdot_ref(a, c):
    """sum_i a_i c_i per row in float64, and its bound: lane l runs ceil(C / 64) fmaf over columns l, l + 64, ...
    in ascending order, then six tree additions: e = (ceil(C / 64) + 6) U sum |a_i c_i|, times MARGIN."""
    a, c = a.astype(np.float64), c.astype(np.float64)
    C = a.shape[-1]
    return (a * c).sum(-1), MARGIN * (-(-C // 64) + 6) * U * np.abs(a * c).sum(-1)


def rowdot_emulate(a, c, defect=None):
    """float32 emulation of wave_rowdot.  defect "drop_last_pass": the last pass of up to 64 columns left out (a
    single pass: its second half)."""
    B, C = a.shape
    n = -(-C // 64)
    pa, pc = np.zeros((B, n * 64), F32), np.zeros((B, n * 64), F32)
    keep = C if defect is None else ((n - 1) * 64 if n > 1 else C // 2)
    pa[:, :keep], pc[:, :keep] = a[:, :keep], c[:, :keep]
    s = np.zeros((B, 64), F32)
    for j in range(n):
        s = fma32(pa[:, j * 64:(j + 1) * 64], pc[:, j * 64:(j + 1) * 64], s)  # (a padded term adds an exact 0)
    return wave_sum32(s)


# ---------------------------------------------------------------------------------------------
# mmf_analyze_mixed's finish (mixed_finish_kernel)
# ---------------------------------------------------------------------------------------------
def single_modality_probs(x, has_t):
    """misinfo_forensics.py:883-899 in exact float32: fake = clip(text ? misinfo : max(deepfake, discrepancy), 0, 1),
    probs = (1 - fake, fake)."""
    x = x.astype(F32)
    fake = np.where(has_t, x[:, 1], np.maximum(x[:, 2], x[:, 4])).astype(F32)
    fake = np.minimum(np.maximum(fake, F32(0)), F32(1))
    return np.stack([(F32(1) - fake).astype(F32), fake], 1)


def mixed_case(B, variant, seed=0):
    """Hand-built operands of one mixed_finish launch over small lists (nT, nI, nC <= 4).  variant: "novault"
    (c_sims null), "vault" (vault present, title null), "titles" (vault and titles), "nopairs" (nC = 0: the fusion
    weights are null and must not be read).  The row maps cycle through every combination of text, image and
    both, with out-of-range and negative positions and "both" positions whose text or image position is absent;
    the image list's vault results hold a clean hit, a top-1 exactly on the threshold, one float32 above it, a NaN
    and an empty slot (-inf, -1)."""
    g = _rng(B, ("novault", "vault", "titles", "nopairs").index(variant), seed, 19)
    nT, nI, nC = 3, 4, (0 if variant == "nopairs" else 3)
    maps = [
        (0, 0, 0),     # a pair; image 0: a clean hit
        (1, -1, -1),   # text only
        (-1, 1, -1),   # image only; image 1: top-1 exactly on the threshold
        (2, 2, 1),     # a pair; image 2: one float32 above the threshold
        (-1, -1, -1),  # nothing
        (0, 3, 2),     # a pair; image 3: NaN top-1
        (1, 1, -1),    # text and image without a pair position
        (-1, 2, 0),    # a pair position whose text is absent
        (2, -7, 1),    # a pair position whose image is absent (negative)
        (nT, 0, 0),    # text position out of range: image only
        (0, nI, 2),    # image position out of range: text only
        (1, 2, nC),    # pair position out of range
        (2, 3, 0),     # a pair on the NaN image
        (1, 1, 0),     # a pair on image 1: top-1 exactly on the threshold, so `>` decides its text_sim
    ]
    # the batches start at different maps: B = 1, 4, 5, 9 take maps 0, 1-4, 5-9 and 10-13 + 0-4, every kind together
    first = {1: 0, 4: 1, 5: 5, 9: 10}.get(B, 0)
    row_map = np.array([maps[(first + i) % len(maps)] for i in range(B)], np.int32)
    text2 = g.uniform(0, 1, (nT, 2)).astype(F32)
    deepfake = g.uniform(0, 1, nI).astype(F32)
    v_emb, t_full = rowdot_inputs(4, 512, seed + 1)
    t_emb = t_full[:3]
    _, at, above = around(T085)
    c_sims = np.sort(g.uniform(0.2, 0.8, (nI, 5)).astype(F32), axis=1)[:, ::-1].copy()
    c_idx = g.integers(0, 6, (nI, 5)).astype(np.int32)
    c_sims[0, 0] = F32(0.93)
    c_sims[1, 0] = at
    c_sims[2, 0] = above
    c_sims[3, 0] = F32(np.nan)
    c_disc = np.array([c_sims[0, 0], 0, above, 0], F32)
    title = rowdot_inputs(6, 512, seed + 2)[1]
    out = dict(row_map=row_map, B=B, nT=nT, nI=nI, nC=nC, text2=text2, deepfake=deepfake, v_emb=v_emb,
               t_emb=t_emb if nC else None, c_sims=None, c_idx=None, c_disc=None, title=None, thresh=T085)
    if variant != "novault":
        out.update(c_sims=c_sims, c_idx=c_idx, c_disc=c_disc)
    if variant in ("titles", "nopairs"):
        out["title"] = title
    return out


def mixed_case_empty_slot(case):
    """The same case with image 0's top-1 an empty slot (-inf, -1): never a hit, whatever the threshold."""
    c = dict(case)
    c["c_sims"], c["c_idx"], c["c_disc"] = case["c_sims"].copy(), case["c_idx"].copy(), case["c_disc"].copy()
    c["c_sims"][0, 0], c["c_idx"][0, 0], c["c_disc"][0] = F32(-np.inf), -1, F32(0)
    return c


def mixed_finish_ref(c):
    """What mixed_finish_kernel must write for a case of mixed_case: the exact gathers (scores5 columns 0-2 and 4,
    top_sims, top_idx, or the absent convention 0 / -1), the float64 cosines with their rowdot bounds (x[3] of a
    pair; text_sim of a pair whose image has a vault hit and titles, else exactly 0 with bound 0), the operand rows
    of those cosines (for the bit comparison with rowdot_kernel), and per row the set of branches it takes.  A
    top1_* tag marks a pair row with vault and titles, the only place where the kernel's `top1 > thresh` decides
    something (text_sim); on any other vault row the top-1 is a plain gather and the tag is gathered_top1_*."""
    rm, B = c["row_map"], c["B"]
    x = np.zeros((B, 5), F32)
    x3, e3, ts, ets = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    top_sims, top_idx = np.zeros((B, 5), F32), np.full((B, 5), -1, np.int32)
    has_t = np.zeros(B, bool)
    has_c = np.zeros(B, bool)
    x3_rows, ts_rows, tags = [], [], []
    for r in range(B):
        ti, ii, ci = (int(v) for v in rm[r])
        t, i = 0 <= ti < c["nT"], 0 <= ii < c["nI"]
        pair = t and i and 0 <= ci < c["nC"]
        vault = i and c["c_sims"] is not None
        has_t[r], has_c[r] = t, pair
        tag = {"t" if t else "no_t", "i" if i else "no_i", "pair" if pair else "single",
               "vault" if vault else "no_vault"}
        if t and i and not pair:
            tag.add("t_i_without_pair")
        if 0 <= ci < c["nC"] and not (t and i):
            tag.add("pair_position_absent_side")
        if t:
            x[r, 0:2] = c["text2"][ti]
        if i:
            x[r, 2] = c["deepfake"][ii]
        if vault:
            x[r, 4] = c["c_disc"][ii]
            top_sims[r], top_idx[r] = c["c_sims"][ii], c["c_idx"][ii]
            top1, id1 = c["c_sims"][ii, 0], int(c["c_idx"][ii, 0])
            kind = ("nan" if np.isnan(top1) else "empty" if id1 < 0 else "at_thresh" if top1 == c["thresh"] else
                    "ulp_above" if top1 == np.nextafter(c["thresh"], F32(np.inf)) else
                    "hit" if top1 > c["thresh"] else "miss")
            # the threshold comparison decides something only on a pair with titles (its text_sim): the top1_*
            # tags count there alone; elsewhere the top-1 is a plain gather
            tag.add(("top1_" if pair and c["title"] is not None else "gathered_top1_") + kind)
        if pair:
            x3[r], e3[r] = (v[0] for v in rowdot_ref(c["v_emb"][ii][None], c["t_emb"][ci][None]))
            x3_rows.append((r, ii, ci))
            if vault and c["title"] is not None and top1 > c["thresh"] and id1 >= 0:
                ts[r], ets[r] = (v[0] for v in rowdot_ref(c["t_emb"][ci][None], c["title"][id1][None]))
                ts_rows.append((r, ci, id1))
                tag.add("text_sim")
            elif vault and c["title"] is None:
                tag.add("pair_vault_no_titles")
        tags.append(tag)
    return dict(x=x, x3=x3, e3=e3, text_sim=ts, e_text_sim=ets, top_sims=top_sims, top_idx=top_idx, has_t=has_t,
                has_c=has_c, x3_rows=x3_rows, ts_rows=ts_rows, tags=tags)


# every branch of the finish that the GPU test asserts it has run (the union over its cases)
MIXED_BRANCHES = {"t", "no_t", "i", "no_i", "pair", "single", "vault", "no_vault", "t_i_without_pair",
                  "pair_position_absent_side", "top1_nan", "top1_empty", "top1_at_thresh", "top1_ulp_above",
                  "top1_hit", "text_sim", "pair_vault_no_titles"}
