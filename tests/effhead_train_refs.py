"""Restatements of the head-stage training (csrc/effhead_train.hip, mmf_effhead_train_epoch and mmf_effhead_eval) in
numpy, shared by tests/test_effhead_train_refs_cpu.py (no GPU) and tests/test_gpu_effhead_train.py.

``epoch(..., dtype=np.float64)`` is the reference of the kernel's contract: a bank of R trunk rows [R, 49, 320];
minibatch s = positions s*batch .. of perm, the last one short; entries clamped into [0, R); labels read as label & 1;

    z = x W^T      s_c = gamma_c / sqrt(var_c + eps)      t_c = beta_c - mean_c s_c      y = s_c z + t_c
    a = y sigmoid(y)      pooled = (sum over the 49 positions) / 49      (BatchNorm in EVAL mode: mean, var are inputs)

then tests/effcls_train_refs.py's contract on the pooled row (xd = pooled keep scale, logits, mean cross-entropy),
the analytic backward to all five tensors (none to the trunk) and torch.optim.Adam's single-tensor update on the flat
vector W | gamma | beta | Wc | bc.  ``dtype=np.float32`` is the same statement in float32, the step-dependent Adam
scalars computed in double and rounded once, in numpy's summation order, not the kernel's: its distance to the
float64 run is the scale the multi-step test measures the kernel against.

``step_bounds`` derives, beside the float64 forward and backward of ONE minibatch and never from what a kernel
returned, per-element bounds for the fp32 pooled rows, logits, loss, the gradient of all five tensors, both moments
and the parameters after the step: absolute values propagated through forward and backward, first-order worst case
times 2, U = 2^-24.  A contraction of length L through an ordered fmaf chain contributes at most L U sum |terms| (the
pool: 49; dW, dgamma, dbeta: M = 49 n; the classifier's tree: effcls_train_refs.DEPTH).  For z, the 320-term chain
every later quantity inherits its error from, that form is too coarse to tell anything about the conv weight's first
step (it leaves the sign of most of its gradient undecided), so the same chain is bounded by its own partial sums,
U sum_k |s_k| <= 320 U sum |terms| (``chain_partials``): a tighter bound of the same fixed order, never a wider one.  SiLU's error is
effnet_refs.act_err, 8 U |a| + U; silu'(y) = sig (1 + y (1 - sig)) is bounded the same way from its own roundings: the
sigmoid (act_err), the subtraction, the product, the addition and the last product.  The first Adam step is
sign-like: the parameter bound is the exact variation of g / (|g| + eps) over the gradient's own interval, as in
effcls_train_refs.

The multi-step floor, per tensor.  An Adam step rounds a parameter once, by at most half an ulp: a tensor whose
entries stay below TOP = the power of two above its largest initial magnitude plus the run's movement has half-ulp
TOP 2^-25, so two correct fp32 evaluations may part by FLOOR = 2 x TOP x 2^-25 per step (``floors``).  The bound of a
tensor is 8 x max(e32, FLOOR x steps, cond), cond = train_refs_common.Drift's conditioning number over the tensor's
slice, fed with the magnitudes of ``_magnitudes``; tests/test_effhead_train_refs_cpu.py asserts on the reference alone
that it stays below 0.1 x the distance the tensor's parameters move.
"""
import functools

import numpy as np

from tests import effcls_train_refs as E
from tests import train_refs_common as C
from tests.train_refs_common import Drift, U, flat, pack_keep  # noqa: F401

KIN, CH, HW = 320, 1280, 49
N_PARAMS = CH * KIN + 2 * CH + 2 * CH + 2  # MMF_EFFHEAD_PARAMS
assert N_PARAMS == 414722
OFF_G, OFF_B, OFF_WC, OFF_BC = CH * KIN, CH * KIN + CH, CH * KIN + 2 * CH, CH * KIN + 4 * CH
SLICES = {"features.8.0.weight": slice(0, OFF_G), "features.8.1.weight": slice(OFF_G, OFF_B),
          "features.8.1.bias": slice(OFF_B, OFF_WC), "classifier.1.weight": slice(OFF_WC, OFF_BC),
          "classifier.1.bias": slice(OFF_BC, N_PARAMS)}
BN_EPS = 1e-5
BETAS, EPS, P_DROP, SCALE = E.BETAS, E.EPS, E.P_DROP, E.SCALE
WORDS = CH // 64

MULTI_CASES = ((37, 16, 2), (10, 1, 1), (70, 64, 2))
MULTI_LR = 1e-4
# per case, chosen on the CPU: test_effhead_train_refs_cpu.py::test_multi_step_cases_qualify
MULTI_SEEDS = {(37, 16, 2): 10, (10, 1, 1): 11, (70, 64, 2): 37}
SINGLE_BATCHES = (1, 2, 5, 16, 64)
SINGLE_SEED = 31
SINGLE_LR = 1e-4
SINGLE_WDS = (0.0, 1e-2)

unpack_keep = E.unpack_keep


def unpack(p):
    """flat [414722] -> (W [1280, 320], gamma [1280], beta [1280], Wc [2, 1280], bc [2]) (views)."""
    return (p[:OFF_G].reshape(CH, KIN), p[OFF_G:OFF_B], p[OFF_B:OFF_WC], p[OFF_WC:OFF_BC].reshape(2, CH), p[OFF_BC:])


@functools.lru_cache(maxsize=None)
def _initial(seed):
    """The distributions mmf_amd/weights.py draws features.8.* and the classifier from: the conv N(0, 1.3^2 / 320),
    the BatchNorm weight 1 + 0.1 N, bias and running mean 0.1 N, running variance U(0.5, 1.5), the classifier
    N(0, 0.1^2) with bias N(0, 0.05^2)."""
    g = np.random.default_rng([seed, 414722])
    p = np.concatenate([g.standard_normal(CH * KIN) * (1.3 / np.sqrt(KIN)), 1.0 + 0.1 * g.standard_normal(CH),
                        0.1 * g.standard_normal(CH), 0.1 * g.standard_normal(2 * CH), 0.05 * g.standard_normal(2)])
    mean, var = 0.1 * g.standard_normal(CH), g.uniform(0.5, 1.5, CH)
    return p.astype(np.float32), mean.astype(np.float32), var.astype(np.float32)


def initial_params(seed: int = 0):
    """(params float32 [414722], bn_mean float32 [1280], bn_var float32 [1280]) (copies)."""
    return tuple(a.copy() for a in _initial(int(seed)))


@functools.lru_cache(maxsize=None)
def _draws(N, seed):
    g = np.random.default_rng([seed, N, 49])
    # the last MBConv block's output: linear (no activation) with a residual -- zero mean, a few large entries
    x = 0.5 * g.standard_normal((N, HW, KIN)) + (g.random((N, HW, KIN)) < 0.01) * 5.0 * g.standard_normal((N, HW, KIN))
    y = (x.mean(1) @ g.standard_normal(KIN) + 0.05 * g.standard_normal(N) > 0).astype(np.int32)
    return x.astype(np.float32), y


def draws(N: int, seed: int = 0):
    """(trunk float32 [N, 49, 320], labels int32 [N]) (copies)."""
    a, b = _draws(int(N), int(seed))
    return a.copy(), b.copy()


def _mult(keep, pos, dtype):
    if keep is None:
        return np.ones((len(pos), CH), dtype)
    return unpack_keep(keep[pos]).astype(dtype) * dtype(SCALE)


def stage(x, params, mean, var, dtype, eps=BN_EPS, div=HW):
    """The head stage of one batch x [n, 49, 320] -> dict(z, s, t, rstd, y, sig, a, pooled)."""
    dt = dtype
    W, gamma, beta = unpack(params)[:3]
    x = x.astype(dt)
    z = x @ W.T
    rstd = dt(1.0) / np.sqrt(var.astype(dt) + dt(eps))
    s = gamma * rstd
    t = beta - mean.astype(dt) * s
    y = s * z + t
    sig = dt(1.0) / (dt(1.0) + np.exp(-y))
    a = y * sig
    pooled = a.sum(1, dtype=dt) / dt(div)
    return dict(x=x, z=z, s=s, t=t, rstd=rstd, y=y, sig=sig, a=a, pooled=pooled, mean=mean.astype(dt))


def forward_backward(x, mult, params, mean, var, y, dtype, eps=BN_EPS, div=HW):
    """One minibatch -> (stage dict, effcls forward_backward dict, flat gradient [414722])."""
    dt = dtype
    W, gamma, beta, Wc, bc = unpack(params)
    h = stage(x, params, mean, var, dt, eps, div)
    r = E.forward_backward(h["pooled"], mult, Wc, bc, y, dt)
    dpooled = mult.astype(dt) * (r["dl"] @ Wc)
    d = h["sig"] * (dt(1.0) + h["y"] * (dt(1.0) - h["sig"]))
    dy = (dpooled / dt(div))[:, None, :] * d
    xh = (h["z"] - h["mean"]) * h["rstd"]
    dgamma = (dy * xh).sum((0, 1), dtype=dt)
    dbeta = dy.sum((0, 1), dtype=dt)
    dW = (dy * h["s"]).reshape(-1, CH).T @ h["x"].reshape(-1, KIN)
    h.update(dpooled=dpooled, d=d, dy=dy, xh=xh)
    return h, r, flat((dW, dgamma, dbeta) + tuple(r["grads"]))


def adam(p, m, v, g, lr, step, dtype, wd=0.0, decoupled=False):
    C.adam(p, m, v, g, lr, step, dtype, wd, "decoupled" if decoupled else "l2", BETAS, EPS)


def _magnitudes(h, r):
    """Per parameter, the magnitude of which ANY fp32 evaluation of the gradient carries at least half an ulp: every
    term of its sum once for its own rounding and once for each operand that is itself a rounded fp32 value (dy, the
    product dy s, the normalised z; dlogits and the rounded pooled row for the classifier)."""
    a = np.abs
    ady = a(h["dy"]).reshape(-1, CH)
    adl = a(r["dl"])
    return np.concatenate([3 * ((ady * a(h["s"])).T @ a(h["x"]).reshape(-1, KIN)).reshape(-1),
                           3 * (ady * a(h["xh"]).reshape(-1, CH)).sum(0), 2 * ady.sum(0),
                           3 * (adl.T @ a(r["xd"])).reshape(-1), 2 * adl.sum(0)])


def epoch(trunk, labels, perm, keep, batch, lr, step0, params, exp_avg, exp_avg_sq, mean, var, dtype=np.float64,
          wd=0.0, drift=None, broken=""):
    """One epoch on flat params / exp_avg / exp_avg_sq (arrays of `dtype`, updated in place) over the bank trunk
    [R, 49, 320] / labels [R]; perm [N] bank rows; keep uint64 [N, 20] or None.  -> (step_loss, step_correct [nsteps],
    loss gradient of the last minibatch flat).  broken: "adamw" (decoupled decay), "pool" (the mean over 49 left out)
    -- the restatements the CPU test holds against torch."""
    N, R = len(perm), len(labels)
    dt = dtype
    losses, correct, g = [], [], None
    for s in range(-(-N // batch)):
        pos = np.arange(s * batch, min(N, (s + 1) * batch))
        src = np.clip(perm[pos].astype(np.int64), 0, R - 1)
        h, r, g = forward_backward(trunk[src], _mult(keep, pos, dt), params, mean, var, labels[src] & 1, dt,
                                  div=1 if broken == "pool" else HW)
        if drift is not None:
            drift.gradient(g, U * _magnitudes(h, r))
        adam(params, exp_avg, exp_avg_sq, g, lr, step0 + s + 1, dt, wd=wd, decoupled=broken == "adamw")
        if drift is not None:
            drift.update(exp_avg, exp_avg_sq, lr, step0 + s + 1)
        losses.append(float(r["loss"]))
        correct.append(r["correct"])
    return np.array(losses), np.array(correct), g


def evaluate(trunk, labels, batch, params, mean, var, dtype=np.float64):
    """validate's forward: no dropout, consecutive batches in row order -> (batch_loss [nb], row_logits [R, 2])."""
    p = params.astype(dtype)
    Wc, bc = unpack(p)[3:]
    losses, lg = [], []
    for a in range(0, len(labels), batch):
        h = stage(trunk[a:a + batch], p, mean, var, dtype)
        r = E.forward(h["pooled"], np.ones_like(h["pooled"]), Wc, bc, labels[a:a + batch] & 1, dtype)
        losses.append(float(r["loss"]))
        lg.append(r["lg"])
    return np.array(losses), np.concatenate(lg)


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def act_err(a):
    """effnet_refs.act_err on a numpy array: an fp32 SiLU / sigmoid with value a."""
    return 8 * U * np.abs(a) + U


def chain_partials(x, W, block=16):
    """An upper bound of sum_k |s_k|, s_k = sum_{j <= k} x[m, j] W[c, j] the partial sums of the ascending-k fmaf chain
    from 0 that forms z (csrc/effhead_train.hip, launch 1): x [M, K], W [C, K] -> [M, C].  Step k of the chain rounds
    s_k once, by at most U |s_k|, so the chain's first-order error is at most U times this sum -- never more than
    K sum |terms|, which takes every |s_k| for the sum of ALL absolute terms.  Here, per block of 16 steps starting at
    the exact float64 partial sum S, |s_k| <= |S| + sum of the block's absolute terms up to k: the block contributes
    16 |S| + sum_j (16 - j) |term_j|, j the term's place in the block.  (Partial sums of signed terms grow like
    sqrt(k), the sum of absolute terms like k: about 11 x tighter on the trunk rows' statistics, at the cost of two
    matrix products.)"""
    M, K = x.shape
    out, S = np.zeros((M, W.shape[0])), np.zeros((M, W.shape[0]))
    for b in range(0, K, block):
        xb, Wb = x[:, b:b + block], W[:, b:b + block]
        w = block - np.arange(xb.shape[1])
        out += xb.shape[1] * np.abs(S) + (np.abs(xb) * w) @ np.abs(Wb).T
        S += xb @ Wb.T
    return out


def stage_bounds(h, params64):
    """First-order bounds (no factor 2) of the fp32 head stage beside its float64 run h -> dict(e_z, e_s, e_y,
    e_pooled)."""
    a = np.abs
    W = unpack(params64)[0]
    e_z = U * chain_partials(h["x"].reshape(-1, KIN), W).reshape(h["z"].shape)
    e_s = 4 * U * a(h["s"])                                  # the fp32 eps, the add, the square root, the division
    e_t = a(h["mean"]) * e_s + U * a(h["t"])                 # one fmaf
    e_y = a(h["s"]) * e_z + a(h["z"]) * e_s + e_t + U * a(h["y"])
    e_a = 1.1 * e_y + act_err(h["a"])                        # |silu'| <= 1.1
    e_pooled = (e_a.sum(1) + HW * U * a(h["a"]).sum(1)) / HW + 2 * U * a(h["pooled"])
    return dict(e_z=e_z, e_s=e_s, e_y=e_y, e_pooled=e_pooled)


def forward_bounds(h, r, params64, mult, dropout):
    """-> (stage_bounds' dict, e_xd [n, 1280], pooled_tol, lg_tol [n, 2], loss_tol): the tolerances with the factor 2."""
    a = np.abs
    Wc = unpack(params64)[3]
    sb = stage_bounds(h, params64)
    n = r["xd"].shape[0]
    e_xd = sb["e_pooled"] * mult + (U * a(r["xd"]) if dropout else 0.0)
    e_lg = e_xd @ a(Wc).T + E.DEPTH * U * (a(r["xd"]) @ a(Wc).T) + U * a(r["lg"])
    p = r["e"] / r["se"][:, None]
    slope = a(p - np.eye(2)[r["y"]])
    e_li = (slope * e_lg).sum(1) + 8 * U * (1.0 + a(r["m"]) + a(np.log(r["se"])) + a(r["lg"]).max(1))
    loss_tol = 2 * (e_li.mean() + U * (n + 2) * a(r["li"]).mean())
    return sb, e_xd, 2 * sb["e_pooled"], 2 * e_lg, float(loss_tol)


def _first_update(g):
    return g / (np.abs(g) + EPS)


def grad_bounds(x, mult, params64, mean, var, y, dropout):
    """The float64 forward / backward of one minibatch and the fp32 kernel's bounds -> dict(r, pooled, pooled_tol, lg,
    lg_tol, loss, loss_tol, margin_ok, grad, grad_tol) (the part of step_bounds that does not depend on the optimizer)."""
    a = np.abs
    mean64, var64 = mean.astype(np.float64), var.astype(np.float64)
    Wc = unpack(params64)[3]
    h, r, g = forward_backward(x, mult, params64, mean64, var64, y, np.float64)
    n, M = x.shape[0], x.shape[0] * HW
    sb, e_xd, pooled_tol, lg_tol, loss_tol = forward_bounds(h, r, params64, mult, dropout)
    e_lg = lg_tol / 2
    p = r["p"]
    rel = U * (10 + a(r["lg"] - r["m"][:, None]))
    e_p = p * (e_lg + (p * e_lg).sum(1, keepdims=True)) + rel * p
    e_dl = (e_p + 3 * U * a(p - r["onehot"])) / n
    adl, axd = a(r["dl"]), a(r["xd"])
    e_gWc = e_dl.T @ axd + adl.T @ e_xd + U * (n + 1) * (adl.T @ axd)
    e_gbc = e_dl.sum(0) + U * n * adl.sum(0)
    # dpooled = mult fmaf(dl1, Wc1, dl0 Wc0): two roundings, the multiplier's a third
    e_dp = mult * (e_dl @ a(Wc) + 2 * U * (adl @ a(Wc))) + U * a(h["dpooled"])
    # silu'(y) = sig (1 + y (1 - sig))
    sig, yv = h["sig"], h["y"]
    e_sig = 0.25 * sb["e_y"] + act_err(sig)
    q = 1 - sig
    e_q = e_sig + U * a(q)
    rr = yv * q
    e_r = a(q) * sb["e_y"] + a(yv) * e_q + U * a(rr)
    w = 1 + rr
    e_w = e_r + U * a(w)
    e_d = a(w) * e_sig + sig * e_w + U * a(h["d"])
    dp49 = h["dpooled"] / HW
    e_dy = (e_dp / HW + U * a(dp49))[:, None, :] * a(h["d"]) + a(dp49)[:, None, :] * e_d + U * a(h["dy"])
    ady = a(h["dy"])
    e_gbeta = e_dy.sum((0, 1)) + M * U * ady.sum((0, 1))
    e_xh = h["rstd"] * sb["e_z"] + 5 * U * a(h["xh"])        # the subtraction, sd's add and square root, the division
    e_ggamma = (e_dy * a(h["xh"]) + ady * e_xh).sum((0, 1)) + M * U * (ady * a(h["xh"])).sum((0, 1))
    ads = ady * a(h["s"])                                    # the MFMA's operand dy s: one more rounding
    e_ads = e_dy * a(h["s"]) + ady * sb["e_s"] + U * ads
    ax = a(h["x"]).reshape(M, KIN)
    e_gW = e_ads.reshape(M, CH).T @ ax + M * U * (ads.reshape(M, CH).T @ ax)
    grad_tol = 2 * flat((e_gW, e_ggamma, e_gbeta, e_gWc, e_gbc))
    margin_ok = bool((a(r["lg"][:, 1] - r["lg"][:, 0]) > lg_tol.sum(1)).all())
    return dict(r=r, pooled=h["pooled"], pooled_tol=pooled_tol, lg=r["lg"], lg_tol=lg_tol, loss=float(r["loss"]),
                loss_tol=loss_tol, margin_ok=margin_ok, grad=g, grad_tol=grad_tol)


def step_bounds(x, mult, params64, mean, var, y, dropout, lr=SINGLE_LR, wd=0.0, gb=None):
    """grad_bounds' dict (gb, or computed here) plus the first Adam step (zero moments, step 1) and its bounds: m,
    m_tol, v, v_tol, p, p_tol."""
    a = np.abs
    gb = grad_bounds(x, mult, params64, mean, var, y, dropout) if gb is None else gb
    g, grad_tol = gb["grad"], gb["grad_tol"]
    gd = g + wd * params64
    gd_tol = grad_tol + (2 * U * a(gd) if wd else 0.0)
    m64, v64 = (1 - BETAS[0]) * gd, (1 - BETAS[1]) * gd * gd
    m_tol = (1 - BETAS[0]) * gd_tol + 4 * U * a(m64)
    v_tol = (1 - BETAS[1]) * (2 * a(gd) * gd_tol + gd_tol * gd_tol) + 4 * U * v64
    f0 = _first_update(gd)
    p64 = params64 - lr * f0
    vary = np.maximum(a(_first_update(gd + gd_tol) - f0), a(_first_update(gd - gd_tol) - f0))  # monotone in g
    p_tol = lr * vary + 2 * (8 * U * lr + U * a(p64))
    return dict(gb, m=m64, m_tol=m_tol, v=v64, v_tol=v_tol, p=p64, p_tol=p_tol)


def eval_bounds(trunk, labels, batch, params64, mean, var):
    """Per batch of mmf_effhead_eval: (loss, loss_tol, lg, lg_tol) from the float64 forward alone."""
    out = []
    mean64, var64 = mean.astype(np.float64), var.astype(np.float64)
    Wc, bc = unpack(params64)[3:]
    for a in range(0, len(labels), batch):
        h = stage(trunk[a:a + batch], params64, mean64, var64, np.float64)
        r = E.forward(h["pooled"], np.ones_like(h["pooled"]), Wc, bc, labels[a:a + batch] & 1, np.float64)
        _, _, pooled_tol, lg_tol, loss_tol = forward_bounds(h, r, params64, np.ones_like(h["pooled"]), False)
        out.append(dict(loss=float(r["loss"]), loss_tol=loss_tol, lg=r["lg"], lg_tol=lg_tol, pooled=h["pooled"],
                        pooled_tol=pooled_tol))
    return out


def floors(p0, moved=0.0):
    """Per tensor name, FLOOR = 2 x the half-ulp below TOP, TOP the power of two above max |p0| + moved."""
    out = {}
    for name, sl in SLICES.items():
        top = 2.0 ** np.ceil(np.log2(float(np.abs(p0[sl]).max()) + moved))
        out[name] = 2 * top * 2.0 ** -25
    return out


@functools.lru_cache(maxsize=None)
def _grad_case(n, dropout):
    R = 2 * n + 3
    for seed in range(SINGLE_SEED, SINGLE_SEED + 16):
        trunk, labels = draws(R, seed)
        p0, mean, var = initial_params(seed)
        g = np.random.default_rng([seed, n, 7])
        perm = g.permutation(R)[:n].astype(np.int32)
        perm[0] = R - 1  # the upper half of the bank
        keep = pack_keep(g.random((n, CH)) >= P_DROP) if dropout else None
        b = grad_bounds(trunk[perm], _mult(keep, np.arange(n), np.float64), p0.astype(np.float64), mean, var,
                        labels[perm], dropout)
        if b["margin_ok"]:
            return trunk, labels, perm, keep, p0, mean, var, b, seed
    raise AssertionError(f"no qualifying seed for n={n} dropout={dropout}")


@functools.lru_cache(maxsize=None)
def _single_case(n, dropout, wd):
    trunk, labels, perm, keep, p0, mean, var, gb, seed = _grad_case(n, dropout)
    b = step_bounds(None, None, p0.astype(np.float64), mean, var, None, dropout, wd=wd, gb=gb)
    return trunk, labels, perm, keep, p0, mean, var, b, seed


def single_case(n, dropout, wd=0.0):
    """(trunk [2n + 3, 49, 320], labels, perm [n], keep or None, params, bn_mean, bn_var float32, step_bounds' dict,
    seed) of a single-step case: the first seed from SINGLE_SEED whose float64 run decides every argmax.  Read-only."""
    return _single_case(int(n), bool(dropout), float(wd))


@functools.lru_cache(maxsize=None)
def _run_case(N, batch, epochs, dtype, seed, lr, broken):
    trunk, labels = draws(N, seed)
    p0, mean, var = initial_params(seed)
    p = p0.astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    g = np.random.default_rng([seed, N, batch, epochs])
    plan, losses, step0 = [], [], 0
    drift = Drift() if dtype == np.float64 and broken in ("", "l2") else None
    wd = 1e-2 if broken in ("adamw", "l2") else 0.0
    for e in range(epochs):
        perm = g.permutation(N).astype(np.int32)
        keep = pack_keep(g.random((N, CH)) >= P_DROP)
        plan.append((perm, keep))
        ls, _, _ = epoch(trunk, labels, perm, keep, batch, lr, step0, p, m, v, mean.astype(dtype), var.astype(dtype),
                         dtype, wd=wd, drift=drift, broken=broken)
        step0 += len(ls)
        losses.append(ls)
    cond = {k: float(drift.total[sl].max()) for k, sl in SLICES.items()} if drift else None
    return p, m, v, losses, plan, cond, p0, mean, var


def run_case(N, batch, epochs, dtype, seed=None, lr=MULTI_LR, broken=""):
    """A multi-step case from the initial parameters and zero moments, epoch by epoch with step0 carried over; per
    epoch a fresh permutation and dropout mask.  broken: "adamw" (decoupled decay 1e-2) or "l2" (the correct Adam with
    weight_decay 1e-2).  -> (params, exp_avg, exp_avg_sq, losses, plan [(perm, keep)], cond per tensor, initial
    params, bn_mean, bn_var).  Shared: read-only."""
    seed = MULTI_SEEDS[(N, batch, epochs)] if seed is None else seed
    return _run_case(int(N), int(batch), int(epochs), dtype, int(seed), float(lr), broken)


def multi_bounds(case, seed=None, broken=""):
    """Per tensor name (bound, e32, floor x steps, cond, moved) of a multi-step case, from the two restatements."""
    p64, _, _, l64, _, cond, p0 = run_case(*case, np.float64, seed, broken=broken)[:7]
    p32 = run_case(*case, np.float32, seed, broken=broken)[0]
    steps = sum(len(l) for l in l64)
    moved_all = float(np.abs(p64 - p0).max())
    fl = floors(p0, moved_all)
    out = {}
    for name, sl in SLICES.items():
        e32 = float(np.abs(p32[sl] - p64[sl]).max())
        out[name] = (8 * max(e32, fl[name] * steps, cond[name]), e32, fl[name] * steps, cond[name],
                     float(np.abs(p64[sl] - p0[sl]).max()))
    return out
