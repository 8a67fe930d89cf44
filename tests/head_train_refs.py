"""Restatements of the RoBERTa text-head training (csrc/head_train.hip, mmf_head_train_epoch and mmf_head_eval) in
numpy, shared by tests/test_head_train_refs_cpu.py (no GPU) and tests/test_gpu_head_train.py.

``epoch(..., dtype=np.float64)`` is the reference: the kernel's contract (minibatch s = positions s*batch .. of
perm, the last one short; labels read as label & 1; pre = X W1^T + b1; h = relu(pre) keep scale with scale = the
float32 value of 1 / (1 - p_drop), keep[i] the mask of the row at POSITION i; logits = h W2^T + b2; the mean
cross-entropy; the analytic backward to all four tensors; clip_grad_norm_'s coefficient max_norm / (norm + 1e-6)
clamped at 1 and always applied; torch.optim.AdamW's single-tensor update with bias correction by step0 + s + 1
and the step's own learning rate) in float64.  ``dtype=np.float32`` is the same statement in float32 -- the
step-dependent Adam scalars computed in double and rounded once, as the kernel does -- in numpy's summation order,
not the kernel's: its distance to the float64 run is the scale the multi-step test measures the kernel against.

``step_bounds`` derives, beside the float64 forward and backward of ONE minibatch and never from what a kernel
returned, a per-element bound for the fp32 clipped gradient, the loss, the total norm and the logits: absolute
values propagated through forward and backward, first-order worst case times 2, U = 2^-24; the error of a chain
whose order the contract fixes is U x the sum of |float64 partial sums| (``chain_err``).  Two branches are decided
by the reference alone.  The clamp of the clip coefficient: the float64 norm must be above 1.5 x max_norm or below
0.67 x max_norm.  The ReLU: every |pre| of the minibatch must exceed its own forward bound, so no fp32 evaluation
can put a hidden unit on the other side; ``single_case`` walks seeds SINGLE_SEED, SINGLE_SEED + 1, ... and takes
the first whose float64 run satisfies both (a function of the reference alone, the same on every machine).

The multi-step floor.  An AdamW step rounds a parameter twice (p * decay, then p - update), each time by at most
half an ulp.  With nn.Linear's default initialisation the head's parameters start below 1 / 16 and stay below
0.125 (half-ulp 2^-28), so two correct fp32 evaluations may part by FLOOR = 2 x 2^-28 = 7.5e-9 per step.

Conditioning of a multi-step case (``Drift``, float64 run only).  Adam divides a gradient by its own running
magnitude, and its first steps are sign-like: a gradient that is tiny against the terms of its own sum can come
out with either sign.  Any fp32 evaluation of a gradient sum_r a_r b_r carries at least half an ulp of every term,
and another half for each operand that is itself a rounded value, however small the result (``_magnitudes``).
``Drift`` (tests/train_refs_common.py) carries that error through AdamW's update to first order, step by step; cond = the largest distance over
the parameters at which two correct fp32 evaluations can end.  Among 196,608 weights some gradient is always tiny
against its own terms, so at the reference's lr = 1e-3 cond lies far above FLOOR x steps and is part of the bound:
K <= 8 x max(e32, FLOOR x steps, cond).  What keeps that bound from hiding a failure is asserted on the reference
alone (tests/test_head_train_refs_cpu.py): it stays below 0.1 x max |p64_final - p_initial|, so a kernel that
trains differently (a missing dropout scale, a wrong bias correction) lands outside it.
"""
import functools

import numpy as np

from tests.train_refs_common import Drift, U, adam, chain_err, clip_coef, flat, pack_keep  # noqa: F401
from tests.train_refs_common import unpack_keep as _unpack_keep

K, H = 768, 256
NW1 = H * K
O_B1, O_W2, O_B2 = NW1, NW1 + H, NW1 + H + 2 * H
N_PARAMS = O_B2 + 2  # MMF_HEAD_PARAMS
BETAS, EPS, WD, MAX_NORM, P_DROP = (0.9, 0.999), 1e-8, 0.01, 1.0, 0.3
SCALE = float(np.float32(1.0 / (1.0 - P_DROP)))  # the contract's dropout scale
FLOOR = 2 * 2.0 ** -28                            # per step: module docstring

# (N, batch, epochs) of the multi-step test, at the reference's own learning rate with its per-step schedule
MULTI_CASES = ((37, 16, 2), (17, 16, 2), (10, 1, 1), (130, 64, 2))
MULTI_LR = 1e-3
MULTI_SEED = 1  # of seeds 1, 2, 3, 7 the one whose bound / movement is smallest on every case
# the single-step test: batches x regimes x dropout
SINGLE_BATCHES = (1, 2, 5, 16, 64)
SINGLE_SEED = 13
# regime -> (feature gain, max_norm): "clip" float64 norms 2.3 .. 25 against 1; "noclip" 0.13 .. 1.0 against 4 (at
# max_norm 1 a one-row batch cannot get below 0.67: dL/db2 alone has norm ~0.7, even with a label the forward favours)
REGIMES = {"clip": (2.0, 1.0), "noclip": (0.05, 4.0)}


@functools.lru_cache(maxsize=None)
def _initial(seed):
    g = np.random.default_rng([seed, 256])
    b1, b2 = 1.0 / np.sqrt(K), 1.0 / np.sqrt(H)
    p = np.empty(N_PARAMS, np.float32)
    p[:NW1] = g.uniform(-b1, b1, NW1)
    p[O_B1:O_W2] = g.uniform(-b1, b1, H)
    p[O_W2:O_B2] = g.uniform(-b2, b2, 2 * H)
    p[O_B2:] = g.uniform(-b2, b2, 2)
    return p


def initial_params(seed: int = 0) -> np.ndarray:
    """Flat float32 [197378] in state-dict order, nn.Linear's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (a copy)."""
    return _initial(int(seed)).copy()


def unpack(flat):
    return flat[:NW1].reshape(H, K), flat[O_B1:O_W2], flat[O_W2:O_B2].reshape(2, H), flat[O_B2:]


@functools.lru_cache(maxsize=None)
def _draws(N, seed, gain):
    g = np.random.default_rng([seed, N])
    x = g.standard_normal((N, K))
    # the label follows a direction of the features: there is something to learn
    y = (x @ g.standard_normal(K) + 0.5 * g.standard_normal(N) > 0).astype(np.int32)
    return (gain * x).astype(np.float32), y


def draws(N: int, seed: int = 0, gain: float = 1.0):
    """(feat float32 [N, 768] of N(0, gain^2) rows, labels int32 [N]) (copies)."""
    a, b = _draws(int(N), int(seed), float(gain))
    return a.copy(), b.copy()


unpack_keep = functools.partial(_unpack_keep, width=H)  # uint64 [N, 4] -> bool [N, 256]; pack_keep is its inverse


def lr_schedule(total_steps: int, lr: float, warmup_ratio: float = 0.1) -> np.ndarray:
    """get_cosine_schedule_with_warmup's learning rate of every step (train_ai_head.py:439-446), restated;
    tests/test_head_train_refs_cpu.py holds it against the real scheduler."""
    warm = int(total_steps * warmup_ratio)
    out = []
    for s in range(total_steps):
        if s < warm:
            f = s / max(1, warm)
        else:
            f = max(0.0, 0.5 * (1.0 + np.cos(np.pi * 0.5 * 2.0 * (s - warm) / max(1, total_steps - warm))))
        out.append(lr * f)
    return np.array(out, np.float64)


def forward(x, mult, W1, b1, W2, b2, y, dtype):
    """One batch forward; mult [B, 256] = keep * scale (ones: no dropout) -> dict(loss, lg [B, 2], ...)."""
    dt = dtype
    x, mult = x.astype(dt), mult.astype(dt)
    B = x.shape[0]
    pre = x @ W1.T + b1
    live = (pre > 0) * (mult != 0)
    h = np.where(pre > 0, pre, dt(0)) * mult
    lg = h @ W2.T + b2
    m = lg.max(1)
    e = np.exp(lg - m[:, None])
    se = e.sum(1, dtype=dt)
    li = (m + np.log(se)) - lg[np.arange(B), y]
    loss = li.sum(dtype=dt) / dt(B)
    correct = int(((lg[:, 1] > lg[:, 0]).astype(np.int64) == y).sum())
    return dict(loss=loss, lg=lg, pre=pre, h=h, live=live, mult=mult, x=x, y=y, m=m, e=e, se=se, li=li, correct=correct)


def forward_backward(x, mult, W1, b1, W2, b2, y, dtype):
    """forward()'s dict plus p, dl, dh, dp and grads (gW1, gb1, gW2, gb2)."""
    dt = dtype
    r = forward(x, mult, W1, b1, W2, b2, y, dt)
    B = x.shape[0]
    p = r["e"] / r["se"][:, None]
    onehot = np.eye(2, dtype=dt)[y]
    dl = (p - onehot) / dt(B)
    dh = dl @ W2
    dp = np.where(r["live"], dh * r["mult"], dt(0))
    r.update(p=p, onehot=onehot, dl=dl, dh=dh, dp=dp,
             grads=(dp.T @ r["x"], dp.sum(0, dtype=dt), dl.T @ r["h"], dl.sum(0, dtype=dt)))
    return r


def adamw(p, m, v, g, lr, step, dtype, betas=BETAS, eps=EPS, wd=WD):
    """torch.optim.AdamW's single-tensor update on flat arrays, in place."""
    adam(p, m, v, g, lr, step, dtype, wd, "decoupled", betas, eps)


def _mult(keep, pos, dtype):
    if keep is None:
        return np.ones((len(pos), H), dtype)
    return unpack_keep(keep[pos]).astype(dtype) * dtype(SCALE)


def epoch(feat, labels, perm, keep, batch, lr_steps, step0, params, exp_avg, exp_avg_sq, dtype=np.float64, wd=WD,
          max_norm=MAX_NORM, drift=None):
    """One epoch on flat params / exp_avg / exp_avg_sq (arrays of `dtype`, updated in place); keep uint64 [N, 4] or
    None.  -> (step_loss, step_correct, step_gnorm [nsteps], clipped grad of the last minibatch flat).  drift: a
    Drift carried from step 0 on (float64 runs), which accumulates the module docstring's conditioning number."""
    N = len(perm)
    dt = dtype
    losses, correct, norms, g = [], [], [], None
    for s in range(-(-N // batch)):
        pos = np.arange(s * batch, min(N, (s + 1) * batch))
        src = np.clip(perm[pos].astype(np.int64), 0, N - 1)
        W1, b1, W2, b2 = unpack(params)
        r = forward_backward(feat[src], _mult(keep, pos, dt), W1, b1, W2, b2, labels[src] & 1, dt)
        g = flat(r["grads"])
        norm = np.sqrt((g * g).sum(dtype=dt))
        coef = clip_coef(norm, max_norm, dt)
        g = g * coef
        if drift is not None:
            drift.gradient(g, float(coef) * U * _magnitudes(r, W2))
        adamw(params, exp_avg, exp_avg_sq, g, float(lr_steps[s]), step0 + s + 1, dt, wd=wd)
        if drift is not None:
            drift.update(exp_avg, exp_avg_sq, float(lr_steps[s]), step0 + s + 1)
        losses.append(float(r["loss"]))
        correct.append(r["correct"])
        norms.append(float(norm))
    return np.array(losses), np.array(correct), np.array(norms), g


def _magnitudes(r, W2):
    """Per parameter, the magnitude of which ANY fp32 evaluation of the gradient carries at least half an ulp
    (module docstring): every term of its sum once for the term's own rounding and once for each operand that is
    itself a rounded fp32 value (dpre, dlogits, h; the features are exact)."""
    a = np.abs
    adp, adl = a(r["dp"]), a(r["dl"])
    return np.concatenate([2 * (adp.T @ a(r["x"])).reshape(-1), 2 * adp.sum(0), 3 * (adl.T @ a(r["h"])).reshape(-1),
                           2 * adl.sum(0)])


def evaluate(feat, labels, batch, params, dtype=np.float64):
    """validate's forward: no dropout, consecutive batches in row order -> (batch_loss [nb], row_logits [N, 2])."""
    N = feat.shape[0]
    W1, b1, W2, b2 = unpack(params.astype(dtype))
    losses, lg = [], []
    for a in range(0, N, batch):
        r = forward(feat[a:a + batch], np.ones((len(feat[a:a + batch]), H), dtype), W1, b1, W2, b2,
                    labels[a:a + batch] & 1, dtype)
        losses.append(float(r["loss"]))
        lg.append(r["lg"])
    return np.array(losses), np.concatenate(lg)


def forward_bounds(r, W2):
    """Per-element bounds of the fp32 forward beside its float64 run r: -> (e_pre [B, 256], e_h, e_lg [B, 2],
    loss_tol), all with the factor 2."""
    a = np.abs
    B = r["x"].shape[0]
    W1 = r["W1"]
    e_pre = chain_err(r["x"], W1) + U * a(r["pre"])            # the chain, then the bias add
    e_h = e_pre * r["mult"] + U * a(r["h"])  # ReLU is 1-Lipschitz: whichever side of 0 an evaluation lands on
    e_lg = e_h @ a(W2).T + chain_err(r["h"], W2) + U * a(r["lg"])
    # a row's loss has slope p - onehot in its logits; expf, logf, the adds: 8 U of the terms
    p = r["e"] / r["se"][:, None]
    slope = a(p - np.eye(2)[r["y"]])
    e_li = (slope * e_lg).sum(1) + 8 * U * (1.0 + a(r["m"]) + a(np.log(r["se"])) + a(r["lg"]).max(1))
    loss_tol = 2 * (e_li.mean() + U * (B + 2) * a(r["li"]).mean())
    return 2 * e_pre, e_h, e_lg, float(loss_tol)


def deployed_head_bounds(x, params64):
    """The inference heads' kernel (csrc/misc.hip text_heads_kernel) beside the float64 head on rows x [B, 768]:
    pre = four ascending-k fmaf chains over K-slices of 192 added in slice order, then the bias; the logits 256
    products reduced inside each wave (depth 6), 3 adds across the waves, then the bias: at most 11 roundings on
    any path, 13 U of the terms taken.  -> (logits float64 [B, 2], their per-element bound with the factor 2)."""
    a = np.abs
    W1, b1, W2, b2 = unpack(params64)
    x = x.astype(np.float64)
    parts = [x[:, k:k + 192] @ W1[:, k:k + 192].T for k in range(0, K, 192)]
    e_pre = sum(chain_err(x[:, k:k + 192], W1[:, k:k + 192]) for k in range(0, K, 192))
    e_pre = e_pre + U * sum(a(s) for s in np.cumsum(parts, axis=0)[1:])
    pre = sum(parts) + b1
    e_pre = e_pre + U * a(pre)
    h = np.maximum(pre, 0.0)
    lg = h @ W2.T + b2
    e_lg = e_pre @ a(W2).T + 13 * U * (h @ a(W2).T) + U * a(lg)
    return lg, 2 * e_lg


def step_bounds(x, mult, params64, y, max_norm=MAX_NORM, check_branches=True):
    """The float64 forward / backward of one minibatch and the fp32 kernel's bounds:
    -> dict(r, grad flat (clipped), grad_tol flat, loss, loss_tol, norm, norm_tol, coef, lg, lg_tol [B, 2],
    relu_ok: every |pre| above its own forward bound, clamp_ok: the norm away from max_norm)."""
    W1, b1, W2, b2 = unpack(params64)
    r = forward_backward(x, mult, W1, b1, W2, b2, y, np.float64)
    r["W1"] = W1
    B = x.shape[0]
    a = np.abs
    e_pre2, e_h, e_lg, loss_tol = forward_bounds(r, W2)
    relu_ok = bool((a(r["pre"]) > e_pre2).all())
    p = r["p"]
    # softmax of two logits: d p_o = p_o (d l_o - sum_q p_q d l_q); exp of a rounded difference, a sum, a division
    rel = U * (10 + a(r["lg"] - r["m"][:, None]))
    e_p = p * (e_lg + (p * e_lg).sum(1, keepdims=True)) + rel * p
    e_dl = (e_p + 3 * U * a(p - r["onehot"])) / B
    adl = a(r["dl"])
    e_dh = e_dl @ a(W2) + 2 * U * (adl @ a(W2))
    e_dp = np.where(r["live"], e_dh * r["mult"], 0.0) + U * a(r["dp"])
    adp, ax, ah = a(r["dp"]), a(r["x"]), a(r["h"])
    e_g = np.concatenate([(e_dp.T @ ax + U * (B + 1) * (adp.T @ ax)).reshape(-1),
                          e_dp.sum(0) + U * B * adp.sum(0),
                          (e_dl.T @ ah + adl.T @ e_h + U * (B + 1) * (adl.T @ ah)).reshape(-1),
                          e_dl.sum(0) + U * B * adl.sum(0)])
    g = flat(r["grads"])
    norm = float(np.sqrt((g * g).sum()))
    # the sum of squares: 4 fmaf + an 8-level tree per block, an 8-level tree + 3 adds across blocks: 32 U of the sum
    e_norm = (float((a(g) * e_g).sum()) / norm + 32 * U * norm) if norm > 0 else float(np.sqrt((e_g * e_g).sum()))
    clamp_ok = norm > 1.5 * max_norm or norm < 0.67 * max_norm
    if check_branches:
        assert clamp_ok, f"the reference's norm {norm} makes the clamp borderline"
        assert relu_ok, "a pre-activation of the reference lies within its own forward bound of 0"
    coef = float(clip_coef(norm, max_norm, np.float64))
    gc = g * coef
    e_gc = e_g if coef == 1.0 else coef * e_g + a(gc) * (e_norm / (norm + 1e-6)) + 3 * U * a(gc)
    return dict(r=r, grad=gc, grad_tol=2 * e_gc, loss=float(r["loss"]), loss_tol=loss_tol, norm=norm,
                norm_tol=2 * e_norm, coef=coef, lg=r["lg"], lg_tol=2 * e_lg, relu_ok=relu_ok, clamp_ok=clamp_ok)


@functools.lru_cache(maxsize=None)
def _single_case(B, regime, dropout):
    gain, max_norm = REGIMES[regime]
    for seed in range(SINGLE_SEED, SINGLE_SEED + 64):
        feat, labels = draws(B, seed, gain)
        p0 = initial_params(seed)
        g = np.random.default_rng([seed, B, 7])
        perm = g.permutation(B).astype(np.int32)
        keep = pack_keep(g.random((B, H)) >= P_DROP) if dropout else None
        b = step_bounds(feat[perm], _mult(keep, np.arange(B), np.float64), p0.astype(np.float64), labels[perm],
                        max_norm, check_branches=False)
        clipped = b["norm"] > 1.5 * max_norm if regime == "clip" else b["norm"] < 0.67 * max_norm
        if b["relu_ok"] and clipped:
            return feat, labels, perm, keep, p0, max_norm, b, seed
    raise AssertionError(f"no qualifying seed for B={B} {regime} dropout={dropout}")


def single_case(B, regime, dropout):
    """(feat, labels, perm, keep or None, params float32, max_norm, step_bounds' dict, seed) of a single-step case:
    the first seed from SINGLE_SEED whose float64 run decides both branches (module docstring).  Shared: treat as
    read-only."""
    return _single_case(int(B), regime, bool(dropout))


@functools.lru_cache(maxsize=None)
def _run_case(N, batch, epochs, dtype, seed, lr):
    feat, labels = draws(N, seed)
    p0 = initial_params(seed)
    p = p0.astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    g = np.random.default_rng([seed, N, batch, epochs])
    spe = -(-N // batch)
    lrs = lr_schedule(spe * epochs, lr)
    plan, losses, norms, step0 = [], [], [], 0
    drift = Drift() if dtype == np.float64 else None
    for e in range(epochs):
        perm = g.permutation(N).astype(np.int32)
        keep = pack_keep(g.random((N, H)) >= P_DROP)
        plan.append((perm, keep, lrs[e * spe:(e + 1) * spe]))
        ls, _, ns, _ = epoch(feat, labels, perm, keep, batch, plan[-1][2], step0, p, m, v, dtype, drift=drift)
        step0 += len(ls)
        losses.append(ls)
        norms.append(ns)
    return p, m, v, losses, norms, plan, (drift.cond if drift else None), p0


def run_case(N, batch, epochs, dtype, seed=MULTI_SEED, lr=MULTI_LR):
    """A multi-step case from the initial parameters and zero moments, epoch by epoch with step0 carried over; per
    epoch a fresh permutation and dropout mask, per step the warmup-cosine learning rate.
    -> (params, exp_avg, exp_avg_sq, losses, norms, plan [(perm, keep, lr_steps)], cond, initial params).  Shared
    among the tests: treat as read-only."""
    return _run_case(int(N), int(batch), int(epochs), dtype, int(seed), float(lr))
