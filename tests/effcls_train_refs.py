"""Restatements of the EfficientNet deepfake-classifier training (csrc/effnet_train.hip, mmf_effcls_train_epoch and
mmf_effcls_eval) in numpy, shared by tests/test_effcls_train_refs_cpu.py (no GPU) and tests/test_gpu_effcls_train.py.

``epoch(..., dtype=np.float64)`` is the reference: the kernel's contract (a bank of R rows; minibatch s = positions
s*batch .. of perm, the last one short; entries clamped into [0, R); labels read as label & 1; xd = x keep scale with
scale = the float32 value of 1 / (1 - p_drop), keep[i] the mask of the row at POSITION i; logits = xd W^T + b; the
mean cross-entropy; the analytic backward to both tensors; torch.optim.Adam's single-tensor update -- weight_decay *
p added to the gradient, bias correction by step0 + s + 1, constant lr) in float64.  ``dtype=np.float32`` is the same
statement in float32 -- the step-dependent Adam scalars computed in double and rounded once, as the kernel does -- in
numpy's summation order, not the kernel's: its distance to the float64 run is the scale the multi-step test measures
the kernel against.

``step_bounds`` derives, beside the float64 forward and backward of ONE minibatch and never from what a kernel
returned, per-element bounds for the fp32 gradient, loss, logits, both moments and the parameters after the step:
absolute values propagated through forward and backward, first-order worst case times 2, U = 2^-24.  A logit is a sum
of 1280 products through a tree whose depth the kernel's header fixes (a 5-term fmaf chain, a 6-level butterfly, 3
adds across the waves, the bias: 15 roundings on any path), so its error is at most DEPTH U x the sum of |terms|, plus
U |term| for every xd that was rounded (x * scale).  The first Adam step is sign-like, p -= lr g / (|g| + eps): the
parameter bound is the exact variation of that function over the gradient's own interval, plus the roundings of the
update (8 of at most U relative on a quantity of at most lr) and of the subtraction.

The multi-step floor.  An Adam step rounds a parameter once (p - update), by at most half an ulp.  With nn.Linear's
default initialisation the classifier's parameters start below 1 / 32 and stay below 1 / 16 (half-ulp 2^-29), so two
correct fp32 evaluations may part by FLOOR = 2 x 2^-29 per step.

Conditioning of a multi-step case: train_refs_common.Drift (float64 run only), fed with this model's gradient
magnitudes (``_magnitudes``): the bound is K <= 8 x max(e32, FLOOR x steps, cond), and what keeps it from hiding a
failure is asserted on the reference alone (tests/test_effcls_train_refs_cpu.py): it stays below 0.1 x
max |p64_final - p_initial|, so a kernel that trains differently (a missing dropout scale, AdamW's decoupled decay in
place of Adam's L2) lands outside it.
"""
import functools

import numpy as np

from tests import train_refs_common as C
from tests.train_refs_common import Drift, U, flat, pack_keep  # noqa: F401

K = 1280
WORDS = K // 64
N_PARAMS = 2 * K + 2  # MMF_EFFCLS_PARAMS
BETAS, EPS, P_DROP = (0.9, 0.999), 1e-8, 0.2
SCALE = float(np.float32(1.0 / (1.0 - P_DROP)))  # the contract's dropout scale
FLOOR = 2 * 2.0 ** -29                            # per step: module docstring
DEPTH = 15                                        # roundings on any path of a logit's tree: module docstring

# (N, batch, epochs) of the multi-step test, at the script's own learning rate
MULTI_CASES = ((37, 16, 2), (17, 16, 2), (10, 1, 1), (130, 64, 2))
MULTI_LR = 1e-4
MULTI_SEED = 3  # chosen on the CPU among seeds 1 .. 8: test_effcls_train_refs_cpu.py::test_multi_step_cases_qualify
SINGLE_BATCHES = (1, 2, 5, 16, 64)
SINGLE_SEED = 21
SINGLE_LR = 1e-4
SINGLE_WDS = (0.0, 1e-2)


@functools.lru_cache(maxsize=None)
def _initial(seed):
    g = np.random.default_rng([seed, 1280])
    b = 1.0 / np.sqrt(K)
    return g.uniform(-b, b, N_PARAMS).astype(np.float32)


def initial_params(seed: int = 0) -> np.ndarray:
    """Flat float32 [2562] in state-dict order, nn.Linear's default U(-1/sqrt(1280), 1/sqrt(1280)) (a copy)."""
    return _initial(int(seed)).copy()


def unpack(flat):
    return flat[:2 * K].reshape(2, K), flat[2 * K:]


@functools.lru_cache(maxsize=None)
def _draws(N, seed):
    g = np.random.default_rng([seed, N, 5])
    # pooled SiLU outputs: mostly small and positive; the label follows a direction of the features
    x = 0.4 * np.abs(g.standard_normal((N, K))) + 0.1 * g.standard_normal((N, K))
    y = ((x - x.mean(0)) @ g.standard_normal(K) + 0.5 * g.standard_normal(N) > 0).astype(np.int32)
    return x.astype(np.float32), y


def draws(N: int, seed: int = 0):
    """(feat float32 [N, 1280], labels int32 [N]) (copies)."""
    a, b = _draws(int(N), int(seed))
    return a.copy(), b.copy()


unpack_keep = functools.partial(C.unpack_keep, width=K)  # uint64 [N, 20] -> bool [N, 1280]; pack_keep is its inverse


def _mult(keep, pos, dtype):
    if keep is None:
        return np.ones((len(pos), K), dtype)
    return unpack_keep(keep[pos]).astype(dtype) * dtype(SCALE)


def forward(x, mult, W, b, y, dtype):
    """One batch forward; mult [B, 1280] = keep * scale (ones: no dropout) -> dict(loss, lg [B, 2], ...)."""
    dt = dtype
    B = x.shape[0]
    xd = x.astype(dt) * mult.astype(dt)
    lg = xd @ W.T + b
    m = lg.max(1)
    e = np.exp(lg - m[:, None])
    se = e.sum(1, dtype=dt)
    li = (m + np.log(se)) - lg[np.arange(B), y]
    loss = li.sum(dtype=dt) / dt(B)
    correct = int(((lg[:, 1] > lg[:, 0]).astype(np.int64) == y).sum())
    return dict(loss=loss, lg=lg, xd=xd, y=y, m=m, e=e, se=se, li=li, correct=correct)


def forward_backward(x, mult, W, b, y, dtype):
    """forward()'s dict plus p, onehot, dl and grads (gW [2, 1280], gb [2])."""
    dt = dtype
    r = forward(x, mult, W, b, y, dt)
    B = x.shape[0]
    p = r["e"] / r["se"][:, None]
    onehot = np.eye(2, dtype=dt)[y]
    dl = (p - onehot) / dt(B)
    r.update(p=p, onehot=onehot, dl=dl, grads=(dl.T @ r["xd"], dl.sum(0, dtype=dt)))
    return r


def adam(p, m, v, g, lr, step, dtype, wd=0.0, betas=BETAS, eps=EPS, decoupled=False):
    """torch.optim.Adam's single-tensor update on flat arrays, in place.  decoupled: AdamW's p *= 1 - lr wd instead
    of g += wd p (the broken restatement of the CPU test)."""
    C.adam(p, m, v, g, lr, step, dtype, wd, "decoupled" if decoupled else "l2", betas, eps)


def _magnitudes(r, dropout):
    """Per parameter, the magnitude of which ANY fp32 evaluation of the gradient carries at least half an ulp: every
    term of its sum once for the term's own rounding and once for each operand that is itself a rounded fp32 value
    (dlogits always; xd where the dropout scale was applied)."""
    adl = np.abs(r["dl"])
    return np.concatenate([(3 if dropout else 2) * (adl.T @ np.abs(r["xd"])).reshape(-1), 2 * adl.sum(0)])


def epoch(feat, labels, perm, keep, batch, lr, step0, params, exp_avg, exp_avg_sq, dtype=np.float64, wd=0.0,
          drift=None, scale=None, decoupled=False):
    """One epoch on flat params / exp_avg / exp_avg_sq (arrays of `dtype`, updated in place) over the bank feat
    [R, 1280] / labels [R]; perm [N] bank rows; keep uint64 [N, 20] or None.  -> (step_loss, step_correct [nsteps],
    loss gradient of the last minibatch flat).  scale: another dropout scale (the broken restatement)."""
    N, R = len(perm), len(labels)
    dt = dtype
    losses, correct, g = [], [], None
    for s in range(-(-N // batch)):
        pos = np.arange(s * batch, min(N, (s + 1) * batch))
        src = np.clip(perm[pos].astype(np.int64), 0, R - 1)
        W, b = unpack(params)
        mult = _mult(keep, pos, dt)
        if scale is not None and keep is not None:
            mult = mult / dt(SCALE) * dt(scale)
        r = forward_backward(feat[src], mult, W, b, labels[src] & 1, dt)
        g = flat(r["grads"])
        if drift is not None:
            drift.gradient(g, U * _magnitudes(r, keep is not None))
        adam(params, exp_avg, exp_avg_sq, g, lr, step0 + s + 1, dt, wd=wd, decoupled=decoupled)
        if drift is not None:
            drift.update(exp_avg, exp_avg_sq, lr, step0 + s + 1)
        losses.append(float(r["loss"]))
        correct.append(r["correct"])
    return np.array(losses), np.array(correct), g


def evaluate(feat, labels, batch, params, dtype=np.float64):
    """validate's forward: no dropout, consecutive batches in row order -> (batch_loss [nb], row_logits [N, 2])."""
    N = feat.shape[0]
    W, b = unpack(params.astype(dtype))
    losses, lg = [], []
    for a in range(0, N, batch):
        x = feat[a:a + batch]
        r = forward(x, np.ones((len(x), K), dtype), W, b, labels[a:a + batch] & 1, dtype)
        losses.append(float(r["loss"]))
        lg.append(r["lg"])
    return np.array(losses), np.concatenate(lg)


def forward_bounds(r, W, dropout):
    """Per-element bounds of the fp32 forward beside its float64 run r -> (e_xd [B, 1280], e_lg [B, 2], loss_tol);
    e_lg and loss_tol with the factor 2, e_xd without (it is propagated)."""
    a = np.abs
    B = r["xd"].shape[0]
    e_xd = U * a(r["xd"]) if dropout else np.zeros_like(r["xd"])
    e_lg = e_xd @ a(W).T + DEPTH * U * (a(r["xd"]) @ a(W).T) + U * a(r["lg"])
    # a row's loss has slope p - onehot in its logits; expf, logf, the adds: 8 U of the terms
    p = r["e"] / r["se"][:, None]
    slope = a(p - np.eye(2)[r["y"]])
    e_li = (slope * e_lg).sum(1) + 8 * U * (1.0 + a(r["m"]) + a(np.log(r["se"])) + a(r["lg"]).max(1))
    loss_tol = 2 * (e_li.mean() + U * (B + 2) * a(r["li"]).mean())
    return e_xd, 2 * e_lg, float(loss_tol)


def _first_update(g):
    """Adam's first step per unit lr: m_hat / (sqrt(v_hat) + eps) = g / (|g| + eps)."""
    return g / (np.abs(g) + EPS)


def step_bounds(x, mult, params64, y, dropout, lr=SINGLE_LR, wd=0.0):
    """The float64 forward / backward / first Adam step of one minibatch (zero moments, step 1) and the fp32 kernel's
    bounds: -> dict(r, grad, grad_tol flat, loss, loss_tol, lg, lg_tol [B, 2], margin_ok, m, m_tol, v, v_tol, p, p_tol)."""
    a = np.abs
    W, b = unpack(params64)
    r = forward_backward(x, mult, W, b, y, np.float64)
    B = x.shape[0]
    e_xd, lg_tol, loss_tol = forward_bounds(r, W, dropout)
    e_lg = lg_tol / 2
    p = r["p"]
    # softmax of two logits: d p_o = p_o (d l_o - sum_q p_q d l_q); exp of a rounded difference, a sum, a division
    rel = U * (10 + a(r["lg"] - r["m"][:, None]))
    e_p = p * (e_lg + (p * e_lg).sum(1, keepdims=True)) + rel * p
    e_dl = (e_p + 3 * U * a(p - r["onehot"])) / B
    adl, axd = a(r["dl"]), a(r["xd"])
    e_g = np.concatenate([(e_dl.T @ axd + adl.T @ e_xd + U * (B + 1) * (adl.T @ axd)).reshape(-1),
                          e_dl.sum(0) + U * B * adl.sum(0)])
    g = flat(r["grads"])
    grad_tol = 2 * e_g
    # the argmax is decided by the reference alone where the margin exceeds both logits' bounds
    margin_ok = bool((a(r["lg"][:, 1] - r["lg"][:, 0]) > lg_tol.sum(1)).all())
    # the step: gd = g + wd p (an fmaf: U of the result), m = (1 - b1) gd, v = (1 - b2) gd^2 (4 U of the value each)
    gd = g + wd * params64
    gd_tol = grad_tol + (2 * U * a(gd) if wd else 0.0)
    m64, v64 = (1 - BETAS[0]) * gd, (1 - BETAS[1]) * gd * gd
    m_tol = (1 - BETAS[0]) * gd_tol + 4 * U * a(m64)
    v_tol = (1 - BETAS[1]) * (2 * a(gd) * gd_tol + gd_tol * gd_tol) + 4 * U * v64
    p64 = params64 - lr * _first_update(gd)
    f0 = _first_update(gd)
    vary = np.maximum(a(_first_update(gd + gd_tol) - f0), a(_first_update(gd - gd_tol) - f0))  # monotone in g
    p_tol = lr * vary + 2 * (8 * U * lr + U * a(p64))
    return dict(r=r, grad=g, grad_tol=grad_tol, loss=float(r["loss"]), loss_tol=loss_tol, lg=r["lg"], lg_tol=lg_tol,
                margin_ok=margin_ok, m=m64, m_tol=m_tol, v=v64, v_tol=v_tol, p=p64, p_tol=p_tol)


def deployed_logit_bounds(pooled, W, b):
    """The inference classifier (gap_classifier_kernel / gap32_kernel) beside the float64 Linear on the pooled rows it
    formed itself (mmf_effnet_pooled returns the same s * inv bit for bit): per thread an fmaf chain of at most 8
    channels, a 6-level butterfly, 3 adds across the waves and the bias: at most 18 roundings on any path of the
    1280-term sum.  -> (logits float64 [B, 2], their per-element bound with the factor 2)."""
    x = np.asarray(pooled, np.float64)
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    lg = x @ W.T + b
    return lg, 2 * (18 * U * (np.abs(x) @ np.abs(W).T) + U * np.abs(lg))


@functools.lru_cache(maxsize=None)
def _single_case(B, dropout, wd):
    R = 2 * B + 3
    for seed in range(SINGLE_SEED, SINGLE_SEED + 64):
        feat, labels = draws(R, seed)
        p0 = initial_params(seed)
        g = np.random.default_rng([seed, B, 7])
        perm = g.permutation(R)[:B].astype(np.int32)
        perm[0] = R - 1  # the upper half of the bank
        keep = pack_keep(g.random((B, K)) >= P_DROP) if dropout else None
        b = step_bounds(feat[perm], _mult(keep, np.arange(B), np.float64), p0.astype(np.float64), labels[perm], dropout,
                        wd=wd)
        if b["margin_ok"]:
            return feat, labels, perm, keep, p0, b, seed
    raise AssertionError(f"no qualifying seed for B={B} dropout={dropout}")


def single_case(B, dropout, wd=0.0):
    """(feat [2B + 3, 1280], labels, perm [B], keep or None, params float32, step_bounds' dict, seed) of a single-step
    case: the first seed from SINGLE_SEED whose float64 run decides every argmax.  Shared: treat as read-only."""
    return _single_case(int(B), bool(dropout), float(wd))


@functools.lru_cache(maxsize=None)
def _run_case(N, batch, epochs, dtype, seed, lr, broken):
    feat, labels = draws(N, seed)
    p0 = initial_params(seed)
    p = p0.astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    g = np.random.default_rng([seed, N, batch, epochs])
    plan, losses, step0 = [], [], 0
    drift = Drift() if dtype == np.float64 and broken in ("", "l2") else None
    kw = {"": {}, "scale": dict(scale=1.0), "adamw": dict(wd=1e-2, decoupled=True), "l2": dict(wd=1e-2)}[broken]
    for e in range(epochs):
        perm = g.permutation(N).astype(np.int32)
        keep = pack_keep(g.random((N, K)) >= P_DROP)
        plan.append((perm, keep))
        ls, _, _ = epoch(feat, labels, perm, keep, batch, lr, step0, p, m, v, dtype, drift=drift, **kw)
        step0 += len(ls)
        losses.append(ls)
    return p, m, v, losses, plan, (drift.cond if drift else None), p0


def run_case(N, batch, epochs, dtype, seed=MULTI_SEED, lr=MULTI_LR, broken=""):
    """A multi-step case from the initial parameters and zero moments, epoch by epoch with step0 carried over; per
    epoch a fresh permutation and dropout mask, the constant learning rate.  broken: "scale" (no dropout scale),
    "adamw" (decoupled decay 1e-2) or "l2" (the correct Adam with weight_decay 1e-2, adamw's counterpart).
    -> (params, exp_avg, exp_avg_sq, losses, plan [(perm, keep)], cond, initial params).  Shared: read-only."""
    return _run_case(int(N), int(batch), int(epochs), dtype, int(seed), float(lr), broken)
