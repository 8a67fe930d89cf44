"""Restatements of one epoch of FusionJudge training (csrc/fusion_train.hip, mmf_fusion_train_epoch) in
numpy, shared by tests/test_fusion_train_refs_cpu.py (no GPU) and tests/test_gpu_fusion_train.py.

``epoch(..., dtype=np.float64)`` is the reference: the kernel's contract (minibatch s = positions
s*batch .. of perm, the last one short with its own mean; keep[i] = the mask of the row at position i,
kept units scaled by 1 / (1 - p_drop); torch.optim.AdamW's single-tensor update with bias correction by
step0 + s + 1) in float64.  ``dtype=np.float32`` is the same statement in float32 -- the step-dependent
Adam scalars computed in double and rounded once, as the kernel does -- in numpy's summation order, not the
kernel's: its distance to the float64 run is the scale the multi-step test measures the kernel against.

``step_bounds`` derives, beside the float64 forward and backward of ONE minibatch and never from what a kernel
returned, a per-element bound for the fp32 gradient, the loss and the logit margin: absolute values propagated
through forward and backward, first-order worst case times 2, U = 2^-24 (the style of tests/effnet32_refs.py).
A ReLU whose pre-activation lies within its own error bound may switch in fp32; where that can happen the
whole upstream gradient magnitude is added to the bound.

Conditioning of a multi-step case (``epoch``'s last result, float64 run only).  Adam divides a gradient by its
own running magnitude: a parameter moves by  sens = lr (1 - beta1) / bc1 / (sqrt(v_hat) + eps)  per unit of
gradient error, up to lr / eps = 1e6 when its gradients are below eps.  The gradient of a weight is
sum_r d[r] act[r], and act[r] = relu(a chain of magnitude S[r]) carries at least half an ulp of S[r] in ANY fp32
evaluation, however small act[r] itself is.  So  cond = max over steps and weights of sens U sum_r |d[r]| S[r]
(live activations only) is the first-order distance at which two correct fp32 evaluations can end; a unit that
is live in a single row with a pre-activation of 1e-6 drives it to 1e-4.  The multi-step test's bound has
the floor 8 x 1e-7 x steps; a case belongs in that test only if cond stays below that floor, like the margin
condition for step_correct.  The plan stream keyed [SEED, N, batch] gave cond 2.1e-4 for (520, 256, 2) -- one
W3 entry whose first gradient is -9e-10, where the kernel ended 7.4e-6 and numpy's float32 1e-6 from float64 --
so the stream is keyed [SEED, N, batch, epochs], for which every case satisfies the condition
(tests/test_fusion_train_refs_cpu.py asserts it).
"""
import functools

import numpy as np

from tests import train_refs_common as C
from tests.train_refs_common import U, flat, pack_keep  # noqa: F401

SHAPES = ((64, 5), (64,), (32, 64), (32,), (2, 32), (2,))  # fusion_layer.{0,3,5}.{weight,bias}
KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "5.weight", "5.bias")
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)
BETAS, EPS, WD, P_DROP = (0.9, 0.999), 1e-8, 0.01, 0.2

# (N, batch, epochs, lr) of the multi-step test; draws from seed 7
MULTI_CASES = ((37, 16, 3, 1e-2), (5, 1, 2, 1e-2), (40, 3, 2, 1e-3), (300, 64, 2, 1e-2), (520, 256, 2, 1e-2))
SEED = 7
# the single-step test: batches, and the seed of its draws (chosen so that the float64 reference alone keeps every
# |logit1 - logit0| above step_bounds' margin_tol: test_fusion_train_refs_cpu.py checks it)
SINGLE_BATCHES = (1, 3, 16, 64, 256)
SINGLE_SEED = 13


@functools.lru_cache(maxsize=None)
def _initial_params() -> np.ndarray:
    import mmf_amd.weights as W
    sd = W.synthetic_detector_state(0)
    return np.concatenate([np.asarray(sd[f"fusion_layer.{k}"], np.float32).reshape(-1) for k in KEYS])


def initial_params() -> np.ndarray:
    """W.synthetic_detector_state(0)'s fusion_layer.*, flat float32 [2530] in state-dict order (a copy)."""
    return _initial_params().copy()


def unpack(flat):
    out, o = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    return out


def draws(N: int, seed: int = SEED):
    """(scores float32 [N, 5] drawn as SURVEY 8d's C1 distribution, labels int32 [N]): the label follows a
    noisy linear rule of the scores, so there is something to learn."""
    import mmf_amd.synthetic as syn
    x = syn.fusion_inputs(N, seed)
    g = np.random.default_rng([seed, N])
    t = 1.5 * x[:, 1] + x[:, 2] + 1.2 * x[:, 4] - x[:, 3] + 0.35 * g.standard_normal(N)
    return x, (t > 1.3).astype(np.int32)


def masks(N: int, seed: int = SEED) -> np.ndarray:
    """bool [N, 64], P(keep) = 0.8."""
    return np.random.default_rng([seed, N, 64]).uniform(size=(N, 64)) >= P_DROP


unpack_keep = functools.partial(C.unpack_keep, width=64)  # uint64 [N] -> bool [N, 64]; pack_keep is its inverse


def forward_backward(x, y, keep_mask, p_drop, P, dtype):
    """One minibatch: x [rows, 5], y [rows], keep_mask bool [rows, 64] or None, P = unpack(params) in dtype.
    -> dict(loss, correct, grads (list like P), logits, z1, a1, z2, h2, dl, dz2, da1, dz1, dh2, scale)."""
    dt = dtype
    W0, b0, W3, b3, W5, b5 = P
    rows = x.shape[0]
    x = x.astype(dt)
    scale = dt(1.0) if keep_mask is None else dt(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))
    km = np.ones((rows, 64), bool) if keep_mask is None else keep_mask
    z1 = x @ W0.T + b0
    a1 = np.where(km, np.maximum(z1, 0) * scale, dt(0))
    z2 = a1 @ W3.T + b3
    h2 = np.maximum(z2, 0)
    lg = h2 @ W5.T + b5
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    den = e.sum(1, keepdims=True)
    onehot = np.eye(2, dtype=dt)[y]
    loss_rows = np.log(den[:, 0]) - ((lg * onehot).sum(1) - m[:, 0])
    loss = loss_rows.sum(dtype=dt) / dt(rows)
    correct = int(((lg[:, 1] > lg[:, 0]).astype(np.int64) == y).sum())  # a tie is class 0
    dl = (e / den - onehot) * (dt(1.0) / dt(rows))
    dh2 = dl @ W5
    dz2 = np.where(h2 > 0, dh2, dt(0))
    da1 = dz2 @ W3
    dz1 = np.where(a1 > 0, da1 * scale, dt(0))
    grads = [dz1.T @ x, dz1.sum(0, dtype=dt), dz2.T @ a1, dz2.sum(0, dtype=dt), dl.T @ h2, dl.sum(0, dtype=dt)]
    return dict(loss=loss, correct=correct, grads=grads, logits=lg, z1=z1, a1=a1, z2=z2, h2=h2, dl=dl, dz2=dz2,
                da1=da1, dz1=dz1, dh2=dh2, scale=scale, km=km, loss_rows=loss_rows)


def adamw(P, M, V, G, lr, step, dtype, betas=BETAS, eps=EPS, wd=WD):
    """torch.optim.AdamW's single-tensor update, in place; the scalars in double, rounded to dtype once."""
    for p, m, v, g in zip(P, M, V, G):
        C.adam(p, m, v, g, lr, step, dtype, wd, "decoupled", betas, eps)


def epoch(scores, labels, perm, keep, p_drop, batch, lr, step0, params, exp_avg, exp_avg_sq, dtype=np.float64,
          wd=WD):
    """One epoch on flat params / exp_avg / exp_avg_sq (arrays of `dtype`, updated in place).
    -> (step_loss [nsteps], step_correct [nsteps], grad of the last minibatch flat, smallest |logit1 - logit0|,
    cond: the module docstring's conditioning number, float64 runs only, else None)."""
    N = len(labels)
    P, M, V = unpack(params), unpack(exp_avg), unpack(exp_avg_sq)
    km_all = None if keep is None else unpack_keep(keep)
    losses, corrects, margin, g, cond = [], [], np.inf, None, (0.0 if dtype == np.float64 else None)
    for s in range(-(-N // batch)):
        pos = np.arange(s * batch, min(N, (s + 1) * batch))
        src = np.clip(perm[pos], 0, N - 1)
        r = forward_backward(scores[src], labels[src].astype(np.int64), None if km_all is None else km_all[pos],
                             p_drop, P, dtype)
        margin = min(margin, float(np.abs(r["logits"][:, 1] - r["logits"][:, 0]).min()))
        g = r["grads"]
        adamw(P, M, V, g, lr, step0 + s + 1, dtype, wd=wd)
        if cond is not None:
            cond = max(cond, _conditioning(r, scores[src], P, V, lr, step0 + s + 1))
        losses.append(float(r["loss"]))
        corrects.append(r["correct"])
    return np.array(losses), np.array(corrects), flat(g), margin, cond


def _conditioning(r, x, P, V, lr, step):
    """One step's part of cond (module docstring): r = the step's float64 forward / backward, V = exp_avg_sq
    after the step.  (The chains' magnitudes are taken with the updated weights: first order all the same.)"""
    aW0, ab0, aW3, ab3, _, _ = (np.abs(q) for q in P)
    S1 = (np.abs(x.astype(np.float64)) @ aW0.T + ab0) * float(r["scale"]) * (r["a1"] > 0)
    S2 = (np.abs(r["a1"]) @ aW3.T + ab3) * (r["h2"] > 0)
    bc1, bc2 = 1.0 - BETAS[0] ** step, 1.0 - BETAS[1] ** step
    worst = 0.0
    for d, S, v in ((r["dz2"], S1, V[2]), (r["dl"], S2, V[4])):
        sens = lr * ((1.0 - BETAS[0]) / bc1) / (np.sqrt(v / bc2) + EPS)
        worst = max(worst, float((sens * U * (np.abs(d).T @ S)).max()))
    return worst


def step_bounds(x, y, keep_mask, p_drop, params64):
    """The float64 forward / backward of one minibatch and the fp32 kernel's bounds:
    -> dict(r = forward_backward(...) in float64, grad flat, grad_tol flat, loss_tol, margin_tol [rows])."""
    P = unpack(params64)
    W0, b0, W3, b3, W5, b5 = (np.abs(p) for p in P)
    r = forward_backward(x, y, keep_mask, p_drop, P, np.float64)
    rows = x.shape[0]
    ax, sc, km = np.abs(x.astype(np.float64)), float(r["scale"]), r["km"]
    # forward: a K-term fmaf chain from the bias rounds K times, each at most U S, S = |b| + sum |w| |x|
    e_z1 = U * (5 + 2) * (ax @ W0.T + b0)
    a1 = np.abs(r["a1"])
    e_a1 = np.where(km, sc * e_z1 + U * a1, 0.0)
    e_z2 = e_a1 @ W3.T + U * (64 + 2) * (a1 @ W3.T + b3)
    h2 = np.abs(r["h2"])
    e_l = e_z2 @ W5.T + U * (32 + 2) * (h2 @ W5.T + b5)
    e_margin = e_l.sum(1)
    # softmax of two logits is sigmoid(l1 - l0), slope <= 1/4; expf x 2, add, divide, subtract: 8 U of p <= 1
    e_p = 0.25 * e_margin + 8 * U
    e_dl = np.repeat(((e_p + 2 * U) / rows)[:, None], 2, 1)
    adl = np.abs(r["dl"])
    # loss_row = log(sum exp(l - m)) - (l_y - m): slope <= 1 in each logit; expf, logf, adds: 8 U of the terms
    e_loss_row = e_margin + 8 * U * (1.0 + np.abs(r["logits"]).sum(1))
    loss_tol = 2 * (e_loss_row.mean() + U * (rows + 1) * np.abs(r["loss_rows"]).mean())
    # backward; flipN: a ReLU that fp32 may evaluate on the other side of zero
    adh2 = adl @ W5
    e_dh2 = e_dl @ W5 + 3 * U * adh2
    flip2 = np.abs(r["z2"]) <= e_z2
    adz2 = np.where(flip2, adh2, np.abs(r["dz2"]))
    e_dz2 = np.where(r["h2"] > 0, e_dh2, 0.0) + np.where(flip2, adh2 + e_dh2, 0.0)
    ada1 = adz2 @ W3
    e_da1 = e_dz2 @ W3 + (32 + 1) * U * ada1
    flip1 = km & (np.abs(r["z1"]) <= e_z1)
    adz1 = np.where(flip1, sc * ada1, np.abs(r["dz1"]))
    e_dz1 = np.where(r["a1"] > 0, sc * e_da1 + U * adz1, 0.0) + np.where(flip1, sc * (ada1 + e_da1), 0.0)

    def wgrad(d, e_d, act, e_act):  # sum_r d[r, o] act[r, i]: rows fmaf steps from zero
        return e_d.T @ act + d.T @ e_act + U * (rows + 1) * (d.T @ act)

    def bgrad(d, e_d):
        return e_d.sum(0) + U * (rows + 1) * d.sum(0)
    tol = [wgrad(adz1, e_dz1, ax, np.zeros_like(ax)), bgrad(adz1, e_dz1), wgrad(adz2, e_dz2, a1, e_a1),
           bgrad(adz2, e_dz2), wgrad(adl, e_dl, h2, e_z2), bgrad(adl, e_dl)]
    return dict(r=r, grad=flat(r["grads"]), grad_tol=2 * flat(tol), loss_tol=float(loss_tol),
                margin_tol=2 * e_margin)


def run_case(N, batch, epochs, lr, dtype, seed=SEED, split=None):
    """A multi-step case from the initial parameters and zero moments, epoch by epoch with step0 carried over;
    per epoch a fresh permutation and masks.
    -> (params, exp_avg, exp_avg_sq, losses, corrects, margin, plan, cond)."""
    x, y = draws(N, seed)
    p = initial_params().astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    g = np.random.default_rng([seed, N, batch, epochs])
    plan, losses, corrects, margin, step0, cond = [], [], [], np.inf, 0, 0.0
    for e in range(epochs):
        perm = g.permutation(N).astype(np.int32)
        keep = pack_keep(g.uniform(size=(N, 64)) >= P_DROP)
        plan.append((perm, keep))
        ls, cs, _, mg, cd = epoch(x, y, perm, keep, P_DROP, batch, lr, step0, p, m, v, dtype)
        cond = max(cond, cd or 0.0)
        step0 += len(ls)
        losses.append(ls)
        corrects.append(cs)
        margin = min(margin, mg)
    return p, m, v, losses, corrects, margin, plan, cond
