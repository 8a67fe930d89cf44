"""Restatements of CLIPDetective's projection-head training (csrc/clip_train.hip, mmf_clip_train_epoch and
mmf_clip_contrastive_eval) in numpy, shared by tests/test_clip_train_refs_cpu.py (no GPU) and
tests/test_gpu_clip_train.py.

``epoch(..., dtype=np.float64)`` is the reference: the kernel's contract (minibatch s = positions s*batch .. of
perm, the last one short; e = P W^T divided by its row norm, no epsilon; logits = exp(logit_scale) I T^T; the mean
of the two cross-entropies against the diagonal; the analytic backward; clip_grad_norm_'s coefficient
max_norm / (norm + 1e-6) clamped at 1 and always applied; torch.optim.AdamW's single-tensor update on all three
parameters with bias correction by step0 + s + 1) in float64.  ``dtype=np.float32`` is the same statement in
float32 -- the step-dependent Adam scalars computed in double and rounded once, as the kernel does -- in numpy's
summation order, not the kernel's: its distance to the float64 run is the scale the multi-step test measures the
kernel against.

``step_bounds`` derives, beside the float64 forward and backward of ONE minibatch and never from what a kernel
returned, a per-element bound for the fp32 clipped gradient, the loss and the total norm: absolute values
propagated through forward and backward, first-order worst case times 2, U = 2^-24 (the style of
tests/fusion_train_refs.py).  The clamp of the clip coefficient is a branch: ``step_bounds`` asserts on the
float64 norm alone that it is either above 1.5 x max_norm or below 0.67 x max_norm, so no fp32 evaluation can
take the other side.

The multi-step floor.  An AdamW step rounds a parameter twice (p * decay, then p - update), each time by at most
half an ulp.  The projections stay below 0.25 (half-ulp 2^-27); logit_scale ~ 2.66 lies in [2, 4), half-ulp 2^-23.
So two correct fp32 evaluations may part by FLOOR = 2 x 2^-23 = 2.4e-7 per step, and the multi-step bound is
8 x max(e32, FLOOR x steps): the project's rule (tests/test_gpu_fusion_train.py) with this floor.

Conditioning of a multi-step case (``epoch``'s last result, float64 run only).  Adam divides a gradient by its own
running magnitude: a parameter moves by  sens = lr (1 - beta1) / bc1 / (sqrt(v_hat) + eps)  per unit of gradient
error.  A weight gradient sum_r de[r][j] P[r][k] carries at least half an ulp of every product in ANY fp32
evaluation, and de = (dy - y (y . dy)) / n at least half an ulp of both terms of its difference, however small the
result.  cond = max over steps and parameters of  sens x coef x U x (that magnitude)  is the first-order
distance at which two correct fp32 evaluations can end.  A case belongs in the multi-step test only if cond stays
below the floor FLOOR x steps (tests/test_clip_train_refs_cpu.py asserts it).  At the reference's default
lr = 1e-4 no seed gives that: among 655,360 weights some gradient is always tiny against its own terms, and cond
came out at 2 to 5 times the floor for every seed tried (1, 2, 3, 4, 7; the float32 restatement parts from float64
by the same 2e-6 .. 6e-6 there).  cond is proportional to lr, so the cases run at lr = 1e-5, the lower end of the
range the reference's own tuning searches (train_clip_detective.py:281), where seed 7 keeps every case below it.
"""
import functools

import numpy as np

from tests.train_refs_common import U, adam, chain_err, clip_coef, flat  # noqa: F401

D, KV, KT = 512, 768, 512
NV, NT = D * KV, D * KT
N_PARAMS = NV + NT + 1
BETAS, EPS, WD, MAX_NORM = (0.9, 0.999), 1e-8, 0.01, 1.0
LOGIT_SCALE0 = float(np.log(1 / 0.07))  # CLIP's initial logit_scale
FLOOR = 2 * 2.0 ** -23                    # per step: module docstring

# (N, batch, epochs) of the multi-step test, their learning rate and the seed of their draws (module docstring)
MULTI_CASES = ((37, 16, 2), (17, 16, 2), (10, 1, 1), (130, 64, 2))
MULTI_LR = 1e-5
MULTI_SEED = 7
# the single-step test: batches x regimes ("clip": the float64 norm above 1.5, "noclip": below 0.67: single_case)
SINGLE_BATCHES = (1, 2, 5, 16, 64)
SINGLE_SEED = 13


@functools.lru_cache(maxsize=None)
def _initial(seed, logit_scale):
    g = np.random.default_rng([seed, 512])
    p = np.empty(N_PARAMS, np.float32)
    p[:NV] = (0.02 * g.standard_normal(NV)).astype(np.float32)
    p[NV:NV + NT] = (0.02 * g.standard_normal(NT)).astype(np.float32)
    p[-1] = np.float32(logit_scale)
    return p


def initial_params(seed: int = 0, logit_scale: float = LOGIT_SCALE0) -> np.ndarray:
    """Flat float32 [655361]: visual [512][768] | text [512][512] (N(0, 0.02), as CLIP initialises them) |
    logit_scale (a copy)."""
    return _initial(int(seed), float(logit_scale)).copy()


def unpack(flat):
    return flat[:NV].reshape(D, KV), flat[NV:NV + NT].reshape(D, KT), flat[NV + NT:]


@functools.lru_cache(maxsize=None)
def _draws(N, seed, gain):
    g = np.random.default_rng([seed, N])
    img = g.standard_normal((N, KV))
    # a caption's features share a direction with its image's: there is something to learn
    txt = 0.7 * g.standard_normal((N, KT)) + 0.7 * img[:, :KT]
    return (gain * img).astype(np.float32), (gain * txt).astype(np.float32)


def draws(N: int, seed: int = 0, gain: float = 1.0):
    """(img_feat float32 [N, 768], txt_feat float32 [N, 512]), N(0, gain^2)-like pooled rows (copies)."""
    a, b = _draws(int(N), int(seed), float(gain))
    return a.copy(), b.copy()


def forward(pi, pt, Wv, Wt, ls, dtype):
    """One batch forward: -> dict(loss, cos [B, B], row_cos [B], ...)."""
    dt = dtype
    pi, pt = pi.astype(dt), pt.astype(dt)
    B = pi.shape[0]
    ei, et = pi @ Wv.T, pt @ Wt.T
    ni, nt = np.sqrt((ei * ei).sum(1, dtype=dt)), np.sqrt((et * et).sum(1, dtype=dt))
    yi, yt = ei / ni[:, None], et / nt[:, None]
    scale = np.exp(dt(ls))
    cos = yi @ yt.T
    lg = scale * cos
    mr, mc = lg.max(1, keepdims=True), lg.max(0, keepdims=True)
    sr, sc = np.exp(lg - mr).sum(1, keepdims=True, dtype=dt), np.exp(lg - mc).sum(0, keepdims=True, dtype=dt)
    diag = np.diag(lg)
    li = ((mr[:, 0] + np.log(sr[:, 0])) - diag)
    lt = ((mc[0] + np.log(sc[0])) - diag)
    loss = (li.sum(dtype=dt) / dt(B) + lt.sum(dtype=dt) / dt(B)) * dt(0.5)
    return dict(loss=loss, cos=cos, row_cos=np.diag(cos).copy(), lg=lg, scale=scale, mr=mr, mc=mc, sr=sr, sc=sc,
                ei=ei, et=et, ni=ni, nt=nt, yi=yi, yt=yt, pi=pi, pt=pt, li=li, lt=lt)


def forward_backward(pi, pt, Wv, Wt, ls, dtype):
    """One minibatch: forward()'s dict plus dl, dls, dyi, dyt, si, st, dei, det and grads (gWv, gWt, gls)."""
    dt = dtype
    r = forward(pi, pt, Wv, Wt, ls, dt)
    B = pi.shape[0]
    lg = r["lg"]
    pr, pc = np.exp(lg - r["mr"]) / r["sr"], np.exp(lg - r["mc"]) / r["sc"]
    dl = ((pr + pc) - dt(2) * np.eye(B, dtype=dt)) * (dt(0.5) / dt(B))
    dls = (dl * lg).sum(dtype=dt)
    c = r["scale"] * dl
    dyi, dyt = c @ r["yt"], c.T @ r["yi"]
    si, st = (r["yi"] * dyi).sum(1, keepdims=True, dtype=dt), (r["yt"] * dyt).sum(1, keepdims=True, dtype=dt)
    dei = (dyi - r["yi"] * si) / r["ni"][:, None]
    det = (dyt - r["yt"] * st) / r["nt"][:, None]
    r.update(pr=pr, pc=pc, dl=dl, dls=dls, c=c, dyi=dyi, dyt=dyt, si=si, st=st, dei=dei, det=det,
             grads=(dei.T @ r["pi"], det.T @ r["pt"], np.array([dls], dt)))
    return r


def adamw(p, m, v, g, lr, step, dtype, betas=BETAS, eps=EPS, wd=WD):
    """torch.optim.AdamW's single-tensor update on flat arrays, in place."""
    adam(p, m, v, g, lr, step, dtype, wd, "decoupled", betas, eps)


def epoch(img, txt, perm, batch, lr, step0, params, exp_avg, exp_avg_sq, dtype=np.float64, wd=WD,
          max_norm=MAX_NORM):
    """One epoch on flat params / exp_avg / exp_avg_sq (arrays of `dtype`, updated in place).
    -> (step_loss [nsteps], step_gnorm [nsteps], clipped grad of the last minibatch flat,
    cond: the module docstring's conditioning number, float64 runs only, else None)."""
    N = len(perm)
    dt = dtype
    losses, norms, g, cond = [], [], None, (0.0 if dtype == np.float64 else None)
    for s in range(-(-N // batch)):
        pos = np.arange(s * batch, min(N, (s + 1) * batch))
        src = np.clip(perm[pos], 0, N - 1)
        Wv, Wt, ls = unpack(params)
        r = forward_backward(img[src], txt[src], Wv, Wt, ls[0], dt)
        g = flat(r["grads"])
        norm = np.sqrt((g * g).sum(dtype=dt))
        coef = clip_coef(norm, max_norm, dt)
        g = g * coef
        adamw(params, exp_avg, exp_avg_sq, g, lr, step0 + s + 1, dt, wd=wd)
        if cond is not None:
            cond = max(cond, _conditioning(r, float(coef), exp_avg_sq, lr, step0 + s + 1))
        losses.append(float(r["loss"]))
        norms.append(float(norm))
    return np.array(losses), np.array(norms), g, cond


def _conditioning(r, coef, V, lr, step):
    """One step's part of cond (module docstring): r = the step's float64 forward / backward, V = exp_avg_sq
    after the step."""
    bc1, bc2 = 1.0 - BETAS[0] ** step, 1.0 - BETAS[1] ** step
    sens = lr * ((1.0 - BETAS[0]) / bc1) / (np.sqrt(V / bc2) + EPS)
    mags = []
    for y, dy, s, n, de, p in ((r["yi"], r["dyi"], r["si"], r["ni"], r["dei"], r["pi"]),
                               (r["yt"], r["dyt"], r["st"], r["nt"], r["det"], r["pt"])):
        de_mag = (np.abs(dy) + np.abs(y * s)) / n[:, None]  # half an ulp of both terms of the difference
        mags.append(((de_mag + np.abs(de)).T @ np.abs(p)).reshape(-1))
    mags.append(np.array([(np.abs(r["dl"]) * np.abs(r["lg"])).sum()]))
    return float((sens * coef * U * np.concatenate(mags)).max())


def evaluate(img, txt, batch, params, dtype=np.float64):
    """validate's forward: consecutive batches in row order -> (batch_loss [nb], row_cos [N])."""
    N = img.shape[0]
    Wv, Wt, ls = unpack(params.astype(dtype))
    losses, cos = [], []
    for a in range(0, N, batch):
        r = forward(img[a:a + batch], txt[a:a + batch], Wv, Wt, ls[0], dtype)
        losses.append(float(r["loss"]))
        cos.append(r["row_cos"])
    return np.array(losses), np.concatenate(cos)


def lower_median_accuracy(cos, labels):
    """calculate_accuracy (train_clip_detective.py:169-187) of one batch: torch.median is the LOWER median;
    cos <= threshold predicts 1."""
    cos, labels = np.asarray(cos), np.asarray(labels)
    thr = np.sort(cos)[(len(cos) - 1) // 2]
    return float(((cos <= thr).astype(np.int64) == labels).mean())


def step_bounds(pi, pt, params64, max_norm=MAX_NORM):
    """The float64 forward / backward of one minibatch and the fp32 kernel's bounds:
    -> dict(r, grad flat (clipped), grad_tol flat, loss, loss_tol, norm, norm_tol, coef, cos_tol [B]: of the
    pairs' own cosines)."""
    Wv, Wt, ls = unpack(params64)
    r = forward_backward(pi, pt, Wv, Wt, ls[0], np.float64)
    B = pi.shape[0]
    a = np.abs
    scale = float(r["scale"])

    def tower(p, W, e, n, y):  # errors of e = P W^T (ascending chain), n = |e| (tree of 512 squares), y = e / n
        e_e = chain_err(p, W)
        S2 = n * n
        e_S2 = 2 * (a(e) * e_e).sum(1) + U * 12 * S2
        e_n = e_S2 / (2 * n) + U * n
        e_y = e_e / n[:, None] + a(y) * (e_n / n)[:, None] + U * a(y)
        return e_n, e_y
    e_ni, e_yi = tower(r["pi"], Wv, r["ei"], r["ni"], r["yi"])
    e_nt, e_yt = tower(r["pt"], Wt, r["et"], r["nt"], r["yt"])
    ayi, ayt = a(r["yi"]), a(r["yt"])
    e_cos = e_yi @ ayt.T + ayi @ e_yt.T + chain_err(r["yi"], r["yt"])
    e_scale = 4 * U * scale  # expf
    lg = r["lg"]
    e_lg = scale * e_cos + a(r["cos"]) * e_scale + U * a(lg)
    # softmax along an axis: d p_k = p_k (d l_k - sum_q p_q d l_q); exp of a rounded difference, a B-term sum, a division
    def softmax_err(p, m, axis):
        rel = U * (B + 8 + a(lg - m))
        return p * (e_lg + (p * e_lg).sum(axis, keepdims=True)) + rel * p
    e_pr, e_pc = softmax_err(r["pr"], r["mr"], 1), softmax_err(r["pc"], r["mc"], 0)
    h = 0.5 / B
    eye = np.eye(B)
    e_dl = h * (e_pr + e_pc) + 3 * U * h * (r["pr"] + r["pc"] + 2 * eye)
    adl = a(r["dl"])
    # loss: a row's lse has slope p in its logits, the diagonal slope 1; expf, logf, adds: 8 U of the terms
    e_li = (r["pr"] * e_lg).sum(1) + np.diag(e_lg) + 8 * U * (1.0 + a(r["mr"][:, 0]) + a(np.log(r["sr"][:, 0])) + a(np.diag(lg)))
    e_lt = (r["pc"] * e_lg).sum(0) + np.diag(e_lg) + 8 * U * (1.0 + a(r["mc"][0]) + a(np.log(r["sc"][0])) + a(np.diag(lg)))
    loss_tol = 2 * (0.5 * (e_li.mean() + e_lt.mean()) + U * (B + 3) * 0.5 * (a(r["li"]).mean() + a(r["lt"]).mean()))
    # d logit_scale = sum_ij dl lg: B-term chains, then a B-term chain
    e_dls = (e_dl * a(lg) + adl * e_lg).sum() + U * (2 * B + 2) * (adl * a(lg)).sum()
    c = a(r["c"])
    e_c = scale * e_dl + adl * e_scale + U * c

    def pull(cc, e_cc, yo, e_yo, y, e_y, dy, s, n, e_n, de, p):
        """dy = cc @ yo (B-term chains), s = y . dy (512-term chain), de = (dy - y s) / n, gW = de^T p"""
        e_dy = e_cc @ a(yo) + cc @ e_yo + U * (B + 1) * (cc @ a(yo))
        e_s = (e_y * a(dy) + a(y) * e_dy).sum(1, keepdims=True) + U * a(np.cumsum(y * dy, 1)).sum(1, keepdims=True)
        ys = a(y * s)
        num = e_dy + e_y * a(s) + a(y) * e_s + U * ys + U * (a(dy) + ys)
        e_de = num / n[:, None] + a(de) * (e_n / n)[:, None] + U * a(de)
        return e_de.T @ a(p) + U * (B + 1) * (a(de).T @ a(p))
    e_gv = pull(c, e_c, r["yt"], e_yt, r["yi"], e_yi, r["dyi"], r["si"], r["ni"], e_ni, r["dei"], r["pi"])
    e_gt = pull(c.T, e_c.T, r["yi"], e_yi, r["yt"], e_yt, r["dyt"], r["st"], r["nt"], e_nt, r["det"], r["pt"])
    g = flat(r["grads"])
    e_g = np.concatenate([e_gv.reshape(-1), e_gt.reshape(-1), [e_dls]])
    norm = float(np.sqrt((g * g).sum()))
    # the sum of squares: 4 fmaf + an 8-level tree per block, 3 + 8 + 1 across blocks: 32 U of the sum
    e_norm = (float((a(g) * e_g).sum()) / norm + 32 * U * norm) if norm > 0 else float(np.sqrt((e_g * e_g).sum()))
    if B > 1:
        assert norm > 1.5 * max_norm or norm < 0.67 * max_norm, f"the reference's norm {norm} makes the clamp borderline"
    coef = float(clip_coef(norm, max_norm, np.float64))
    gc = g * coef
    e_gc = e_g if coef == 1.0 else coef * e_g + a(gc) * (e_norm / (norm + 1e-6)) + 3 * U * a(gc)
    return dict(r=r, grad=gc, grad_tol=2 * e_gc, loss=float(r["loss"]), loss_tol=float(loss_tol), norm=norm,
                norm_tol=2 * e_norm, coef=coef, cos_tol=2 * np.diag(e_cos))


def single_case(B, regime, seed=SINGLE_SEED):
    """(img, txt, params float32) of a single-step case.  "clip": CLIP's initial logit_scale ln(1 / 0.07) on
    N(0, 1) rows (float64 norms 5.7 .. 24).  "noclip": logit_scale 0, which divides the logits' slope by 14.3,
    and weights x 8, which leaves the unit embeddings as they were and divides the weight gradients by 8
    (de ~ 1 / |e|): float64 norms 0.05 .. 0.18."""
    img, txt = draws(B, seed)
    if regime == "clip":
        return img, txt, initial_params(seed)
    p = initial_params(seed, 0.0)
    p[:-1] *= np.float32(8.0)
    return img, txt, p


def run_case(N, batch, epochs, dtype, seed=MULTI_SEED, lr=MULTI_LR):
    """A multi-step case from the initial parameters and zero moments, epoch by epoch with step0 carried over;
    per epoch a fresh permutation.  -> (params, exp_avg, exp_avg_sq, losses, norms, plan, cond)."""
    img, txt = draws(N, seed)
    p = initial_params(seed).astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    g = np.random.default_rng([seed, N, batch, epochs])
    plan, losses, norms, step0, cond = [], [], [], 0, 0.0
    for _ in range(epochs):
        perm = g.permutation(N).astype(np.int32)
        plan.append(perm)
        ls, ns, _, cd = epoch(img, txt, perm, batch, lr, step0, p, m, v, dtype)
        cond = max(cond, cd or 0.0)
        step0 += len(ls)
        losses.append(ls)
        norms.append(ns)
    return p, m, v, losses, norms, plan, cond
