"""What the four trainers' numpy restatements (tests/{fusion,clip,head,effcls}_train_refs.py) share: the packed dropout
masks, the Adam / AdamW update with its scalars rounded once, clip_grad_norm_'s coefficient, the first-order error of a
fixed-order chain, and the conditioning number of a multi-step float64 run (``Drift``).  The four modules import from
here and keep their public names; tests/test_*_train_refs_cpu.py hold them against the real torch.optim."""
import numpy as np

U = 2.0 ** -24
BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim's defaults, all four reference scripts'


def pack_keep(mask) -> np.ndarray:
    """bool [N, width] (width a multiple of 64) -> uint64 [N, width / 64]: word w bit j = unit 64 w + j.  A single
    word per row (width 64, the FusionJudge's) comes without the word axis: uint64 [N]."""
    m = np.asarray(mask, bool)
    m = m.reshape(len(m), m.shape[-1] // 64, 64).astype(np.uint64)
    keep = (m << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return keep.reshape(-1) if keep.shape[1] == 1 else keep


def unpack_keep(keep, width) -> np.ndarray:
    """uint64 [N, width / 64] (or [N] for width 64) -> bool [N, width]."""
    k = np.asarray(keep, np.uint64).reshape(-1, width // 64, 1)
    return ((k >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1, width)


def flat(grads):
    return np.concatenate([g.reshape(-1) for g in grads])


def clip_coef(norm, max_norm, dtype):
    dt = dtype
    return min(dt(max_norm) / (dt(norm) + dt(1e-6)), dt(1.0))


def adam(p, m, v, g, lr, step, dtype, wd, decay, betas=BETAS, eps=EPS):
    """torch.optim's single-tensor Adam update on arrays, in place; the scalars in double, rounded to dtype once.
    decay: "decoupled" (torch.optim.AdamW: p *= 1 - lr wd first), "l2" (torch.optim.Adam: g += wd p where wd != 0)
    or None."""
    dt = dtype
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    w1, fb2, w2 = dt(1.0 - b1), dt(b2), dt(1.0 - b2)
    step_size, bc2s, feps = dt(lr / bc1), dt(np.sqrt(bc2)), dt(eps)
    if decay == "decoupled":
        p *= dt(1.0 - lr * wd)
    elif decay == "l2" and wd != 0:
        g = g + dt(wd) * p
    m += w1 * (g - m)
    v *= fb2
    v += w2 * (g * g)
    p -= step_size * (m / (np.sqrt(v) / bc2s + feps))


def chain_err(x, w):
    """First-order rounding error of the ascending-index fmaf chains x[i] . w[j] (the kernel's contract fixes the
    order): every step rounds its partial sum once, so the error is at most U sum_k |partial sum k|, from the
    float64 partial sums.  x [M, K], w [N, K] -> [M, N]."""
    return U * np.stack([np.abs(np.cumsum(w * xi, axis=1)).sum(1) for xi in x])


class Drift:
    """The conditioning number of a float64 run, accumulated over its steps.  Adam is elementwise: the update of
    step t is u_t = lr_t m_hat / (sqrt(v_hat) + eps), m and v the running means of the gradients g_s, s <= t, so
        du_t / dg_s = lr_t [ (1 - b1) b1^(t-s) / bc1 / D  -  (m / bc1) (1 - b2) b2^(t-s) g_s / (bc2 sqrt(v_hat) D^2) ],
    D = sqrt(v_hat) + eps.  (At step 1 the two terms cancel to lr eps / (|g| + eps)^2: the update is the gradient's
    sign.)  A gradient error dg_s therefore moves the parameter after T steps by sum_t |du_t / dg_s| dg_s, each
    step's part capped at 2 lr_t, the distance between the two signs.  cond = the largest such sum over the
    parameters, with dg_s = coef_s U x (the magnitude the model's ``_magnitudes`` gives).  The feedback of a moved
    parameter into later gradients is second order at these distances and left out."""

    def __init__(self):
        self.g, self.dg, self.total = [], [], None

    def gradient(self, g, dg):
        self.g.append(g.copy())
        self.dg.append(dg)

    def update(self, m, v, lr, step):
        b1, b2 = BETAS
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        rv = np.sqrt(v / bc2)
        D = rv + EPS
        t = len(self.g) - 1
        part = np.zeros_like(m)
        for s, (g, dg) in enumerate(zip(self.g, self.dg)):
            d = (1.0 - b1) * b1 ** (t - s) / bc1 / D - (m / bc1) * (1.0 - b2) * b2 ** (t - s) * g / (bc2 * np.maximum(rv, 1e-300) * D * D)
            part += np.abs(d) * dg
        part = np.minimum(lr * part, 2.0 * lr)
        self.total = part if self.total is None else self.total + part

    @property
    def cond(self):
        return float(self.total.max()) if self.total is not None else 0.0
