"""What the four device trainers (fusion_training, clip_training, head_training, cifake_training) share: the packed
dropout masks, the validation of cached rows, the optimizer state dict of a checkpoint and the per-epoch metrics of
the two classifiers.  The ``fit`` loops stay with their trainers: checkpoint formats and best-epoch rules differ,
following the four reference scripts."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import io_utils


def pack_keep(mask) -> np.ndarray:
    """bool [N, width] (width a multiple of 64) -> uint64 [N, width / 64]: word w bit j = unit 64 w + j kept.  A
    single word per row (width 64, the FusionJudge's) comes without the word axis: uint64 [N]."""
    m = np.asarray(mask, dtype=bool)
    m = m.reshape(len(m), m.shape[-1] // 64, 64).astype(np.uint64)
    keep = (m << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return keep.reshape(-1) if keep.shape[1] == 1 else keep


def unpack_keep(keep, width: int) -> np.ndarray:
    """uint64 [N, width / 64] (or [N] for width 64) -> bool [N, width]."""
    k = np.asarray(keep, np.uint64).reshape(-1, width // 64, 1)
    return ((k >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1, width)


def check_rows(what: str, feats: Sequence, widths: Sequence[int], labels=None, noun: str = "features"):
    """Cached rows as the engine's wrappers take them: every array of ``feats`` float32 [N, its width], contiguous
    and finite, N >= 1, and ``labels`` (where given) [N] of 0 / 1 -> the arrays, then the labels as int32."""
    xs = [np.ascontiguousarray(np.asarray(a, dtype=np.float32)) for a in feats]
    y = None if labels is None else np.asarray(labels)
    n = xs[0].shape[0] if xs[0].ndim else 0
    if n == 0 or any(x.ndim != 2 or x.shape[1] != w or len(x) != n for x, w in zip(xs, widths)) \
            or (y is not None and y.shape != (n,)):
        got = [str(x.shape) for x in xs] + ([f"labels {y.shape}"] if y is not None else [])
        want = [f"[N, {w}]" for w in widths] + (["[N]"] if y is not None else [])
        raise ValueError(f"{what} {noun} {' / '.join(got)} must be {' / '.join(want)}, N >= 1")
    if not all(np.isfinite(x).all() for x in xs):
        raise ValueError(f"{what} {noun} must be finite")
    if y is None:
        return xs
    if not np.isin(y, (0, 1)).all():
        raise ValueError(f"{what} labels must be 0 or 1")
    return (*xs, y.astype(np.int32))


def split_like(flat: torch.Tensor, like) -> List[torch.Tensor]:
    """Consecutive pieces of a flat tensor in the shapes of ``like``."""
    out, o = [], 0
    for p in like:
        out.append(flat[o:o + p.numel()].reshape(p.shape))
        o += p.numel()
    return out


def _black():
    """The stand-in for an image that cannot be opened."""
    return io_utils.Image.new("RGB", (224, 224), (0, 0, 0))


def adamw_state_dict(parameters, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, steps: int, lr: float,
                     initial_lr: float, weight_decay: float, device: Optional[str] = None) -> dict:
    """The state dict ``torch.optim.AdamW(parameters)`` would hold with these moments (flat, in the parameters'
    order) and step count: built by a real AdamW, so it loads into one.  The moments go to ``device``, or with
    None to each parameter's own."""
    prm = list(parameters)
    opt = torch.optim.AdamW(prm, lr=initial_lr, weight_decay=weight_decay)
    for p, m, v in zip(prm, split_like(exp_avg, prm), split_like(exp_avg_sq, prm)):
        to = p.device if device is None else device
        opt.state[p] = {"step": torch.tensor(float(steps)), "exp_avg": m.detach().clone().to(to),
                        "exp_avg_sq": v.detach().clone().to(to)}
    sd = opt.state_dict()
    for gr in sd["param_groups"]:
        gr["lr"] = lr
        gr["initial_lr"] = initial_lr  # the key a scheduler adds to the groups it schedules
    return sd


def classifier_epoch_metrics(epoch: int, step_loss, step_correct, batch_loss, row_logits, N: int, val_labels):
    """An epoch of a two-class trainer as its reference script reports it -> (train_loss, train_acc, val_loss,
    val_acc, pred): the losses are means over the minibatches (total_loss / len(dataloader)), summed on the host
    in double; the accuracies are percentages; pred is the validation rows' argmax."""
    train_loss = float(step_loss.cpu().numpy().astype(np.float64).mean())
    train_acc = float(100 * int(step_correct.cpu().numpy().astype(np.int64).sum()) / N)
    val_loss = float(batch_loss.cpu().numpy().astype(np.float64).mean())
    if not (np.isfinite(train_loss) and np.isfinite(val_loss)):
        raise FloatingPointError(f"epoch {epoch}: the loss is not finite")
    lg = row_logits.cpu().numpy()
    pred = (lg[:, 1] > lg[:, 0]).astype(np.int64)  # torch.argmax / torch.max: a tie is class 0
    val_acc = float(100 * int((pred == val_labels).sum()) / len(val_labels))
    return train_loss, train_acc, val_loss, val_acc, pred
