"""The RoBERTa text heads -- ai_head and misinfo_head -- trained on the device (train_ai_head.py:160-527).

The script freezes everything but the head (:415-420) and still runs the 12-layer encoder for every minibatch of
every epoch.  With the encoder frozen the CLS row is a function of the text alone:

* ``extract_text_features``: the rows the heads read -- last_hidden_state[:, 0, :] -- for a whole data set, once,
  through the HIP tower (``Engine.text_pooled``), with HC3Dataset's tokenisation.
* ``split_indices``: the script's 80 / 20 ``random_split``.
* ``plan``: per epoch the permutation, the dropout masks and the per-step learning rates of the real
  warmup-cosine schedule.
* ``HeadTrainer``: one ``mmf_head_train_epoch`` and one ``mmf_head_eval`` call per epoch on the cached rows, the
  reference's checkpoint dict on a lower validation loss, the best head put back into the detector.
* ``train_head`` / ``python -m mmf_amd.head_training``: the script's entry point.

The head is the DEPLOYED one, Linear(768,256)-ReLU-Dropout(0.3)-Linear(256,2) on the CLS row
(misinfo_forensics.py:57-69, 95), not the script's Linear(768, 2) on pooler_output (:50), whose file the
inference constructor silently ignores: the checkpoint written here is one that
``MisinfoForensics(ai_head_weights=...)`` / ``misinfo_head_weights=`` loads.  Further deviations, documented in
DESIGN.md §7g: fp32 with fp32 master weights (no fp16 autocast / GradScaler), a seeded generator instead of the
global RNG, and eval-mode features -- the script's ``model.train()`` leaves RoBERTa's dropout 0.1 on, so its frozen
encoder is stochastic per minibatch; caching removes that noise (a linear probe on deterministic features).
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import io_utils
from . import training_common as TC
from . import weights as W
from .training_common import pack_keep, split_like as _split  # pack_keep here: bool [N, 256] -> uint64 [N, 4]

BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.AdamW defaults (train_ai_head.py:433-437)
P_DROP = 0.3                     # the heads' Dropout (misinfo_forensics.py:60, 67)
HIDDEN, WIDTH = 256, 768
PARAM_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias")
N_PARAMS = HIDDEN * WIDTH + HIDDEN + 2 * HIDDEN + 2  # MMF_HEAD_PARAMS
HEADS = ("ai_head", "misinfo_head")
DEFAULT_FILES = {"ai_head": "ai_head_best.pth", "misinfo_head": "roberta_detective_best.pth"}


# ---------------------------------------------------------------------------------------------
# cached features
# ---------------------------------------------------------------------------------------------
def _tokenize(tok, texts: List[str], max_length: int) -> List[List[int]]:
    """HC3Dataset.__getitem__'s tokenisation (train_ai_head.py:189-195) without its padding to max_length
    (padding never reaches the CLS row through the masked attention): unpadded id lists, truncated."""
    try:
        enc = tok(list(texts), return_tensors="pt", max_length=max_length, truncation=True, padding=True)
        seqs = io_utils._strip_padded(enc["input_ids"], enc["attention_mask"], len(texts))
    except (TypeError, KeyError, ValueError):  # a tokenizer object that only takes single strings
        seqs = []
        for t in texts:
            enc = tok(t, return_tensors="pt", max_length=max_length, truncation=True, padding=True)
            seqs.extend(io_utils._strip_padded(enc["input_ids"], enc["attention_mask"], 1))
    return [s[:max_length] for s in seqs]


def extract_text_features(forensics, texts: Sequence[str], max_length: int = 256) -> np.ndarray:
    """What the frozen encoder gives for every row of an HC3Dataset -> float32 [N, 768], in ``max_batch`` chunks
    through ``Engine.text_pooled``; each text is tokenised once, truncated at ``max_length``."""
    if forensics.roberta_tokenizer is None:
        raise RuntimeError("no RoBERTa tokenizer (pass roberta_tokenizer=)")
    if not 1 <= int(max_length) <= 512:
        raise ValueError(f"max_length must be in 1..512, got {max_length}")
    texts = [str(t) for t in texts]
    N = len(texts)
    out = np.zeros((N, WIDTH), np.float32)
    cap = forensics.engine.max_batch
    chunks = [(a, min(a + cap, N)) for a in range(0, N, cap)]
    if not chunks:
        return out
    forensics.detector.sync(("text",))

    def host_stage(a, b):
        seqs = _tokenize(forensics.roberta_tokenizer, texts[a:b], int(max_length))
        ids, mask = io_utils.pad_ids(seqs, W.ROBERTA["pad_id"])
        return a, b, ids, mask

    def device_part(staged):
        a, b, ids, mask = staged
        forensics._fit_text(ids.shape[1])
        out[a:b] = forensics.engine.text_pooled(ids, mask).cpu().numpy()

    forensics._run_chunks(chunks, host_stage, device_part)
    return out


# ---------------------------------------------------------------------------------------------
# the split and the epoch plan
# ---------------------------------------------------------------------------------------------
def split_indices(N: int, val_fraction: float = 0.2, seed: int = 42) -> Tuple[np.ndarray, np.ndarray]:
    """(train, val) row indices as ``random_split(dataset, [N - int(f N), int(f N)],
    torch.Generator().manual_seed(seed))`` gives them (train_ai_head.py:347-353)."""
    n_val = int(val_fraction * N)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed))).numpy()
    return perm[:N - n_val].astype(np.int64), perm[N - n_val:].astype(np.int64)


def _scheduler(total_steps: int, lr: float, warmup_ratio: float):
    from transformers import get_cosine_schedule_with_warmup
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return opt, get_cosine_schedule_with_warmup(opt, num_warmup_steps=int(total_steps * warmup_ratio),
                                                num_training_steps=total_steps)


def plan(N: int, batch_size: int, epochs: int, lr: float, seed: int, warmup_ratio: float = 0.1):
    """Per epoch (perm int32 [N], keep uint64 [N, 4], lr_steps float64 [steps_per_epoch]): the DataLoader's
    shuffle as ``torch.randperm`` and the dropout masks as ``torch.rand(N, 256) >= 0.3`` (row i = the row at
    position i of the epoch order) from one ``torch.Generator().manual_seed(seed)``; the learning rate of every
    step as a real ``get_cosine_schedule_with_warmup`` holds it, stepped after every minibatch
    (train_ai_head.py:241, 439-446).  Its first value is 0 whenever there is a warmup step."""
    g = torch.Generator().manual_seed(int(seed))
    spe = -(-N // batch_size)
    opt, sched = _scheduler(spe * epochs, lr, warmup_ratio)
    out = []
    for _ in range(epochs):
        perm = torch.randperm(N, generator=g).to(torch.int32).numpy()
        keep = pack_keep((torch.rand(N, HIDDEN, generator=g) >= P_DROP).numpy())
        lrs = []
        for _ in range(spe):
            lrs.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sched.step()
        out.append((perm, keep, np.asarray(lrs, np.float64)))
    return out


def _scheduler_state(total_steps: int, lr: float, warmup_ratio: float, done: int) -> Tuple[dict, float]:
    """(state_dict of the reference's scheduler after `done` steps, the learning rate its optimizer holds then)."""
    opt, sched = _scheduler(total_steps, lr, warmup_ratio)
    for _ in range(done):
        opt.step()
        sched.step()
    return sched.state_dict(), float(opt.param_groups[0]["lr"])


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
def flatten_head(head) -> torch.Tensor:
    """A head's parameters as one float32 [197378] tensor, state-dict order."""
    sd = head.state_dict()
    flat = torch.cat([sd[k].detach().reshape(-1).float() for k in PARAM_KEYS])
    if flat.numel() != N_PARAMS:
        raise ValueError(f"a head of {flat.numel()} parameters, expected {N_PARAMS}")
    return flat


def optimizer_state_dict(head, exp_avg, exp_avg_sq, steps: int, lr: float, initial_lr: float,
                         weight_decay: float) -> dict:
    """The state dict the reference's ``AdamW(filter(requires_grad, model.parameters()))`` would hold with these
    moments and step count: built by a real AdamW over the head's ``parameters()``, so it loads into one."""
    return TC.adamw_state_dict(head.parameters(), exp_avg, exp_avg_sq, steps, lr, initial_lr, weight_decay,
                               device="cpu")


class HeadTrainer:
    """The training loop of train_ai_head.py:466-506 on cached CLS rows: per epoch one training call and one
    validation call on the device.  ``fit`` ends with ONE re-pack of the detector's text component
    (``detector.sync``), which also re-runs the load-time precision calibration on the new head."""

    def __init__(self, forensics, head: str = "ai_head", batch_size: int = 16, epochs: int = 3, lr: float = 1e-3,
                 weight_decay: float = 0.01, max_norm: float = 1.0, seed: int = 0, warmup_ratio: float = 0.1):
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}, got {head!r}")
        if not 1 <= int(batch_size) <= 64:
            raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
        self.forensics, self.head, self.batch_size, self.epochs = forensics, head, int(batch_size), int(epochs)
        self.lr, self.weight_decay, self.max_norm = float(lr), float(weight_decay), float(max_norm)
        self.seed, self.warmup_ratio = int(seed), float(warmup_ratio)

    @staticmethod
    def _data(feats, labels, what):
        return TC.check_rows(what, (feats,), (WIDTH,), labels)

    def fit(self, train_feats, train_labels, val_feats, val_labels, checkpoint_path: Optional[str] = None,
            save_full_model: bool = True) -> List[dict]:
        f = self.forensics
        eng, det = f.engine, f.detector
        dev = eng.device
        module = getattr(det, self.head)
        xt, yt = self._data(train_feats, train_labels, "training")
        xv, yv = self._data(val_feats, val_labels, "validation")
        N, bs = len(yt), self.batch_size
        xt, yt_d, xv, yv_d = (torch.from_numpy(a).to(dev) for a in (xt, yt, xv, yv))
        params = flatten_head(module).to(dev).contiguous()
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        spe = -(-N // bs)
        history, best_loss, best, step0 = [], float("inf"), None, 0
        self.val_predictions = None
        for epoch, (perm, keep, lrs) in enumerate(plan(N, bs, self.epochs, self.lr, self.seed, self.warmup_ratio), 1):
            sl, sc, _ = eng.head_train_epoch(xt, yt_d, torch.from_numpy(perm).to(dev),
                                             torch.from_numpy(keep.view(np.int64)).to(dev), P_DROP, bs, lrs, BETAS,
                                             EPS, self.weight_decay, self.max_norm, step0, params, m, v)
            bl, lg = eng.head_eval(xv, yv_d, bs, params)
            step0 += spe
            # train_ai_head.py:255, :294
            train_loss, train_acc, val_loss, val_acc, pred = TC.classifier_epoch_metrics(epoch, sl, sc, bl, lg, N, yv)
            history.append({"epoch": epoch, "train_loss": train_loss, "train_acc": train_acc, "val_loss": val_loss,
                            "val_acc": val_acc, "lr": float(lrs[-1])})
            if val_loss < best_loss:  # :491
                best_loss, best = val_loss, params.clone()
                self.val_predictions = pred
                if checkpoint_path:
                    sched, next_lr = _scheduler_state(spe * self.epochs, self.lr, self.warmup_ratio, step0)
                    torch.save({"epoch": epoch,
                                "model_state_dict": self._model_state(best, save_full_model),
                                "optimizer_state_dict": optimizer_state_dict(module, m, v, step0, next_lr, self.lr,
                                                                             self.weight_decay),
                                "scheduler_state_dict": sched,
                                "val_loss": val_loss, "val_acc": val_acc, "train_loss": train_loss,
                                "train_acc": train_acc}, checkpoint_path)
        self._install(best if best is not None else params)
        return history

    def _head_tensors(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        module = getattr(self.forensics.detector, self.head)
        prm = [module.state_dict()[k] for k in PARAM_KEYS]
        return {f"{self.head}.{k}": t.detach().cpu().clone() for k, t in zip(PARAM_KEYS, _split(flat, prm))}

    def _model_state(self, flat: torch.Tensor, full: bool) -> Dict[str, torch.Tensor]:
        """detector.state_dict() with the trained head, as the reference saves (:497); ``full`` False: the head's
        four tensors alone (what the constructor's fallback path reads of it)."""
        head = self._head_tensors(flat)
        if not full:
            return head
        sd = {k: t.detach().cpu() for k, t in self.forensics.detector.state_dict().items()}
        sd.update(head)
        return sd

    def _install(self, flat: torch.Tensor) -> None:
        """In-place copies bump the parameters' version counters; detector.sync() then re-packs the text component
        (RoBERTa + both heads) and re-runs check_text_precision, whose calibration depends on the heads' logits."""
        det = self.forensics.detector
        prm = list(getattr(det, self.head).parameters())
        with torch.no_grad():
            for p, src in zip(prm, _split(flat, prm)):
                p.copy_(src)
        det.sync(("text",))


# ---------------------------------------------------------------------------------------------
# the script's entry point
# ---------------------------------------------------------------------------------------------
def confusion_matrix(labels, predictions) -> np.ndarray:
    """2 x 2 counts, rows = true class, columns = predicted class (sklearn's layout, :487)."""
    cm = np.zeros((2, 2), np.int64)
    np.add.at(cm, (np.asarray(labels, np.int64), np.asarray(predictions, np.int64)), 1)
    return cm


def train_head(csv: str, head: str = "ai_head", checkpoint_path: Optional[str] = None, batch_size: int = 16,
               epochs: int = 3, lr: float = 1e-3, max_length: int = 256, device: str = "cuda", *, forensics=None,
               seed: int = 0, save_full_model: bool = True, max_samples: Optional[int] = None):
    """train_ai_head.py:301-527 for either head: the CSV's ``text`` / ``label`` columns, rows stripped and empty
    texts dropped (:176-177), the 80 / 20 split of :347-353, one feature extraction, then the trainer.  Returns
    the history (None when the CSV is missing)."""
    import pandas as pd
    if head not in HEADS:
        raise ValueError(f"head must be one of {HEADS}, got {head!r}")
    if not os.path.exists(csv):
        print(f"✗ Error: {csv} not found!")
        return None
    if checkpoint_path is None:
        checkpoint_path = DEFAULT_FILES[head]
    if forensics is None:
        from .api import MisinfoForensics
        forensics = MisinfoForensics(device=device)
    df = pd.read_csv(csv)
    df["text"] = df["text"].astype(str).str.strip()
    df = df[df["text"].str.len() > 0].reset_index(drop=True)
    if max_samples:
        df = df.head(max_samples)
    print(f"Loaded {len(df)} samples")
    print(f"Label distribution: {df['label'].value_counts().to_dict()}")
    labels = np.asarray([int(v) for v in df["label"]])
    tr, va = split_indices(len(df))
    print(f"  Training: {len(tr)} samples\n  Validation: {len(va)} samples")
    feats = extract_text_features(forensics, list(df["text"]), max_length=max_length)
    trainer = HeadTrainer(forensics, head=head, batch_size=batch_size, epochs=epochs, lr=lr, seed=seed)
    history = trainer.fit(feats[tr], labels[tr], feats[va], labels[va], checkpoint_path=checkpoint_path,
                          save_full_model=save_full_model)
    for h in history:
        print(f"Epoch {h['epoch']}/{epochs}  Train Loss: {h['train_loss']:.4f} | Train Acc: {h['train_acc']:.2f}%  "
              f"Val Loss: {h['val_loss']:.4f} | Val Acc: {h['val_acc']:.2f}%")
    if trainer.val_predictions is not None:
        print(f"Confusion Matrix ({head}, best epoch):\n{confusion_matrix(labels[va], trainer.val_predictions)}")
    return history


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m mmf_amd.head_training",
                                 description="Train the RoBERTa ai / misinfo head on cached CLS rows")
    ap.add_argument("--csv", required=True, help="training CSV (text, label)")
    ap.add_argument("--head", choices=HEADS, default="ai_head")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--max-length", type=int, default=256)
    ap.add_argument("--checkpoint", default=None, help="default: ai_head_best.pth / roberta_detective_best.pth")
    a = ap.parse_args(argv)
    train_head(a.csv, head=a.head, checkpoint_path=a.checkpoint, batch_size=a.batch_size, epochs=a.epochs, lr=a.lr,
               max_length=a.max_length)


if __name__ == "__main__":
    main()
