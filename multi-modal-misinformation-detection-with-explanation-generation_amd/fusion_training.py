"""FusionJudge training on the device (train_fusion_judge.py).

* ``extract_scores``: the ``[N, 5]`` score matrix of a training set through the batched five-signal path
  (one ``analyze_batch`` launch sequence per ``max_batch`` rows) instead of four single-sample calls per
  row and epoch, with the reference's row-level failure rule (any failure zeroes the row).
* ``plan``: an epoch's permutation, dropout masks and learning rate from one seeded generator.
* ``FusionTrainer``: one ``mmf_fusion_train_epoch`` launch per epoch (forward, cross-entropy, backward and
  AdamW for every minibatch), the reference's checkpoint dict, the trained layer copied into the detector.
* ``train_fusion_layer`` / ``python -m mmf_amd.fusion_training``: the reference script's entry points.

Deviations from the reference, both documented in DESIGN.md: the trainer computes in fp32 (no fp16
autocast / GradScaler), and shuffling and dropout draw from a seeded generator, not the global RNG.
"""
from __future__ import annotations

import argparse
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import io_utils
from . import training_common as TC
from . import weights as W
from .precision import rerun_if
from .training_common import pack_keep, split_like as _split  # pack_keep here: bool [N, 64] -> uint64 [N]

P_DROP = 0.2  # fusion_layer's Dropout (misinfo_forensics.py:86)
BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.AdamW defaults (train_fusion_judge.py:179-183)
PARAM_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "5.weight", "5.bias")  # state-dict order
N_PARAMS = 2530


# ---------------------------------------------------------------------------------------------
# score extraction
# ---------------------------------------------------------------------------------------------
def _row_scores(forensics, text: str, image_path: str) -> List[float]:
    """train_fusion_judge.py:72-94: the reference's four per-sample calls."""
    t = forensics.analyze_text(text)
    i = forensics.analyze_image(image_path)
    c = forensics.analyze_consistency(text, image_path)
    v = forensics.search_vault(image_path)
    return [t["ai_score"], t["misinfo_score"], i["deepfake_score"], c["clip_similarity"], v["vault_discrepancy"]]


def extract_scores(forensics, texts: Sequence[str], image_paths: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """What ``FusionTrainingDataset.__getitem__`` (train_fusion_judge.py:53-104) returns per row, for all
    rows, through the batched path -> (scores float32 [N, 5], ok bool [N]).

    A row the reference would zero is zero here, with ``ok`` False: its image path does not exist (:61),
    its caption has more than 77 CLIP tokens (analyze_consistency does not truncate: quirk Q8), or its
    image cannot be decoded (:97).  Existence and token length are screened before anything is staged;
    each text is tokenised once.  If a chunk still raises, that chunk is redone row by row with the
    reference's four calls inside try / except.  The vault search takes no caption (:85), and
    vault_discrepancy does not depend on one, so column 4 is the batched value."""
    if len(texts) != len(image_paths):
        raise ValueError(f"{len(texts)} texts vs {len(image_paths)} images")
    if forensics.roberta_tokenizer is None:
        raise RuntimeError("no RoBERTa tokenizer (pass roberta_tokenizer=)")
    if forensics.clip_processor is None:
        raise RuntimeError("no CLIP processor (pass clip_processor=)")
    texts = [str(t) for t in texts]
    paths = [str(p) for p in image_paths]
    N = len(texts)
    scores = np.zeros((N, 5), np.float32)
    ok = np.zeros(N, bool)
    cap = forensics.engine.max_batch
    chunks = [(a, min(a + cap, N)) for a in range(0, N, cap)]
    if not chunks:
        return scores, ok
    forensics._ensure_jpeg_stager()

    def host_stage(a, b):
        rows = [i for i in range(a, b) if os.path.exists(paths[i])]
        try:
            if rows:
                seqs = io_utils.tokenize_clip(forensics.clip_processor, [texts[i] for i in rows])
                keep = [k for k, s in enumerate(seqs) if len(s) <= 77]
                rows, seqs = [rows[k] for k in keep], [seqs[k] for k in keep]
            if not rows:
                return rows, None
            cid, cm = io_utils.pad_ids(seqs, forensics.clip_eos_token_id)
            rob = io_utils.tokenize_roberta_batch(forensics.roberta_tokenizer, [texts[i] for i in rows])
            rid, rm = io_utils.pad_ids(rob, W.ROBERTA["pad_id"])
            return rows, (rid, rm, cid, cm, forensics._stage_images([paths[i] for i in rows]))
        except Exception as e:  # noqa: BLE001  (an undecodable image, ...: this chunk goes row by row)
            return rows, e

    def device_part(staged):
        rows, st = staged
        if st is None:
            return
        try:
            if isinstance(st, Exception):
                raise st
            rid, rm, cid, cm, rgb = st
            forensics._fit_text(rid.shape[1])
            eff, clp = forensics._windows(*rgb)
            # (a tower that switches precision on these scores: the batch runs again)
            scores[rows] = rerun_if(forensics.engine.scores_overflow,
                                    lambda: forensics.analyze_batch(rid, rm, cid, cm, eff, clp)["scores"].cpu().numpy())
            ok[rows] = True
        except Exception:  # noqa: BLE001
            for i in rows:
                try:
                    scores[i] = _row_scores(forensics, texts[i], paths[i])
                    ok[i] = True
                except Exception as e:  # noqa: BLE001  (train_fusion_judge.py:97-99)
                    print(f"⚠ Error processing sample {i}: {e}")
                    scores[i] = 0.0

    forensics._run_chunks(chunks, host_stage, device_part)
    return scores, ok


# ---------------------------------------------------------------------------------------------
# the epoch plan
# ---------------------------------------------------------------------------------------------
def plan(N: int, batch_size: int, epochs: int, lr: float, seed: int):
    """Per epoch (perm int32 [N], keep uint64 [N], lr): the DataLoader's shuffle as ``torch.randperm``, the
    Dropout(0.2) masks as ``torch.rand(N, 64) >= 0.2`` (row i = the row at position i of the epoch's
    order), both from one ``torch.Generator().manual_seed(seed)``; lr as a real
    ``CosineAnnealingLR(T_max=epochs, eta_min=0.1 * lr)`` holds it during that epoch.  (The masks are per
    position, so the plan does not depend on batch_size.)"""
    g = torch.Generator().manual_seed(int(seed))
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr * 0.1)
    out = []
    for _ in range(epochs):
        perm = torch.randperm(N, generator=g).to(torch.int32).numpy()
        keep = pack_keep((torch.rand(N, 64, generator=g) >= P_DROP).numpy())
        out.append((perm, keep, float(opt.param_groups[0]["lr"])))
        opt.step()
        sched.step()
    return out


def _scheduler_state(epochs: int, lr: float, done: int) -> dict:
    """state_dict of the reference's scheduler after `done` scheduler steps."""
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr * 0.1)
    for _ in range(done):
        opt.step()
        sched.step()
    return sched.state_dict()


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
def flatten_fusion(fusion_layer) -> torch.Tensor:
    """fusion_layer's parameters as one float32 [2530] tensor, state-dict order."""
    sd = fusion_layer.state_dict()
    return torch.cat([sd[k].detach().reshape(-1).float() for k in PARAM_KEYS])


def optimizer_state_dict(fusion_layer, exp_avg, exp_avg_sq, steps: int, lr: float, initial_lr: float,
                         weight_decay: float) -> dict:
    """The state dict ``torch.optim.AdamW(fusion_layer.parameters())`` would hold with these moments and
    step count: built by a real AdamW, so it loads into one."""
    return TC.adamw_state_dict(fusion_layer.parameters(), exp_avg, exp_avg_sq, steps, lr, initial_lr, weight_decay)


class FusionTrainer:
    """The training loop of train_fusion_judge.py:179-272 with every epoch as one kernel launch."""

    def __init__(self, forensics, batch_size: int = 16, epochs: int = 10, lr: float = 1e-3,
                 weight_decay: float = 0.01, seed: int = 0):
        if not 1 <= int(batch_size) <= 256:
            raise ValueError(f"batch_size must be in 1..256, got {batch_size}")
        self.forensics, self.batch_size, self.epochs = forensics, int(batch_size), int(epochs)
        self.lr, self.weight_decay, self.seed = float(lr), float(weight_decay), int(seed)

    def fit(self, scores, labels, checkpoint_path: Optional[str] = None) -> List[dict]:
        f = self.forensics
        eng, det = f.engine, f.detector
        scores, labels = TC.check_rows("training", (scores,), (5,), labels, noun="scores")
        N, dev = len(labels), eng.device
        x = torch.from_numpy(scores).to(dev)
        y = torch.from_numpy(labels).to(dev)
        params = flatten_fusion(det.fusion_layer).to(dev).contiguous()
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        steps_per_epoch = -(-N // self.batch_size)
        rows = np.minimum(self.batch_size, N - self.batch_size * np.arange(steps_per_epoch)).astype(np.float64)
        history, best, step0 = [], 0.0, 0
        for epoch, (perm, keep, lr) in enumerate(plan(N, self.batch_size, self.epochs, self.lr, self.seed), 1):
            sl, sc = eng.fusion_train_epoch(x, y, torch.from_numpy(perm).to(dev),
                                            torch.from_numpy(keep.view(np.int64)).to(dev), P_DROP, self.batch_size,
                                            lr, BETAS, EPS, self.weight_decay, step0, params, m, v)
            step0 += steps_per_epoch
            # running_loss += loss.item() * rows; correct += ...: summed on the host in double (:230-243)
            loss = float((sl.cpu().numpy().astype(np.float64) * rows).sum() / N)
            acc = float(100 * int(sc.cpu().numpy().astype(np.int64).sum()) / N)
            if not np.isfinite(loss):
                raise FloatingPointError(f"epoch {epoch}: the loss is not finite")
            history.append({"epoch": epoch, "loss": loss, "accuracy": acc, "lr": lr})
            if acc > best:  # :252
                best = acc
                self._copy_in(params)
                if checkpoint_path:
                    torch.save({"epoch": epoch,
                                "fusion_layer_state_dict": det.fusion_layer.state_dict(),
                                "full_model_state_dict": det.state_dict(),
                                "optimizer_state_dict": optimizer_state_dict(det.fusion_layer, m, v, step0, lr,
                                                                             self.lr, self.weight_decay),
                                "scheduler_state_dict": _scheduler_state(self.epochs, self.lr, epoch - 1),
                                "loss": loss, "accuracy": acc}, checkpoint_path)
        self._copy_in(params)
        return history

    def _copy_in(self, params: torch.Tensor) -> None:
        """In-place copies bump the parameters' version counters, so detector.sync() re-packs the engine's
        fusion weights before the next device call."""
        prm = list(self.forensics.detector.fusion_layer.parameters())
        with torch.no_grad():
            for p, src in zip(prm, _split(params, prm)):
                p.copy_(src)


def train_fusion_layer(csv_file: str = "Final_Fusion_Train.csv", batch_size: int = 16, epochs: int = 10,
                       lr: float = 1e-3, device: str = "cuda", *, forensics=None, seed: int = 0,
                       checkpoint_path: str = "forensics_master_final.pth", max_samples: Optional[int] = None):
    """train_fusion_judge.py:107-282: the CSV's ``text`` / ``image_path`` / ``label`` columns -> one batched
    score extraction -> FusionTrainer.  Returns the forensics object (None when the CSV is missing, as
    the reference)."""
    import pandas as pd
    if not os.path.exists(csv_file):
        print(f"✗ Error: {csv_file} not found!")
        return None
    if forensics is None:
        from .api import MisinfoForensics
        forensics = MisinfoForensics(device=device)
    df = pd.read_csv(csv_file)
    if max_samples:
        df = df.head(max_samples)
    print(f"Loaded {len(df)} samples for fusion training")
    texts = [str(t) for t in df["text"]]
    paths = [str(p) for p in df["image_path"]]
    labels = np.asarray([int(v) for v in df["label"]])
    scores, ok = extract_scores(forensics, texts, paths)
    print(f"Scores extracted: {int(ok.sum())} rows, {int((~ok).sum())} zeroed")
    trainer = FusionTrainer(forensics, batch_size=batch_size, epochs=epochs, lr=lr, seed=seed)
    for h in trainer.fit(scores, labels, checkpoint_path=checkpoint_path):
        print(f"Epoch {h['epoch']}/{epochs}  Loss: {h['loss']:.4f}  Accuracy: {h['accuracy']:.2f}%  "
              f"Learning Rate: {h['lr']:.6f}")
    return forensics


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m mmf_amd.fusion_training", description="Train the FusionJudge")
    ap.add_argument("--csv", default="Final_Fusion_Train.csv", help="training CSV (text, image_path, label)")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    a = ap.parse_args(argv)
    train_fusion_layer(csv_file=a.csv, batch_size=a.batch_size, epochs=a.epochs, lr=a.lr)


if __name__ == "__main__":
    main()
