"""CLIPDetective's projection heads trained on the device (train_clip_detective.py:76-424).

CLIPDetective freezes both encoders (:89-99) and trains visual_projection.weight, text_projection.weight and
logit_scale.  CLIP has no dropout, so the frozen part is a pure function of the inputs:

* ``extract_features``: the rows the projections read -- post_layernorm(CLS) and final_layer_norm(EOS) -- for a
  whole data set, once, through the HIP towers (``Engine.clip_pooled``), with the reference's dataset rules.
* ``plan``: an epoch's permutation and learning rate.
* ``ClipProjectionTrainer``: one ``mmf_clip_train_epoch`` and one ``mmf_clip_contrastive_eval`` call per epoch on
  the cached features, the reference's checkpoint dict on a better validation accuracy, the best projections put
  back into the engine.
* ``sample_trials`` / ``ClipProjectionTuner``: the script's ``--tune`` mode (:427-454) as a study of up to 16
  trials per launch: epoch e of every trial still running in ONE ``mmf_clip_train_epoch_trials`` and one
  ``mmf_clip_contrastive_eval_trials`` call, each trial bit-identical to the same trial trained alone.
* ``train_clip_detective`` / ``run_hyperparameter_tuning`` / ``python -m mmf_amd.clip_training [--tune]``: the
  reference script's entry points.

Deviations from the reference, documented in DESIGN.md §7f: the trainer computes in fp32 (no fp16 autocast /
GradScaler), shuffling draws from a seeded generator instead of the global RNG, and the features are cached once
(exact: the encoders are frozen and dropout-free).  The study draws its trials up front from a seeded generator
(Optuna's TPE sampler suggests from earlier results, which trials that run side by side do not have), does not
prune, and writes the winning trial's checkpoint rather than the last improving one's.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import io_utils
from . import training_common as TC
from .training_common import _black

BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.AdamW defaults (train_clip_detective.py:345-349)
N_VISUAL, N_TEXT = 512 * 768, 512 * 512
N_PARAMS = N_VISUAL + N_TEXT + 1  # MMF_CLIP_TRAIN_PARAMS: visual | text | logit_scale
KEYS = ("visual_projection.weight", "text_projection.weight", "logit_scale")
TRIALS_MAX, TRIAL_STRIDE = 16, 655364  # MMF_CLIP_TRIALS_MAX, MMF_CLIP_TRIAL_STRIDE (floats from one trial to the next)


# ---------------------------------------------------------------------------------------------
# cached features
# ---------------------------------------------------------------------------------------------
def extract_features(forensics, texts: Sequence[str], image_paths: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """What the frozen encoders of CLIPDetective give for every row of a GuardianCLIPDataset
    (train_clip_detective.py:39-73) -> (img_feat float32 [N, 768], txt_feat float32 [N, 512]), in
    ``max_batch`` chunks through ``Engine.clip_pooled``.  The dataset's rules, not analyze_consistency's:
    an image that cannot be opened becomes a black 224x224 image (:44-48), and captions are truncated at 77
    tokens (:62-69)."""
    if len(texts) != len(image_paths):
        raise ValueError(f"{len(texts)} texts vs {len(image_paths)} images")
    if forensics.clip_processor is None:
        raise RuntimeError("no CLIP processor (pass clip_processor=)")
    texts = [str(t) for t in texts]
    paths = list(image_paths)
    N = len(texts)
    img = np.zeros((N, 768), np.float32)
    txt = np.zeros((N, 512), np.float32)
    cap = forensics.engine.max_batch
    chunks = [(a, min(a + cap, N)) for a in range(0, N, cap)]
    if not chunks:
        return img, txt
    forensics._ensure_jpeg_stager()

    def host_stage(a, b):
        seqs = [s[:77] for s in io_utils.tokenize_clip(forensics.clip_processor, texts[a:b], truncation=True)]
        cid, cm = io_utils.pad_ids(seqs, forensics.clip_eos_token_id)
        try:
            rgb = forensics._stage_images(paths[a:b])
        except Exception:  # noqa: BLE001  (a file of the chunk does not open: each on its own, black where it fails)
            pils = []
            for p in paths[a:b]:
                try:
                    pils.append(io_utils.to_pil(p))
                except Exception:  # noqa: BLE001  (train_clip_detective.py:46-48)
                    pils.append(_black())
            rgb = forensics._stage_images(pils)
        return a, b, cid, cm, rgb

    def device_part(staged):
        a, b, cid, cm, rgb = staged
        _, clp = forensics._windows(*rgb)
        ip, tp = forensics.engine.clip_pooled(clp, cid, cm)
        img[a:b] = ip.cpu().numpy()
        txt[a:b] = tp.cpu().numpy()

    forensics._run_chunks(chunks, host_stage, device_part)
    return img, txt


# ---------------------------------------------------------------------------------------------
# the epoch plan
# ---------------------------------------------------------------------------------------------
def _scheduler(epochs: int, lr: float):
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=lr * 0.01)


def plan(N: int, epochs: int, lr: float, seed: int):
    """Per epoch (perm int32 [N], lr): the DataLoader's shuffle as ``torch.randperm`` from a
    ``torch.Generator().manual_seed(seed)``; lr as a real ``CosineAnnealingLR(T_max=epochs, eta_min=0.01 * lr)``
    holds it during that epoch (train_clip_detective.py:352-354, 379)."""
    g = torch.Generator().manual_seed(int(seed))
    opt, sched = _scheduler(epochs, lr)
    out = []
    for _ in range(epochs):
        out.append((torch.randperm(N, generator=g).to(torch.int32).numpy(), float(opt.param_groups[0]["lr"])))
        opt.step()
        sched.step()
    return out


def _scheduler_state(epochs: int, lr: float, done: int) -> dict:
    """state_dict of the reference's scheduler after `done` scheduler steps."""
    opt, sched = _scheduler(epochs, lr)
    for _ in range(done):
        opt.step()
        sched.step()
    return sched.state_dict()


def batch_accuracy(cos, labels) -> float:
    """calculate_accuracy (train_clip_detective.py:169-187) of one validation batch from the pairs' own cosines:
    the threshold is ``torch.median`` of the batch (the LOWER median of an even count), and
    ``cos <= threshold`` predicts 1 (mismatched)."""
    cos = torch.as_tensor(np.asarray(cos))
    thr = cos.median().item()
    pred = (cos <= thr).long()
    return (pred == torch.as_tensor(np.asarray(labels)).long()).float().mean().item()


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
class _Heads(torch.nn.Module):
    """The trainable part of a CLIPDetective, registered as transformers' CLIPModel registers it (logit_scale is
    a parameter of the model itself; the projections are bias-free Linear children), so ``parameters()`` yields
    them in the order the reference's optimizer holds them."""

    def __init__(self):
        super().__init__()
        self.clip = torch.nn.Module()
        self.clip.visual_projection = torch.nn.Linear(768, 512, bias=False)
        self.clip.text_projection = torch.nn.Linear(512, 512, bias=False)
        self.clip.logit_scale = torch.nn.Parameter(torch.zeros(()))


def flatten_heads(clip_state: Dict) -> torch.Tensor:
    """visual_projection.weight | text_projection.weight | logit_scale of a CLIPModel state dict, float32
    [655361]."""
    parts = [torch.as_tensor(np.asarray(_host(clip_state[k]), dtype=np.float32)).reshape(-1) for k in KEYS]
    flat = torch.cat(parts)
    if flat.numel() != N_PARAMS:
        raise ValueError(f"projection heads of {flat.numel()} parameters, expected {N_PARAMS}")
    return flat


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


def split_heads(flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    flat = flat.detach().cpu()
    return {KEYS[0]: flat[:N_VISUAL].reshape(512, 768).clone(),
            KEYS[1]: flat[N_VISUAL:N_VISUAL + N_TEXT].reshape(512, 512).clone(),
            KEYS[2]: flat[N_VISUAL + N_TEXT].reshape(()).clone()}


def optimizer_state_dict(exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, steps: int, lr: float, initial_lr: float,
                         weight_decay: float) -> dict:
    """The state dict the reference's ``AdamW([p for p in model.parameters() if p.requires_grad])`` would hold
    with these moments and step count: built by a real AdamW over a CLIPDetective-shaped module, so the
    parameter order is the module's own and the dict loads into one."""
    named = [(n[len("clip."):], p) for n, p in _Heads().named_parameters()]

    def in_module_order(flat):
        parts = split_heads(flat)
        return torch.cat([parts[n].reshape(-1) for n, _ in named])
    return TC.adamw_state_dict([p for _, p in named], in_module_order(exp_avg), in_module_order(exp_avg_sq), steps, lr,
                               initial_lr, weight_decay, device="cpu")


class ClipProjectionTrainer:
    """The training loop of train_clip_detective.py:358-398 on cached features: per epoch one training call and
    one validation call on the device."""

    def __init__(self, forensics, batch_size: int = 16, epochs: int = 10, lr: float = 1e-4,
                 weight_decay: float = 0.01, max_norm: float = 1.0, seed: int = 0):
        if not 1 <= int(batch_size) <= 64:
            raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
        self.forensics, self.batch_size, self.epochs = forensics, int(batch_size), int(epochs)
        self.lr, self.weight_decay, self.max_norm, self.seed = float(lr), float(weight_decay), float(max_norm), int(seed)

    @staticmethod
    def _feats(feats, what):
        img, txt = feats
        return TC.check_rows(what, (img, txt), (768, 512))

    def fit(self, train_feats, val_feats, val_labels, checkpoint_path: Optional[str] = None) -> List[dict]:
        f = self.forensics
        eng = f.engine
        dev = eng.device
        ti, tt = (torch.from_numpy(a).to(dev) for a in self._feats(train_feats, "training"))
        vi, vt = (torch.from_numpy(a).to(dev) for a in self._feats(val_feats, "validation"))
        labels = np.asarray(val_labels).astype(np.int64)
        if labels.shape != (vi.shape[0],):
            raise ValueError(f"val_labels {labels.shape} must be [{vi.shape[0]}]")
        N, bs = ti.shape[0], self.batch_size
        params = flatten_heads(f.clip_state).to(dev).contiguous()
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        steps_per_epoch = -(-N // bs)
        history, best_acc, best, step0 = [], 0.0, None, 0
        for epoch, (perm, lr) in enumerate(plan(N, self.epochs, self.lr, self.seed)):
            sl, _ = eng.clip_train_epoch(ti, tt, torch.from_numpy(perm).to(dev), bs, lr, BETAS, EPS,
                                         self.weight_decay, self.max_norm, step0, params, m, v)
            bl, cos = eng.clip_contrastive_eval(vi, vt, bs, params)
            step0 += steps_per_epoch
            train_loss = float(sl.cpu().numpy().astype(np.float64).mean())  # total_loss / len(dataloader) (:231)
            val_loss = float(bl.cpu().numpy().astype(np.float64).mean())
            cos = cos.cpu().numpy()
            if not (np.isfinite(train_loss) and np.isfinite(val_loss)):
                raise FloatingPointError(f"epoch {epoch + 1}: the loss is not finite")
            accs = [batch_accuracy(cos[a:a + bs], labels[a:a + bs]) for a in range(0, len(labels), bs)]
            val_acc = float(np.mean(accs))
            history.append({"epoch": epoch, "train_loss": train_loss, "val_loss": val_loss, "val_accuracy": val_acc,
                            "lr": lr})
            if val_acc > best_acc:  # :384
                best_acc, best = val_acc, split_heads(params)
                if checkpoint_path:
                    torch.save(self._checkpoint(history[-1], best, m, v, step0), checkpoint_path)
        self._install(best if best is not None else split_heads(params))
        return history

    def _checkpoint(self, entry: dict, heads: Dict[str, torch.Tensor], m, v, steps: int) -> dict:
        """The reference's checkpoint dict (:387-397) after the epoch of history entry `entry`, `steps` optimizer
        steps in.  The reference steps its scheduler before it saves (:379, :390): epoch + 1 steps, and the
        optimizer's group already holds the next epoch's learning rate."""
        sched = _scheduler_state(self.epochs, self.lr, entry["epoch"] + 1)
        return {"epoch": entry["epoch"],
                "model_state_dict": self._model_state(heads),
                "optimizer_state_dict": optimizer_state_dict(m, v, steps, float(sched["_last_lr"][0]), self.lr,
                                                             self.weight_decay),
                "scheduler_state_dict": sched,
                "val_loss": entry["val_loss"], "val_accuracy": entry["val_accuracy"],
                "train_loss": entry["train_loss"]}

    def _model_state(self, heads: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """CLIPDetective.state_dict(): the CLIPModel under ``clip.`` with the trained tensors."""
        sd = {}
        for k, val in self.forensics.clip_state.items():
            sd["clip." + k] = heads[k].clone() if k in heads else torch.as_tensor(np.array(_host(val)))
        return sd

    def _install(self, heads: Dict[str, torch.Tensor]) -> None:
        """The trained tensors into forensics.clip_state and the engine's towers; a loaded vault is set again
        through set_vault, so its title embeddings are recomputed with the new text projection."""
        f = self.forensics
        for k, val in heads.items():
            old = f.clip_state[k]
            f.clip_state[k] = val.clone() if isinstance(old, torch.Tensor) else val.numpy().astype(np.float32)
        f.engine.set_clip_projections(heads[KEYS[0]], heads[KEYS[1]])
        if getattr(f, "_emb_cache", None) is not None:
            f._emb_cache = None
        if getattr(f, "vault_loaded", False):
            f.set_vault(f.vault_embeddings, f.vault_metadata)


# ---------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------
LR_RANGE, BATCH_SIZES, EPOCH_RANGE = (1e-5, 1e-3), (8, 12, 16), (5, 15)  # train_clip_detective.py:281-283


def sample_trials(n_trials: int, seed: int = 0) -> List[dict]:
    """`n_trials` draws from the reference's search space: lr log-uniform in [1e-5, 1e-3], batch_size one of
    8 / 12 / 16, epochs an integer in 5..15, from ``numpy.random.default_rng(seed)``."""
    g = np.random.default_rng(int(seed))
    lo, hi = np.log(LR_RANGE[0]), np.log(LR_RANGE[1])
    out = []
    for _ in range(int(n_trials)):
        lr = float(np.clip(np.exp(g.uniform(lo, hi)), *LR_RANGE))
        out.append({"lr": lr, "batch_size": int(g.choice(BATCH_SIZES)),
                    "epochs": int(g.integers(EPOCH_RANGE[0], EPOCH_RANGE[1] + 1))})
    return out


class ClipProjectionTuner:
    """run_hyperparameter_tuning's study (train_clip_detective.py:427-454) on cached features.  Trials run in
    groups of up to 16; within a group, epoch e is one training call over the trials that still have an epoch e
    and one validation call.  Every trial starts from the forensics' current heads and follows its own
    ``plan(N, epochs, lr, seed)``; its bookkeeping is ``ClipProjectionTrainer.fit``'s, so its history is the one
    ``fit`` gives for it alone.  A trial's value is the validation loss at its best-accuracy epoch (:385, :424),
    ``inf`` when no epoch improved or a loss turned non-finite; the study minimises it, ties to the lower number."""

    def __init__(self, forensics, trials: Optional[Sequence[dict]] = None, n_trials: int = 10, seed: int = 0,
                 weight_decay: float = 0.01, max_norm: float = 1.0):
        self.forensics, self.seed = forensics, int(seed)
        self.weight_decay, self.max_norm = float(weight_decay), float(max_norm)
        self.trials = [dict(t) for t in (sample_trials(n_trials, seed) if trials is None else trials)]
        if not self.trials:
            raise ValueError("a study needs at least one trial")
        for i, t in enumerate(self.trials):
            if not (1 <= int(t["batch_size"]) <= 64 and int(t["epochs"]) >= 1 and float(t["lr"]) > 0):
                raise ValueError(f"trial {i}: batch_size in 1..64, epochs >= 1 and lr > 0 expected, got {t}")

    def _trainer(self, t: dict) -> ClipProjectionTrainer:
        """The single-trial trainer of a trial: its settings, and the checkpoint / install path."""
        return ClipProjectionTrainer(self.forensics, batch_size=t["batch_size"], epochs=t["epochs"], lr=t["lr"],
                                     weight_decay=t.get("weight_decay", self.weight_decay), max_norm=self.max_norm,
                                     seed=t.get("seed", self.seed))

    def tune(self, train_feats, val_feats, val_labels, checkpoint_path: Optional[str] = None) -> dict:
        dev = self.forensics.engine.device
        ti, tt = (torch.from_numpy(a).to(dev) for a in ClipProjectionTrainer._feats(train_feats, "training"))
        vi, vt = (torch.from_numpy(a).to(dev) for a in ClipProjectionTrainer._feats(val_feats, "validation"))
        labels = np.asarray(val_labels).astype(np.int64)
        if labels.shape != (vi.shape[0],):
            raise ValueError(f"val_labels {labels.shape} must be [{vi.shape[0]}]")
        start = flatten_heads(self.forensics.clip_state)
        runs = []
        for a in range(0, len(self.trials), TRIALS_MAX):
            runs += self._group([self._trainer(t) for t in self.trials[a:a + TRIALS_MAX]], start, ti, tt, vi, vt, labels)
        results = [{"number": i, "params": {k: t[k] for k in ("lr", "batch_size", "epochs")}, "value": r["value"],
                    "history": r["history"]} for i, (t, r) in enumerate(zip(self.trials, runs))]
        best = min(range(len(runs)), key=lambda i: (runs[i]["value"], i))
        snap = runs[best]["best"]
        if snap is not None:  # (none: no trial ever improved on accuracy 0, or every loss was non-finite)
            trainer = self._trainer(self.trials[best])
            heads = split_heads(snap["params"][:N_PARAMS])
            if checkpoint_path:
                torch.save(trainer._checkpoint(snap["entry"], heads, snap["m"][:N_PARAMS].cpu(),
                                               snap["v"][:N_PARAMS].cpu(), snap["steps"]), checkpoint_path)
            trainer._install(heads)
        return {"best_trial": best, "best_value": runs[best]["value"], "best_params": results[best]["params"],
                "trials": results}

    def _group(self, trainers: List[ClipProjectionTrainer], start: torch.Tensor, ti, tt, vi, vt, labels) -> List[dict]:
        """Up to 16 trials side by side -> per trial {history, value, best: the best epoch's device snapshot
        {params, m, v, steps, entry} or None}."""
        eng = self.forensics.engine
        dev = eng.device
        T, N = len(trainers), ti.shape[0]
        params = torch.zeros(T, TRIAL_STRIDE, dtype=torch.float32, device=dev)
        params[:, :N_PARAMS] = start.to(dev)
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        bs = [t.batch_size for t in trainers]
        plans = [plan(N, t.epochs, t.lr, t.seed) for t in trainers]
        steps_per_epoch = [-(-N // b) for b in bs]
        val_batches = [-(-len(labels) // b) for b in bs]
        step0 = [0] * T
        runs = [{"history": [], "value": float("inf"), "best": None, "best_acc": 0.0, "failed": False} for _ in trainers]
        for epoch in range(max(t.epochs for t in trainers)):
            active = [t.epochs > epoch and not r["failed"] for t, r in zip(trainers, runs)]
            if not any(active):
                break
            perm = np.zeros((T, N), np.int32)
            lr = [0.0] * T
            for t in range(T):
                if active[t]:
                    perm[t], lr[t] = plans[t][epoch]
            sl, _ = eng.clip_train_epoch_trials(ti, tt, torch.from_numpy(perm).to(dev), bs, lr, BETAS, EPS,
                                                [t.weight_decay for t in trainers], [t.max_norm for t in trainers],
                                                step0, params, m, v, active=active)
            bl, cos = eng.clip_contrastive_eval_trials(vi, vt, bs, params, active=active)
            sl, bl, cos = (x.cpu().numpy() for x in (sl, bl, cos))
            for t in range(T):
                if not active[t]:
                    continue
                step0[t] += steps_per_epoch[t]
                train_loss = float(sl[t, :steps_per_epoch[t]].astype(np.float64).mean())
                val_loss = float(bl[t, :val_batches[t]].astype(np.float64).mean())
                if not (np.isfinite(train_loss) and np.isfinite(val_loss)):  # fit raises; a study goes on
                    runs[t].update(failed=True, value=float("inf"), best=None)
                    continue
                accs = [batch_accuracy(cos[t, a:a + bs[t]], labels[a:a + bs[t]]) for a in range(0, len(labels), bs[t])]
                entry = {"epoch": epoch, "train_loss": train_loss, "val_loss": val_loss,
                         "val_accuracy": float(np.mean(accs)), "lr": lr[t]}
                runs[t]["history"].append(entry)
                if entry["val_accuracy"] > runs[t]["best_acc"]:  # :384
                    runs[t].update(best_acc=entry["val_accuracy"], value=val_loss,
                                   best={"params": params[t].clone(), "m": m[t].clone(), "v": v[t].clone(),
                                         "steps": step0[t], "entry": entry})
        return runs


# ---------------------------------------------------------------------------------------------
# the script's entry points
# ---------------------------------------------------------------------------------------------
def _load_study_data(train_csv: str, val_csv: str, forensics, device: str, max_samples: Optional[int]):
    """The script's data (train_clip_detective.py:300-330): training rows are the matched pairs (``label == 0``,
    :319), validation uses every row (:322); one feature extraction per file.
    -> (forensics, train_feats, val_feats, val_labels), or None when a CSV is missing."""
    import pandas as pd
    for p in (train_csv, val_csv):
        if not os.path.exists(p):
            print(f"✗ Error: {p} not found!")
            return None
    if forensics is None:
        from .api import MisinfoForensics
        forensics = MisinfoForensics(device=device)
    tr, va = pd.read_csv(train_csv), pd.read_csv(val_csv)
    total = len(tr)
    tr = tr[tr["label"] == 0].reset_index(drop=True)
    print(f"  Filtered to {len(tr)} matched pairs (from {total} total)")
    if max_samples:
        tr, va = tr.head(max_samples), va.head(max_samples)
    print(f"Train samples: {len(tr)}")
    print(f"Val samples: {len(va)}")
    train_feats = extract_features(forensics, [str(t) for t in tr["text"]], [str(p) for p in tr["image_path"]])
    val_feats = extract_features(forensics, [str(t) for t in va["text"]], [str(p) for p in va["image_path"]])
    return forensics, train_feats, val_feats, [int(x) for x in va["label"]]


def train_clip_detective(train_csv: str = "clip_train.csv", val_csv: str = "clip_val.csv", batch_size: int = 16,
                         epochs: int = 10, lr: float = 1e-4, device: str = "cuda", *, forensics=None, seed: int = 0,
                         checkpoint_path: str = "clip_detective_best.pth", max_samples: Optional[int] = None):
    """train_clip_detective.py:276-424 without the Optuna branch (run_hyperparameter_tuning below): the script's
    data, then the trainer.  Returns the history (None when a CSV is missing)."""
    data = _load_study_data(train_csv, val_csv, forensics, device, max_samples)
    if data is None:
        return None
    forensics, train_feats, val_feats, labels = data
    trainer = ClipProjectionTrainer(forensics, batch_size=batch_size, epochs=epochs, lr=lr, seed=seed)
    history = trainer.fit(train_feats, val_feats, labels, checkpoint_path=checkpoint_path)
    for h in history:
        print(f"Epoch {h['epoch'] + 1}/{epochs}  Train Loss: {h['train_loss']:.4f}  Val Loss: {h['val_loss']:.4f} | "
              f"Val Acc: {h['val_accuracy']:.4f}  Learning Rate: {h['lr']:.2e}")
    return history


def run_hyperparameter_tuning(n_trials: int = 10, train_csv: str = "clip_train.csv", val_csv: str = "clip_val.csv", *,
                              forensics=None, seed: int = 0, checkpoint_path: str = "clip_detective_best.pth",
                              device: str = "cuda", max_samples: Optional[int] = None):
    """run_hyperparameter_tuning (train_clip_detective.py:432-454): `n_trials` draws of ``sample_trials`` on one
    feature extraction for the whole study; prints what the reference prints of its study and returns the
    tuner's result (None when a CSV is missing)."""
    print(f"Number of trials: {n_trials}")
    data = _load_study_data(train_csv, val_csv, forensics, device, max_samples)
    if data is None:
        return None
    forensics, train_feats, val_feats, labels = data
    res = ClipProjectionTuner(forensics, n_trials=n_trials, seed=seed).tune(train_feats, val_feats, labels,
                                                                            checkpoint_path=checkpoint_path)
    print(f"Best trial: {res['best_trial']}")
    print(f"Best val loss: {res['best_value']:.4f}")
    print("Best hyperparameters:")
    for key, value in res["best_params"].items():
        print(f"  {key}: {value}")
    return res


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m mmf_amd.clip_training",
                                 description="Train CLIPDetective's projection heads")
    ap.add_argument("--train-csv", default="clip_train.csv", help="training CSV (text, image_path, label)")
    ap.add_argument("--val-csv", default="clip_val.csv", help="validation CSV (text, image_path, label)")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--checkpoint", default="clip_detective_best.pth")
    ap.add_argument("--tune", action="store_true", help="run the hyperparameter study instead of one training")
    ap.add_argument("--trials", type=int, default=10, help="number of trials of the study")
    a = ap.parse_args(argv)
    if a.tune:
        run_hyperparameter_tuning(n_trials=a.trials, train_csv=a.train_csv, val_csv=a.val_csv,
                                  checkpoint_path=a.checkpoint)
        return
    train_clip_detective(train_csv=a.train_csv, val_csv=a.val_csv, batch_size=a.batch_size, epochs=a.epochs, lr=a.lr,
                         checkpoint_path=a.checkpoint)


if __name__ == "__main__":
    main()
