"""Fusion training on the device against the reference's way (train_fusion_judge.py), on one box.

    python tools/fusion_train_bench.py [--rows 1024] [--train-rows 4096] [--epochs 20] [--out FILE]

Prints one JSON object with two pairs of numbers:

  train    microseconds per optimizer step at batch 16: mmf_fusion_train_epoch (one launch per epoch, timed by
           device events over `--epochs` epochs) against the loop body of train_fusion_judge.py:213-233 on the same
           device and the same scores (autocast + GradScaler + AdamW + the .item() statistics; host clock around
           a loop that ends in a synchronise), both after a warm-up epoch;
  extract  rows/s of extract_scores (one batched five-signal pass over JPEG files) against the per-row four-call
           extraction of FusionTrainingDataset.__getitem__ on the same files (the path bench.py reports as
           per_sample.fusion_dataset_rows, there on images already in memory).
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _forensics(n):
    import mmf_amd.synthetic as syn
    from mmf_amd.api import MisinfoForensics
    texts, rob, clp = syn.text_tables(n, 77)
    tid, tm = syn.clip_ids(2170, 77, 99, np.random.default_rng(5).integers(3, 78, 2170).tolist())
    meta = []
    for j in range(2170):
        clp.table[f"title {j}"] = tid[j, :int(tm[j].sum())].tolist()
        meta.append({"title": f"title {j}", "url": "N/A", "date": "N/A"})
    mf = MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, roberta_tokenizer=rob,
                          clip_processor=clp, verbose=False)
    mf.set_vault(syn.vault(2170, 512, 77), meta)
    return mf, texts


def bench_train(mf, n_rows, epochs, batch=16, lr=1e-3):
    import torch.nn as nn
    import mmf_amd.fusion_training as FT
    import mmf_amd.synthetic as syn
    eng, dev = mf.engine, mf.engine.device
    x = syn.fusion_inputs(n_rows, 7)
    y = (np.random.default_rng(7).uniform(size=n_rows) < 0.5).astype(np.int32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    steps = -(-n_rows // batch)
    # ---- the kernel: one launch per epoch
    plans = [(torch.from_numpy(p).to(dev), torch.from_numpy(k.view(np.int64)).to(dev), lr_e)
             for p, k, lr_e in FT.plan(n_rows, batch, epochs + 1, lr, 0)]
    params = FT.flatten_fusion(mf.detector.fusion_layer).to(dev).contiguous()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step0 = 0

    def run(e):
        nonlocal step0
        out = eng.fusion_train_epoch(xd, yd, plans[e][0], plans[e][1], FT.P_DROP, batch, plans[e][2], FT.BETAS, FT.EPS,
                                     0.01, step0, params, m, v)
        step0 += steps
        return out
    run(0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    ev[0].record()
    for e in range(1, epochs + 1):
        sl, sc = run(e)
    ev[1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kernel_us = 1e3 * ev[0].elapsed_time(ev[1]) / (epochs * steps)
    assert torch.isfinite(sl).all()
    # ---- the reference's loop body on the same device and scores (train_fusion_judge.py:213-233)
    from torch.cuda.amp import GradScaler, autocast
    det = mf.detector
    det.fusion_layer.train()
    opt = torch.optim.AdamW(det.fusion_layer.parameters(), lr=lr, weight_decay=0.01)
    crit = nn.CrossEntropyLoss()
    yl = yd.long()

    def torch_epoch(scaler):
        running_loss, correct, total = 0.0, 0, 0
        perm = torch.randperm(n_rows, device=dev)
        for s in range(steps):
            idx = perm[s * batch:(s + 1) * batch]
            scores, labels = xd[idx], yl[idx]
            opt.zero_grad()
            with autocast():
                logits = det.forward_fusion(scores)
                loss = crit(logits, labels)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            running_loss += loss.item() * scores.size(0)
            _, predicted = torch.max(logits, 1)
            total += labels.size(0)
            correct += (predicted == labels).sum().item()
        return running_loss / total
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        scaler = GradScaler()
        torch_epoch(scaler)
        torch.cuda.synchronize()
        t_epochs = max(1, min(epochs, 3))
        t0 = time.perf_counter()
        for _ in range(t_epochs):
            torch_epoch(scaler)
        torch.cuda.synchronize()
        torch_us = 1e6 * (time.perf_counter() - t0) / (t_epochs * steps)
    det.fusion_layer.eval()
    return {"rows": n_rows, "batch": batch, "steps_per_epoch": steps, "epochs_timed": epochs,
            "kernel_us_per_step": round(kernel_us, 3), "kernel_wall_us_per_step": round(1e6 * wall / (epochs * steps), 3),
            "torch_loop_us_per_step": round(torch_us, 1), "torch_epochs_timed": t_epochs,
            "ratio": round(torch_us / kernel_us, 1)}


def bench_extract(mf, texts, n_rows, per_row_rows):
    from PIL import Image
    import mmf_amd.fusion_training as FT
    import mmf_amd.synthetic as syn
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, a in enumerate(syn.images(n_rows, 77)):
            paths.append(os.path.join(d, f"img{i}.jpg"))
            Image.fromarray(a).save(paths[-1], quality=90)
        warm = min(n_rows, mf.engine.max_batch)
        FT.extract_scores(mf, texts[:warm], paths[:warm])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores, ok = FT.extract_scores(mf, texts[:n_rows], paths)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert ok.all()
        for i in range(10):
            FT._row_scores(mf, texts[i], paths[i])
        t0 = time.perf_counter()
        rows = np.array([FT._row_scores(mf, texts[i], paths[i]) for i in range(per_row_rows)], np.float32)
        dt_row = time.perf_counter() - t0
    return {"rows": n_rows, "extract_scores_rows_per_s": round(n_rows / dt, 1),
            "per_row_rows_per_s": round(per_row_rows / dt_row, 1), "per_row_rows": per_row_rows,
            "ratio": round((n_rows / dt) / (per_row_rows / dt_row), 1),
            "max_abs_diff": float(np.abs(scores[:per_row_rows] - rows).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024, help="rows of the extraction comparison")
    ap.add_argument("--per-row-rows", type=int, default=128)
    ap.add_argument("--train-rows", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fusion_train_bench needs a HIP device")
    mf, texts = _forensics(a.rows)
    res = {"train": bench_train(mf, a.train_rows, a.epochs),
           "extract": bench_extract(mf, texts, a.rows, min(a.per_row_rows, a.rows))}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
