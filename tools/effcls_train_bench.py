"""Deepfake-classifier training on the device against the reference's way (train_cifake_forensics.py), on one box.

    python tools/effcls_train_bench.py [--rows 512] [--train-rows 4000] [--epochs 10] [--out FILE]

Prints one JSON object:

  extract  rows/s of extract_image_features on `--rows` 32 x 32 JPEG files (CIFAKE's size), one view and two views.
  train    microseconds per optimizer step at batch 16 on `--train-rows` cached pooled rows (a two-view bank of twice
           as many): mmf_effcls_train_epoch (ONE launch per epoch, timed by device events over `--epochs` epochs, and
           by the host clock to a synchronise) against the loop body of train_cifake_forensics.py:187-216 restated
           in torch for the deployed classifier on the SAME cached rows on the same device (autocast + GradScaler +
           Adam + loss.item() + torch.max; host clock around a loop that ends in a synchronise), both after a
           warm-up epoch: the step-only comparison.  `eval_us_per_batch`: the validation call.
  tower    what the reference does in addition per minibatch -- the EfficientNet forward on 16 images -- as this
           package's own HIP tower takes for it (effnet_pooled, device events): the part of a step that caching the
           features removes.  The reference's torch tower (and its backward through it) is not timed here.
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


def _forensics():
    from mmf_amd.api import MisinfoForensics
    return MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, verbose=False)


def _events():
    return [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def bench_extract(mf, n_rows):
    import mmf_amd.cifake_training as CT
    from PIL import Image
    g = np.random.default_rng(5)
    out = {"rows": n_rows, "image": "32x32 JPEG"}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(n_rows):
            paths.append(os.path.join(d, f"{i:05d}.jpg"))
            Image.fromarray(g.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(paths[-1], quality=92)
        warm = min(n_rows, mf.engine.max_batch)
        CT.extract_image_features(mf, paths[:warm], flip=True)
        for flip, key in ((False, "one_view_rows_per_s"), (True, "two_views_rows_per_s")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = CT.extract_image_features(mf, paths, flip=flip)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res[-1].all() and np.isfinite(res[0]).all()
            out[key] = round(n_rows / dt, 1)
    return out


def bench_train(mf, n_rows, epochs, batch=16, lr=1e-4):
    import torch.nn as nn
    import mmf_amd.cifake_training as CT
    eng, dev = mf.engine, mf.engine.device
    g = np.random.default_rng(7)
    x = (0.4 * np.abs(g.standard_normal((2 * n_rows, 1280)))).astype(np.float32)
    y = ((x[:n_rows] - x[:n_rows].mean(0)) @ g.standard_normal(1280) > 0).astype(np.int32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(np.concatenate([y, y])).to(dev)
    steps = -(-n_rows // batch)
    # ---- the kernel: one launch per epoch
    plans = [(torch.from_numpy(p).to(dev), torch.from_numpy(k.view(np.int64)).to(dev))
             for p, k, _ in CT.plan(n_rows, batch, epochs + 1, 0, True)]
    params = CT.flatten_classifier(mf.detector).to(dev).contiguous()
    p0 = params.clone()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step0 = 0

    def run(e):
        nonlocal step0
        out = eng.effcls_train_epoch(xd, yd, plans[e][0], plans[e][1], CT.P_DROP, batch, lr, CT.BETAS, CT.EPS, 0.0, step0,
                                     params, m, v)
        step0 += steps
        return out
    first = run(0)[0]
    torch.cuda.synchronize()
    ev = _events()
    t0 = time.perf_counter()
    ev[0].record()
    for e in range(1, epochs + 1):
        sl, sc = run(e)
    ev[1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kernel_us = 1e3 * ev[0].elapsed_time(ev[1]) / (epochs * steps)
    assert torch.isfinite(sl).all()
    xv, yv = xd[:n_rows], yd[:n_rows]
    eng.effcls_eval(xv, yv, batch, params)
    torch.cuda.synchronize()
    ev = _events()
    ev[0].record()
    eng.effcls_eval(xv, yv, batch, params)
    ev[1].record()
    torch.cuda.synchronize()
    eval_us = 1e3 * ev[0].elapsed_time(ev[1]) / steps
    # ---- the reference's loop body on the same device and the same cached rows, for the deployed classifier
    from torch.cuda.amp import GradScaler, autocast
    net = nn.Sequential(nn.Dropout(0.2), nn.Linear(1280, 2)).to(dev)
    with torch.no_grad():
        net[1].weight.copy_(p0[:2560].reshape(2, 1280))
        net[1].bias.copy_(p0[2560:])
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    t_epochs = max(1, min(epochs, 3))
    criterion = nn.CrossEntropyLoss()
    yl = yd.long()

    def torch_epoch(scaler):
        net.train()
        total_loss, correct, total = 0.0, 0, 0
        perm = torch.randperm(n_rows, device=dev)
        for s in range(steps):
            idx = perm[s * batch:(s + 1) * batch]
            labels = yl[idx]
            opt.zero_grad()
            with autocast():
                logits = net(xd[idx])
                loss = criterion(logits, labels)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            total_loss += loss.item()
            _, predicted = torch.max(logits, 1)
            correct += (predicted == labels).sum().item()
            total += labels.size(0)
        return total_loss / steps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaler = GradScaler()
        torch_epoch(scaler)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(t_epochs):
            last = torch_epoch(scaler)
        torch.cuda.synchronize()
        torch_us = 1e6 * (time.perf_counter() - t0) / (t_epochs * steps)
    return {"rows": n_rows, "bank_rows": 2 * n_rows, "batch": batch, "steps_per_epoch": steps, "epochs_timed": epochs,
            "launches_per_epoch": 1, "kernel_us_per_step": round(kernel_us, 3),
            "kernel_wall_us_per_step": round(1e6 * wall / (epochs * steps), 3), "eval_us_per_batch": round(eval_us, 3),
            "torch_loop_us_per_step": round(torch_us, 1), "torch_epochs_timed": t_epochs,
            "ratio": round(torch_us / kernel_us, 2), "first_epoch_loss": round(float(first.mean()), 4),
            "last_epoch_loss": round(float(sl.mean()), 4), "torch_last_epoch_loss": round(last, 4)}


def bench_tower(mf, batch=16, reps=20):
    import mmf_amd.synthetic as syn
    eng = mf.engine
    img = eng._u8(syn.images(batch, 3))
    eng.effnet_pooled(img)
    torch.cuda.synchronize()
    ev = _events()
    ev[0].record()
    for _ in range(reps):
        eng.effnet_pooled(img)
    ev[1].record()
    torch.cuda.synchronize()
    return {"batch": batch, "effnet_pooled_us_per_call": round(1e3 * ev[0].elapsed_time(ev[1]) / reps, 1),
            "fp32_tower": eng.get_option("effnet_fp32"), "note": "includes the overflow trap's read-back per call"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512, help="images of the extraction measurement")
    ap.add_argument("--train-rows", type=int, default=4000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("effcls_train_bench needs a HIP device")
    mf = _forensics()
    res = {"extract": bench_extract(mf, a.rows), "train": bench_train(mf, a.train_rows, a.epochs),
           "tower": bench_tower(mf)}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
