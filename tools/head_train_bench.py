"""Text-head training on the device against the reference's way (train_ai_head.py), on one box.

    python tools/head_train_bench.py [--rows 512] [--train-rows 2048] [--epochs 10] [--out FILE]

Prints one JSON object:

  train    microseconds per optimizer step at batch 16 on `--train-rows` cached CLS rows: mmf_head_train_epoch (four
           launches per step, timed by device events over `--epochs` epochs) against the loop body of
           train_ai_head.py:215-241 restated in torch for the deployed head on the SAME cached rows on the same
           device (autocast + GradScaler + clip_grad_norm_ + AdamW + the per-step warmup-cosine scheduler +
           loss.item() + argmax; host clock around a loop that ends in a synchronise), both after a warm-up epoch:
           the step-only comparison.  `eval_us_per_batch`: the validation call.
  tower    what the reference does in addition per minibatch -- the 12-layer RoBERTa forward on 16 rows of 256
           tokens -- as this package's own HIP tower takes for it (text_pooled, device events): the part of a
           step that caching the features removes.  The reference's torch tower is not timed here.
  extract  rows/s of extract_text_features on texts of 256 tokens.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _forensics(n):
    import mmf_amd.synthetic as syn
    from mmf_amd.api import MisinfoForensics
    texts, rob, _ = syn.text_tables(n, 77, rob_len=256)
    mf = MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, roberta_tokenizer=rob,
                          max_text_len=256, verbose=False)
    return mf, texts


def _events():
    return [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def bench_train(mf, n_rows, epochs, batch=16, lr=1e-3):
    import torch.nn as nn
    from transformers import get_cosine_schedule_with_warmup
    import mmf_amd.head_training as HT
    eng, dev = mf.engine, mf.engine.device
    g = np.random.default_rng(7)
    x = g.standard_normal((n_rows, 768)).astype(np.float32)
    y = (x @ g.standard_normal(768) > 0).astype(np.int32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    steps = -(-n_rows // batch)
    # ---- the kernels: four launches per step
    plans = [(torch.from_numpy(p).to(dev), torch.from_numpy(k.view(np.int64)).to(dev), lrs)
             for p, k, lrs in HT.plan(n_rows, batch, epochs + 1, lr, 0)]
    params = HT.flatten_head(mf.detector.ai_head).to(dev).contiguous()
    p0 = params.clone()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step0 = 0

    def run(e):
        nonlocal step0
        out = eng.head_train_epoch(xd, yd, plans[e][0], plans[e][1], HT.P_DROP, batch, plans[e][2], HT.BETAS, HT.EPS,
                                   0.01, 1.0, step0, params, m, v)
        step0 += steps
        return out
    first = run(0)[0]
    torch.cuda.synchronize()
    ev = _events()
    t0 = time.perf_counter()
    ev[0].record()
    for e in range(1, epochs + 1):
        sl, sc, sg = run(e)
    ev[1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kernel_us = 1e3 * ev[0].elapsed_time(ev[1]) / (epochs * steps)
    assert torch.isfinite(sl).all() and torch.isfinite(sg).all()
    eng.head_eval(xd, yd, batch, params)
    torch.cuda.synchronize()
    ev = _events()
    ev[0].record()
    eng.head_eval(xd, yd, batch, params)
    ev[1].record()
    torch.cuda.synchronize()
    eval_us = 1e3 * ev[0].elapsed_time(ev[1]) / steps
    # ---- the reference's loop body on the same device and the same cached rows, for the deployed head
    from torch.cuda.amp import GradScaler, autocast
    net = nn.Sequential(nn.Linear(768, 256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 2)).to(dev)
    with torch.no_grad():
        for p, src in zip(net.parameters(), HT._split(p0, list(net.parameters()))):
            p.copy_(src)
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=0.01)
    t_epochs = max(1, min(epochs, 3))
    total = steps * (t_epochs + 1)
    sched = get_cosine_schedule_with_warmup(opt, int(total * 0.1), total)
    criterion = nn.CrossEntropyLoss()
    yl = yd.long()

    def torch_epoch(scaler):
        net.train()
        total_loss, correct = 0.0, 0
        perm = torch.randperm(n_rows, device=dev)
        for s in range(steps):
            idx = perm[s * batch:(s + 1) * batch]
            opt.zero_grad()
            with autocast():
                logits = net(xd[idx])
                loss = criterion(logits, yl[idx])
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            scaler.step(opt)
            scaler.update()
            sched.step()
            total_loss += loss.item()
            correct += (torch.argmax(logits, dim=-1) == yl[idx]).sum().item()
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
    return {"rows": n_rows, "batch": batch, "steps_per_epoch": steps, "epochs_timed": epochs, "launches_per_step": 4,
            "kernel_us_per_step": round(kernel_us, 3), "kernel_wall_us_per_step": round(1e6 * wall / (epochs * steps), 3),
            "eval_us_per_batch": round(eval_us, 3), "torch_loop_us_per_step": round(torch_us, 1),
            "torch_epochs_timed": t_epochs, "ratio": round(torch_us / kernel_us, 2),
            "first_epoch_loss": round(float(first.mean()), 4), "last_epoch_loss": round(float(sl.mean()), 4),
            "torch_last_epoch_loss": round(last, 4)}


def bench_tower(mf, batch=16, L=256, reps=20):
    import mmf_amd.synthetic as syn
    eng = mf.engine
    ids, mask = syn.roberta_ids(batch, L, 3)
    ids, mask = eng._i32(ids), eng._i32(mask)
    eng.text_pooled(ids, mask)
    torch.cuda.synchronize()
    ev = _events()
    ev[0].record()
    for _ in range(reps):
        eng.text_pooled(ids, mask)
    ev[1].record()
    torch.cuda.synchronize()
    return {"batch": batch, "tokens": L, "text_pooled_us_per_call": round(1e3 * ev[0].elapsed_time(ev[1]) / reps, 1),
            "layout": eng.get_option("text_hilo_effective"), "note": "includes the overflow trap's read-back per call"}


def bench_extract(mf, texts, n_rows):
    import mmf_amd.head_training as HT
    warm = min(n_rows, mf.engine.max_batch)
    HT.extract_text_features(mf, texts[:warm], max_length=256)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fe = HT.extract_text_features(mf, texts[:n_rows], max_length=256)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(fe).all()
    return {"rows": n_rows, "tokens": 256, "extract_text_features_rows_per_s": round(n_rows / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512, help="rows of the extraction measurement")
    ap.add_argument("--train-rows", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_train_bench needs a HIP device")
    mf, texts = _forensics(a.rows)
    res = {"train": bench_train(mf, a.train_rows, a.epochs), "tower": bench_tower(mf),
           "extract": bench_extract(mf, texts, a.rows)}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
