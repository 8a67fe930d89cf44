"""Projection-head training on the device against the reference's way (train_clip_detective.py), on one box.

    python tools/clip_train_bench.py [--rows 512] [--train-rows 2048] [--epochs 10] [--out FILE]

Prints one JSON object:

  train    microseconds per optimizer step at batch 16 on `--train-rows` cached rows: mmf_clip_train_epoch (six
           launches per step, timed by device events over `--epochs` epochs) against the loop body of
           train_clip_detective.py:203-225 restated in torch on the SAME cached features on the same device
           (autocast + GradScaler + clip_grad_norm_ + AdamW + loss.item(); host clock around a loop that ends in a
           synchronise), both after a warm-up epoch: the step-only comparison.  `eval_us_per_batch`: the validation
           call.
  tune     the study's launches (mmf_clip_train_epoch_trials): microseconds per step-of-all-trials at batch 16 on the
           same cached rows for T = 1, 4, 10 and 16 concurrent trials, against T sequential single-trial epochs
           through mmf_clip_train_epoch in the same process, both by device events after a warm-up epoch,
           interleaved over three rounds (`*_us_per_step`: the rounds; `ratio`: sequential / concurrent of the
           medians; `spread`: (max - min) / median of the rounds, the larger of the two sides).  `mixed`: one group
           of nine trials with batch sizes 8 / 12 / 16 (256 steps, the 12s and 16s finishing early) per epoch,
           against the nine epochs one after another.
  towers   what the reference does in addition per minibatch -- both 12-layer towers forward on 16 rows -- as
           this package's own HIP towers take for it (clip_pooled at batch 16, device events): the part of a step
           that caching the features removes.  The reference's torch towers are not timed here.
  extract  rows/s of extract_features on text + 224x224 JPEG files.
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
    mf = MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, roberta_tokenizer=rob,
                          clip_processor=clp, verbose=False)
    return mf, texts


def _events():
    return [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def bench_train(mf, n_rows, epochs, batch=16, lr=1e-4):
    import torch.nn as nn
    import mmf_amd.clip_training as CT
    eng, dev = mf.engine, mf.engine.device
    g = np.random.default_rng(7)
    img = g.standard_normal((n_rows, 768)).astype(np.float32)
    txt = (0.7 * g.standard_normal((n_rows, 512)) + 0.7 * img[:, :512]).astype(np.float32)
    ti, tt = torch.from_numpy(img).to(dev), torch.from_numpy(txt).to(dev)
    steps = -(-n_rows // batch)
    # ---- the kernels: six launches per step
    plans = [(torch.from_numpy(p).to(dev), lr_e) for p, lr_e in CT.plan(n_rows, epochs + 1, lr, 0)]
    params = CT.flatten_heads(mf.clip_state).to(dev).contiguous()
    p0 = params.clone()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step0 = 0

    def run(e):
        nonlocal step0
        out = eng.clip_train_epoch(ti, tt, plans[e][0], batch, plans[e][1], CT.BETAS, CT.EPS, 0.01, 1.0, step0, params,
                                   m, v)
        step0 += steps
        return out
    first = run(0)[0]
    torch.cuda.synchronize()
    ev = _events()
    t0 = time.perf_counter()
    ev[0].record()
    for e in range(1, epochs + 1):
        sl, sg = run(e)
    ev[1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kernel_us = 1e3 * ev[0].elapsed_time(ev[1]) / (epochs * steps)
    assert torch.isfinite(sl).all() and torch.isfinite(sg).all()
    eng.clip_contrastive_eval(ti, tt, batch, params)
    torch.cuda.synchronize()
    ev = _events()
    ev[0].record()
    eng.clip_contrastive_eval(ti, tt, batch, params)
    ev[1].record()
    torch.cuda.synchronize()
    eval_us = 1e3 * ev[0].elapsed_time(ev[1]) / steps
    # ---- the reference's loop body on the same device and the same cached features
    from torch.cuda.amp import GradScaler, autocast

    class Heads(nn.Module):
        def __init__(self):
            super().__init__()
            self.visual_projection = nn.Linear(768, 512, bias=False)
            self.text_projection = nn.Linear(512, 512, bias=False)
            self.logit_scale = nn.Parameter(torch.zeros(()))
    net = Heads().to(dev)
    with torch.no_grad():
        h = CT.split_heads(p0)
        net.visual_projection.weight.copy_(h[CT.KEYS[0]])
        net.text_projection.weight.copy_(h[CT.KEYS[1]])
        net.logit_scale.copy_(h[CT.KEYS[2]])
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=0.01)

    def torch_epoch(scaler):
        total = 0.0
        perm = torch.randperm(n_rows, device=dev)
        for s in range(steps):
            idx = perm[s * batch:(s + 1) * batch]
            opt.zero_grad()
            with autocast():
                ie, te = net.visual_projection(ti[idx]), net.text_projection(tt[idx])
                ie = ie / ie.norm(dim=-1, keepdim=True)
                te = te / te.norm(dim=-1, keepdim=True)
                logits = net.logit_scale.exp() * ie @ te.t()
                target = torch.arange(idx.shape[0], device=dev)
                loss = (nn.functional.cross_entropy(logits, target) + nn.functional.cross_entropy(logits.t(), target)) / 2
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            scaler.step(opt)
            scaler.update()
            total += loss.item()
        return total / steps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        scaler = GradScaler()
        torch_epoch(scaler)
        torch.cuda.synchronize()
        t_epochs = max(1, min(epochs, 3))
        t0 = time.perf_counter()
        for _ in range(t_epochs):
            last = torch_epoch(scaler)
        torch.cuda.synchronize()
        torch_us = 1e6 * (time.perf_counter() - t0) / (t_epochs * steps)
    return {"rows": n_rows, "batch": batch, "steps_per_epoch": steps, "epochs_timed": epochs, "launches_per_step": 6,
            "kernel_us_per_step": round(kernel_us, 3), "kernel_wall_us_per_step": round(1e6 * wall / (epochs * steps), 3),
            "eval_us_per_batch": round(eval_us, 3), "torch_loop_us_per_step": round(torch_us, 1),
            "torch_epochs_timed": t_epochs, "ratio": round(torch_us / kernel_us, 2),
            "first_epoch_loss": round(float(first.mean()), 4), "last_epoch_loss": round(float(sl.mean()), 4),
            "torch_last_epoch_loss": round(last, 4)}


def bench_tune(mf, n_rows, batch=16, rounds=3, reps=10, lr=1e-4):
    import mmf_amd.clip_training as CT
    eng, dev = mf.engine, mf.engine.device
    g = np.random.default_rng(7)
    img = g.standard_normal((n_rows, 768)).astype(np.float32)
    txt = (0.7 * g.standard_normal((n_rows, 512)) + 0.7 * img[:, :512]).astype(np.float32)
    ti, tt = torch.from_numpy(img).to(dev), torch.from_numpy(txt).to(dev)
    TM = CT.TRIALS_MAX
    start = CT.flatten_heads(mf.clip_state).to(dev)
    perms = torch.stack([torch.randperm(n_rows, generator=torch.Generator().manual_seed(t)).to(torch.int32)
                         for t in range(TM)]).to(dev)
    lrs = [lr * (1 + 0.1 * t) for t in range(TM)]

    def fresh():
        p = torch.zeros(TM, CT.TRIAL_STRIDE, dtype=torch.float32, device=dev)
        p[:, :CT.N_PARAMS] = start
        return p, torch.zeros_like(p), torch.zeros_like(p)

    def timed(fn):
        ev = _events()
        ev[0].record()
        for _ in range(reps):
            out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        assert not any(torch.isinf(o).any() for o in out)  # (NaN: the padding of a trial with fewer steps)
        return 1e3 * ev[0].elapsed_time(ev[1]) / reps  # microseconds per epoch of all trials

    def concurrent(state, bs):
        T = len(bs)
        p, m, v = (x[:T] for x in state)
        return lambda: eng.clip_train_epoch_trials(ti, tt, perms[:T], bs, lrs[:T], CT.BETAS, CT.EPS, [0.01] * T,
                                                   [1.0] * T, [0] * T, p, m, v)

    def sequential(state, bs):
        p, m, v = state

        def run():
            for t, b in enumerate(bs):
                out = eng.clip_train_epoch(ti, tt, perms[t], b, lrs[t], CT.BETAS, CT.EPS, 0.01, 1.0, 0,
                                           p[t, :CT.N_PARAMS], m[t, :CT.N_PARAMS], v[t, :CT.N_PARAMS])
            return out
        return run

    groups = {f"T{T}": [batch] * T for T in (1, 4, 10, 16)}
    groups["mixed"] = [8, 12, 16] * 3
    runs = {k: (concurrent(fresh(), bs), sequential(fresh(), bs)) for k, bs in groups.items()}
    for con, seq in runs.values():  # the warm-up epoch of every group, both ways
        con()
        seq()
    torch.cuda.synchronize()
    times = {k: ([], []) for k in groups}
    for _ in range(rounds):
        for k, (con, seq) in runs.items():
            times[k][0].append(timed(con))
            times[k][1].append(timed(seq))
    out = {"rows": n_rows, "batch": batch, "rounds": rounds, "epochs_per_timing": reps}
    for k, bs in groups.items():
        steps = max(-(-n_rows // b) for b in bs)
        con, seq = (np.array(x) for x in times[k])
        spread = max(float((x.max() - x.min()) / np.median(x)) for x in (con, seq))
        out[k] = {"trials": len(bs), "batch_sizes": sorted(set(bs)), "steps_of_all_trials": steps,
                  "concurrent_us_per_step": [round(float(x) / steps, 2) for x in con],
                  "sequential_us_per_step": [round(float(x) / steps, 2) for x in seq],
                  "ratio": round(float(np.median(seq) / np.median(con)), 3), "spread": round(spread, 4)}
    return out


def bench_towers(mf, batch=16, reps=20):
    import mmf_amd.synthetic as syn
    eng = mf.engine
    imgs = torch.from_numpy(syn.images(batch, 3)).to(eng.device)
    cid, cm = syn.clip_ids(batch, 77, 3)
    eng.clip_pooled(imgs, cid, cm)
    torch.cuda.synchronize()
    cid, cm = eng._i32(cid), eng._i32(cm)
    ev = _events()
    ev[0].record()
    for _ in range(reps):
        eng.clip_pooled(imgs, cid, cm)
    ev[1].record()
    torch.cuda.synchronize()
    return {"batch": batch, "clip_pooled_us_per_call": round(1e3 * ev[0].elapsed_time(ev[1]) / reps, 1),
            "note": "includes the overflow trap's read-back per call"}


def bench_extract(mf, texts, n_rows):
    from PIL import Image
    import mmf_amd.clip_training as CT
    import mmf_amd.synthetic as syn
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, a in enumerate(syn.images(n_rows, 77)):
            paths.append(os.path.join(d, f"img{i}.jpg"))
            Image.fromarray(a).save(paths[-1], quality=90)
        warm = min(n_rows, mf.engine.max_batch)
        CT.extract_features(mf, texts[:warm], paths[:warm])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fi, ft = CT.extract_features(mf, texts[:n_rows], paths)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert np.isfinite(fi).all() and np.isfinite(ft).all()
    return {"rows": n_rows, "extract_features_rows_per_s": round(n_rows / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512, help="rows of the extraction measurement")
    ap.add_argument("--train-rows", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_train_bench needs a HIP device")
    mf, texts = _forensics(a.rows)
    res = {"train": bench_train(mf, a.train_rows, a.epochs), "tune": bench_tune(mf, a.train_rows),
           "towers": bench_towers(mf), "extract": bench_extract(mf, texts, a.rows)}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
