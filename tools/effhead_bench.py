"""Head-stage training (features.8 + classifier) on the device against the same step in torch, on one box.

    python tools/effhead_bench.py [--train-rows 4000] [--trials 7] [--out FILE]

Prints one JSON object:

  train    per batch size (16 and 64), microseconds per optimizer step on `--train-rows` cached trunk rows (a two-view
           bank of twice as many): mmf_effhead_train_epoch (three launches per step, no host synchronisation; one
           epoch per trial, timed by device events after a warm-up epoch; the median of `--trials` trials with their
           minimum and maximum) against the loop body of train_cifake_forensics.py:187-216 restated in torch on the
           SAME cached trunk on the same device: conv 1x1 + BatchNorm (eval) + SiLU + pool + dropout + linear under
           autocast + GradScaler + Adam + loss.item() (host clock around an epoch that ends in a synchronise, same
           number of trials).  `floor_us`: 2 * 2 * M * 320 * 1280 FLOP (the two contractions) at 155 TFLOP/s, the
           fp32 matrix rate measured for this device.  `eval_us_per_batch`: the validation call.
  tower    mmf_effnet_trunk beside mmf_effnet_pooled on 16 images (device events, median of the trials): images / s.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MATRIX_TFLOPS = 155.0


def _forensics():
    from mmf_amd.api import MisinfoForensics
    return MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, verbose=False)


def _events():
    return [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def _spread(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def bench_train(mf, n_rows, trials, batch, lr=1e-4):
    import torch.nn as nn
    import mmf_amd.cifake_training as CT
    eng, dev = mf.engine, mf.engine.device
    g = np.random.default_rng(7)
    x = (0.5 * g.standard_normal((2 * n_rows, 49, 320))).astype(np.float32)
    y = (x[:n_rows].mean(1) @ g.standard_normal(320) > 0).astype(np.int32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(np.concatenate([y, y])).to(dev)
    steps = -(-n_rows // batch)
    plans = [(torch.from_numpy(p).to(dev), torch.from_numpy(k.view(np.int64)).to(dev))
             for p, k, _ in CT.plan(n_rows, batch, trials + 1, 0, True)]
    params, mean, var = (t.to(dev).contiguous() for t in CT.flatten_head_stage(mf.detector))
    p0 = params.clone()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step0 = 0

    def run(e):
        nonlocal step0
        out = eng.effhead_train_epoch(xd, yd, plans[e][0], plans[e][1], CT.P_DROP, batch, mean, var, CT.BN_EPS, lr,
                                      CT.BETAS, CT.EPS, 0.0, step0, params, m, v)
        step0 += steps
        return out
    first = run(0)[0]
    torch.cuda.synchronize()
    kernel_us = []
    for e in range(1, trials + 1):
        ev = _events()
        ev[0].record()
        sl, _ = run(e)
        ev[1].record()
        torch.cuda.synchronize()
        kernel_us.append(1e3 * ev[0].elapsed_time(ev[1]) / steps)
    assert torch.isfinite(sl).all()
    xv, yv = xd[:n_rows], yd[:n_rows]
    eng.effhead_eval(xv, yv, batch, params, mean, var, CT.BN_EPS)
    torch.cuda.synchronize()
    eval_us = []
    for _ in range(trials):
        ev = _events()
        ev[0].record()
        eng.effhead_eval(xv, yv, batch, params, mean, var, CT.BN_EPS)
        ev[1].record()
        torch.cuda.synchronize()
        eval_us.append(1e3 * ev[0].elapsed_time(ev[1]) / steps)

    # ---- the same step in torch on the same device and the same cached trunk
    from torch.cuda.amp import GradScaler, autocast

    class Stage(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(320, 1280, 1, bias=False)
            self.bn = nn.BatchNorm2d(1280, eps=CT.BN_EPS)
            self.drop, self.lin = nn.Dropout(0.2), nn.Linear(1280, 2)

        def forward(self, t):  # t [n, 49, 320]
            img = t.reshape(-1, 7, 7, 320).permute(0, 3, 1, 2)
            a = nn.functional.silu(self.bn(self.conv(img)))
            return self.lin(self.drop(a.mean((2, 3))))

    net = Stage().to(dev)
    with torch.no_grad():
        net.conv.weight.copy_(p0[:409600].reshape(1280, 320, 1, 1))
        net.bn.weight.copy_(p0[409600:410880])
        net.bn.bias.copy_(p0[410880:412160])
        net.bn.running_mean.copy_(mean)
        net.bn.running_var.copy_(var)
        net.lin.weight.copy_(p0[412160:414720].reshape(2, 1280))
        net.lin.bias.copy_(p0[414720:])
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    criterion = nn.CrossEntropyLoss()
    yl = yd.long()

    def torch_epoch(scaler):
        net.train()
        net.bn.eval()  # the statistics stay frozen, as in the kernel
        total_loss = 0.0
        perm = torch.randperm(n_rows, device=dev)
        for s in range(steps):
            idx = perm[s * batch:(s + 1) * batch]
            opt.zero_grad()
            with autocast():
                logits = net(xd[idx])
                loss = criterion(logits, yl[idx])
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            total_loss += loss.item()
        return total_loss / steps
    torch_us = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaler = GradScaler()
        torch_epoch(scaler)
        torch.cuda.synchronize()
        for _ in range(trials):
            t0 = time.perf_counter()
            last = torch_epoch(scaler)
            torch.cuda.synchronize()
            torch_us.append(1e6 * (time.perf_counter() - t0) / steps)
    floor_us = 2 * 2 * (49 * batch) * 320 * 1280 / (FP32_MATRIX_TFLOPS * 1e12) * 1e6
    k, t = _spread(kernel_us), _spread(torch_us)
    return {"rows": n_rows, "bank_rows": 2 * n_rows, "batch": batch, "steps_per_epoch": steps, "trials": trials,
            "launches_per_step": 3, "kernel_us_per_step": k, "eval_us_per_batch": _spread(eval_us),
            "torch_loop_us_per_step": t, "ratio": round(t["median"] / k["median"], 2), "floor_us": round(floor_us, 2),
            "first_epoch_loss": round(float(first.mean()), 4), "last_epoch_loss": round(float(sl.mean()), 4),
            "torch_last_epoch_loss": round(last, 4)}


def bench_tower(mf, trials, batch=16, reps=20):
    import mmf_amd.synthetic as syn
    eng = mf.engine
    img = eng._u8(syn.images(batch, 3))
    out = {"batch": batch, "fp32_tower": eng.get_option("effnet_fp32"),
           "note": "each call includes the overflow trap's read-back"}
    for name, fn in (("effnet_pooled", eng.effnet_pooled), ("effnet_trunk", eng.effnet_trunk)):
        fn(img)
        torch.cuda.synchronize()
        us = []
        for _ in range(trials):
            ev = _events()
            ev[0].record()
            for _ in range(reps):
                fn(img)
            ev[1].record()
            torch.cuda.synchronize()
            us.append(1e3 * ev[0].elapsed_time(ev[1]) / reps)
        out[name + "_us_per_call"] = _spread(us)
        out[name + "_images_per_s"] = round(batch / (statistics.median(us) * 1e-6), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-rows", type=int, default=4000)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("effhead_bench needs a HIP device")
    mf = _forensics()
    res = {"train": [bench_train(mf, a.train_rows, a.trials, batch) for batch in (16, 64)],
           "tower": bench_tower(mf, a.trials)}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
