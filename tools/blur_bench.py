"""GaussianBlur on the device (mmf_gaussian_blur_u8) against the only way there was before it, on one box.

    python tools/blur_bench.py [--windows 256] [--reps 500] [--out FILE]

Prints one JSON object:

  kernel   `--windows` staged 224 x 224 windows through the 5 x 9 kernel, sigmas drawn by blur_params: device events
           over `--reps` calls in five groups after a warm-up call, on preallocated buffers (the weights already on
           the device: forming them is host work of microseconds per window, outside the launch).  `all` blurs
           every window, `p03` the mix RandomApply(p=0.3) draws (the others are copied).  `bytes` is what the call
           has to move, every window read once and written once, and `hbm_floor_us` that traffic at 6.3 TB/s, the
           streaming rate measured on this GPU; `valu_floor_us` is 90 float32 operations per blurred byte (45
           products, 45 adds, no FMA by specification) at 78.6 T operations/s, the chip's plain (unpacked, unfused)
           float32 rate -- half its 157.3 TFLOP/s, which counts an FMA as two.
  host     the same work the only way possible without the kernel: the windows to the host, torch's float32
           pad / conv2d / round on 16 CPU threads (one grouped conv2d for the batch, each window its own weights),
           the windows back; host clock, ending in a synchronise, the second of two passes.
  check    the two results against each other under the tie rule of tests/blur_refs.py: bytes whose float64 value
           is farther than 1e-3 from a half-integer must be equal, the others at most one apart.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12   # streaming rate measured on the MI355X (float4 copy)
VALU_OPS_PER_S = 78.6e12   # plain float32 operations: 157.3 TFLOP/s counts an FMA as two
KX, KY = 5, 9
SIDE = 224


def _windows(n, dev):
    import mmf_amd.synthetic as syn
    return torch.from_numpy(np.ascontiguousarray(syn.images(n, 3))).to(dev)


def bench_kernel(src, weights, applies, reps):
    import mmf_amd.hip as hip
    lib = hip.load()
    dev = src.device
    n = src.shape[0]
    dst = torch.empty_like(src)
    w = torch.from_numpy(weights).to(dev)
    out = {}
    for name, apply in applies.items():
        a = torch.from_numpy(apply.astype(np.int32)).to(dev)

        def call():
            hip.check(lib.mmf_gaussian_blur_u8(hip.ptr(src), hip.ptr(dst), n, SIDE, SIDE, KX, KY, hip.ptr(w), hip.ptr(a),
                                               hip.stream_ptr()), "mmf_gaussian_blur_u8")
        call()
        torch.cuda.synchronize()
        groups, per = [], max(1, reps // 5)
        for _ in range(5):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(per):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            groups.append(1e3 * ev[0].elapsed_time(ev[1]) / per)
        us = float(np.median(groups))
        nbytes = 2 * src.numel()
        blurred = int(apply.sum()) * SIDE * SIDE * 3
        floor, valu = 1e6 * nbytes / HBM_BYTES_PER_S, 1e6 * 90 * blurred / VALU_OPS_PER_S
        out[name] = {"blurred": int(apply.sum()), "us_per_call": round(us, 2),
                     "us_min_max": [round(min(groups), 2), round(max(groups), 2)], "bytes": nbytes,
                     "hbm_floor_us": round(floor, 2), "x_hbm_floor": round(us / floor, 2),
                     "valu_floor_us": round(valu, 2), "x_valu_floor": round(us / valu, 2) if blurred else None,
                     "windows_per_s": round(n / (us * 1e-6))}
    return out


def host_route(src, weights, threads=16):
    """Windows to the host, torch's float32 conv2d on `threads` CPU threads, windows back."""
    dev = src.device
    n = src.shape[0]
    torch.set_num_threads(threads)
    kernel = torch.from_numpy(weights)[:, None].expand(n, 3, KY, KX).reshape(3 * n, 1, KY, KX).contiguous()
    for _ in range(2):  # the first pass warms the pool and the convolution's set-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = src.cpu()
        x = host.permute(0, 3, 1, 2).reshape(1, 3 * n, SIDE, SIDE).to(torch.float32)
        x = F.pad(x, [KX // 2, KX // 2, KY // 2, KY // 2], mode="reflect")
        y = torch.round(F.conv2d(x, kernel, groups=3 * n)).to(torch.uint8)
        res = y.reshape(n, 3, SIDE, SIDE).permute(0, 2, 3, 1).contiguous()
        back = res.to(dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"windows": n, "threads": threads, "ms": round(1e3 * dt, 2), "windows_per_s": round(n / dt)}, back


def check(src, weights, device_out, host_out, delta=1e-3):
    n = src.shape[0]
    x = src.cpu().permute(0, 3, 1, 2).reshape(1, 3 * n, SIDE, SIDE).to(torch.float64)
    x = F.pad(x, [KX // 2, KX // 2, KY // 2, KY // 2], mode="reflect")
    kernel = torch.from_numpy(weights).to(torch.float64)[:, None].expand(n, 3, KY, KX).reshape(3 * n, 1, KY, KX)
    real = F.conv2d(x, kernel.contiguous(), groups=3 * n).reshape(n, 3, SIDE, SIDE).permute(0, 2, 3, 1)
    near = (real - torch.floor(real) - 0.5).abs() <= delta
    diff = device_out.cpu().to(torch.int32) - host_out.cpu().to(torch.int32)
    return {"bytes": int(diff.numel()), "near_a_tie": int(near.sum()), "differ": int((diff != 0).sum()),
            "differ_away_from_a_tie": int(((diff != 0) & ~near).sum()), "largest_difference": int(diff.abs().max()),
            "tie_share": round(float(near.float().mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blur_bench needs a HIP device")
    import mmf_amd.cifake_training as CT
    import mmf_amd.hip as hip
    dev = torch.device("cuda", 0)
    src = _windows(a.windows, dev)
    apply, sigma = (x[0] for x in CT.blur_params(a.windows, 1, seed=0))
    weights = CT.gaussian_kernel2d(sigma)
    everyone = np.ones(a.windows, bool)
    kernel = bench_kernel(src, weights, {"all": everyone, "p03": apply}, a.reps)
    host, back = host_route(src, weights)
    lib = hip.load()
    got = torch.empty_like(src)
    w, on = torch.from_numpy(weights).to(dev), torch.from_numpy(everyone.astype(np.int32)).to(dev)
    hip.check(lib.mmf_gaussian_blur_u8(hip.ptr(src), hip.ptr(got), a.windows, SIDE, SIDE, KX, KY, hip.ptr(w), hip.ptr(on),
                                       hip.stream_ptr()), "mmf_gaussian_blur_u8")
    torch.cuda.synchronize()
    verdict = check(src, weights, got, back)
    verdict["ok"] = verdict["differ_away_from_a_tie"] == 0 and verdict["largest_difference"] <= 1
    host["x_device"] = round(1e3 * host["ms"] / kernel["all"]["us_per_call"], 1)
    res = {"windows": a.windows, "reps": a.reps, "kernel": kernel, "host": host, "check": verdict}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not verdict["ok"]:
        raise SystemExit("the device and the host route differ away from a tie")


if __name__ == "__main__":
    main()
