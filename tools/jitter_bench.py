"""ColorJitter on the device (mmf_color_jitter_u8) against the only way there was before it, on one box.

    python tools/jitter_bench.py [--windows 256] [--files 512] [--views 10] [--reps 500] [--out FILE]

Prints one JSON object:

  kernels  `--windows` staged 224 x 224 windows with four-operation chains (jitter_params' draws): the two launches
           of one call, by device events over `--reps` calls after a warm-up call, on preallocated buffers.  Also
           chains of one operation each, to show where the time goes: brightness alone (a blend per byte), contrast
           alone (both launches do work), hue alone (the float32 / double HSV round trip).  `bytes` is what the call
           has to move -- 3 bytes per pixel in for the sum of L, 3 in and 3 out for the chain -- and `hbm_floor_us`
           that traffic at 6.3 TB/s, the streaming rate measured on this GPU; `x_floor` = time / floor.
  host     the same work the only way possible without the kernels: the windows to the host, Pillow (pil_chain) on 16
           threads, the windows back; host clock, ending in a synchronise.  The results are compared byte for byte.
  extract  extract_image_features on `--files` 32 x 32 JPEG files with both flips: one view (no jitter) against
           `--views` jittered views; host clock to a synchronise.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12  # streaming rate measured on the MI355X (float4 copy)


def _forensics():
    from mmf_amd.api import MisinfoForensics
    return MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, verbose=False)


def _windows(n, dev):
    import mmf_amd.synthetic as syn
    return torch.from_numpy(np.ascontiguousarray(syn.images(n, 3))).to(dev)


def bench_kernels(n, reps, dev):
    import mmf_amd.cifake_training as CT
    import mmf_amd.hip as hip
    lib = hip.load()
    src = _windows(n, dev)
    dst = torch.empty_like(src)
    ws = torch.empty((n, hip.JITTER_CHUNKS), dtype=torch.int64, device=dev)
    ops, fac, shift = (a[0] for a in CT.jitter_params(n, 1, seed=0))
    pixels = n * 224 * 224
    out = {"windows": n, "reps": reps}

    def timed(name, ops_np, with_sum):
        o, f, h = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ops_np, fac, shift))

        def call():
            hip.check(lib.mmf_color_jitter_u8(hip.ptr(src), hip.ptr(dst), n, 224, 224, hip.ptr(o), hip.ptr(f),
                                              hip.ptr(h), hip.ptr(ws), hip.stream_ptr()), "mmf_color_jitter_u8")
        call()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        us = 1e3 * ev[0].elapsed_time(ev[1]) / reps
        nbytes = pixels * 3 * (3 if with_sum else 2)
        floor = 1e6 * nbytes / HBM_BYTES_PER_S
        out[name] = {"us_per_call": round(us, 2), "bytes": nbytes, "hbm_floor_us": round(floor, 2),
                     "x_floor": round(us / floor, 2), "windows_per_s": round(n / (us * 1e-6))}
    timed("four_ops", ops, True)
    for k, name in enumerate(("brightness_only", "contrast_only", "saturation_only", "hue_only")):
        timed(name, np.where(ops == k, k, -1).astype(np.int32), k == 1)
    return out, (src, ops, fac, shift)


def bench_host(case, dev, threads=16):
    """Windows to the host, Pillow on `threads` threads, windows back."""
    from tests import jitter_refs as J
    src, ops, fac, shift = case
    n = src.shape[0]

    def one(i):
        return J.pil_chain(host[i:i + 1], ops[i:i + 1], fac[i:i + 1], shift[i:i + 1])[0]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        for _ in range(2):  # the first pass warms Pillow and the pool
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = src.cpu().numpy()
            res = np.stack(list(ex.map(one, range(n))))
            back = torch.from_numpy(res).to(dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    return {"windows": n, "threads": threads, "ms": round(1e3 * dt, 2), "windows_per_s": round(n / dt)}, back


def bench_extract(mf, n_files, views):
    import mmf_amd.cifake_training as CT
    from PIL import Image
    g = np.random.default_rng(5)
    out = {"files": n_files, "image": "32x32 JPEG", "flip": True, "views": views}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(n_files):
            paths.append(os.path.join(d, f"{i:05d}.jpg"))
            Image.fromarray(g.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(paths[-1], quality=92)
        warm = min(n_files, mf.engine.max_batch)
        CT.extract_image_features(mf, paths[:warm], flip=True, jitter=CT.jitter_params(warm, 1, 0))
        for key, jit in (("one_view_s", None), ("jittered_views_s", CT.jitter_params(n_files, views, 0))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = CT.extract_image_features(mf, paths, flip=True, jitter=jit)
            torch.cuda.synchronize()
            out[key] = round(time.perf_counter() - t0, 4)
            assert res[-1].all() and np.isfinite(res[0]).all()
    out["rows_per_s_one_view"] = round(2 * n_files / out["one_view_s"], 1)
    out["rows_per_s_jittered"] = round(2 * n_files * views / out["jittered_views_s"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jitter_bench needs a HIP device")
    mf = _forensics()
    dev = mf.engine.device
    kernels, case = bench_kernels(a.windows, a.reps, dev)
    host, back = bench_host(case, dev)
    got = mf.engine.color_jitter(case[0], *case[1:])
    host["equal_to_device"] = bool(torch.equal(got, back))
    host["x_device"] = round(1e3 * host["ms"] / kernels["four_ops"]["us_per_call"], 1)
    res = {"kernels": kernels, "host": host, "extract": bench_extract(mf, a.files, a.views)}
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
