"""The JPEG save-and-reload round trip on the device (mmf_jpeg_roundtrip_u8) against the only way there was before
it, on one box.

    python tools/jpeg_roundtrip_bench.py [--windows 256] [--files 512] [--views 10] [--reps 200] [--rounds 5]
                                         [--out FILE]

Prints one JSON object:

  kernels  `--windows` staged 224 x 224 windows at qualities drawn as jpeg_params draws them (40..80): one call --
           the flags cleared and the two launches -- by device events over `--reps` calls after a warm-up call, on
           preallocated buffers, `--rounds` times over: the median, the least and the greatest round.  Also all
           windows at quality 1 and at 100 (the arithmetic does not depend on the data, so these should agree), and
           at 0: the first launch returns at once and the second copies, which leaves the cost of two launches and
           6 bytes per pixel.  `bytes` is what the call has to move: 3 bytes per pixel in and 1.5 of samples out in
           the first launch (a chroma thread reads its 16 x 16 pixels again, from the cache at best), 1.5 in and 3 out
           in the second; `hbm_floor_us` is that traffic at 6.3 TB/s, the streaming rate measured on this GPU;
           `x_floor` = median / floor.
  host     the same work without the kernels: the windows to the host, Pillow's save and load on 16 threads, the
           windows back; host clock, ending in a synchronise, `--rounds` times after a warm-up pass.  The results
           are compared byte for byte with Engine.jpeg_compress's.
  extract  extract_image_features on `--files` 32 x 32 JPEG files with both flips: one view against `--views` JPEG
           views; host clock to a synchronise.
"""
import argparse
import io
import json
import os
import statistics
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


def _spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits),
            "max": round(max(values), digits)}


def bench_kernels(n, reps, rounds, dev):
    import mmf_amd.cifake_training as CT
    import mmf_amd.hip as hip
    lib = hip.load()
    src = _windows(n, dev)
    dst = torch.empty_like(src)
    per_image = int(lib.mmf_jpeg_roundtrip_ws_bytes(224, 224))
    ws = torch.empty(n * per_image // 8, dtype=torch.int64, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    drawn = CT.jpeg_params(n, 1, seed=0)[0]
    pixels = n * 224 * 224
    out = {"windows": n, "reps": reps, "rounds": rounds, "ws_bytes_per_window": per_image}

    def timed(name, quality, bytes_per_pixel):
        q = torch.from_numpy(np.ascontiguousarray(quality, dtype=np.int32)).to(dev)

        def call():
            hip.check(lib.mmf_jpeg_roundtrip_u8(hip.ptr(src), hip.ptr(dst), n, 224, 224, hip.ptr(q), hip.ptr(ws),
                                                hip.ptr(flags), hip.stream_ptr()), "mmf_jpeg_roundtrip_u8")
        call()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(1e3 * ev[0].elapsed_time(ev[1]) / reps)
        assert not flags.any()
        nbytes = int(pixels * bytes_per_pixel)
        floor = 1e6 * nbytes / HBM_BYTES_PER_S
        med = statistics.median(us)
        out[name] = {"us_per_call": _spread(us), "bytes": nbytes, "hbm_floor_us": round(floor, 2),
                     "x_floor": round(med / floor, 2), "windows_per_s": round(n / (med * 1e-6))}
    timed("drawn_40_80", drawn, 9)
    timed("quality_1", np.full(n, 1), 9)
    timed("quality_100", np.full(n, 100), 9)
    timed("copy_quality_0", np.zeros(n), 6)
    return out, (src, drawn)


def _pil_roundtrip(rgb, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=int(q), optimize=False)
    buf.seek(0)
    im = Image.open(buf)
    im.load()
    return np.asarray(im.convert("RGB"))


def bench_host(case, rounds, dev, threads=16):
    """Windows to the host, Pillow's save and load on `threads` threads, windows back."""
    src, quality = case
    n = src.shape[0]
    ms = []
    with ThreadPoolExecutor(max_workers=threads) as ex:
        for r in range(rounds + 1):  # the first pass warms Pillow and the pool
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = src.cpu().numpy()
            res = np.stack(list(ex.map(lambda i: _pil_roundtrip(host[i], quality[i]), range(n))))
            back = torch.from_numpy(res).to(dev)
            torch.cuda.synchronize()
            if r:
                ms.append(1e3 * (time.perf_counter() - t0))
    return {"windows": n, "threads": threads, "ms": _spread(ms), "windows_per_s": round(n / (1e-3 * statistics.median(ms)))}, back


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
        CT.extract_image_features(mf, paths[:warm], flip=True, jpeg=CT.jpeg_params(warm, 1, 0))
        for key, jpeg in (("one_view_s", None), ("jpeg_views_s", CT.jpeg_params(n_files, views, 0))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = CT.extract_image_features(mf, paths, flip=True, jpeg=jpeg)
            torch.cuda.synchronize()
            out[key] = round(time.perf_counter() - t0, 4)
            assert res[-1].all() and np.isfinite(res[0]).all()
    out["rows_per_s_one_view"] = round(2 * n_files / out["one_view_s"], 1)
    out["rows_per_s_jpeg_views"] = round(2 * n_files * views / out["jpeg_views_s"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-extract", action="store_true", help="the kernels and the host path only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_roundtrip_bench needs a HIP device")
    mf = _forensics()
    dev = mf.engine.device
    kernels, case = bench_kernels(a.windows, a.reps, a.rounds, dev)
    host, back = bench_host(case, a.rounds, dev)
    got = mf.engine.jpeg_compress(*case)
    host["equal_to_device"] = bool(torch.equal(got, back))
    host["x_device"] = round(1e3 * host["ms"]["median"] / kernels["drawn_40_80"]["us_per_call"]["median"], 1)
    res = {"kernels": kernels, "host": host}
    if not a.no_extract:
        res["extract"] = bench_extract(mf, a.files, a.views)
    mf.engine.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
