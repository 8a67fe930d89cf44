"""Interleaved, event-timed comparison of the two vault search paths (option vault_fused 0 = similarity
matrix + top-k kernels, 1 = the fused similarity + top-k kernels) through mmf_vault_topk, on synthetic
unit rows (one process, one device, queries device-resident, k = 5):

    N in {2170, 16384, 131072, 1048576}  x  B in {1, 256}

Per shape and path: time per call (median, min, max over the rounds; the two paths alternate inside
every round, so drift of the box hits both), the search workspace the handle holds beside the vault,
the vault bytes read once per call as GB/s, and the fraction of the fp32-MFMA peak (157.3 TFLOP/s) that
2 B N 512 FLOP per call amount to.  `spread` is (max - min) / median of a path's rounds.

    python tools/vault_bench.py [--rounds 5 --sizes 2170,16384,131072,1048576 --out profiles/vault_fused_ab.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="2170,16384,131072,1048576")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the report there as well as printing it")
    a = ap.parse_args()
    import mmf_amd.weights as W
    from mmf_amd.engine import Engine
    sizes = [int(x) for x in a.sizes.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = Engine(0, None, W.synthetic_clip_state(0), max_batch=max(batches))
    base = eng.device_bytes
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((max(sizes), 512), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    say(f"vault search, vault_fused 0 vs 1, top_k = {a.top_k}, {a.rounds} interleaved rounds, event-timed; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"{'N':>8} {'B':>4} {'path':>6} {'ms/call':>9} {'min':>9} {'max':>9} {'spread':>7} {'ws bytes':>12} "
        f"{'GB/s':>8} {'mfma %':>7}")
    for N in sizes:
        eng.set_vault(rows[:N])
        for B in batches:
            # queries: half of them near a vault row (hits), half random
            q = rng.standard_normal((B, 512), dtype=np.float32)
            q[::2] = rows[rng.integers(0, N, len(q[::2]))] + 0.02 * q[::2]
            qu = torch.nn.functional.normalize(torch.as_tensor(q)).cuda()
            times, ws, outs = {0: [], 1: []}, {}, {}
            for r in range(a.rounds):
                for mode in (0, 1) if r % 2 == 0 else (1, 0):
                    eng.set_option("vault_fused", mode)
                    ws[mode] = eng.device_bytes - base - N * 2048
                    out = eng.vault_topk(qu, a.top_k, 0.85)  # warm-up, and the answer
                    torch.cuda.synchronize()
                    outs[mode] = [t.clone() for t in out[:3]]
                    ev[0].record()
                    eng.vault_topk(qu, a.top_k, 0.85)
                    ev[1].record()
                    torch.cuda.synchronize()
                    iters = int(min(200, max(3, 100.0 / max(ev[0].elapsed_time(ev[1]), 1e-3))))  # ~0.1 s per sample
                    ev[0].record()
                    for _ in range(iters):
                        eng.vault_topk(qu, a.top_k, 0.85)
                    ev[1].record()
                    torch.cuda.synchronize()
                    times[mode].append(ev[0].elapsed_time(ev[1]) / iters)
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0], outs[1]))
            med = {m: statistics.median(t) for m, t in times.items()}
            spread = {m: (max(t) - min(t)) / med[m] for m, t in times.items()}
            for m in (0, 1):
                t = med[m] * 1e-3
                say(f"{N:>8} {B:>4} {'fused' if m else 'two-k':>6} {med[m]:>9.4f} {min(times[m]):>9.4f} "
                    f"{max(times[m]):>9.4f} {100 * spread[m]:>6.1f}% {ws[m]:>12d} {N * 2048 / t / 1e9:>8.1f} "
                    f"{100 * 2.0 * B * N * 512 / t / PEAK_F32_MFMA:>6.1f}%")
            ratio = med[0] / med[1]
            sp = max(spread.values())
            verdict = "fused faster" if ratio > 1 + sp else "two-kernel faster" if ratio < 1 - sp else "within the spread"
            say(f"{'':>8} {'':>4} two-kernel / fused = {ratio:.3f} (spread {100 * sp:.1f}%): {verdict}; "
                f"outputs bit-identical: {same}")
    eng.set_option("vault_fused", 2)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
