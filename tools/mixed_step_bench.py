"""Interleaved, event-timed comparison of the mixed-modality step with the ways the same posts can be
served without it (one process, one device, inputs device-resident, B = 256, L = 128):

  a1, a2  analyze_batch on 256 pairs, timed twice in every round: their difference is the box's spread
  b       analyze_mixed on the same 256 rows, all "both"
  c       analyze_mixed on 128 both + 64 text-only + 64 image-only posts in shuffled row order
  d       the same 256 posts through the separate entry points, back to back: analyze_batch(128), then
          text_forward(64), then effnet_forward + clip_image + vault_topk on 64
  d_text, d_img, d_pairs   the three parts of d on their own (per-tower times)

    python tools/mixed_step_bench.py [--rounds 7 --iters 20 --json profiles/mixed_step_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None, help="write the result there as well as printing it")
    a = ap.parse_args()
    import bench
    import mmf_amd.weights as W
    from mmf_amd.engine import Engine
    B = a.batch
    eng = Engine(0, W.synthetic_detector_state(0), W.synthetic_clip_state(0), max_batch=B)
    t = bench.build_inputs(eng, B, 0)  # (also sets the 2170-row vault and its titles)
    out = eng.alloc_outputs(B)
    out2 = eng.alloc_outputs(B)

    # c / d: half the posts pairs, a quarter text only, a quarter image only, shuffled
    mod = np.array([3] * (B // 2) + [1] * (B // 4) + [2] * (B - B // 2 - B // 4), np.uint8)
    np.random.default_rng(0).shuffle(mod)
    dev = eng.device
    sel = {k: torch.as_tensor(np.flatnonzero(m), device=dev) for k, m in
           (("t", mod & 1 != 0), ("i", mod & 2 != 0), ("c", mod == 3), ("t1", mod == 1), ("i1", mod == 2))}
    mix = dict(rid=t["rid"][sel["t"]].contiguous(), rm=t["rm"][sel["t"]].contiguous(),
               cid=t["cid"][sel["c"]].contiguous(), cm=t["cm"][sel["c"]].contiguous(), img=t["img"][sel["i"]].contiguous())
    pairs = {k: t[k][sel["c"]].contiguous() for k in ("rid", "rm", "cid", "cm", "img")}
    tx = {k: t[k][sel["t1"]].contiguous() for k in ("rid", "rm")}
    im = t["img"][sel["i1"]].contiguous()
    all_both = np.full(B, 3, np.uint8)
    out_p = eng.alloc_outputs(len(sel["c"]))

    def d_pairs():
        eng.analyze_batch(pairs["rid"], pairs["rm"], pairs["cid"], pairs["cm"], pairs["img"], out=out_p)

    def d_text():
        eng.text_forward(tx["rid"], tx["rm"])

    def d_img():
        eng.effnet_forward(im)
        eng.vault_topk(eng.clip_image(im), 5, 0.85, None)

    def d():
        d_pairs()
        d_text()
        d_img()

    steps = {
        "a1": lambda: eng.analyze_batch(t["rid"], t["rm"], t["cid"], t["cm"], t["img"], out=out),
        "a2": lambda: eng.analyze_batch(t["rid"], t["rm"], t["cid"], t["cm"], t["img"], out=out),
        "b": lambda: eng.analyze_mixed(all_both, t["rid"], t["rm"], t["cid"], t["cm"], t["img"], out=out2),
        "c": lambda: eng.analyze_mixed(mod, mix["rid"], mix["rm"], mix["cid"], mix["cm"], mix["img"], out=out2),
        "d": d, "d_pairs": d_pairs, "d_text": d_text, "d_img": d_img,
    }
    # b computes what a computes
    steps["a1"]()
    steps["b"]()
    torch.cuda.synchronize()
    same = all(torch.equal(out[k], out2[k]) for k in out)
    print(f"b outputs identical to a: {same}", flush=True)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]) / a.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"batch": B, "text_len": 128, "rounds": a.rounds, "iters": a.iters, "unit": "ms per step (event-timed)",
           "rows": {"pairs": int((mod == 3).sum()), "text_only": int((mod == 1).sum()), "image_only": int((mod == 2).sum())},
           "b_identical_to_a": bool(same), "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(min(v), 4) for k, v in times.items()},
           "all_ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
           "spread_a_ms": round(abs(med["a1"] - med["a2"]), 4),
           "b_minus_a_ms": round(med["b"] - min(med["a1"], med["a2"]), 4),
           "c_minus_d_ms": round(med["c"] - med["d"], 4)}
    for k in steps:
        print(f"{k:8s} {med[k]:8.3f} ms/step  (min {min(times[k]):.3f})  [{', '.join(f'{x:.2f}' for x in times[k])}]", flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
