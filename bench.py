"""Benchmark: text+image pairs/sec through the full analyze() 5-signal path (BASELINE.json metric),
batch 256 pairs per GPU, synthetic inputs, random-init weights of the reference architectures
(RoBERTa-base + 2 heads, EfficientNet-B0, CLIP ViT-B/32, 2170-row Truth-Vault, FusionJudge).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

Both multi-GPU forms run the same ranks: started directly with --gpus N > 1 (no WORLD_SIZE in the
environment), this process launches N rank processes itself (benchrun.launch_ranks: RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* set as torchrun sets them, before anything touches the GPU),
relays rank 0's JSON line and exits with the first failing rank's code.

`value` follows SURVEY.md §8d: each step's inputs (int32 token ids + uint8 images, 38.96 MB per 256
pairs) start in pinned HOST memory and cross PCIe inside the timed region (double-buffered H2D on a
copy stream, engine.HostPipeline), and the result tensors come back D2H.  The HBM-resident rate
(inputs already on the device) is reported beside it as `hbm_resident`.  Tokenisation and JPEG
decode stay outside (the reference's tokenizers / vocab files are not available offline).

One process per GPU; the batch is sharded (weak scaling: 256 pairs per GPU, no collective on the
data path -- the barrier and the max-over-ranks time reduction of mmf_amd.benchrun are the only
RCCL traffic).  Rank 0 prints one JSON line.

A plain run does what the headline needs and nothing else: engine and inputs, W warm-up steps, K
timed steps, the line.  --full adds the secondary measurements to the same line: the HBM-resident
rate, the dominant kernel's roofline, the per-config numbers of BASELINE configs[1..3], the
per-sample and text+JPEG lines (N = 1 only) and the CPU baseline; each --no-* option leaves one of
them out of a --full run.  --dump-outputs DIR writes the result arrays of the last timed step (what
HostPipeline.result returns to a caller) as DIR/<name>.npy, float32; the inputs are seeded, so two
builds run with the same arguments can be compared array for array.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from mmf_amd import benchrun  # noqa: E402

# algorithmic work: GFLOP per unit, ViT counted once per pair
GFLOP_PER_PAIR = 37.90
GFLOP_ROBERTA_L128 = 22.35
GFLOP_VIT, GFLOP_CLIP_TEXT_L77 = 8.82, 5.96
EFFNET_FLOOR_BYTES_PER_IMG, EFFNET_WEIGHT_BYTES = 4.35e6, 8.0e6
PEAK_TFLOPS, PEAK_GBS = 2500.0, 8000.0


def encoder_gflop(L: int, H: int, I: int, heads: int, layers: int = 12, compact_last: bool = False,
                  q1_last: bool = False) -> float:
    """GFLOP of one sequence through a transformer encoder (2 flops per MAC; attention 4 L^2 d per
    head).  compact_last: the last layer's out-proj / FFN run on the pooled row only; q1_last: its
    QKV GEMM computes K / V of every row and Q of the pooled row, and its attention one query (the
    device path's compact last layers, capi.cpp run_text / run_clip_encoder)."""
    d = H // heads
    qkv, o, ffn, att = 2 * L * H * 3 * H, 2 * L * H * H, 4 * L * H * I, 4 * heads * L * L * d
    full = qkv + o + ffn + att
    if not compact_last:
        return layers * full / 1e9
    if q1_last:
        last = 2 * L * H * 2 * H + 2 * H * H + 4 * heads * L * d
    else:
        last = qkv + att
    last += 2 * H * H + 4 * H * I  # out-proj + FFN of the pooled row
    return ((layers - 1) * full + last) / 1e9


# executed work per unit: what the kernels compute, with the compact last layers
# (RoBERTa: K / V + one query in its last layer; CLIP towers: full last-layer attention, pooled-row
# out-proj / FFN), against the algorithmic counts above, which price every layer in full
GFLOP_EXEC_ROBERTA_L128 = round(encoder_gflop(128, 768, 3072, 12, compact_last=True, q1_last=True), 3)
GFLOP_EXEC_VIT = round(2 * 49 * 3072 * 768 / 1e9 + encoder_gflop(50, 768, 3072, 12, compact_last=True), 3)
GFLOP_EXEC_CLIP_TEXT_L77 = round(encoder_gflop(77, 512, 2048, 8, compact_last=True), 3)
GFLOP_EXEC_EFFNET = 0.769
GFLOP_EXEC_PER_PAIR = round(GFLOP_EXEC_ROBERTA_L128 + GFLOP_EXEC_VIT + GFLOP_EXEC_CLIP_TEXT_L77 + GFLOP_EXEC_EFFNET, 2)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result arrays of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (HBM-resident rate, per-kernel roofline, BASELINE "
                         "configs[1..3], per-sample and text+JPEG lines, CPU baseline); the --no-* options "
                         "below each leave one of them out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="time budget of CPU mode (i)")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel event-timed pass")
    ap.add_argument("--no-configs", action="store_true", help="skip the BASELINE configs[1..3] lines")
    ap.add_argument("--no-per-sample", action="store_true", help="skip the B=1 / per-row API lines")
    ap.add_argument("--no-e2e", action="store_true", help="skip the text+JPEG analyze_pairs line")
    ap.add_argument("--cpu-standin", action="store_true",
                    help="TEST ONLY: the rank launch, gloo barriers and max-over-ranks timing around a CPU "
                         "stand-in step (no GPU, no HIP library); the JSON line says so in `data`")
    return ap.parse_args()


def build_inputs(eng, B, rank, n_vault=2170):
    import mmf_amd.synthetic as syn
    seed = benchrun.input_seed(rank)
    rid, rm = syn.roberta_ids(B, 128, seed)
    cid, cm = syn.clip_ids(B, 77, seed)
    imgs = syn.images(B, seed)
    dev = eng.device
    t = dict(rid=torch.from_numpy(rid).to(dev), rm=torch.from_numpy(rm).to(dev),
             cid=torch.from_numpy(cid).to(dev), cm=torch.from_numpy(cm).to(dev),
             img=torch.from_numpy(imgs).to(dev))
    # Truth-Vault: N(0,1) rows with 1/8 of this batch's image embeddings planted (exercises the
    # > 0.85 branch and the text_similarity gather), titles with random CLIP token ids
    vault = syn.vault(n_vault, 512, 77)
    emb = eng.clip_image(t["img"]).cpu().numpy()
    g = np.random.Generator(np.random.PCG64(4242 + rank))
    rows = g.choice(n_vault, size=B // 8, replace=False)
    for i, r in enumerate(rows):
        vault[r] = emb[i * 8] * 2.0
    t_lens = g.integers(3, 78, n_vault)
    tid, tm = syn.clip_ids(n_vault, 77, 99, t_lens.tolist())
    eng.set_vault(vault, tid, tm)
    return t


def cpu_baseline(seconds: float, batch: int = 256):
    """Oracle (fp32 PyTorch CPU restatement, test infrastructure) on bounded samples, all of the
    host cores this process may use (affinity, capped by the cgroup CPU quota):
    (i) reference-faithful per-pair analyze() (B=1, ViT twice, numpy vault renormalised per call);
    (ii) batched (B up to 256, ViT once, vault normalised once), the best a CPU port could do."""
    from oracle import pipeline as P
    import mmf_amd.synthetic as syn
    import mmf_amd.weights as W
    cores = benchrun.usable_cpus()
    torch.set_num_threads(cores)
    benchrun.progress(f"cpu baseline on {cores} threads (affinity {len(os.sched_getaffinity(0))})")
    det, clip = W.synthetic_detector_state(0), W.synthetic_clip_state(0)
    n = 64
    rid, rm = syn.roberta_ids(max(n, batch), 128, 7)
    cid, cm = syn.clip_ids(max(n, batch), 77, 7)
    imgs = syn.images(max(n, batch), 7)
    vault = syn.vault(2170, 512, 77)
    meta = [{"title": f"t{j}", "url": "N/A", "date": "N/A"} for j in range(2170)]
    orc = P.OracleForensics(det, clip, vault, meta, [cid[j % n] for j in range(2170)])
    with torch.no_grad():
        orc.analyze(text=(rid[0], cid[0]), image=imgs[0])  # warm-up
        t0 = time.perf_counter()
        done = 0
        while done < n and (time.perf_counter() - t0) < seconds:
            orc.analyze(text=(rid[done], cid[done]), image=imgs[done])
            done += 1
        dt = time.perf_counter() - t0
        per_pair = dt / done
        benchrun.progress(f"cpu mode (i): {done} pairs in {dt:.1f} s")
        # batched mode: bounded to ~20 s from the per-pair time (a batch runs ~2x more efficiently)
        b2 = int(min(batch, max(8, 20.0 / (0.5 * per_pair))))
        t1 = time.perf_counter()
        P.batched_scores(det, clip, rid[:b2], rm[:b2], cid[:b2], cm[:b2], imgs[:b2], vault)
        dt2 = time.perf_counter() - t1
    return {"value": round(done / dt, 3), "unit": "pairs/s", "cores": cores, "kind": "port",
            "sample": f"mode (i): {done} text+image pairs (L=128 text, 77-token caption, 224x224 image, 2170-row "
                      f"vault) through oracle.OracleForensics.analyze one pair at a time (reference-faithful: B=1, "
                      f"ViT twice, vault renormalised per call), fp32, {dt:.1f} s",
            "batched_mode": {"value": round(b2 / dt2, 3), "unit": "pairs/s", "batch": b2,
                             "sample": f"mode (ii): one oracle.pipeline.batched_scores call on {b2} pairs (ViT once, "
                                       f"vault normalised once), fp32, {dt2:.1f} s"}}


def config_lines(eng, t, steps, warmup, det):
    """BASELINE configs[1..3] on this GPU (secondary numbers, each with its own roofline)."""
    import mmf_amd.synthetic as syn
    from mmf_amd.hip import check, ptr, stream_ptr
    sync = torch.cuda.synchronize
    lib, h, dev = eng.lib, eng.h, eng.device
    out = {}
    B = t["rid"].shape[0]
    benchrun.progress("configs[1..3]")
    # configs[1]: RoBERTa-base dual-head text-only forward, L=128, B=256
    ai, mi, sc = (torch.empty(B, 2, device=dev) for _ in range(3))

    def text():
        check(lib.mmf_text_forward(h, ptr(t["rid"]), ptr(t["rm"]), B, 128, ptr(ai), ptr(mi), ptr(sc), stream_ptr()))
    dt = benchrun.timed_steps(text, steps, warmup, None, sync)
    tf = B * GFLOP_ROBERTA_L128 * steps / dt / 1e3
    tfx = B * GFLOP_EXEC_ROBERTA_L128 * steps / dt / 1e3
    out["roberta_text_b256"] = {
        "config": "BASELINE configs[1]: RoBERTa-base dual-head text-only forward, seq_len=128, batch=256",
        "value": round(B * steps / dt, 1), "unit": "texts/s", "ms_per_step": round(1000 * dt / steps, 3),
        "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(tf / PEAK_TFLOPS, 4), "work": f"{GFLOP_ROBERTA_L128} GFLOP/text",
                     "executed_achieved": round(tfx, 1), "executed_frac": round(tfx / PEAK_TFLOPS, 4),
                     "executed_work": f"{GFLOP_EXEC_ROBERTA_L128} GFLOP/text (compact last layer)"}}
    # configs[3]: CLIP ViT-B/32 image + text towers + cosine, B=256
    cons = {"img_emb": torch.empty(B, 512, device=dev), "txt_emb": torch.empty(B, 512, device=dev),
            "sim": torch.empty(B, device=dev)}
    dt = benchrun.timed_steps(lambda: eng.clip_consistency(t["img"], t["cid"], t["cm"], out=cons), steps, warmup,
                              None, sync)
    tf = B * (GFLOP_VIT + GFLOP_CLIP_TEXT_L77) * steps / dt / 1e3
    tfx = B * (GFLOP_EXEC_VIT + GFLOP_EXEC_CLIP_TEXT_L77) * steps / dt / 1e3
    out["clip_b256"] = {
        "config": "BASELINE configs[3]: CLIP ViT-B/32 image+text encoders + cosine similarity, batch=256",
        "value": round(B * steps / dt, 1), "unit": "image-text pairs/s", "ms_per_step": round(1000 * dt / steps, 3),
        "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(tf / PEAK_TFLOPS, 4),
                     "work": f"{GFLOP_VIT} + {GFLOP_CLIP_TEXT_L77} GFLOP/pair (L=77 text)",
                     "executed_achieved": round(tfx, 1), "executed_frac": round(tfx / PEAK_TFLOPS, 4),
                     "executed_work": f"{GFLOP_EXEC_VIT} + {GFLOP_EXEC_CLIP_TEXT_L77} GFLOP/pair (compact last layers)"}}
    # configs[2]: EfficientNet-B0, 224x224, B=512 (workspaces re-reserved for 512 rows)
    Be = 512
    eng.reserve(Be, 128, 77)
    imgs = torch.from_numpy(syn.images(Be, benchrun.input_seed(0) + 100)).to(dev)
    lg, ds = torch.empty(Be, 2, device=dev), torch.empty(Be, device=dev)

    def effnet():
        check(lib.mmf_effnet_forward(h, ptr(imgs), Be, ptr(lg), ptr(ds), stream_ptr()))
    dt = benchrun.timed_steps(effnet, steps, warmup, None, sync)
    gbs = (Be * EFFNET_FLOOR_BYTES_PER_IMG + EFFNET_WEIGHT_BYTES) * steps / dt / 1e9
    out["effnet_b512"] = {
        "config": "BASELINE configs[2]: EfficientNet-B0 image forward, 224x224, batch=512",
        "value": round(Be * steps / dt, 1), "unit": "images/s", "ms_per_step": round(1000 * dt / steps, 3),
        "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_GBS, "unit": "GB/s",
                     "frac": round(gbs / PEAK_GBS, 4),
                     "work": "4.35 MB/img block-fused activation floor + 8 MB weights (0.769 GFLOP/img)"}}
    # the same workload on the fp32 tower (option effnet_fp32, the ill-conditioned-weights mode)
    prev = eng.get_option("effnet_fp32")
    eng.set_option("effnet_fp32", 1)
    try:
        dt = benchrun.timed_steps(effnet, steps, warmup, None, sync)
    finally:
        eng.set_option("effnet_fp32", prev)
    out["effnet_fp32_b512"] = {
        "config": "configs[2] workload on the fp32-activation EfficientNet tower (option effnet_fp32)",
        "value": round(Be * steps / dt, 1), "unit": "images/s", "ms_per_step": round(1000 * dt / steps, 3)}
    eng.reserve(B, 128, 77)
    return out


def per_sample_lines(n_lat: int = 200, n_rows: int = 64, warmup: int = 10):
    """The reference's per-sample callers through the drop-in API:
    * `analyze(text, image)` one pair per call -- the dashboard path (forensics_dashboard.py:180-185):
      p50 / p99 / mean latency from the call to the returned dict, B = 1;
    * FusionTrainingDataset.__getitem__'s extraction (train_fusion_judge.py:72-86): analyze_text,
      analyze_image, analyze_consistency, search_vault (no caption) per row -> rows/s.
    Inputs: 224x224 PIL images in memory (decode excluded), L = 128 texts, 77-token captions through an
    id-table tokenizer (tokenisation is a dict lookup), 2170-row vault with titles."""
    from PIL import Image
    import mmf_amd.synthetic as syn
    from mmf_amd.api import MisinfoForensics
    n = max(n_lat, n_rows) + warmup
    seed = benchrun.input_seed(0) + 200
    texts, rob, clp = syn.text_tables(n, seed)
    pils = [Image.fromarray(a) for a in syn.images(n, seed)]
    tid, tm = syn.clip_ids(2170, 77, 99, np.random.default_rng(5).integers(3, 78, 2170).tolist())
    meta = []
    for j in range(2170):
        clp.table[f"title {j}"] = tid[j, :int(tm[j].sum())].tolist()
        meta.append({"title": f"title {j}", "url": "N/A", "date": "N/A"})
    mf = MisinfoForensics(fusion_weights="", faiss_index_path="", synthetic_seed=0, roberta_tokenizer=rob,
                          clip_processor=clp, verbose=False)
    mf.set_vault(syn.vault(2170, 512, 77), meta)
    benchrun.progress("per-sample lines: analyze() at B=1")
    for i in range(warmup):
        mf.analyze(text=texts[i], image_path=pils[i], verbose=False)
    lat = []
    for i in range(warmup, warmup + n_lat):
        t0 = time.perf_counter()
        mf.analyze(text=texts[i], image_path=pils[i], verbose=False)
        lat.append(time.perf_counter() - t0)
    lat_ms = np.asarray(lat) * 1e3
    benchrun.progress("per-sample lines: FusionTrainingDataset rows")

    def row(i):
        ts = mf.analyze_text(texts[i])
        im = mf.analyze_image(pils[i])
        cs = mf.analyze_consistency(texts[i], pils[i])
        vr = mf.search_vault(pils[i])
        return [ts["ai_score"], ts["misinfo_score"], im["deepfake_score"], cs["clip_similarity"],
                vr["vault_discrepancy"]]
    for i in range(warmup):
        row(i)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + n_rows):
        row(i)
    dt = time.perf_counter() - t0
    # before: one ViT pass per call, as the reference does (quirk Q6)
    mf.reuse_image_embedding = False
    t0 = time.perf_counter()
    for i in range(warmup, warmup + n_rows):
        row(i)
    dt_before = time.perf_counter() - t0
    mf.engine.close()
    return {"analyze_b1": {"config": "analyze(text, image) one pair per call (dashboard path, "
                                     "forensics_dashboard.py:180-185), 224x224 PIL image, L=128 text",
                           "p50_ms": round(float(np.percentile(lat_ms, 50)), 3),
                           "p99_ms": round(float(np.percentile(lat_ms, 99)), 3),
                           "mean_ms": round(float(lat_ms.mean()), 3), "calls": n_lat,
                           "value": round(1000.0 / float(lat_ms.mean()), 1), "unit": "pairs/s"},
            "fusion_dataset_rows": {"config": "FusionTrainingDataset.__getitem__ extraction (train_fusion_judge.py:"
                                              "72-86): analyze_text + analyze_image + analyze_consistency + "
                                              "search_vault per row",
                                    "value": round(n_rows / dt, 1), "unit": "rows/s",
                                    "ms_per_row": round(1000 * dt / n_rows, 3), "rows": n_rows,
                                    "before_vit_reuse": {"value": round(n_rows / dt_before, 1), "unit": "rows/s",
                                                         "note": "search_vault re-runs the ViT on the image "
                                                                 "analyze_consistency just embedded (reference "
                                                                 "behaviour, misinfo_forensics.py:395, 438)"}}}


METRIC = "text+image pairs/sec through full analyze() 5-signal path, batch=256"
WORKLOAD = ("Full MisinfoForensics.analyze() 5-signal pipeline incl. Truth-Vault lookup (BASELINE configs[4]), "
            "text L=128, caption L=77, 224x224 images; inputs H2D and results D2H inside the timed region "
            "(SURVEY.md §8d)")


def result_line(a, world: int, B: int, dt: float, value: float, data: str, **extra) -> dict:
    """The one JSON line rank 0 prints (the driver's contract)."""
    res = {"metric": METRIC, "value": round(value, 2), "unit": "pairs/s", "n_gpus": world, "steps": a.steps,
           "warmup": a.warmup, "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "fp16", "data": data,
           "config": {"workload": WORKLOAD, "global_batch": world * B, "batch_per_gpu": B, "seq_len": 128,
                      "parallelism": f"replicas x{world} (no data-path collective)"}}
    cfg_extra = extra.pop("config_extra", None)
    if cfg_extra:
        res["config"].update(cfg_extra)
    res.update(extra)
    return res


def dump_outputs(dirname: str, arrays: dict, rank: int) -> None:
    """--dump-outputs: one float32 .npy per result array (the int32 verdict / rule / top_idx values are
    small integers, exact in float32).  Rank 0 writes DIR/<name>.npy, rank r > 0 DIR/<name>.rank<r>.npy."""
    os.makedirs(dirname, exist_ok=True)
    suffix = "" if rank == 0 else f".rank{rank}"
    for name, v in arrays.items():
        np.save(os.path.join(dirname, f"{name}{suffix}.npy"), v.detach().cpu().numpy().astype(np.float32))


def standin_main(a, world: int, rank: int) -> None:
    """--cpu-standin: everything bench.py does around the step -- the rank environment, gloo
    barriers, exactly K timed steps, the max over ranks, the whole-job rate and the JSON line --
    with a CPU stand-in step (a [B,768]x[768,768] matmul per pair batch) instead of the HIP path.
    tests/test_multiproc_cpu.py runs `python bench.py --gpus 2 --cpu-standin` through it."""
    fail = os.environ.get("MMF_STANDIN_FAIL_RANK", "")
    if fail.isdigit() and int(fail) == rank:
        raise SystemExit(f"rank {rank}: failing on request (MMF_STANDIN_FAIL_RANK)")
    torch.set_num_threads(1)
    dist = benchrun.init_dist(world, "gloo")
    B = a.batch
    g = torch.Generator().manual_seed(benchrun.input_seed(rank))
    x, w = torch.randn(B, 768, generator=g), torch.randn(768, 768, generator=g)
    y = torch.empty(B, 768)
    dt = benchrun.timed_steps(lambda: torch.mm(x, w, out=y), a.steps, a.warmup, dist)
    value = benchrun.whole_job_rate(world, B, a.steps, dt)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {"standin": y}, rank)
    if rank == 0:
        res = result_line(a, world, B, dt, value, "cpu stand-in step (test of the rank launch; not a measurement)",
                          config_extra={"rank_launch": "bench.py" if os.environ.get("MMF_BENCH_PARENT") else
                                        "external"})
        print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


def main():
    a = parse()
    if benchrun.needs_launch(a.gpus):
        # the driver's `python bench.py --gpus N`: become the parent of N ranks (never touches the GPU)
        os.environ["MMF_BENCH_PARENT"] = "1"
        cmd = [sys.executable, "-u", os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(benchrun.launch_ranks(a.gpus, cmd, check_devices=not (a.cpu_standin or
                                                                        os.environ.get("MMF_BENCH_SHARE_GPU") == "1")))
    world, rank, local = benchrun.rank_env()
    if world != a.gpus:
        benchrun.progress(f"note: --gpus {a.gpus} but the launcher started {world} rank(s); reporting {world}")
    if a.cpu_standin:
        return standin_main(a, world, rank)
    # MMF_BENCH_SHARE_GPU=1 (rehearsal only, never a measurement): N ranks share the visible GPUs
    # round-robin and time over gloo -- the whole multi-rank path (launch, per-rank engines and
    # inputs, barriers, max-over-ranks) on a box with fewer GPUs than ranks
    share = os.environ.get("MMF_BENCH_SHARE_GPU") == "1"
    if share:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # MMF_BENCH_FORCE_DIST=1: the process group even at world 1, so the one-GPU box exercises the
    # RCCL branch of the timing (tests/test_gpu_rccl.py)
    force_dist = os.environ.get("MMF_BENCH_FORCE_DIST") == "1"
    backend = "gloo" if share else "nccl"
    dist = benchrun.init_dist(world, backend, dev, force=force_dist)
    tdev = None if share else dev  # device of the max-over-ranks reduction (gloo: host)

    import mmf_amd.weights as W
    from mmf_amd.engine import Engine

    B = a.batch
    benchrun.progress(f"rank {rank}/{world}: building the engine on cuda:{local}")
    det = W.synthetic_detector_state(0)
    t_build = time.perf_counter()
    eng = Engine(local, det, W.synthetic_clip_state(0), max_batch=B)
    t_build = time.perf_counter() - t_build  # weight packing + load-time calibrations
    t = build_inputs(eng, B, rank)
    # each rank's engine build (N engines packing and calibrating side by side)
    build_s = benchrun.gather_per_rank(t_build, world, rank, dist, tdev)
    sync = torch.cuda.synchronize

    benchrun.progress("timed region: PCIe-inclusive (headline)")
    # headline: inputs from pinned host memory every step, results back to the host
    host = {k: v.cpu().pin_memory() for k, v in t.items()}
    pipe = eng.host_pipeline(B, host["rid"].shape[1], host["cid"].shape[1])
    dt = benchrun.timed_steps(lambda: pipe.submit(host), a.steps, a.warmup, dist, sync, tdev)
    value = benchrun.whole_job_rate(world, B, a.steps, dt)
    h2d = sum(v.numel() * v.element_size() for v in host.values())
    benchrun.progress(f"headline {value:.1f} pairs/s")
    if a.dump_outputs:
        if pipe.i == 0:
            raise SystemExit("--dump-outputs needs at least one step")
        # what the caller of the last timed submit receives: that slot's pinned host result tensors
        dump_outputs(a.dump_outputs, pipe.result((pipe.i - 1) % pipe.n), rank)

    hbm_resident = roofline = configs = per_sample = cpu = None
    if a.full:
        benchrun.progress("timed region: HBM-resident")
        # secondary: inputs already resident in HBM
        out = eng.alloc_outputs(B)

        def step():
            eng.analyze_batch(t["rid"], t["rm"], t["cid"], t["cm"], t["img"], out=out)
        dt_hbm = benchrun.timed_steps(step, a.steps, a.warmup, dist, sync, tdev)
        hbm = benchrun.whole_job_rate(world, B, a.steps, dt_hbm)
        hbm_resident = {"value": round(hbm, 2), "unit": "pairs/s", "ms_per_step": round(1000 * dt_hbm / a.steps, 3),
                        "note": "same step with inputs already in HBM and results left on the device"}
        if not a.no_profile:
            benchrun.progress("per-kernel event-timed pass")
            from mmf_amd.profiling import kernel_roofline
            roofline = kernel_roofline(eng, step, a.steps)
        if world == 1 and not a.no_configs:
            configs = config_lines(eng, t, a.steps, a.warmup, det)
        if world == 1 and not a.no_per_sample:
            per_sample = per_sample_lines()
        if world == 1 and not a.no_e2e:
            benchrun.progress("text + JPEG line: analyze_pairs")
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
            import e2e_pairs_bench
            per_sample = dict(per_sample or {}, text_jpeg_pairs=e2e_pairs_bench.bench_line())
        if rank == 0 and world == 1 and not a.no_cpu_baseline:
            cpu = cpu_baseline(a.cpu_seconds)
    if rank == 0:
        res = result_line(
            a, world, B, dt, value,
            "synthetic (seeded token ids, structured uint8 images, 2170-row vault); random-init weights",
            config_extra=dict({"h2d_bytes_per_step_per_gpu": h2d,
                               "engine_build_s_per_rank": [round(x, 2) for x in build_s],
                               "timing_collective": (f"{'rccl' if backend == 'nccl' else backend}: barrier + "
                                                     f"all_reduce(MAX) over {world} rank(s)" if dist else None)},
                              **({"rehearsal": f"{world} ranks sharing {torch.cuda.device_count()} GPU(s) over gloo "
                                                "(MMF_BENCH_SHARE_GPU=1): a functional check, not a measurement"}
                                 if share else {})),
            hbm_resident=hbm_resident,
            achieved_tflops_whole_path=round(value * GFLOP_PER_PAIR / 1e3, 1),
            achieved_tflops_whole_path_executed=round(value * GFLOP_EXEC_PER_PAIR / 1e3, 1),
            work_per_pair={"algorithmic_gflop": GFLOP_PER_PAIR, "executed_gflop": GFLOP_EXEC_PER_PAIR,
                           "note": "algorithmic = every encoder layer in full (SURVEY.md §8d); executed = what "
                                   "the kernels compute (compact last layers: pooled rows only after the "
                                   "attention)"},
            roofline=roofline, configs=configs, per_sample=per_sample, cpu_baseline=cpu)
        print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
