"""Option clip_qkv_attn at the towers' level: the CLIP encoders with the attention of every layer run inside the
lazy-LN QKV consumer's epilogue (csrc/gemm.hip epi 5) against the two-launch form (consumer GEMM, then
attention_kernel), on one engine.  The epilogue performs the same operations in the same order, so every output
is bit-identical: embeddings, clip_consistency and analyze_batch, with ragged captions (the text tower's causal
and key-padding masks), batches whose last tile is partly filled, a batch below the lazy path's threshold (which
must not change at all) and repeated calls."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 37


@pytest.fixture(scope="module")
def eng(det_sd, clip_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.synthetic as syn
    from mmf_amd.engine import Engine
    e = Engine(0, det_sd, clip_sd, max_batch=CAP)
    e.set_vault(syn.vault(300, 512, 5))
    yield e
    e.close()


def _inputs(B, seed):
    import mmf_amd.synthetic as syn
    rid, rm = syn.roberta_ids(B, 128, seed, [128, 60, 7])
    cid, cm = syn.clip_ids(B, 77, seed, [77, 33, 3, 50, 12])      # captions of 3 .. 77 tokens
    return rid, rm, cid, cm, syn.images(B, seed)


def _both(eng, fn):
    """fn() under clip_qkv_attn = 0, 1, 1 again, then per tower (2: ViT only, 4: text tower only) -> outputs."""
    old = eng.get_option("clip_qkv_attn")
    outs = []
    try:
        for v in (0, 1, 1, 2, 4):
            eng.set_option("clip_qkv_attn", v)
            o = fn()
            torch.cuda.synchronize()
            outs.append({k: t.clone() for k, t in o.items()})
    finally:
        eng.set_option("clip_qkv_attn", old)
    return outs


def _all_equal(outs):
    for i, o in enumerate(outs[1:], 1):
        for k, t in outs[0].items():
            assert torch.equal(t, o[k]), (i, k, (t.float() - o[k].float()).abs().max().item())


@pytest.mark.parametrize("B", [6, 37])      # ViT M = 300 / 1850, text M = 462 / 2849: the lazy path, ragged last tiles
def test_embeddings_bit_identical(eng, B):
    rid, rm, cid, cm, imgs = _inputs(B, 41)
    outs = _both(eng, lambda: {"img": eng.clip_image(imgs), "txt": eng.clip_text(cid, cm)})
    assert all(bool(torch.isfinite(t).all()) for t in outs[0].values())
    _all_equal(outs)


@pytest.mark.parametrize("B", [6, 37])
def test_consistency_and_analyze_bit_identical(eng, B):
    rid, rm, cid, cm, imgs = _inputs(B, 43)

    def run():
        o = {"cons_" + k: v for k, v in eng.clip_consistency(imgs, cid, cm).items()}
        o.update(eng.analyze_batch(rid, rm, cid, cm, imgs))
        return o
    _all_equal(_both(eng, run))


def test_small_batch_unchanged(eng):
    """B = 2 (M = 100 / 154 rows) runs the materialised LayerNorms whatever the option says."""
    rid, rm, cid, cm, imgs = _inputs(2, 47)
    _all_equal(_both(eng, lambda: {"img": eng.clip_image(imgs), "txt": eng.clip_text(cid, cm)}))


def test_fused_launch_is_taken(eng):
    """The event profiler sees the 24 stand-alone attention launches of the two towers turn into epi 5 GEMMs."""
    from mmf_amd.profiling import profile_kernels
    rid, rm, cid, cm, imgs = _inputs(6, 53)
    old = eng.get_option("clip_qkv_attn")
    counts = {}
    try:
        for v in (0, 1):
            eng.set_option("clip_qkv_attn", v)
            rows = profile_kernels(eng, lambda: eng.clip_consistency(imgs, cid, cm), 1)
            counts[v] = (sum(r["launches_per_step"] for r in rows if r["kernel"] == "attention"),
                         sum(r["launches_per_step"] for r in rows if r["kernel"].endswith("epi=5")))
    finally:
        eng.set_option("clip_qkv_attn", old)
    assert counts[0] == (24, 0) and counts[1] == (0, 24), counts
