"""Batches of posts with a text, an image or both (mmf_analyze_mixed / Engine.analyze_mixed /
MisinfoForensics.analyze_many) on the MI355X: the reference's own single-modality results
(tests/golden/golden.json), and bit-identity with the separate entry points -- analyze_batch for
the pairs, text_forward / effnet_forward / clip_image + vault_topk for the rest (the project holds a
row's results independent of the batch it runs in: test_gpu_parity.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("scores", "text_similarity", "probs", "verdict", "confidence", "rule", "top_sims", "top_idx")
F32 = np.float32


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run_mixed(eng, golden, imgs, mod, rows):
    """analyze_mixed on batch rows = golden samples `rows` with modalities `mod` (compact inputs)."""
    mod, rows = np.asarray(mod), np.asarray(rows)
    t, i, c = rows[mod & 1 != 0], rows[mod & 2 != 0], rows[mod == 3]
    return _np(eng.analyze_mixed(mod, golden["rob_ids"][t] if len(t) else None, golden["rob_mask"][t] if len(t) else None,
                                 golden["clip_ids"][c] if len(c) else None, golden["clip_mask"][c] if len(c) else None,
                                 imgs[i] if len(i) else None))


def _rule(s):
    """The explanation cascade over (ai, misinfo, deepfake, clip_similarity, vault_discrepancy), fp32."""
    r = np.where(s[:, 3] < F32(0.3), 4, 5)
    for col, idx in ((1, 3), (0, 2), (2, 1), (4, 0)):
        r = np.where(s[:, col] > F32(0.7), idx, r)
    return r.astype(np.int32)


def _separate(eng, golden, imgs, mod, rows, vault=True):
    """The same posts through the separate entry points: what analyze_mixed must equal bit for bit."""
    mod, rows = np.asarray(mod), np.asarray(rows)
    B = len(mod)
    exp = {"scores": np.zeros((B, 5), F32), "text_similarity": np.zeros(B, F32), "top_sims": np.zeros((B, 5), F32),
           "top_idx": np.full((B, 5), -1, np.int32)}
    mt, mi, mc = mod & 1 != 0, mod & 2 != 0, mod == 3
    if mt.any():
        exp["scores"][mt, :2] = eng.text_forward(golden["rob_ids"][rows[mt]], golden["rob_mask"][rows[mt]])[2].cpu().numpy()
    if mi.any():
        exp["scores"][mi, 2] = eng.effnet_forward(imgs[rows[mi]])[1].cpu().numpy()
        if vault:
            sims, idx, disc, _ = eng.vault_topk(eng.clip_image(imgs[rows[mi]]), 5, 0.85, None)
            exp["top_sims"][mi], exp["top_idx"][mi] = sims.cpu().numpy(), idx.cpu().numpy()
            exp["scores"][mi, 4] = disc.cpu().numpy()
    pairs = None
    if mc.any():
        # analyze_batch's rows are bit-identical across batch sizes only while each tower stays on the
        # same side of its small-batch threshold (RoBERTa <= 512 stream rows and CLIP
        # < 256 run materialised LayerNorms with split-K GEMMs).  The reference batch is the pairs
        # alone, or every row of the batch as a pair (the golden samples all have both), whichever
        # puts the three towers in the regimes of the mixed batch's lists.
        want = _regimes(mt.sum(), mi.sum(), mc.sum())
        if _regimes(mc.sum(), mc.sum(), mc.sum()) == want:
            r, pick = rows[mc], slice(None)
        else:
            assert _regimes(B, B, B) == want, (want, "no reference batch in the same regimes")
            r, pick = rows, mc
        ab = _np(eng.analyze_batch(golden["rob_ids"][r], golden["rob_mask"][r], golden["clip_ids"][r],
                                   golden["clip_mask"][r], imgs[r]))
        pairs = {k: v[pick] for k, v in ab.items()}
    return exp, pairs


def _regimes(n_text, n_img, n_cap, Lr=128, Lc=77):
    return int(n_text) * Lr > 512, int(n_img) * 50 >= 256, int(n_cap) * Lc >= 256


def _check_mixed(eng, golden, imgs, mod, rows, vault=True):
    mod = np.asarray(mod)
    got = _run_mixed(eng, golden, imgs, mod, rows)
    exp, pairs = _separate(eng, golden, imgs, mod, rows, vault)
    B = len(mod)
    for k in KEYS:
        assert got[k].shape[0] == B and np.isfinite(got[k]).all(), k
    mc = mod == 3
    if pairs is not None:  # the pairs: every output key equals analyze_batch on those rows
        for k in KEYS:
            np.testing.assert_array_equal(got[k][mc], pairs[k], err_msg=k)
        # their towers' scores also equal the separate tower calls (the rows ran in other batches there)
        np.testing.assert_array_equal(got["scores"][mc][:, [0, 1, 2, 4]], exp["scores"][mc][:, [0, 1, 2, 4]])
        np.testing.assert_array_equal(got["top_sims"][mc], exp["top_sims"][mc])
        np.testing.assert_array_equal(got["top_idx"][mc], exp["top_idx"][mc])
    single = ~mc
    if not single.any():
        return got
    # single-modality rows: tower outputs from the separate calls, absent slots exactly 0 / -1
    for k in ("scores", "text_similarity", "top_sims", "top_idx"):
        np.testing.assert_array_equal(got[k][single], exp[k][single], err_msg=k)
    s = got["scores"][single]
    text_only = (mod == 1)[single]
    assert (s[text_only][:, 2:] == 0).all() and (got["top_idx"][single][text_only] == -1).all()
    assert (s[~text_only][:, [0, 1, 3]] == 0).all() and (got["text_similarity"][single] == 0).all()
    if vault and (~text_only).any():
        assert (got["top_idx"][single][~text_only] >= 0).all()
    # the reference's verdict without fusion (misinfo_forensics.py:883-899), restated in fp32 from those scores
    fake = np.clip(np.where(text_only, s[:, 1], np.maximum(s[:, 2], s[:, 4])), F32(0), F32(1)).astype(F32)
    real = (F32(1) - fake).astype(F32)
    verdict = fake > F32(0.5)
    np.testing.assert_array_equal(got["probs"][single], np.stack([real, fake], 1))
    np.testing.assert_array_equal(got["verdict"][single], verdict.astype(np.int32))
    np.testing.assert_array_equal(got["confidence"][single], np.where(verdict, fake, real))
    np.testing.assert_array_equal(got["rule"], _rule(got["scores"]))
    return got


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine_base(det_sd, clip_sd, golden_inputs):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    eng = Engine(0, det_sd, clip_sd, eos_token_id=golden_inputs["eos"], max_batch=72)
    assert eng.ready == 31
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def no_vault_checked(engine_base, golden, golden_inputs):
    """The no-vault cases, run on the engine before `engine` sets its vault."""
    assert engine_base.ready == 31
    imgs = golden_inputs["imgs"]
    got = _check_mixed(engine_base, golden, imgs, [2, 1, 3, 2, 3], [0, 1, 2, 3, 4], vault=False)
    got1 = _check_mixed(engine_base, golden, imgs, [2, 2], [5, 6], vault=False)
    return got, got1


@pytest.fixture(scope="module")
def engine(engine_base, no_vault_checked, golden, golden_inputs):
    gi = golden_inputs
    tmask = np.zeros((2170, 77), np.int32)
    for j, t in enumerate(gi["title_ids"]):
        tmask[j, :len(t)] = 1
    engine_base.set_vault(gi["vault"], golden["title_clip_ids"], tmask)
    assert engine_base.ready == 63
    return engine_base


ORDER = [4, 0, 2, 5, 1, 3, 6, 7]          # batch order of the golden samples
MOD = [3, 1, 2, 3, 1, 2, 3, 3]            # samples 0, 1 text only; 2, 3 image only; the rest both


def test_no_vault(no_vault_checked):
    """No vault set: vault outputs 0 / -1 on every row, the image-only verdict from deepfake alone."""
    for got in no_vault_checked:
        assert (got["scores"][:, 4] == 0).all() and (got["top_sims"] == 0).all() and (got["top_idx"] == -1).all()
        assert (got["text_similarity"] == 0).all()
    got = no_vault_checked[1]
    np.testing.assert_array_equal(got["probs"][:, 1], np.clip(got["scores"][:, 2], 0, 1))


def test_mixed_batch_equals_separate_entry_points(engine, golden, golden_inputs):
    got = _check_mixed(engine, golden, golden_inputs["imgs"], MOD, ORDER)
    # the planted vault rows are found on image rows (samples 2 and 3 among them), never on text-only rows
    assert (got["scores"][np.asarray(MOD) == 2, 4] > 0.85).all()


def test_all_pairs_batch_equals_analyze_batch(engine, golden, golden_inputs):
    imgs = golden_inputs["imgs"]
    got = _run_mixed(engine, golden, imgs, [3] * 8, list(range(8)))
    ref = _np(engine.analyze_batch(golden["rob_ids"], golden["rob_mask"], golden["clip_ids"], golden["clip_mask"], imgs))
    for k in KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("mod,rows", [
    ([1], [3]), ([2], [3]), ([3], [3]),                        # B = 1 of each modality
    ([1, 3, 3, 2, 2], [0, 1, 2, 3, 4]),                        # B = 5: the second block holds one row
    ([3, 1, 2, 1, 1], [7, 6, 5, 4, 3]),
    ([1] * 6, [0, 1, 2, 3, 4, 5]),                             # text only: no image or CLIP-text input at all
    ([2] * 6, [2, 3, 4, 5, 6, 7]),                             # image only
    ([(1, 2, 3)[i % 3] for i in range(70)], [i % 8 for i in range(70)]),  # B = 70 > mt_enqueue = 64
], ids=["B1_text", "B1_image", "B1_both", "B5_a", "B5_b", "text_only", "image_only", "B70_event_chain"])
def test_edge_shapes(engine, golden, golden_inputs, mod, rows):
    if len(mod) > 64:
        assert engine.get_option("mt_enqueue") == 64  # above it: the event-chained enqueue, not the host threads
    _check_mixed(engine, golden, golden_inputs["imgs"], mod, rows)


def test_row_without_modality_is_rejected(engine, golden, golden_inputs, golden_json):
    with pytest.raises(ValueError) as e:
        _run_mixed(engine, golden, golden_inputs["imgs"], [1, 0, 3], [0, 1, 2])
    assert str(e.value) == golden_json["analyze_no_input_error"]


def test_counts_must_describe_the_batch(engine, golden, golden_inputs):
    """The C entry point checks the counts against B before anything is launched."""
    import ctypes
    from mmf_amd import hip
    out = engine.alloc_outputs(4)
    dmap = torch.zeros((4, 3), dtype=torch.int32, device=engine.device)
    ids = torch.zeros((4, 8), dtype=torch.int32, device=engine.device)
    p = hip.ptr
    for nT, nI, nC in ((3, 0, 0), (4, 0, 1), (2, 1, 0), (5, 0, 0)):
        rc = engine.lib.mmf_analyze_mixed(engine.h, p(dmap), 4, nT, nI, nC, p(ids), p(ids), 8, None, None, 0, None, None,
                                          p(out["scores"]), None, p(out["probs"]), None, None, None, None, None,
                                          hip.stream_ptr())
        assert rc == -22, (nT, nI, nC)


def test_out_of_range_map_entries_count_as_absent(engine, golden, golden_inputs):
    """A row map with positions outside its lists: those entries are treated as absent (no read past
    the compact buffers), the other rows are unaffected."""
    from mmf_amd import hip
    mod, rows = np.asarray([1, 3, 2, 3]), np.asarray([0, 1, 2, 3])
    good = _run_mixed(engine, golden, golden_inputs["imgs"], mod, rows)
    row_map, (nT, nI, nC) = engine.mixed_plan(mod)
    bad = row_map.copy()
    bad[0] = [1 << 30, -5, 7]       # row 0: nothing valid -> an all-zero row
    bad[2] = [-1, nI, -1]           # row 2: image position one past the list -> absent
    t, i, c = rows[mod & 1 != 0], rows[mod & 2 != 0], rows[mod == 3]
    args = [engine._i32(golden["rob_ids"][t]), engine._i32(golden["rob_mask"][t]), engine._i32(golden["clip_ids"][c]),
            engine._i32(golden["clip_mask"][c]), engine._u8(golden_inputs["imgs"][i])]
    dmap = torch.from_numpy(bad).to(engine.device)
    out = engine.alloc_outputs(4)
    p = hip.ptr
    hip.check(engine.lib.mmf_analyze_mixed(
        engine.h, p(dmap), 4, nT, nI, nC, p(args[0]), p(args[1]), args[0].shape[1], p(args[2]), p(args[3]),
        args[2].shape[1], p(args[4]), None, p(out["scores"]), p(out["text_similarity"]), p(out["probs"]),
        p(out["verdict"]), p(out["confidence"]), p(out["rule"]), p(out["top_sims"]), p(out["top_idx"]),
        hip.stream_ptr()), "mmf_analyze_mixed")
    got = _np(out)
    for r in (0, 2):
        assert (got["scores"][r] == 0).all() and (got["top_idx"][r] == -1).all() and (got["top_sims"][r] == 0).all()
        assert got["probs"][r].tolist() == [1.0, 0.0] and got["verdict"][r] == 0
    for k in KEYS:
        np.testing.assert_array_equal(got[k][[1, 3]], good[k][[1, 3]], err_msg=k)


def test_ready_mask_per_batch(det_sd, golden, golden_inputs):
    """Only the components a batch uses must be loaded: a detector-only engine (no CLIP) runs a
    text-only batch, and refuses a batch with an image row with MMF_EINVAL."""
    from mmf_amd import hip
    from mmf_amd.engine import Engine
    eng = Engine(0, det_sd, None, max_batch=8)
    try:
        assert eng.ready & 12 == 0
        got = _run_mixed(eng, golden, golden_inputs["imgs"], [1, 1, 1], [0, 1, 2])
        ref = eng.text_forward(golden["rob_ids"][:3], golden["rob_mask"][:3])[2].cpu().numpy()
        np.testing.assert_array_equal(got["scores"][:, :2], ref)
        assert (got["scores"][:, 2:] == 0).all()
        np.testing.assert_array_equal(got["probs"][:, 1], np.clip(ref[:, 1], 0, 1))
        with pytest.raises(hip.MMFError, match=r"\(-22\)"):
            _run_mixed(eng, golden, golden_inputs["imgs"], [1, 2, 1], [0, 1, 2])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forensics(golden, golden_inputs, det_sd, clip_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    from test_gpu_api import _tables
    rob, clp = _tables(golden, golden_inputs)
    mf = MisinfoForensics(fusion_weights="/nonexistent", faiss_index_path="/nonexistent",
                          roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=TableClipProcessor(clp),
                          detector_state=det_sd, clip_state=clip_sd, max_batch=8, verbose=False)
    mf.set_vault(golden_inputs["vault"], golden_inputs["meta"])
    yield mf
    mf.engine.close()


def _feed(golden_inputs, order, mod):
    from PIL import Image
    texts = [f"sample text {g}" if m & 1 else None for g, m in zip(order, mod)]
    images = [Image.fromarray(golden_inputs["imgs"][g]) if m & 2 else None for g, m in zip(order, mod)]
    return texts, images


def test_analyze_many_matches_reference(forensics, golden_json, golden_inputs):
    """One mixed batch through analyze_many against the reference's own analyze() results: text only,
    image only and pairs."""
    from test_gpu_api import _check
    res = forensics.analyze_many(*_feed(golden_inputs, ORDER, MOD))
    assert len(res) == 8
    for got, g, m in zip(res, ORDER, MOD):
        ref = (golden_json["analyze_text_only"][g] if m == 1 else
               golden_json["analyze_image_only"][g - 2] if m == 2 else golden_json["analyze"][g])
        _check(got, ref)
        if m == 1:
            assert got["vault_matches"] == []


def test_analyze_many_chunks_past_capacity(forensics, golden_inputs):
    """More posts than the reserved batch (8): two chunks (8 + 3 posts) with different modality
    mixes, the dicts in order and equal to the same posts analysed in other batches (5 + 6) at the
    project's tolerance (small batches take the towers' small-batch paths, which round differently)."""
    from test_gpu_api import _check
    order = ORDER + [2, 0, 3]
    mod = MOD + [2, 1, 3]
    res = forensics.analyze_many(*_feed(golden_inputs, order, mod))
    assert len(res) == 11
    head = forensics.analyze_many(*_feed(golden_inputs, order[:5], mod[:5]))
    tail = forensics.analyze_many(*_feed(golden_inputs, order[5:], mod[5:]))
    for a, b in zip(res, head + tail):
        _check(a, b)
