"""CPU checks of the mixed-modality batch (posts with a text, an image or both): the host-only plan
helper mmf_mixed_plan through ctypes against a numpy restatement, and analyze_many's argument
handling and compaction with a stub engine (no GPU)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

EINVAL = -22


def _plan(mod):
    import mmf_amd.hip as hip
    lib = hip.load()
    m = np.ascontiguousarray(mod, dtype=np.uint8)
    B = m.size
    # exact-size outputs behind guard rows: the helper must write [B][3] and [3], nothing else
    rm = np.full((B + 2, 3), 77, np.int32)
    cnt = np.full(5, 77, np.int32)
    rc = lib.mmf_mixed_plan(m.ctypes.data_as(ctypes.c_void_p), B, rm[1:].ctypes.data_as(ctypes.c_void_p),
                            cnt[1:].ctypes.data_as(ctypes.c_void_p))
    assert (rm[0] == 77).all() and (rm[B + 1] == 77).all() and cnt[0] == 77 and cnt[4] == 77
    return rc, rm[1:B + 1], cnt[1:4]


def _plan_ref(mod):
    """Position of each row in the text / image / both lists (ascending batch order), -1 where absent."""
    m = np.asarray(mod)
    rm = np.full((m.size, 3), -1, np.int32)
    for l, sel in enumerate((m & 1 != 0, m & 2 != 0, m == 3)):
        rm[sel, l] = np.arange(sel.sum())
    return rm, np.array([(m & 1 != 0).sum(), (m & 2 != 0).sum(), (m == 3).sum()], np.int32)


_SEEDED = [np.random.default_rng(s).integers(1, 4, n) for s, n in ((0, 70), (1, 257), (2, 8))]


@pytest.mark.parametrize("mod", [[1] * 6, [2] * 6, [3] * 6, [1], [2], [3], [1, 3, 2, 3, 1], [3, 2, 2, 1, 2],
                                 [1, 2] * 5, [1, 2, 3] * 4, [3, 1] * 3] + _SEEDED,
                         ids=lambda m: "m" + "".join(str(int(v)) for v in m[:12]) + f"_B{len(m)}")
def test_mixed_plan_matches_numpy(mod):
    rc, rm, cnt = _plan(mod)
    ref_rm, ref_cnt = _plan_ref(mod)
    assert rc == 0
    np.testing.assert_array_equal(rm, ref_rm)
    np.testing.assert_array_equal(cnt, ref_cnt)
    assert cnt[0] + cnt[1] - cnt[2] == len(mod)


def test_mixed_plan_hand_written():
    rc, rm, cnt = _plan([1, 3, 2, 3, 1])
    assert rc == 0
    assert rm.tolist() == [[0, -1, -1], [1, 0, 0], [-1, 1, -1], [2, 2, 1], [3, -1, -1]]
    assert cnt.tolist() == [4, 3, 2]


@pytest.mark.parametrize("mod", [[0], [3, 0, 1], [1, 2, 0], [4], [1, 255]])
def test_mixed_plan_rejects_bad_rows(mod):
    assert _plan(mod)[0] == EINVAL


def test_mixed_plan_rejects_bad_arguments():
    import mmf_amd.hip as hip
    lib = hip.load()
    m = np.ones(4, np.uint8)
    rm, cnt = np.zeros((4, 3), np.int32), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.mmf_mixed_plan(p(m), 0, p(rm), p(cnt)) == EINVAL
    assert lib.mmf_mixed_plan(None, 4, p(rm), p(cnt)) == EINVAL
    assert lib.mmf_mixed_plan(p(m), 4, None, p(cnt)) == EINVAL
    assert lib.mmf_mixed_plan(p(m), 4, p(rm), None) == EINVAL


# ------------------------------------------------------------------------------------------------
# analyze_many with a stub engine
# ------------------------------------------------------------------------------------------------
class _StubEngine:
    max_batch, max_text_len, max_clip_len = 4, 128, 77

    def __init__(self):
        self.calls = []

    def resize_supported(self, w, h):
        return True

    def resize_images(self, rgb):
        # every test image is one solid colour: its red value names it
        eff = torch.stack([torch.full((224, 224, 3), int(a[0, 0, 0]), dtype=torch.uint8) for a in rgb])
        return eff, eff.clone()

    def analyze_mixed(self, modality, rid, rm, cid, cm, img, img_clip=None, out=None):
        self.calls.append(dict(modality=np.asarray(modality).tolist(), rid=rid, rm=rm, cid=cid, cm=cm, img=img,
                               img_clip=img_clip))
        B = len(modality)
        return {"scores": torch.zeros(B, 5), "text_similarity": torch.zeros(B), "probs": torch.zeros(B, 2),
                "verdict": torch.zeros(B, dtype=torch.int32), "confidence": torch.zeros(B),
                "rule": torch.full((B,), 5, dtype=torch.int32), "top_sims": torch.full((B, 5), 0.5),
                "top_idx": torch.zeros((B, 5), dtype=torch.int32)}

    def scores_overflow(self, scores):
        return False


class _CountingTokenizer:
    def __init__(self, tok):
        self.tok, self.calls = tok, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.tok(*a, **k)


@pytest.fixture()
def stub_forensics():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    mf = MisinfoForensics.__new__(MisinfoForensics)
    mf.engine = _StubEngine()
    mf.device = torch.device("cpu")
    mf.device_jpeg, mf._jpeg, mf._verbose = False, None, False
    mf.roberta_tokenizer = _CountingTokenizer(TableRobertaTokenizer({f"t{i}": [0, 100 + i, 2] for i in range(8)}))
    mf.clip_processor = TableClipProcessor({f"t{i}": [49406, 300 + i, 49407] for i in range(8)})
    mf.clip_eos_token_id = 49407
    mf.detector = types.SimpleNamespace(sync=lambda *a: None)
    mf.vault_loaded = True
    mf.vault_metadata = [{"title": "T"}]
    return mf


def _img(i):
    from PIL import Image
    return Image.fromarray(np.full((40 + 3 * i, 50 + i, 3), 10 + i, np.uint8))


def test_analyze_many_length_mismatch(stub_forensics):
    with pytest.raises(ValueError):
        stub_forensics.analyze_many(["t0", "t1"], [_img(0)])
    assert stub_forensics.engine.calls == []


@pytest.mark.parametrize("texts,images", [(["t0", None], [None, None]), (["t0", ""], [_img(0), None]),
                                          ([None], [None]), (["t0", "t1", ""], [None, None, b""])])
def test_analyze_many_row_without_input(stub_forensics, golden_json, texts, images):
    with pytest.raises(ValueError) as e:
        stub_forensics.analyze_many(texts, images)
    assert str(e.value) == golden_json["analyze_no_input_error"]
    assert stub_forensics.engine.calls == [] and stub_forensics.roberta_tokenizer.calls == 0


def test_analyze_many_compacts_in_batch_order(stub_forensics):
    """Six posts through a stub engine of max_batch 4: two chunks; each chunk's compact lists hold
    the right texts and images at the right positions, and the dicts come back one per post."""
    texts = ["t0", "t1", None, "t3", "", "t5"]
    images = [None, _img(1), _img(2), _img(3), _img(4), None]
    res = stub_forensics.analyze_many(texts, images)
    c0, c1 = stub_forensics.engine.calls
    assert c0["modality"] == [1, 3, 2, 3] and c1["modality"] == [2, 1]
    assert c0["rid"][:, 1].tolist() == [100, 101, 103] and (np.asarray(c0["rm"]) == 1).all()
    assert c0["cid"][:, 1].tolist() == [301, 303]
    assert c0["img"][:, 0, 0, 0].tolist() == [11, 12, 13] and c0["img_clip"][:, 0, 0, 0].tolist() == [11, 12, 13]
    assert c1["rid"][:, 1].tolist() == [105] and c1["cid"] is None and c1["cm"] is None
    assert c1["img"][:, 0, 0, 0].tolist() == [14]
    assert len(res) == 6
    # rows without an image report no vault matches; the stub's top-5 reaches the others
    assert [len(r["vault_matches"]) for r in res] == [0, 5, 5, 5, 5, 0]
    assert all(r["verdict_text"] == "REAL" and set(r) == {"verdict", "verdict_text", "confidence", "scores",
                                                          "vault_matches", "explanation"} for r in res)


def test_analyze_many_text_only_and_image_only_feeds(stub_forensics):
    stub_forensics.analyze_many(["t0", "t1"], [None, None])
    c = stub_forensics.engine.calls[-1]
    assert c["modality"] == [1, 1] and c["img"] is None and c["cid"] is None and c["rid"].shape[0] == 2
    stub_forensics.analyze_many([None, ""], [_img(0), _img(1)])
    c = stub_forensics.engine.calls[-1]
    assert c["modality"] == [2, 2] and c["rid"] is None and c["cid"] is None
    assert c["img"][:, 0, 0, 0].tolist() == [10, 11]
    assert stub_forensics.analyze_many([], []) == []
