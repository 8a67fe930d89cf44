"""The embeddings database's readers on the CPU: io_utils.load_vault_db (the full schema that
generate_embeddings_database pickles, behind the restricted unpickler) and
vault_builder.search_similar_articles (train_clip_detective.py:610-688) with numpy stand-ins for the
CLIP towers and for the device search; on the GPU tests/test_gpu_vault_fused.py runs both on the HIP
kernels.  Also: the C header and the library agree on the raw search entries."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "mmf_hip.h")
N = 12
KEYS = ["rank", "article_id", "similarity", "text", "image_path"]


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _db(n=N, seed=3):
    rng = np.random.default_rng(seed)
    return {
        "article_ids": [f"id{i}" for i in range(n)],
        "text_contents": [f"article {i} " + "x" * (90 + 3 * i) for i in range(n)],
        "image_paths": [f"/data/img{i}.png" for i in range(n)],
        "image_embeddings": _unit(rng.standard_normal((n, 512))),
        "text_embeddings": _unit(rng.standard_normal((n, 512))),
        "metadata": {"model_path": "/m.pth", "total_articles": n, "embedding_dim": 512, "val_accuracy": 0.5},
    }


def _Proc(table):
    """Tokenizer stand-in: one fixed id sequence per text."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from tables import TableClipProcessor
    return TableClipProcessor(table)


def _np_search(q, rows, k):
    s = np.dot(np.asarray(rows), q)
    top = np.argsort(s)[::-1][:k]
    return s[top], top


def _encoder(text_row=None, image_row=None, seen=None):
    """(pixels, ids, mask) -> (image rows, text rows): fixed un-normalised rows, the absent one None."""
    def enc(px, ids, mask):
        if seen is not None:
            seen.append((None if px is None else px.shape, None if ids is None else ids.shape))
        return (None if px is None else image_row[None] * 3.0, None if ids is None else text_row[None] * 3.0)
    return enc


def test_load_vault_db_round_trip(tmp_path):
    """A database written by generate_embeddings_database (stand-in encoder) comes back whole."""
    import json
    import torch
    from PIL import Image
    import mmf_amd.synthetic as syn
    from mmf_amd import io_utils
    from mmf_amd.vault_builder import generate_embeddings_database
    tmp = str(tmp_path)
    n = 5
    imgs = syn.images(n, 9)
    arts, table = [], {}
    for i in range(n):
        p = os.path.join(tmp, f"a{i}.png")
        Image.fromarray(imgs[i]).save(p)
        table[f"text {i}"] = [49406, 300 + i, 49407]
        arts.append({"article_id": f"id{i}", "text_content": f"text {i}", "image_local_path": p})
    with open(os.path.join(tmp, "seed.json"), "w") as f:
        json.dump(arts, f)
    rng = np.random.default_rng(0)
    proj_i, proj_t = rng.standard_normal((3, 512)), rng.standard_normal((77, 512))

    def enc(px, ids, mask):  # any deterministic map to non-zero rows
        pi = px.reshape(len(px), -1, 3).mean(1) @ proj_i
        pt = (ids * mask).astype(np.float64) @ proj_t
        return torch.as_tensor(_unit(pi)), torch.as_tensor(_unit(pt))

    out = os.path.join(tmp, "db.pkl")
    db = generate_embeddings_database("m.pth", os.path.join(tmp, "seed.json"), out, processor=_Proc(table), encode=enc,
                                      val_accuracy=0.75, batch=2)
    got = io_utils.load_vault_db(out)
    assert list(got) == list(io_utils.VAULT_DB_KEYS) == ["article_ids", "text_contents", "image_paths",
                                                         "image_embeddings", "text_embeddings", "metadata"]
    for k in ("article_ids", "text_contents", "image_paths", "metadata"):
        assert got[k] == db[k], k
    for k in ("image_embeddings", "text_embeddings"):
        assert got[k].dtype == np.float32 and got[k].shape == (n, 512)
        np.testing.assert_array_equal(got[k], db[k])
    # load_vault (the analysis path's reader) still reads the same file its own way
    emb, meta = io_utils.load_vault(out)
    np.testing.assert_array_equal(emb, db["image_embeddings"])
    assert meta[0]["title"] == "text 0"


def test_load_vault_db_missing_and_unsafe(tmp_path):
    from mmf_amd import io_utils
    assert io_utils.load_vault_db(str(tmp_path / "nope.pkl")) is None
    bad = dict(_db(), metadata={"cb": os.getcwd})  # a pickled function reference: posix/nt.getcwd
    p = str(tmp_path / "bad.pkl")
    with open(p, "wb") as f:
        pickle.dump(bad, f)
    with pytest.raises(pickle.UnpicklingError):
        io_utils.load_vault_db(p)
    with open(p, "wb") as f:
        pickle.dump({"embeddings": np.zeros((2, 512), np.float32), "metadata": []}, f)
    with pytest.raises(ValueError):
        io_utils.load_vault_db(p)  # the analysis path's format is not an embeddings database


def test_search_similar_articles_text_and_image(tmp_path, capsys):
    from PIL import Image
    from mmf_amd.vault_builder import search_similar_articles
    db = _db()
    proc = _Proc({"a caption": [49406, 320, 1125, 49407]})
    seen = []
    enc = _encoder(text_row=db["text_embeddings"][7], image_row=db["image_embeddings"][2], seen=seen)
    res = search_similar_articles("a caption", top_k=5, search_mode="text", processor=proc, encode=enc,
                                  search=_np_search, db=db)
    out = capsys.readouterr().out
    assert "Searching for similar articles (mode: text, top_k: 5)..." in out and "Top 5 similar articles:" in out
    assert seen == [(None, (1, 77))]  # the text tower only, one padded row
    assert len(res) == 5 and all(list(r) == KEYS for r in res)
    assert [r["rank"] for r in res] == [1, 2, 3, 4, 5]
    s = db["text_embeddings"] @ db["text_embeddings"][7]
    order = np.argsort(s)[::-1][:5]
    assert [r["article_id"] for r in res] == [f"id{i}" for i in order] and order[0] == 7
    np.testing.assert_allclose([r["similarity"] for r in res], s[order], atol=1e-6)
    assert all(isinstance(r["similarity"], float) for r in res)
    assert all(a["similarity"] >= b["similarity"] for a, b in zip(res, res[1:]))
    for r, i in zip(res, order):
        assert r["text"] == db["text_contents"][i][:100] + "..." and len(r["text"]) == 103
        assert r["image_path"] == db["image_paths"][i]
    assert f"1. [{res[0]['similarity']:.4f}] id7" in out
    # image mode: the file through the CLIP geometry, ranked against the image table
    p = str(tmp_path / "q.png")
    Image.fromarray(np.full((40, 60, 3), 90, np.uint8)).save(p)
    seen.clear()
    res = search_similar_articles(None, p, top_k=3, search_mode="image", encode=enc, search=_np_search, db=db)
    assert seen == [((1, 224, 224, 3), None)]
    s = db["image_embeddings"] @ db["image_embeddings"][2]
    assert [r["article_id"] for r in res] == [f"id{i}" for i in np.argsort(s)[::-1][:3]]
    assert res[0]["article_id"] == "id2" and abs(res[0]["similarity"] - 1.0) < 1e-6
    # top_k beyond the database: every row, once
    res = search_similar_articles("a caption", top_k=40, processor=proc, encode=enc, search=_np_search, db=db)
    assert len(res) == N and sorted(r["article_id"] for r in res) == sorted(db["article_ids"])
    # a search that pads short results with index -1 (the device convention) loses the padding
    res = search_similar_articles("a caption", top_k=3, processor=proc, encode=enc, db=db,
                                  search=lambda q, rows, k: (np.array([0.5, -np.inf, -np.inf]), np.array([4, -1, -1])))
    assert [r["article_id"] for r in res] == ["id4"]


def test_search_similar_articles_from_file(tmp_path):
    from mmf_amd.vault_builder import search_similar_articles
    db = _db()
    p = str(tmp_path / "db.pkl")
    with open(p, "wb") as f:
        pickle.dump(db, f)
    proc = _Proc({"q": [49406, 320, 49407]})
    enc = _encoder(text_row=db["text_embeddings"][1])
    res = search_similar_articles("q", embeddings_db_path=p, top_k=2, processor=proc, encode=enc, search=_np_search)
    assert res[0]["article_id"] == "id1"
    with pytest.raises(FileNotFoundError):
        search_similar_articles("q", embeddings_db_path=str(tmp_path / "none.pkl"), processor=proc, encode=enc,
                                search=_np_search)


@pytest.mark.parametrize("kw", [
    dict(query_text="q", search_mode="multimodal"), dict(query_text="q", query_image_path="x.png", search_mode="multimodal"),
    dict(query_text="q", search_mode="audio"), dict(query_text=None, search_mode="text"),
    dict(query_text="", search_mode="text"), dict(query_text="q", query_image_path=None, search_mode="image"),
    dict(query_image_path="x.png", search_mode="text"),
])
def test_search_similar_articles_rejects(kw):
    from mmf_amd.vault_builder import search_similar_articles
    with pytest.raises(ValueError, match="Invalid search mode or missing query"):
        search_similar_articles(db=_db(), encode=_encoder(), search=_np_search, processor=None, **kw)


def test_search_similar_articles_raw_dot():
    """Database rows are not renormalised (np.dot(db, q), train_clip_detective.py:664): a long row
    outranks the query's own unit row."""
    from mmf_amd.vault_builder import search_similar_articles
    db = _db()
    q = db["text_embeddings"][3].copy()
    long = _unit(q + 0.9 * db["text_embeddings"][5]) * np.float32(4.0)  # cosine < 1, dot > 1
    db["text_embeddings"][9] = long
    res = search_similar_articles("q", top_k=2, processor=_Proc({"q": [49406, 320, 49407]}),
                                  encode=_encoder(text_row=q), search=_np_search, db=db)
    assert [r["article_id"] for r in res] == ["id9", "id3"]
    assert abs(res[0]["similarity"] - float(long @ q)) < 1e-5 and res[0]["similarity"] > 1.5
    assert abs(res[1]["similarity"] - 1.0) < 1e-6


def test_header_declares_and_library_exports_search_entries():
    import mmf_amd.hip as hip
    text = open(HEADER).read()
    assert re.search(r"int64_t\s+mmf_vault_search_ws_bytes\(int B, int k, int nblocks\);", text)
    assert re.search(r"int\s+mmf_vault_search_rows\(const float\* q_unit, const float\* bank_unit, int B, int N, int D, "
                     r"int k, float thresh,", text)
    lib = hip.load()
    for name in ("mmf_vault_search_rows", "mmf_vault_search_ws_bytes"):
        assert name in hip.SIGNATURES and getattr(lib, name) is not None
    # host-only size rule: candidates (value, index) per block, query and slot; 0 = the automatic 256 blocks
    assert lib.mmf_vault_search_ws_bytes(5, 8, 3) == 3 * 5 * 8 * 8
    assert lib.mmf_vault_search_ws_bytes(256, 5, 0) == 256 * 256 * 5 * 8
    assert lib.mmf_vault_search_ws_bytes(4, 9, 0) == 0 and lib.mmf_vault_search_ws_bytes(0, 5, 0) == 0
    # argument checks come before any device call
    assert lib.mmf_vault_search_rows(None, None, 1, 1, 512, 5, 0.85, None, None, None, 1, None, None, None, None, 0, 0,
                                     None) != 0
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, Nn, D, k, ws_bytes in ((1, 1, 256, 5, 1 << 20), (1, 1, 512, 9, 1 << 20), (1, 1, 512, 0, 1 << 20),
                                  (1, 1, 512, 5, 8), (0, 1, 512, 5, 1 << 20), (1, 0, 512, 5, 1 << 20)):
        rc = lib.mmf_vault_search_rows(p, p, B, Nn, D, k, 0.85, None, None, None, 1, None, None, None, p, ws_bytes, 0,
                                       None)
        assert rc != 0, (B, Nn, D, k, ws_bytes)
        assert lib.mmf_last_error()
    assert "vault_fused" in [lib.mmf_option_name(i).decode() for i in range(64) if lib.mmf_option_name(i)]
    assert hip.get_process_option("vault_fused") == int(os.environ.get("MMF_VAULT_FUSED", 2))
