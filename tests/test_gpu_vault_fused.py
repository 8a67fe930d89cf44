"""Fused Truth-Vault search (vault_search_partial_kernel + merge, option vault_fused, the raw entry
mmf_vault_search_rows) against the two-kernel path it replaces on large vaults -- the similarity
matrix + register / LDS-sort top-k, which stay the vault_fused = 0 and vault_ref paths.  Both rank
the same fp32-MFMA chains under one strict total order, so everything is compared BIT for bit (NaN
similarities of zero rows included: the comparison is on the bit patterns)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.vault_refs import rank as _rank  # the project's ranking in numpy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
CAP = 40  # reserved batch of the shared engine (the raw-entry shapes go up to B = 37)


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


@pytest.fixture(scope="module")
def engine(clip_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    eng = Engine(0, None, clip_sd, max_batch=CAP)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine8(clip_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    eng = Engine(0, None, clip_sd, max_batch=8)
    yield eng
    eng.close()


def _title_inputs(N):
    ids = np.full((N, 77), 49407, np.int32)
    ids[:, 0] = 49406
    mask = np.zeros_like(ids)
    mask[:, :2] = 1
    return ids, mask


@pytest.mark.parametrize("N", [1, 3, 7, 63, 64, 65, 1001, 2171])
def test_raw_entry_matches_two_kernel_path(engine, N):
    """mmf_vault_search_rows (Engine.search_rows) against engine.vault_topk at vault_fused = 0 -- the
    similarity-matrix path as it was before the fused kernels existed -- on ragged vault sizes, query
    counts around the 16-query MFMA group, every register k (k > N included: the two-kernel entry
    takes k <= N, so its N results are compared with the first N slots and the rest must be the
    (-inf, -1) padding), and vault partitions of 1, 2, 3 blocks (2 blocks at N = 1001: 8 tiles each)
    and the automatic grid.  The vault holds planted hits above 0.85, two bit-equal rows that the
    first query ties on, and one zero row (a NaN similarity for every query)."""
    from mmf_amd import io_utils
    rng = np.random.default_rng(100 + N)
    vault = rng.standard_normal((N, 512)).astype(np.float32)
    BMAX = 37
    q = rng.standard_normal((BMAX, 512)).astype(np.float32)
    q[:5] = vault[rng.integers(0, N, 5)] * 3.0  # planted hits
    a = b = z = -1
    if N >= 3:
        a, b, z = (int(x) for x in rng.choice(N, 3, replace=False))
        vault[b] = vault[a]              # bit-equal duplicates: an exact tie ...
        q[0] = vault[a] * 2.0            # ... at the top of query 0
    ids, mask = _title_inputs(N)
    # the title bank as mmf_set_vault_titles computes it: the CLIP text tower in batches of the reserved size
    titles = torch.cat([engine.clip_text(ids[i:i + CAP], mask[i:i + CAP]) for i in range(0, N, CAP)])
    qu = torch.as_tensor(q / np.linalg.norm(q, axis=1, keepdims=True)).cuda()
    temb = torch.nn.functional.normalize(torch.randn(BMAX, 512, generator=torch.Generator().manual_seed(N))).cuda()
    old = engine.get_option("vault_fused")
    engine.set_option("vault_fused", 0)
    try:
        # without and with the zero row (its NaN tops every query, so nothing is a hit beside it)
        for zero_row in ((False, True) if N >= 3 else (False,)):
            if zero_row:
                vault[z] = 0.0           # 0 / 0 = NaN
            engine.set_vault(vault, ids, mask)
            bank = torch.as_tensor(np.ascontiguousarray(io_utils.vault_unit_rows(vault), dtype=np.float32)).cuda()
            hits = 0
            for B in (1, 5, 16, 17, 37):
                for k in (1, 3, 5, 8):
                    kr = min(k, N)
                    ref = [t.clone() for t in engine.vault_topk(qu[:B], kr, 0.85, temb[:B])]
                    hits += int((ref[2] > 0.85).sum())
                    for nblocks in (1, 2, 3, 0):
                        got = engine.search_rows(qu[:B], bank, k, 0.85, temb[:B], titles, nblocks)
                        torch.cuda.synchronize()
                        what = (N, zero_row, B, k, nblocks)
                        assert _bits_equal(got[0][:, :kr].contiguous(), ref[0]), ("sims",) + what
                        assert _bits_equal(got[1][:, :kr].contiguous(), ref[1]), ("idx",) + what
                        assert _bits_equal(got[2], ref[2]), ("disc",) + what
                        assert _bits_equal(got[3], ref[3]), ("text_sim",) + what
                        assert bool((got[1][:, kr:] == -1).all()) and bool(torch.isneginf(got[0][:, kr:]).all()), what
            s1, i1, d1, t1 = engine.search_rows(qu[:1], bank, 3, 0.85, temb[:1], titles)
            if zero_row:   # the NaN row ranks first, the tie behind it by descending index; NaN is no hit
                assert bool(torch.isnan(s1[0, 0])) and i1[0].tolist() == [z] + sorted((a, b), reverse=True)
                assert hits == 0 and float(d1) == 0.0 and float(t1) == 0.0
            else:          # the planted rows exercise the hit and caption-similarity branch
                assert hits > 0 and float(d1) > 0.85 and float(t1) != 0.0
                assert N < 3 or i1[0, :2].tolist() == sorted((a, b), reverse=True)
    finally:
        engine.set_option("vault_fused", old)


@pytest.mark.parametrize("name", ["fp16", "ties", "zero", "threshold"])
def test_fused_vault_edge_case(engine8, name):
    """The reference's own search_vault results (tests/golden/golden_vault_edge.json, k = 5) with the
    vault served by the fused kernels (vault_fused = 1): the comparisons of
    tests/test_gpu_vault_edge.py::test_vault_edge_case."""
    import zlib
    import vault_edge as VE
    from mmf_amd import io_utils
    with open(os.path.join(HERE, "golden", "golden_vault_edge.json")) as f:
        case = json.load(f)["cases"][name]
    vault, q = VE.case(name)
    assert str(vault.dtype) == case["dtype"] and zlib.crc32(np.ascontiguousarray(vault).tobytes()) == case["vault_crc"]
    old = engine8.get_option("vault_fused")
    engine8.set_option("vault_fused", 1)
    try:
        engine8.set_vault(vault)
        qt = torch.as_tensor(q)
        qu = (qt / qt.norm(dim=-1, keepdim=True)).numpy()
        sims_np = io_utils.vault_unit_rows(vault) @ qu.T
        results = [r for r in case["results"] if r["top_k"] == 5]
        assert len(results) == VE.NQ
        for r in results:
            i, k = r["query"], r["top_k"]
            sims, idx, disc, _ = engine8.vault_topk(torch.as_tensor(qu[i:i + 1]).cuda(), k, 0.85)
            torch.cuda.synchronize()
            sims, idx, disc = sims.cpu().numpy()[0], idx.cpu().numpy()[0], float(disc.item())
            ref_s = np.array(r["sims"], dtype=np.float64)
            np.testing.assert_array_equal(np.isnan(sims), np.isnan(ref_s), err_msg=f"{name} q{i} NaN rows")
            fin = ~np.isnan(ref_s)
            np.testing.assert_allclose(sims[fin], ref_s[fin], atol=1e-6, err_msg=f"{name} q{i}")
            assert abs(disc - r["vault_discrepancy"]) < 1e-6, (name, i, disc, r["vault_discrepancy"])
            for p, (a, b) in enumerate(zip(idx.tolist(), r["idx"])):
                if a == b:
                    continue
                sa, sb = sims_np[a, i], sims_np[b, i]
                same = (np.isnan(sa) and np.isnan(sb)) or abs(float(sa) - float(sb)) <= 1e-6
                assert same, f"{name} q{i} pos {p}: got row {a} ({sa}), reference row {b} ({sb})"
    finally:
        engine8.set_option("vault_fused", old)


def test_large_vault_top5_and_top12(engine8):
    """A vault just past the 16384-row threshold under the default options: top-5 comes from the fused
    kernels, top-12 from the chunked sort (two chunks, 16384 + 64 rows) -- a call the library used to
    refuse.  Expected: a numpy ranking of the similarities that the VALU reference kernel (vault_ref =
    1) computes over the two 8224-row halves, each set as a vault of its own (a full top-N of a half
    returns every similarity with its row)."""
    N, H, B = 16448, 8224, 8
    rng = np.random.default_rng(16448)
    vault = rng.standard_normal((N, 512)).astype(np.float32)
    q = rng.standard_normal((B, 512)).astype(np.float32)
    q[0] = vault[16400] * 2.0   # a hit in the second chunk's 64 rows
    q[1] = vault[5] * 2.0
    vault[9000] = vault[16383]  # a tie across the chunk boundary ...
    q[2] = vault[9000] * 2.0
    vault[12345] = 0.0          # ... and a NaN row
    qu = torch.as_tensor(q / np.linalg.norm(q, axis=1, keepdims=True)).cuda()
    assert engine8.get_option("vault_fused") == 2 and engine8.get_option("vault_ref") == 0
    S = np.empty((B, N), np.float32)
    engine8.set_option("vault_ref", 1)
    try:
        for h in range(2):
            engine8.set_vault(vault[h * H:(h + 1) * H])
            s, i, _, _ = engine8.vault_topk(qu, H, 0.85)
            s, i = s.cpu().numpy(), i.cpu().numpy().astype(np.int64)
            assert (np.sort(i, axis=1) == np.arange(H)).all()
            np.put_along_axis(S[:, h * H:(h + 1) * H], i, s, axis=1)
    finally:
        engine8.set_option("vault_ref", 0)
    assert np.isnan(S[:, 12345]).all() and np.isnan(S).sum() == B
    engine8.set_vault(vault)
    for k in (5, 12):
        sims, idx, disc, _ = engine8.vault_topk(qu, k, 0.85)
        torch.cuda.synchronize()
        sims, idx, disc = sims.cpu().numpy(), idx.cpu().numpy(), disc.cpu().numpy()
        for b in range(B):
            es, ei = _rank(S[b], k)
            np.testing.assert_array_equal(idx[b], ei, err_msg=f"k={k} query {b}")
            np.testing.assert_array_equal(sims[b].view(np.int32), es.view(np.int32), err_msg=f"k={k} query {b}")
            assert np.isnan(es[0]) and disc[b] == 0.0  # (slot 0 is the NaN row, never a hit)
        assert idx[0, 1] == 16400 and idx[1, 1] == 5 and idx[2, 1:3].tolist() == [16383, 9000]
    with pytest.raises(Exception, match="top_k"):
        engine8.vault_topk(qu, 65, 0.85)


def test_search_workspace_does_not_grow_with_the_vault(clip_sd):
    """Two engines, vaults of 20000 and 40000 rows, one top-5 search each: the handles' device bytes
    differ by the 20000 vault rows alone (2048 bytes each; the similarity matrix used to add
    8 * 20000 * 4 bytes), within 64 KB (the per-chunk results of top_k > 8: 4 KB per 16384 rows)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    used = []
    for n in (20000, 40000):
        eng = Engine(0, None, clip_sd, max_batch=8)
        try:
            rng = np.random.default_rng(n)
            vault = rng.standard_normal((n, 512)).astype(np.float32)
            eng.set_vault(vault)
            qu = torch.nn.functional.normalize(torch.as_tensor(vault[[7, n - 1]] + 0.01)).cuda()
            _, idx, disc, _ = eng.vault_topk(qu, 5, 0.85)
            torch.cuda.synchronize()
            assert idx[:, 0].tolist() == [7, n - 1] and bool((disc > 0.85).all())
            used.append(eng.device_bytes)
        finally:
            eng.close()
    assert abs((used[1] - used[0]) - 20000 * 2048) <= 64 << 10, used


def test_analyze_batch_on_a_large_vault(det_sd, clip_sd):
    """The 5-signal batch over a 16448-row vault (served fused by default): the vault outputs equal
    vault_topk on the same embeddings, and the whole step is bit-identical with the vault on the
    two-kernel path (vault_fused = 0) and on the fused one (1)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.synthetic as syn
    from mmf_amd.engine import Engine
    B, N = 4, 16448
    eng = Engine(0, det_sd, clip_sd, max_batch=B, max_text_len=32)
    try:
        rid, rm = syn.roberta_ids(B, 32, 5, [32, 20, 7, 3])
        cid, cm = syn.clip_ids(B, 77, 5, [77, 12, 5, 2])
        imgs = syn.images(B, 5)
        emb = eng.clip_image(imgs)
        vault = syn.vault(N, 512, 7)
        vault[16390] = emb[1].cpu().numpy() * 2.0  # a planted hit for pair 1 (> 0.85)
        eng.set_vault(vault)
        assert eng.get_option("vault_fused") == 2
        out = {k: v.clone() for k, v in eng.analyze_batch(rid, rm, cid, cm, imgs).items()}
        s_all, i_all, d_all, _ = eng.vault_topk(emb, 5, 0.85)
        torch.cuda.synchronize()
        assert _bits_equal(out["top_idx"], i_all) and _bits_equal(out["top_sims"], s_all)
        assert _bits_equal(out["scores"][:, 4].contiguous(), d_all)
        assert out["scores"][1, 4].item() > 0.85 and int(out["top_idx"][1, 0]) == 16390
        for mode in (0, 1):
            eng.set_option("vault_fused", mode)
            got = eng.analyze_batch(rid, rm, cid, cm, imgs)
            torch.cuda.synchronize()
            assert set(got) == set(out)
            for k in out:
                assert _bits_equal(got[k], out[k]), (mode, k)
    finally:
        eng.close()


def test_text_and_image_search_on_the_device(engine, tmp_path, capsys):
    """search_similar_articles on the HIP towers and the fused search over a 300-row database made by
    the builder's encoder (one article per call): both modes return the rows numpy ranks first on the
    database's own embeddings (similarities within 1e-6, the bound of the other fp32 vault dots; rows whose numpy
    similarities are within 1e-6 of each other may swap), and an article's own text / image comes back
    first with similarity 1."""
    from PIL import Image
    from tables import TableClipProcessor
    import mmf_amd.synthetic as syn
    from mmf_amd.vault_builder import engine_encoder, search_similar_articles
    n = 300
    imgs = syn.images(n, 31)
    lens = [(7 * i) % 74 + 4 for i in range(n)]  # (>= 2 random tokens each: no two texts alike)
    ids, mask = syn.clip_ids(n, 77, 32, lens)
    enc = engine_encoder(engine)
    img_rows, txt_rows = [], []
    # one article per call, as the reference builds its database (train_clip_detective.py:533-566) and
    # as a query is encoded: the fp16 towers' rows are reproducible per batch shape, not across shapes
    for s in range(n):
        ie, te = enc(imgs[s:s + 1], ids[s:s + 1], mask[s:s + 1])
        img_rows.append(ie.cpu().numpy())
        txt_rows.append(te.cpu().numpy())
    img_e, txt_e = np.concatenate(img_rows), np.concatenate(txt_rows)
    db = {"article_ids": [f"id{i}" for i in range(n)], "text_contents": [f"t{i}" for i in range(n)],
          "image_paths": [f"/img/{i}.png" for i in range(n)],
          "image_embeddings": (img_e / np.linalg.norm(img_e, axis=1, keepdims=True)).astype(np.float32),
          "text_embeddings": (txt_e / np.linalg.norm(txt_e, axis=1, keepdims=True)).astype(np.float32),
          "metadata": {}}
    proc = TableClipProcessor({f"t{i}": ids[i, :lens[i]].tolist() for i in range(n)})

    def check(res, rows, q, own):
        s = np.dot(rows, q)
        order = np.argsort(s)[::-1][:len(res)]
        assert len(res) == 5 and [r["rank"] for r in res] == [1, 2, 3, 4, 5]
        for r, j in zip(res, order):
            i = int(r["article_id"][2:])
            assert abs(r["similarity"] - float(s[i])) <= 1e-6, (r, float(s[i]))
            assert i == j or abs(float(s[i]) - float(s[j])) <= 1e-6, (r, int(j), float(s[j]))
            assert r["text"] == f"t{i}..." and r["image_path"] == f"/img/{i}.png"
        assert res[0]["article_id"] == f"id{own}" and abs(res[0]["similarity"] - 1.0) <= 1e-6, res[0]

    for own in (0, 123, 299):
        res = search_similar_articles(f"t{own}", top_k=5, search_mode="text", processor=proc, engine=engine, db=db)
        qe = engine.clip_text(ids[own:own + 1], mask[own:own + 1]).cpu().numpy()[0]
        check(res, db["text_embeddings"], qe / np.linalg.norm(qe), own)
        p = str(tmp_path / f"q{own}.png")
        Image.fromarray(imgs[own]).save(p)
        res = search_similar_articles(None, p, top_k=5, search_mode="image", engine=engine, db=db)
        qe = engine.clip_image(imgs[own:own + 1]).cpu().numpy()[0]
        check(res, db["image_embeddings"], qe / np.linalg.norm(qe), own)
    assert "Top 5 similar articles:" in capsys.readouterr().out
    # the tables were uploaded once per database object
    from mmf_amd import vault_builder as VB
    banks = [b for d, b in VB._BANKS if d is db]
    assert len(banks) == 1 and sorted(m for m, _ in banks[0]) == ["image", "text"]
    with pytest.raises(ValueError, match="top_k"):
        search_similar_articles("t0", top_k=9, processor=proc, engine=engine, db=db)
