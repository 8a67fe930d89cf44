"""Device JPEG decode (csrc/jpeg_host.cpp + csrc/jpeg.hip, mmf_amd/jpeg.py) on the MI355X: decoded
pixels bit-exact with Pillow's decoder (the reference's Image.open(...).convert("RGB")) on every
supported kind of file, and analyze_pairs over encoded files equal -- dict for dict -- to the same
call with every image decoded by Pillow, including chunks that mix device-decoded JPEGs with files
the device path declines (CMYK, lossless, PNG) and PIL images; progressive files included."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(det_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mmf_amd.engine import Engine
    e = Engine(0, det_sd, None, max_batch=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stager():
    from mmf_amd import jpeg
    s = jpeg.JpegStager(workers=4)
    yield s
    s.close()


def test_device_pixels_match_pillow(engine, stager):
    from mmf_amd import jpeg
    cases = C.supported_jpegs(large=True, progressive=True)
    st = stager.stage([d for _, d in cases])
    assert st.index == list(range(len(cases)))
    got = jpeg.device_rgb(engine, stager, st)
    for (name, d), g in zip(cases, got):
        np.testing.assert_array_equal(g, C.pillow_rgb(d), err_msg=name)


def test_staging_slot_growth(engine):
    """A first packed-section guess far too small: records that do not fit are placed after the slot
    grows, and the pixels are unchanged."""
    from mmf_amd import jpeg
    s = jpeg.JpegStager(workers=3)
    s.guess_bytes_per_block = 1
    try:
        cases = C.supported_jpegs(large=True, progressive=True)
        for _ in range(2):  # second pass: the grown slots are reused
            st = s.stage([d for _, d in cases])
            got = jpeg.device_rgb(engine, s, st)
            for (name, d), g in zip(cases, got):
                np.testing.assert_array_equal(g, C.pillow_rgb(d), err_msg=name)
    finally:
        s.close()


def test_declined_files_are_left_to_pillow(engine, stager):
    from mmf_amd import jpeg
    files = C.unsupported_files()
    good = C.supported_jpegs()[0][1]
    st = stager.stage([files[0][1], good, files[1][1], None, files[2][1], good])
    assert st.index == [1, 5]
    a, b = jpeg.device_rgb(engine, stager, st)
    np.testing.assert_array_equal(a, C.pillow_rgb(good))
    np.testing.assert_array_equal(b, a)


def test_oversized_jpeg_left_to_the_host_path(engine, stager):
    """a JPEG whose shortest side is past mmf_resize_pil's tap budget is not staged for the
    device (its windows would fail the whole chunk); the smaller file beside it is."""
    big = C.encode(C.photo_like(5400, 5300, seed=1), quality=60)
    info = np.zeros(16, np.int32)
    assert engine.lib.mmf_jpeg_header(big, len(big), info.ctypes.data) == 0
    assert not engine.resize_supported(5400, 5300)
    good = C.supported_jpegs()[0][1]
    st = stager.stage([big, good])
    assert st.index == [1]


def test_windows_match_pillow_resampling(engine, stager):
    """Device decode -> device resampling == Pillow decode -> Pillow resampling (io_utils)."""
    from PIL import Image

    from mmf_amd import io_utils, jpeg
    cases = C.supported_jpegs(large=True, progressive=True)
    st = stager.stage([d for _, d in cases])
    eff, clp = jpeg.device_windows(engine, stager, st)
    for k, (name, d) in enumerate(cases):
        pil = Image.open(io.BytesIO(d)).convert("RGB")
        np.testing.assert_array_equal(eff[k].cpu().numpy(), io_utils.effnet_pixels(pil), err_msg=name)
        np.testing.assert_array_equal(clp[k].cpu().numpy(), io_utils.clip_pixels(pil), err_msg=name)


@pytest.fixture(scope="module")
def forensics(golden, golden_inputs, det_sd, clip_sd):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from tables import TableClipProcessor, TableRobertaTokenizer
    from misinfo_forensics import MisinfoForensics
    from tests.test_gpu_api import _tables
    rob, clp = _tables(golden, golden_inputs)
    mf = MisinfoForensics(fusion_weights="/nonexistent", faiss_index_path="/nonexistent",
                          roberta_tokenizer=TableRobertaTokenizer(rob), clip_processor=TableClipProcessor(clp),
                          detector_state=det_sd, clip_state=clip_sd, max_batch=4, verbose=False)
    mf.set_vault(golden_inputs["vault"], golden_inputs["meta"])
    return mf


def test_analyze_pairs_on_encoded_files(forensics, golden_inputs, tmp_path):
    """10 pairs in chunks of 4 (both pinned staging slots reused): JPEG bytes, a JPEG file path,
    a progressive JPEG, a CMYK JPEG and a PNG (both declined: Pillow), a PIL image, against the
    all-Pillow run of the same call."""
    from PIL import Image
    imgs = golden_inputs["imgs"]
    n = imgs.shape[0]
    items = []
    for i in range(10):
        a = imgs[i % n]
        if i == 3:
            items.append(C.encode(a, quality=90, progressive=True))
        elif i == 5:
            items.append(C.encode(a, "CMYK", quality=90))
        elif i == 6:
            b = io.BytesIO()
            Image.fromarray(a).save(b, "PNG")
            items.append(b.getvalue())
        elif i == 7:
            items.append(Image.fromarray(a))
        elif i == 8:
            p = tmp_path / "pair8.jpg"
            p.write_bytes(C.encode(a, quality=85, subsampling=1))
            items.append(str(p))
        else:
            items.append(C.encode(a, quality=80 + i, subsampling=2 if i % 2 else 0))
    texts = [f"sample text {i % n}" for i in range(10)]
    forensics.device_jpeg = True
    dev = forensics.analyze_pairs(texts, items)
    forensics.device_jpeg = False
    try:
        host = forensics.analyze_pairs(texts, items)
    finally:
        forensics.device_jpeg = True
    assert len(dev) == 10
    assert dev == host


def test_analyze_pairs_oversized_and_truncated_jpegs(forensics, golden_inputs):
    """An oversized JPEG (shortest side 5300 px > the device resampler's budget) goes through Pillow
    decode + host resampling inside the same chunk, with dicts equal to the all-Pillow call; a
    truncated JPEG raises Pillow's OSError, as the reference's Image.open(...).convert does."""
    imgs = golden_inputs["imgs"]
    big = C.encode(C.photo_like(5400, 5300, seed=1), quality=60)
    items = [C.encode(imgs[0], quality=90), big, C.encode(imgs[1], quality=85)]
    texts = ["sample text 0", "sample text 1", "sample text 1"]
    forensics.device_jpeg = True
    dev = forensics.analyze_pairs(texts, items)
    forensics.device_jpeg = False
    try:
        host = forensics.analyze_pairs(texts, items)
    finally:
        forensics.device_jpeg = True
    assert dev == host
    cut = items[0][:len(items[0]) * 2 // 3]
    with pytest.raises(OSError, match="truncated"):
        forensics.analyze_pairs(texts[:2], [items[2], cut])


# ---- files whose quantisation tables were rewritten (tests/jpeg_cases.py hostile_tables): inside the
# restatement's range predicate the device decodes them as Pillow does; outside, the host decoder
# declines them after entropy decoding and the stager leaves them to Pillow.

def _in_range(seq, _cache={}):
    from oracle import jpeg_decode as J
    info = J.parse(seq)
    key = seq[info.scan_data_at:]
    if key not in _cache:
        _cache[key] = J.entropy_decode(seq, info)
    return J.in_exact_range(_cache[key], info)


def test_hostile_and_extreme_files_staged_exactly_when_in_range(engine, stager):
    """Every hostile_tables() and extreme_legit() file, in chunks that mix both kinds: the stager keeps
    exactly the files inside the range, and their device pixels equal Pillow's."""
    from mmf_amd import jpeg
    files = [(n, d, _in_range(seq)) for n, d, seq in C.hostile_tables()]
    files += [(n, d, True) for n, d in C.extreme_legit()]
    assert sum(i for _, _, i in files) >= 140 and sum(not i for _, _, i in files) >= 100
    for a in range(0, len(files), 64):
        chunk = files[a:a + 64]
        st = stager.stage([d for _, d, _ in chunk])
        assert st.index == [k for k, (_, _, inside) in enumerate(chunk) if inside], [n for n, _, _ in chunk]
        for k, g in zip(st.index, jpeg.device_rgb(engine, stager, st)):
            np.testing.assert_array_equal(g, C.pillow_rgb(chunk[k][1]), err_msg=chunk[k][0])


@pytest.mark.parametrize("batch_call", [True, False])
def test_stager_drops_out_of_range_files_and_restages(engine, batch_call):
    """A chunk of [good, hostile outside, good, hostile inside] (and one where every file is
    declined): st.index == [0, 2, 3], the staged tables, block offsets and records equal per-file
    staging, the pixels equal Pillow's -- by the chunk call and by the per-file pool calls."""
    import ctypes

    from mmf_amd import jpeg
    hostile = C.hostile_tables()
    out = [d for _, d, seq in hostile if not _in_range(seq)]
    ins = [d for n, d, seq in hostile if _in_range(seq) and "-x1" not in n]
    good = [d for _, d in C.supported_jpegs()[:2]]
    chunk = [good[0], out[0], good[1], ins[-1]]
    s = jpeg.JpegStager(workers=3)
    s.batch_call = batch_call
    try:
        assert s.stage([out[0], None, out[-1]]).index == []
        for files, want in ((chunk, [0, 2, 3]), ([out[1]] + chunk + [out[2]], [1, 3, 4])):
            st = s.stage(files)
            assert st.index == want
            host, sec, lib = s.buf[st.slot].numpy(), st.sections, engine.lib
            pk_off = host[sec["pk_off"]:sec["pk_off"] + 8 * len(want)].view(np.int64)
            base = 0
            for k, i in enumerate(want):
                d, blocks = files[i], int(st.infos[k, 11])
                ref = np.zeros(int(lib.mmf_jpeg_packed_bound(blocks)), np.uint8)
                boff = np.zeros(blocks, np.uint32)
                qt = np.zeros(192, np.uint16)
                used = ctypes.c_int64(0)
                assert lib.mmf_jpeg_entropy_packed(d, len(d), ref.ctypes.data, ref.size, boff.ctypes.data,
                                                   qt.ctypes.data, ctypes.byref(used)) == 0
                o = sec["packed"] + int(pk_off[k])
                np.testing.assert_array_equal(host[o:o + used.value], ref[:used.value])
                o = sec["block_off"] + 4 * base
                np.testing.assert_array_equal(host[o:o + 4 * blocks].view(np.uint32), boff)
                ncomp = int(st.infos[k, 2])
                o = sec["qt"] + 384 * k
                np.testing.assert_array_equal(host[o:o + 128 * ncomp].view(np.uint16), qt[:64 * ncomp])
                base += blocks
            assert st.blocks == base
            for i, g in zip(want, jpeg.device_rgb(engine, s, st)):
                np.testing.assert_array_equal(g, C.pillow_rgb(files[i]))
    finally:
        s.close()


def test_analyze_pairs_on_rewritten_tables(forensics, golden_inputs):
    """analyze_pairs over chunks that mix ordinary files with rewritten-table files inside and outside
    the range (sequential and progressive, a 16-bit table): device_jpeg=True equals device_jpeg=False
    dict for dict -- the files outside reach Pillow in both."""
    imgs = golden_inputs["imgs"]
    n = imgs.shape[0]
    lib = forensics.engine.lib
    items = []
    for i in range(10):
        a = imgs[i % n]
        base = C.encode(a, quality=(90, 75, 50)[i % 3], subsampling=2 if i % 2 else 0, progressive=i in (4, 7))
        scale = (1, 2, 16, 3, 2, 1, 64, 4, 2, 255)[i]
        if i == 8:
            items.append(C.rewrite_dqt(base, lambda tq, q: np.r_[q[:1], q[1:] * 300], sixteen=True))
        else:
            items.append(C.rewrite_dqt(base, lambda tq, q, s=scale: np.minimum(q * s, 255)) if scale > 1 else base)
    info = np.zeros(16, np.int32)
    codes = []
    for d in items:
        assert lib.mmf_jpeg_header(d, len(d), info.ctypes.data) == 0
        co = np.zeros((int(info[11]), 64), np.int16)
        qt = np.zeros(192, np.uint16)
        codes.append(lib.mmf_jpeg_entropy(d, len(d), co.ctypes.data, qt.ctypes.data))
    assert codes == [0, 0, -95, 0, 0, 0, -95, -95, -95, -95]  # the last chunk of 4 is declined whole
    texts = [f"sample text {i % n}" for i in range(10)]
    forensics.device_jpeg = True
    dev = forensics.analyze_pairs(texts, items)
    forensics.device_jpeg = False
    try:
        host = forensics.analyze_pairs(texts, items)
    finally:
        forensics.device_jpeg = True
    assert len(dev) == 10
    assert dev == host
