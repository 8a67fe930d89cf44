"""JPEG test inputs shared by tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py: encoded in the test
run by Pillow's encoder (deterministic), covering the decoder paths -- 4:2:0 / 4:2:2 / 4:4:4 /
grayscale, odd sizes and 1x1, optimised Huffman tables, restart intervals (per blocks and per MCU
rows), low and high quality, progressive files -- plus files the device path must hand back to
Pillow, files whose quantisation tables were rewritten after encoding (hostile_tables), encoder
output at its coefficient extremes (extreme_legit) and a writer of files that carry given
coefficients (encode_coefficients)."""
import io

import numpy as np
from PIL import Image


def photo_like(w, h, seed=0):
    """Smooth gradients + texture + noise: coefficient statistics of a photo, not of white noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, ((xx + yy) * 5) % 256], -1).astype(np.float64)
    tex = 40 * np.sin(xx[..., None] / 3.0 + np.array([0, 1, 2])) * np.cos(yy[..., None] / 5.0)
    a = base * 0.75 + tex + rng.normal(0, 12, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, mode="RGB", **kw):
    im = Image.fromarray(a)
    if mode != "RGB":
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


# (w, h, mode, save kwargs)
SUPPORTED = [
    (64, 48, "RGB", dict(quality=90, subsampling=2)),
    (65, 49, "RGB", dict(quality=75, subsampling=2)),
    (33, 17, "RGB", dict(quality=95, subsampling=1)),
    (40, 40, "RGB", dict(quality=50, subsampling=0)),
    (31, 23, "L", dict(quality=80)),
    (97, 61, "RGB", dict(quality=85, subsampling=2, optimize=True)),
    (8, 8, "RGB", dict(quality=100, subsampling=2)),
    (1, 1, "RGB", dict(quality=90)),
    (3, 5, "RGB", dict(quality=10, subsampling=2)),
    (300, 200, "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=7)),
    (301, 203, "RGB", dict(quality=70, subsampling=1, restart_marker_rows=1)),
    (70, 50, "L", dict(quality=60, restart_marker_blocks=3)),
    (127, 129, "RGB", dict(quality=98, subsampling=0, optimize=True)),
]
LARGE = [(640, 480, "RGB", dict(quality=90, subsampling=2)), (1023, 767, "RGB", dict(quality=80, subsampling=1))]


# progressive (SOF2): Pillow's scan script has DC first / refine and AC first / refine scans with
# successive approximation, optimised tables per scan (DHT between scans)
PROGRESSIVE = [(w, h, m, dict(kw, progressive=True)) for w, h, m, kw in (
    (64, 48, "RGB", dict(quality=90, subsampling=2)),
    (65, 49, "RGB", dict(quality=75, subsampling=2)),
    (33, 17, "RGB", dict(quality=95, subsampling=1)),
    (40, 40, "RGB", dict(quality=50, subsampling=0)),
    (31, 23, "L", dict(quality=80)),
    (1, 1, "RGB", dict(quality=90)),
    (300, 200, "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=7)),
    (127, 129, "RGB", dict(quality=98, subsampling=0)),
)]
LARGE_PROGRESSIVE = [(640, 480, "RGB", dict(quality=90, subsampling=2, progressive=True))]


def _cases(cases):
    return [(f"{w}x{h}-{m}-{kw}", encode(photo_like(w, h, seed=w * 31 + h), m, **kw)) for w, h, m, kw in cases]


def supported_jpegs(large=False, progressive=False):
    cases = SUPPORTED + (LARGE if large else [])
    if progressive:
        cases = cases + PROGRESSIVE + (LARGE_PROGRESSIVE if large else [])
    return _cases(cases)


def progressive_pairs():
    """(name, progressive file, sequential file of the same pixels and settings): the quantised
    coefficients of the two are the same (progression only changes the entropy coding)."""
    out = []
    for w, h, m, kw in PROGRESSIVE:
        a = photo_like(w, h, seed=w * 31 + h)
        seq = {k: v for k, v in kw.items() if k != "progressive"}
        out.append((f"{w}x{h}-{m}-{kw}", encode(a, m, **kw), encode(a, m, **seq)))
    return out


def unsupported_files():
    """Files the device path declines (MMF_EUNSUPPORTED or not JPEG): Pillow decodes them."""
    a = photo_like(48, 40, seed=5)
    seq = bytearray(encode(a, quality=90))
    i = seq.index(b"\xff\xc0")
    seq[i + 1] = 0xC3  # the same file relabelled lossless (SOF3)
    out = [("lossless", bytes(seq)),
           ("cmyk", encode(a, "CMYK", quality=90))]
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG")
    out.append(("png", b.getvalue()))
    return out


def _segments(d: bytes):
    """(marker, start, end) of each marker segment before the first SOS's entropy data."""
    out, p = [], 2
    while p + 4 <= len(d):
        m = d[p + 1]
        L = (d[p + 2] << 8) | d[p + 3]
        out.append((m, p, p + 2 + L))
        if m == 0xDA:
            break
        p += 2 + L
    return out


def rewrite_dqt(data: bytes, fn, sixteen=False) -> bytes:
    """The file with every quantisation table q (int64[64], zigzag order as the file carries it:
    q[0] is DC's) replaced by fn(tq, q); the entropy-coded data is untouched, so the file stays valid
    and its quantised coefficients are the same.  Tables are written with 8-bit entries (Pq = 0; the
    values must fit) or, with sixteen=True, as 16-bit tables (Pq = 1)."""
    out, last = bytearray(), 0
    for m, a, b in _segments(data):
        if m != 0xDB:
            continue
        seg, q, body = data[a + 4:b], 0, bytearray()
        while q < len(seg):
            pq, tq = seg[q] >> 4, seg[q] & 15
            q += 1
            if pq:
                vals = [(seg[q + 2 * i] << 8) | seg[q + 2 * i + 1] for i in range(64)]
            else:
                vals = list(seg[q:q + 64])
            q += 128 if pq else 64
            new = np.asarray(fn(tq, np.array(vals, np.int64)), np.int64)
            assert new.shape == (64,) and new.min() >= 1 and new.max() <= (65535 if sixteen else 255)
            if sixteen:
                body += bytes([0x10 | tq]) + new.astype(">u2").tobytes()
            else:
                body += bytes([tq]) + new.astype(np.uint8).tobytes()
        out += data[last:a] + b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
        last = b
    return bytes(out + data[last:])


def _test_images(w, h):
    rng = np.random.default_rng(w * 131 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return [("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
            ("satnoise", (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)),
            ("checker1", np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)),
            ("checker3", np.stack([((xx // 3 + yy // 3) & 1) * 255, ((xx // 3) & 1) * 255,
                                   ((yy // 3) & 1) * 255], -1).astype(np.uint8))]


HOSTILE_SCALES = (1, 2, 3, 4, 6, 8, 16, 64, 255)


def _scaled(scale, cap=255):
    return lambda tq, q: np.minimum(q * scale, cap)


_hostile = []


def hostile_tables():
    """(name, file, sequential twin): valid files whose quantisation tables were rewritten after
    encoding -- what a tampered file looks like -- so that the dequantised coefficients grow until the
    integer IDCT leaves the range in which the device decode equals Pillow's.  The twin is the file
    itself, or for a progressive file the sequential file of the same pixels, settings and tables
    (the same quantised coefficients: oracle/jpeg_decode.py reads only sequential files).
    5 images x quality {100, 90, 50, 10} x {4:4:4, 4:2:0} x table scale HOSTILE_SCALES (entries
    capped at 255) at 48x40, then progressive variants, grayscale files, DC-only rewrites and
    16-bit tables (Pq = 1, entries above 255)."""
    if _hostile:
        return _hostile
    w, h = 48, 40
    images = _test_images(w, h) + [("photo", photo_like(w, h, seed=11))]
    out = []
    for iname, a in images:
        for q in (100, 90, 50, 10):
            for ss in (0, 2):
                base = encode(a, quality=q, subsampling=ss)
                for s in HOSTILE_SCALES:
                    f = rewrite_dqt(base, _scaled(s))
                    out.append((f"{iname}-q{q}-ss{ss}-x{s}", f, f))
    noise, photo = images[0][1], images[4][1]
    for iname, a, q, ss in (("noise", noise, 100, 2), ("photo", photo, 90, 2), ("photo", photo, 50, 0)):
        seq = encode(a, quality=q, subsampling=ss)
        prog = encode(a, quality=q, subsampling=ss, progressive=True)
        for s in (1, 2, 4, 16):
            out.append((f"prog-{iname}-q{q}-ss{ss}-x{s}", rewrite_dqt(prog, _scaled(s)), rewrite_dqt(seq, _scaled(s))))
    for iname, a, q in (("noise", noise, 100), ("photo", photo, 90), ("photo", photo, 10)):
        base = encode(a, "L", quality=q)
        for s in (1, 3, 8, 64):
            f = rewrite_dqt(base, _scaled(s))
            out.append((f"gray-{iname}-q{q}-x{s}", f, f))

    def dc_only(s):
        def fn(tq, q):
            q = q.copy()
            q[0] = min(q[0] * s, 255)
            return q
        return fn
    for iname, a, q in (("satnoise", images[1][1], 100), ("photo", photo, 90), ("checker3", images[3][1], 50)):
        base = encode(a, quality=q, subsampling=0)
        for s in (2, 4, 8, 255):
            f = rewrite_dqt(base, dc_only(s))
            out.append((f"dconly-{iname}-q{q}-x{s}", f, f))
    for iname, a, q, ss in (("photo", photo, 10, 2), ("photo", photo, 50, 0), ("noise", noise, 100, 0)):
        base = encode(a, quality=q, subsampling=ss)
        for s in (2, 3, 300):
            f = rewrite_dqt(base, _scaled(s, 65535), sixteen=True)
            out.append((f"pq1-{iname}-q{q}-ss{ss}-x{s}", f, f))
    # a smooth image at quality 10: entries above 255 (16-bit tables) that stay inside the range
    flat = np.full((h, w, 3), 120, np.uint8)
    flat[:, w // 2:] += 9
    base = encode(flat, quality=10, subsampling=0)
    for s in (2, 3, 4):
        f = rewrite_dqt(base, lambda tq, q, s=s: np.r_[q[:1], q[1:] * s], sixteen=True)
        out.append((f"pq1-flat-q10-acx{s}", f, f))
    _hostile.extend(out)
    return _hostile


_legit = []


def extreme_legit():
    """(name, file): unmodified files of Pillow's encoder at the coefficient extremes an encoder
    reaches -- noise, saturated noise and checkerboards at quality 1 .. 100 -- all inside the range."""
    if not _legit:
        for iname, a in _test_images(48, 40):
            for q in (1, 2, 5, 10, 100):
                for ss in (0, 2):
                    _legit.append((f"{iname}-q{q}-ss{ss}", encode(a, quality=q, subsampling=ss)))
    return _legit


def encode_coefficients(width, height, sampling, qts, coefs) -> bytes:
    """A baseline file that carries exactly the given quantised coefficients (no encoder's DCT or
    quantiser in the way).  sampling: luma (h, v), or None for one component; qts: a natural-order
    table (<= 255) per component; coefs: per component int [bh_c, bw_c, 64] natural order over the
    MCU-padded block grid.  Huffman tables: every DC symbol 0..15 as a 5-bit code, AC symbols
    0..127 as 9-bit codes (code = symbol) and 128..255 as 10-bit codes (code = symbol + 128)."""
    from oracle.jpeg_decode import ZIGZAG
    nc = len(coefs)
    hv = [(1, 1)] if sampling is None else [tuple(sampling), (1, 1), (1, 1)]
    assert nc == len(hv) == len(qts)
    out = bytearray(b"\xff\xd8")
    for c, q in enumerate(qts):
        out += b"\xff\xdb\x00\x43" + bytes([c]) + bytes(np.asarray(q)[ZIGZAG].astype(np.uint8))
    out += b"\xff\xc0" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + \
        width.to_bytes(2, "big") + bytes([nc])
    for c, (h, v) in enumerate(hv):
        out += bytes([c + 1, h << 4 | v, c])
    dc_bits, ac_bits = [0] * 16, [0] * 16
    dc_bits[4], ac_bits[8], ac_bits[9] = 16, 128, 128
    out += b"\xff\xc4" + (2 + 17 + 16).to_bytes(2, "big") + b"\x00" + bytes(dc_bits) + bytes(range(16))
    out += b"\xff\xc4" + (2 + 17 + 256).to_bytes(2, "big") + b"\x10" + bytes(ac_bits) + bytes(range(256))
    out += b"\xff\xda" + (6 + 2 * nc).to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        out += bytes([c + 1, 0x00])
    out += b"\x00\x3f\x00"
    bits = []  # (value, length)

    def put_ac(sym):
        bits.append((sym, 9) if sym < 128 else (sym + 128, 10))

    def put_value(v):
        s = int(abs(v)).bit_length()
        bits.append((v if v >= 0 else v + (1 << s) - 1, s))

    pred = [0] * nc
    hmax, vmax = hv[0]
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    for my in range(mcuy):
        for mx in range(mcux):
            for c, (h, v) in enumerate(hv):
                for yy in range(v):
                    for xx in range(h):
                        blk = np.asarray(coefs[c][my * v + yy, mx * h + xx], np.int64)[ZIGZAG]
                        diff = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        bits.append((abs(diff).bit_length(), 5))
                        if diff:
                            put_value(diff)
                        run = 0
                        last = max(np.flatnonzero(blk), default=0)
                        for k in range(1, last + 1):
                            if blk[k] == 0:
                                run += 1
                                continue
                            while run > 15:
                                put_ac(0xF0)
                                run -= 16
                            put_ac(run << 4 | int(abs(blk[k])).bit_length())
                            put_value(int(blk[k]))
                            run = 0
                        if last < 63:
                            put_ac(0x00)
    acc = n = 0
    for v, s in bits:
        acc, n = (acc << s) | v, n + s
    pad = -n % 8
    acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
    for byte in acc.to_bytes(n // 8, "big"):
        out.append(byte)
        if byte == 0xFF:
            out.append(0)
    return bytes(out + b"\xff\xd9")


def rgb_component_ids() -> bytes:
    """A 3-component file with no JFIF / Adobe marker whose component ids are 'R' 'G' 'B':
    libjpeg (default_decompress_parms) decodes it as RGB, without the YCbCr transform."""
    d = bytearray(encode(photo_like(40, 32, seed=9), quality=90, subsampling=0))
    segs = _segments(bytes(d))
    for m, a, b in segs:
        if m in (0xC0, 0xDA):
            ids = [a + 10 + 3 * i for i in range(3)] if m == 0xC0 else [a + 5 + 2 * i for i in range(3)]
            for k, i in enumerate(ids):
                d[i] = (82, 71, 66)[k]
    app0 = [(a, b) for m, a, b in segs if m == 0xE0]
    for a, b in reversed(app0):
        del d[a:b]
    return bytes(d)


def duplicate_sos_ids() -> bytes:
    """SOF ids 1, 2, 3 but SOS ids 1, 1, 1 (libjpeg: JERR_BAD_COMPONENT_ID)."""
    d = bytearray(encode(photo_like(32, 24, seed=4), quality=90))
    for m, a, b in _segments(bytes(d)):
        if m == 0xDA:
            for i in range(3):
                d[a + 5 + 2 * i] = 1
    return bytes(d)


def short_sos_at_eof() -> bytes:
    """A file ending in an SOS segment whose length field claims only the length itself (L = 2)."""
    d = encode(photo_like(16, 16, seed=2), quality=90)
    sos = [a for m, a, b in _segments(d) if m == 0xDA][0]
    return d[:sos] + b"\xff\xda\x00\x02"


def pillow_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
