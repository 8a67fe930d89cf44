"""References for mmf_jpeg_roundtrip_u8 (csrc/jpeg_encode.hip): the reference's RandomJPEGCompression
(misinformation_dataset.py:18-57), ``image.save(buffer, format="JPEG", quality=q, optimize=False)``, reopen,
``convert("RGB")``.

``pil_roundtrip`` is that, through Pillow: the authority the kernels are tested against.  ``pil_coefs`` reads the
quantised coefficients out of the file Pillow wrote (oracle.jpeg_decode.parse / entropy_decode), cropped to the block
grids that reach a pixel.

The ``np_*`` functions restate the forward half of libjpeg in numpy, in 64-bit integers: jpeg_set_quality's tables,
jccolor.c's RGB -> YCbCr, jcprepct.c's and jcsample.c's edge replication out to the block grid, h2v2 downsampling, jfdctint.c's
forward DCT and jcdctmgr.c's quantisation.  They are the readable specification of the kernel's arithmetic;
tests/test_jpeg_encode_refs_cpu.py holds them to Pillow.  The inverse half is oracle.jpeg_decode's.
"""
import io

import numpy as np
from PIL import Image

from oracle import jpeg_decode as JD

# ITU T.81 Annex K tables K.1 and K.2, natural (row-major) order
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64)


# ---------------------------------------------------------------------------------------------
# Pillow
# ---------------------------------------------------------------------------------------------
def pil_file(img_u8, q: int) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img_u8), "RGB").save(buf, format="JPEG", quality=int(q), optimize=False)
    return buf.getvalue()


def pil_roundtrip(img_u8, q: int) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [H, W, 3], what RandomJPEGCompression.__call__ returns at quality q."""
    im = Image.open(io.BytesIO(pil_file(img_u8, q)))
    im.load()
    return np.asarray(im.convert("RGB"))


def pil_roundtrip_batch(img_u8, quality) -> np.ndarray:
    """uint8 [B, H, W, 3], quality [B] (0: the image unchanged) -> uint8 [B, H, W, 3]."""
    img_u8 = np.asarray(img_u8)
    return np.stack([pil_roundtrip(x, q) if q else x for x, q in zip(img_u8, np.asarray(quality).tolist())])


def grids(H: int, W: int):
    """((luma block rows, columns), (chroma block rows, columns)) of the blocks that reach a pixel."""
    ch, cw = -(-H // 2), -(-W // 2)
    return (-(-H // 8), -(-W // 8)), (-(-ch // 8), -(-cw // 8))


def pil_coefs(img_u8, q: int):
    """-> ([Y, Cb, Cr] int64 [by, bx, 64] quantised coefficients of Pillow's file, cropped from the MCU-padded grid
    to ``grids``; its three tables int64 [64] natural order; (info, uncropped planes) for in_exact_range)."""
    data = pil_file(img_u8, q)
    info = JD.parse(data)
    assert [(c[1], c[2]) for c in info.comps] == [(2, 2), (1, 1), (1, 1)], "Pillow's default for RGB is 4:2:0"
    full = JD.entropy_decode(data, info)
    H, W = np.asarray(img_u8).shape[:2]
    g0, gc = grids(H, W)
    crop = [full[0][:g0[0], :g0[1]], full[1][:gc[0], :gc[1]], full[2][:gc[0], :gc[1]]]
    return [c.astype(np.int64) for c in crop], [info.qt[c[3]] for c in info.comps], (info, full)


# ---------------------------------------------------------------------------------------------
# the forward half in numpy
# ---------------------------------------------------------------------------------------------
def np_qtable(q: int, std) -> np.ndarray:
    """jpeg_set_quality(q, force_baseline = TRUE): jpeg_quality_scaling, then jpeg_add_quant_table."""
    q = int(q)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(std, np.int64) * s + 50) // 100, 1, 255)


def np_qtables(q: int):
    return [np_qtable(q, STD_LUMA), np_qtable(q, STD_CHROMA), np_qtable(q, STD_CHROMA)]


def _fix(x):
    return int(x * 65536 + 0.5)


def np_ycc(img_u8):
    """jccolor.c rgb_ycc_convert: uint8 [..., 3] -> (Y, Cb, Cr) int64."""
    r, g, b = (np.asarray(img_u8)[..., k].astype(np.int64) for k in range(3))
    half, off = 1 << 15, 128 << 16
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def _extend(p, h, w):
    """The last column and the last row replicated out to h x w."""
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def np_h2v2(p):
    """jcsample.c h2v2_downsample on an even-sized plane: bias 1 on even output columns, 2 on odd ones."""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias) >> 2


def np_sample_blocks(img_u8):
    """uint8 [H, W, 3] -> [Y, Cb, Cr] level-shifted sample blocks int64 [by, bx, 64] on ``grids``."""
    H, W = np.asarray(img_u8).shape[:2]
    (h0, w0), (hc, wc) = grids(H, W)
    y, cb, cr = np_ycc(img_u8)
    # jcprepct.c: the input gets the one row that makes its height even, each component is downsampled, and the rest
    # of the block grid repeats the last DOWNSAMPLED row -- for an even H that is no multiple of 16 not what
    # downsampling a replicated last input row would give.  Columns (jcsample.c expand_right_edge) are replicated in
    # the input, out to twice the chroma grid.
    ch = -(-H // 2)
    planes = [_extend(y, 8 * h0, 8 * w0)] + [_extend(np_h2v2(_extend(c, 2 * ch, 16 * wc)), 8 * hc, 8 * wc)
                                             for c in (cb, cr)]
    out = []
    for p in planes:
        by, bx = p.shape[0] // 8, p.shape[1] // 8
        out.append(p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).reshape(by, bx, 64) - 128)
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint.c, one pass over d[0..7] (arrays): pass 1 scales up by PASS1_BITS = 2, pass 2 removes it."""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return o


def np_fdct(blocks):
    """Level-shifted samples int [..., 64] -> jpeg_fdct_islow's coefficients int64 [..., 64] (8 times the DCT)."""
    b = np.asarray(blocks, np.int64).reshape(np.shape(blocks)[:-1] + (8, 8))
    rows = np.stack(_fdct_1d([b[..., :, k] for k in range(8)], True), -1)      # along each row
    cols = np.stack(_fdct_1d([rows[..., k, :] for k in range(8)], False), -2)  # down each column
    return cols.reshape(np.shape(blocks))


def np_quantise(coef, qt):
    """jcdctmgr.c: sign(c) * ((|c| + (qv >> 1)) // qv), qv = 8 t."""
    qv = np.asarray(qt, np.int64) << 3
    return np.sign(coef) * ((np.abs(coef) + (qv >> 1)) // qv)


def np_block_roundtrip(blocks, qt):
    """What mmf_jpeg_block_roundtrip_raw computes: level-shifted sample blocks int [n, 64], a table [64] ->
    (quantised coefficients int64 [n, 64], samples uint8 [n, 64], out of the exact range int32 [n])."""
    qt = np.asarray(qt, np.int64)
    coef = np_quantise(np_fdct(blocks), qt)
    d, ws, out = JD._idct_passes(coef, qt)
    bad = ((np.abs(d).max(-1) > 32767) | (np.abs(ws).max((-1, -2)) > 32767) | (out.min((-1, -2)) < -512)
           | (out.max((-1, -2)) > 511))
    return coef, JD._range_limit(out).astype(np.uint8).reshape(coef.shape), bad.astype(np.int32)


def np_coefs(img_u8, q: int):
    """uint8 [H, W, 3] -> [Y, Cb, Cr] quantised coefficients int64 [by, bx, 64] on ``grids``."""
    return [np_quantise(np_fdct(s), t) for s, t in zip(np_sample_blocks(img_u8), np_qtables(q))]


class _Info:
    """What oracle.jpeg_decode.reconstruct / in_exact_range read of a JpegInfo, for a 4:2:0 file of this size."""

    def __init__(self, H, W, q):
        self.height, self.width = H, W
        self.comps = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
        t = np_qtables(q)
        self.qt = {0: t[0], 1: t[1]}


def np_roundtrip(img_u8, q: int) -> np.ndarray:
    """The restatement end to end: the forward half here, the inverse half oracle.jpeg_decode.reconstruct."""
    H, W = np.asarray(img_u8).shape[:2]
    return JD.reconstruct(np_coefs(img_u8, q), _Info(H, W, q))


def np_in_exact_range(img_u8, q: int) -> bool:
    H, W = np.asarray(img_u8).shape[:2]
    return JD.in_exact_range(np_coefs(img_u8, q), _Info(H, W, q))


# ---------------------------------------------------------------------------------------------
# test images
# ---------------------------------------------------------------------------------------------
# (H, W); 24 x 40 and 20 x 12: an even height that is no multiple of 16, where the chroma rows below the image are
# copies of the last downsampled row
SIZES = ((1, 1), (7, 9), (15, 16), (16, 15), (17, 33), (32, 32), (24, 40), (20, 12), (224, 224))
QUALITIES = (1, 40, 57, 80, 95, 100)
PRIMARIES = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                      [0, 0, 0], [255, 255, 255]], np.uint8)


def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def primaries(H, W):
    """Saturated primaries in 3 x 5 patches, so that every block holds several."""
    yy, xx = np.mgrid[:H, :W]
    return PRIMARIES[(yy // 3 * 3 + xx // 5) % len(PRIMARIES)]


def gradient_with_edge(H, W):
    """A smooth ramp in every channel with a sharp vertical edge two thirds across."""
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    r = 255 * xx / max(W - 1, 1)
    g = 255 * yy / max(H - 1, 1)
    b = 255 * (xx + yy) / max(H + W - 2, 1)
    img = np.stack([r, g, b], -1)
    img[:, (2 * W) // 3:] = 255 - img[:, (2 * W) // 3:]
    return np.round(img).astype(np.uint8)


def extremes(H, W):
    """{name: uint8 [H, W, 3]}: all 0, all 255, the one-pixel checkerboard, saturated primaries."""
    return {"zeros": np.zeros((H, W, 3), np.uint8), "ones": np.full((H, W, 3), 255, np.uint8),
            "checkerboard": checkerboard(H, W), "primaries": primaries(H, W)}


def range_conditions(coef, qt):
    """in_exact_range's three conditions per block, True where one FAILS: bool [n] each."""
    d, ws, out = JD._idct_passes(np.asarray(coef, np.int64), np.asarray(qt, np.int64))
    return (np.abs(d).max(-1) > 32767, np.abs(ws).max((-1, -2)) > 32767,
            (out.min((-1, -2)) < -512) | (out.max((-1, -2)) > 511))


def outside_blocks():
    """(level-shifted sample blocks int16 [6, 64] within +-1024, a table int64 [64] of ones, per block which
    conditions of the exact range fail: (), (3,) or (2, 3)).  A single sample of +-900 in a block of zeros comes
    back near +-900 through a small workspace: the third alone.  A flat block of +-1024 has the workspace 32 * 1024,
    one past the limit, and comes back as +-1024: the second and the third.

    No block within the bound can fail the first, and none at all the second alone.  A dequantised value is
    t * round(c / (8 t)), at most |c| / 8 + t / 2, and |c| / 8 is a DCT coefficient of the samples: at most 8 * 1024.
    And each pass of the IDCT is, up to rounding, an orthogonal transform times a constant -- a workspace row w gives
    the outputs o with sum o^2 = 8 sum (w / 32)^2 -- so one |w| > 32767 forces an output of magnitude 1024 or so."""
    blocks = np.zeros((6, 64), np.int16)
    blocks[0] = 100
    blocks[1] = np.arange(64) * 2 - 64
    blocks[2] = 1024
    blocks[3] = -1024
    blocks[4, 27] = 900
    blocks[5, 36] = -900
    return blocks, np.ones(64, np.int64), [(), (), (2, 3), (2, 3), (3,), (3,)]
