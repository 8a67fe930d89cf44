"""Synthetic operands and expected pixels for the per-element tests of the device JPEG reconstruction
(csrc/jpeg.hip: jpeg_idct_kernel, jpeg_color_kernel) through the raw mmf_jpeg_reconstruct: quantised
coefficient planes made here, packed here into the H2D record format (mmf_jpeg_entropy_packed's), and
reconstructed by the restatement (oracle/jpeg_decode.py: idct_islow, _fancy, the colour tables) for
the expected RGBX bytes.  No file, no entropy decoder and no encoder's DCT in the way, so the kernels
are driven to the edges files of Pillow's encoder never reach.  Every image built here must satisfy
the restatement's range predicate (in_exact_range): the product never hands the kernel anything else."""
import numpy as np

from oracle import jpeg_decode as J

INFO_LEN = 16
GUARD = 64  # bytes left after every image's RGBX pixels (and after the sample planes): must stay untouched
FILL = 0xA5


def pack_records(blocks, share_zero=True):
    """blocks int [n][64] natural order -> (records uint8, block_off uint32[n]): the all-zero record
    at offset 0, then per block a uint64 mask of its nonzero zigzag positions and their int16 values
    in zigzag order, padded to 8 bytes.  An all-zero block points at record 0 (share_zero: what the
    host does for padding blocks) or gets a record of its own with an empty mask (what it does for a
    coded block)."""
    blocks = np.asarray(blocks)
    out = bytearray(8)
    off = np.zeros(len(blocks), np.uint32)
    for b, blk in enumerate(blocks):
        zz = blk[J.ZIGZAG].astype(np.int64)
        ks = np.flatnonzero(zz)
        if len(ks) == 0 and share_zero:
            continue
        off[b] = len(out)
        mask = sum(1 << int(k) for k in ks)
        rec = mask.to_bytes(8, "little") + zz[ks].astype("<i2").tobytes()
        out += rec + bytes(-len(rec) % 8)
    return np.frombuffer(bytes(out), np.uint8), off


class Image:
    """One synthetic image: width, height, luma sampling (h, v) or None for grayscale, a natural-order
    table per component, quantised coefficients per component [bh_c][bw_c][64] (natural order, the
    MCU-padded block grid)."""

    def __init__(self, width, height, sampling, qts, coefs, share_zero=True):
        self.width, self.height, self.sampling = width, height, sampling
        hv = [(1, 1)] if sampling is None else [tuple(sampling), (1, 1), (1, 1)]
        self.info = info = J.JpegInfo()
        info.width, info.height = width, height
        info.comps = [(c + 1, h, v, c) for c, (h, v) in enumerate(hv)]
        info.qt = {c: np.asarray(q, np.int64) for c, q in enumerate(qts)}
        hmax, vmax, mcux, mcuy = J.geometry(info)
        self.coefs = [np.asarray(c, np.int16) for c in coefs]
        for c, (h, v) in zip(self.coefs, hv):
            assert c.shape == (mcuy * v, mcux * h, 64), (c.shape, mcuy * v, mcux * h)
        assert all(0 < q.min() and q.max() <= 65535 for q in info.qt.values())
        assert J.in_exact_range(self.coefs, info), "outside the exact range: not an input of the device kernels"
        self.share_zero = share_zero
        self.header = np.zeros(INFO_LEN, np.int32)
        self.header[:5] = [width, height, len(hv), hmax, vmax]
        for c, (h, v) in enumerate(hv):
            self.header[5 + 2 * c], self.header[6 + 2 * c] = mcux * h, mcuy * v
        self.header[11] = self.blocks = sum(c.shape[0] * c.shape[1] for c in self.coefs)

    def expected_rgbx(self):
        rgb = J.reconstruct(self.coefs, self.info).astype(np.uint8)
        return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], -1)


def grid(width, height, sampling):
    """Block-grid shapes [(bh_c, bw_c)] of the components."""
    hv = [(1, 1)] if sampling is None else [tuple(sampling), (1, 1), (1, 1)]
    mcux, mcuy = -(-width // (8 * hv[0][0])), -(-height // (8 * hv[0][1]))
    return [(mcuy * v, mcux * h) for h, v in hv]


def random_image(rng, width, height, sampling, share_zero=True):
    """Sparse random coefficients that keep most samples inside 0..255 and clamp some at both ends."""
    shapes = grid(width, height, sampling)
    qts = [rng.integers(1, 9, 64) for _ in shapes]
    coefs = []
    for bh, bw in shapes:
        c = np.zeros((bh, bw, 64), np.int64)
        m = rng.random(c.shape) < 0.2
        c[m] = rng.integers(-6, 7, int(m.sum()))
        c[..., 0] = rng.integers(-110, 111, (bh, bw))
        coefs.append(c)
    return Image(width, height, sampling, qts, coefs, share_zero)


def _align(n, a=256):
    return (n + a - 1) // a * a


class Batch:
    """The device operands of one mmf_jpeg_reconstruct call as one host buffer with its sections'
    byte offsets (tables | infos | block bases | RGBX offsets | record offsets | block-record offsets
    | packed records, each 256-byte aligned as mmf_amd/jpeg.py stages them), the output layout (every
    image's pixels followed by GUARD bytes) and the expected output bytes."""

    def __init__(self, images):
        self.images = images
        n = len(images)
        blocks = np.array([im.blocks for im in images], np.int64)
        pixels = np.array([im.width * im.height for im in images], np.int64)
        self.coef_blocks = np.r_[0, np.cumsum(blocks)[:-1]].astype(np.int64)
        self.out_off = np.r_[0, np.cumsum(pixels * 4 + GUARD)[:-1]].astype(np.int64)
        self.out_bytes = int((pixels * 4 + GUARD).sum())
        self.sample_bytes = int(blocks.sum()) * 64
        self.max_blocks, self.max_pixels = int(blocks.max()), int(pixels.max())
        qt = np.ones((n, 3, 64), np.uint16)
        recs, boffs, pk_off, cur = [], [], np.zeros(n, np.int64), 0
        for k, im in enumerate(images):
            for c in range(len(im.coefs)):
                qt[k, c] = im.info.qt[c]
            r, o = pack_records(np.concatenate([c.reshape(-1, 64) for c in im.coefs]), im.share_zero)
            recs.append(r)
            boffs.append(o)
            pk_off[k] = cur
            cur += _align(len(r), 8)
        parts = (("qt", qt), ("infos", np.stack([im.header for im in images])), ("coef_blocks", self.coef_blocks),
                 ("out_off", self.out_off), ("pk_off", pk_off), ("block_off", np.concatenate(boffs)))
        self.sections, off = {}, 0
        for name, a in parts:
            self.sections[name] = off
            off = _align(off + a.nbytes)
        self.sections["packed"] = off
        host = np.zeros(off + cur + 256, np.uint8)  # a zero tail behind the last record
        for name, a in parts:
            host[self.sections[name]:self.sections[name] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        for k, r in enumerate(recs):
            o = off + int(pk_off[k])
            host[o:o + len(r)] = r
        self.host = host
        exp = np.full(self.out_bytes, FILL, np.uint8)
        for k, im in enumerate(images):
            px = im.expected_rgbx().reshape(-1)
            exp[self.out_off[k]:self.out_off[k] + px.size] = px
        self.expected = exp
