"""Per-element tests of the device JPEG reconstruction kernels (csrc/jpeg.hip: jpeg_idct_kernel,
jpeg_color_kernel) on a real MI355X, through the raw mmf_jpeg_reconstruct on synthetic packed
records (tests/jpeg_refs.py) against the restatement's integers (oracle/jpeg_decode.py: idct_islow,
_fancy, the colour tables), byte for byte: the range limit over its whole exact domain, every shape
of packed record, one launch over images that differ in components, sampling and size, and every
clamp of the colour conversion.  The output starts as a fill pattern with guard bytes behind every
image and behind the sample planes: a pixel not written, or a write past an image, fails too.  Every
input satisfies the range predicate (jpeg_refs.Image asserts it): what lies outside is declined on
the host and never reaches these kernels."""
import ctypes

import numpy as np
import pytest
import torch

from tests import jpeg_refs as R

pytestmark = pytest.mark.gpu
EINVAL = -22


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    lib = hip.load()
    h = ctypes.c_void_p()
    hip.check(lib.mmf_create(0, ctypes.byref(h)), "mmf_create")
    yield lib, h
    torch.cuda.synchronize()
    lib.mmf_destroy(h)


def _call(ctx, batch, src, out, samples, B=None, max_blocks=None, max_pixels=None, null=None, handle=True):
    import mmf_amd.hip as hip
    lib, h = ctx
    p, sec = src.data_ptr(), batch.sections
    args = {name: p + sec[name] for name in ("packed", "block_off", "pk_off", "qt", "coef_blocks", "infos", "out_off")}
    args["samples"], args["out"] = samples.data_ptr(), out.data_ptr()
    if null:
        args[null] = None
    rc = lib.mmf_jpeg_reconstruct(h if handle else None, args["packed"], args["block_off"], args["pk_off"], args["qt"],
                                  args["coef_blocks"], args["infos"], args["out_off"],
                                  len(batch.images) if B is None else B,
                                  batch.max_blocks if max_blocks is None else max_blocks,
                                  batch.max_pixels if max_pixels is None else max_pixels, args["samples"], args["out"],
                                  hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _buffers(batch):
    src = torch.from_numpy(batch.host).cuda()
    out = torch.full((batch.out_bytes,), R.FILL, dtype=torch.uint8, device="cuda")
    samples = torch.full((batch.sample_bytes + R.GUARD,), R.FILL, dtype=torch.uint8, device="cuda")
    return src, out, samples


def _check(ctx, images, what):
    """One launch over `images`: every RGBX byte equals the restatement's, the guard bytes behind every
    image and behind the sample planes are untouched."""
    batch = R.Batch(images)
    src, out, samples = _buffers(batch)
    assert _call(ctx, batch, src, out, samples) == 0
    got = out.cpu().numpy()
    for k, im in enumerate(images):
        o, n = int(batch.out_off[k]), im.width * im.height * 4
        bad = np.flatnonzero(got[o:o + n] != batch.expected[o:o + n])
        assert bad.size == 0, (f"{what}: image {k} ({im.width}x{im.height}, sampling {im.sampling}): {bad.size} of {n} "
                               f"bytes differ, first at pixel {bad[0] // 4} channel {bad[0] % 4}: "
                               f"{got[o + bad[0]]} vs {batch.expected[o + bad[0]]}")
        assert (got[o + n:o + n + R.GUARD] == R.FILL).all(), f"{what}: image {k}: wrote past its pixels"
    assert (samples[batch.sample_bytes:].cpu().numpy() == R.FILL).all(), f"{what}: wrote past the sample planes"
    return batch


def _gray(blocks, q=None, width=None, share_zero=True):
    """A grayscale image of the given blocks [n][64] in `width` block columns (default: one row)."""
    blocks = np.asarray(blocks, np.int64)
    bw = width or len(blocks)
    assert len(blocks) % bw == 0
    return R.Image(8 * bw, 8 * (len(blocks) // bw), None, [np.ones(64, np.int64) if q is None else q],
                   [blocks.reshape(-1, bw, 64)], share_zero)


def test_range_limit_over_its_whole_exact_domain(ctx):
    """DC-only blocks decode to the flat centred sample v = (d + 4) >> 3: d = -4100 .. 4091 sweeps every
    v in -512 .. 511 (eight times each), both ends and each seam of range_limit_idct (v = -129 / -128,
    127 / 128 and the wrap of v & 1023 at -1 / 0) included; a second image reaches the same values as
    val * q with q = 4."""
    d = np.arange(-4100, 4092)
    assert len(d) == 8192 and ((d[0] + 4) >> 3, (d[-1] + 4) >> 3) == (-512, 511)
    blocks = np.zeros((len(d), 64), np.int64)
    blocks[:, 0] = d
    d4 = np.arange(-1025, 1023)  # * 4: -4100 .. 4088
    b4 = np.zeros((len(d4), 64), np.int64)
    b4[:, 0] = d4
    q4 = np.full(64, 4, np.int64)
    batch = _check(ctx, [_gray(blocks, width=128), _gray(b4, q4, width=64)], "range limit")
    px = batch.images[0].expected_rgbx()[::8, ::8, 0].reshape(-1)  # one sample per block
    assert px[0] == 0 and px[-1] == 255 and set(px.tolist()) == set(range(256))


def test_record_formats(ctx):
    """Every shape of packed record: all 64 positions, only bit 63, only bits >= 32, only bit 0, an
    empty mask, blocks sharing record 0, negative values, val = +-1023 with q = 1, coef = +-1 with a
    16-bit table (4000 for DC, 2000 for AC), and blocks that fill the exact range on both sides (random
    AC scaled until the extreme sample lands in 480 .. 511, and the negated block)."""
    rng = np.random.default_rng(11)
    z = np.zeros(64, np.int64)

    def at(**kv):
        b = z.copy()
        for k, v in kv.items():
            b[int(k[1:])] = v
        return b
    full = rng.integers(1, 4, 64) * rng.choice([-1, 1], 64)
    hi = z.copy()
    hi[R.J.ZIGZAG[32:]] = rng.integers(-5, 6, 32)
    small = [full, -full, at(n63=7), at(n63=-7), hi, at(n0=-100), at(n0=100), z, at(n1=-3, n8=3, n9=-3)]
    q = rng.integers(1, 5, 64)
    imgs = [_gray(small + [z, z, full], q, width=4), _gray(small + [z, z, z], q, width=3, share_zero=False)]
    big = [at(n1=1023), at(n1=-1023), at(n8=-1023), at(n63=1023), at(n0=1023, n63=-1023), at(n0=-1023, n36=1023)]
    imgs.append(_gray(big))
    q16 = np.r_[4000, np.full(63, 2000)]
    imgs.append(_gray([at(n0=1), at(n0=-1), at(n9=1), at(n9=-1), at(n63=-1), at(n1=1), at(n8=-1)], q16))
    fill = []
    for _ in range(6):
        ac = np.r_[0, rng.integers(-40, 41, 63)]
        out = R.J._idct_passes(ac * 64, np.ones(64, np.int64))[2]
        s = 64 * 495.5 / np.abs(out).max()
        for step in range(64):  # a few integer nudges settle the rounding
            b = np.round(ac * s).astype(np.int64)
            m = np.abs(R.J._idct_passes(b, np.ones(64, np.int64))[2]).max()
            if 480 <= m <= 511:
                break
            s *= 495.5 / m
        assert 480 <= m <= 511
        fill += [b, -b]
    ext = R.J._idct_passes(np.array(fill), np.ones(64, np.int64))[2]
    assert ext.max() >= 480 and ext.min() <= -480
    imgs.append(_gray(fill))
    _check(ctx, imgs, "record formats")


SIZES = (1, 2, 3, 15, 16, 17)


def test_batch_geometry_in_one_launch(ctx):
    """One launch over 146 images that differ in component count, sampling (grayscale, 1x1, 2x1, 2x2)
    and size -- widths and heights 1, 2, 3, 15, 16, 17 for every sampling (the dw - 1 / dh - 1 clamps
    of the fancy upsampler, odd sizes whose last chroma sample is replicated), a 40x24 image and one
    with more than 256 blocks (two thread blocks of the IDCT grid) -- so the early exits of both
    kernels, the component-locating loop and the plane offsets are all exercised."""
    rng = np.random.default_rng(12)
    imgs = [R.random_image(rng, 130, 70, (2, 2))]
    assert imgs[0].blocks > 256
    for sampling in (None, (1, 1), (2, 1), (2, 2)):
        for w in SIZES:
            for h in SIZES:
                imgs.append(R.random_image(rng, w, h, sampling, share_zero=bool((w + h) & 1)))
    imgs.append(R.random_image(rng, 40, 24, (2, 1)))
    batch = _check(ctx, imgs, "batch geometry")
    assert batch.max_blocks == imgs[0].blocks and min(im.blocks for im in imgs) == 1
    # the inputs reach both clamps of the samples and a spread of chroma
    px = np.concatenate([im.expected_rgbx()[..., :3].reshape(-1) for im in imgs])
    assert (px == 0).any() and (px == 255).any() and len(set(px.tolist())) == 256


def test_batch_order_does_not_matter(ctx):
    """The same images in reverse order (other block bases, record offsets and grid extents)."""
    rng = np.random.default_rng(13)
    imgs = [R.random_image(rng, w, h, s) for w, h, s in ((17, 3, (2, 2)), (8, 8, None), (40, 24, (2, 2)), (1, 1, (1, 1)),
                                                         (33, 9, (2, 1)))]
    _check(ctx, imgs, "order")
    _check(ctx, imgs[::-1], "reverse order")


def test_colour_conversion_reaches_every_clamp(ctx):
    """343 flat 8x8 4:4:4 images over Y, Cb, Cr in {0, 1, 127, 128, 129, 254, 255}^3 (DC-only: the
    sample is val + 128 with q = 8): every clamp of R, G and B at both ends and the unclamped middle."""
    levels = (0, 1, 127, 128, 129, 254, 255)
    q = [np.full(64, 8, np.int64)] * 3
    imgs = []
    for y in levels:
        for cb in levels:
            for cr in levels:
                coefs = []
                for t in (y, cb, cr):
                    c = np.zeros((1, 1, 64), np.int64)
                    c[0, 0, 0] = t - 128
                    coefs.append(c)
                imgs.append(R.Image(8, 8, (1, 1), q, coefs, share_zero=False))
    batch = _check(ctx, imgs, "colour")
    rgb = np.stack([im.expected_rgbx()[0, 0, :3] for im in imgs]).astype(np.int64)
    ycc = np.array([(y, cb, cr) for y in levels for cb in levels for cr in levels], np.float64)
    ideal = np.stack([ycc[:, 0] + 1.402 * (ycc[:, 2] - 128),
                      ycc[:, 0] - 0.34414 * (ycc[:, 1] - 128) - 0.71414 * (ycc[:, 2] - 128),
                      ycc[:, 0] + 1.772 * (ycc[:, 1] - 128)], -1)
    for ch in range(3):  # the case set holds values clamped low, clamped high and in between, per channel
        assert (ideal[:, ch] < -1).any() and (ideal[:, ch] > 256).any()
        assert (rgb[ideal[:, ch] < -1, ch] == 0).all() and (rgb[ideal[:, ch] > 256, ch] == 255).all()
    assert len(batch.images) == 343


def test_reconstruct_rejects(ctx):
    """What mmf_jpeg_reconstruct refuses -- a null handle, a negative image count, a null operand,
    max_blocks / max_pixels <= 0 -- is MMF_EINVAL with nothing launched: output and sample planes
    untouched.  An empty batch is a successful no-op."""
    rng = np.random.default_rng(14)
    batch = R.Batch([R.random_image(rng, 17, 9, (2, 2)), R.random_image(rng, 8, 8, None)])
    src, out, samples = _buffers(batch)
    cases = [dict(handle=False), dict(B=-1), dict(max_blocks=0), dict(max_blocks=-3), dict(max_pixels=0),
             dict(max_pixels=-1)]
    cases += [dict(null=n) for n in ("packed", "block_off", "pk_off", "qt", "coef_blocks", "infos", "out_off", "samples",
                                     "out")]
    for kw in cases:
        assert _call(ctx, batch, src, out, samples, **kw) == EINVAL, kw
    assert _call(ctx, batch, src, out, samples, B=0) == 0
    assert _call(ctx, batch, src, out, samples, B=0, max_blocks=0, null="packed") == 0
    assert bool((out == R.FILL).all()) and bool((samples == R.FILL).all())
    assert _call(ctx, batch, src, out, samples) == 0  # the same operands are good ones
    np.testing.assert_array_equal(out.cpu().numpy(), batch.expected)
