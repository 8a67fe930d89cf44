"""References for mmf_color_jitter_u8 (csrc/jitter.hip): torchvision's ColorJitter on a PIL image, as
train_cifake_forensics.py:39-45 applies it before ToTensor.

torchvision itself cannot be imported here, so ``pil_chain`` composes the Pillow calls its PIL backend makes
(torchvision/transforms/_functional_pil.py): adjust_brightness / adjust_contrast / adjust_saturation are
``ImageEnhance.Brightness / Contrast / Color(img).enhance(factor)``; adjust_hue is ``convert("HSV")``, a uint8
wrap-around add on H, ``merge`` and ``convert("RGB")``.  Pillow is the authority the kernels are tested against.

The ``np_*`` functions restate Pillow's uint8 arithmetic in numpy.  They are the readable specification of the
kernel's arithmetic; tests/test_jitter_refs_cpu.py holds them to Pillow on all 2^24 RGB triples.

Op codes (include/mmf_hip.h): 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 skip.
"""
import numpy as np
from PIL import Image, ImageEnhance

BRIGHTNESS, CONTRAST, SATURATION, HUE, SKIP = 0, 1, 2, 3, -1


# ---------------------------------------------------------------------------------------------
# Pillow, composed as torchvision's PIL backend composes it
# ---------------------------------------------------------------------------------------------
def pil_op(im: Image.Image, op: int, factor: float = 1.0, shift: int = 0) -> Image.Image:
    if op == BRIGHTNESS:
        return ImageEnhance.Brightness(im).enhance(factor)
    if op == CONTRAST:
        return ImageEnhance.Contrast(im).enhance(factor)
    if op == SATURATION:
        return ImageEnhance.Color(im).enhance(factor)
    if op == HUE:
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h = np_h + np.uint8(shift)  # uint8 wrap-around
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return im


def pil_chain(img_u8, ops, factors, hue_shift) -> np.ndarray:
    """uint8 [B, H, W, 3] -> uint8 [B, H, W, 3]: for image b the operations ops[b][0..3] in that order, with
    factors[b] = (brightness, contrast, saturation) and the H shift hue_shift[b] (0..255)."""
    img_u8 = np.asarray(img_u8)
    out = np.empty_like(img_u8)
    for b in range(img_u8.shape[0]):
        im = Image.fromarray(np.ascontiguousarray(img_u8[b]), "RGB")
        for op in np.asarray(ops[b]).tolist():
            im = pil_op(im, int(op), float(np.float32(factors[b][op])) if 0 <= op <= 2 else 1.0, int(hue_shift[b]))
        out[b] = np.asarray(im)
    return out


def all_triples() -> np.ndarray:
    """uint8 [4096, 4096, 3]: every RGB triple once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


# ---------------------------------------------------------------------------------------------
# the numpy restatement
# ---------------------------------------------------------------------------------------------
def np_luma(rgb: np.ndarray) -> np.ndarray:
    """convert("L"): (R 19595 + G 38470 + B 7471 + 0x8000) >> 16."""
    c = rgb.astype(np.uint32)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def np_blend(deg: np.ndarray, img: np.ndarray, a) -> np.ndarray:
    """Image.blend(deg, img, a) = enhance(a): float32 throughout, the product rounded before the add (no FMA);
    truncation for 0 <= a <= 1, clipping outside."""
    a32 = np.float32(a)
    d = deg.astype(np.int32)
    prod = a32 * (img.astype(np.int32) - d).astype(np.float32)  # float32 product, rounded
    t = d.astype(np.float32) + prod
    if 0.0 <= a32 <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def np_brightness(rgb, a):
    return np_blend(np.zeros_like(rgb), rgb, a)


def np_saturation(rgb, a):
    return np_blend(np.repeat(np_luma(rgb)[..., None], 3, -1), rgb, a)


def np_contrast_mean(rgb) -> int:
    """int(ImageStat.Stat(L).mean[0] + 0.5): the integer sum over the count, in double."""
    L = np_luma(rgb)
    return int(float(int(L.sum(dtype=np.uint64))) / float(L.size) + 0.5)


def np_contrast(rgb, a):
    return np_blend(np.full_like(rgb, np_contrast_mean(rgb)), rgb, a)


def np_rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """convert("HSV"): float32 differences and quotients, the hue sum in float32 when R is the maximum and in
    double otherwise, rounded to float32, then h/6 + 1, fmod and the scale by 255 in double."""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(np.float32)
    mxf = np.where(grey, 1, mx).astype(np.float32)
    s = np.clip(((cr / mxf).astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
    h_r = bc - gc  # float32
    h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32)
    h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    hh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, hh), np.where(grey, 0, s), mx], -1).astype(np.uint8)


def np_hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """convert("RGB") of an HSV image: double throughout, round-half-even."""
    H, S, V = (hsv[..., i].astype(np.float64) for i in range(3))
    h = H * 6.0 / 255.0
    i = np.floor(h)
    f = h - i
    fs = S / 255.0
    p = np.clip(np.round(V * (1.0 - fs)), 0, 255)
    q = np.clip(np.round(V * (1.0 - fs * f)), 0, 255)
    t = np.clip(np.round(V * (1.0 - fs * (1.0 - f))), 0, 255)
    k = i.astype(np.int32) % 6
    table = ((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q))
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.select([k == j for j in range(6)], [table[j][c] for j in range(6)]).astype(np.uint8)
    grey = hsv[..., 1] == 0
    out[grey] = hsv[..., 2][grey][:, None]
    return out


def np_hue(rgb, shift: int):
    hsv = np_rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + (int(shift) & 255)).astype(np.uint8)
    return np_hsv_to_rgb(hsv)


def np_chain(img_u8, ops, factors, hue_shift) -> np.ndarray:
    """pil_chain by the restatement, with the kernel's rules for values out of range: an op code outside -1..3 and
    a second contrast are skipped, the shift is taken & 255."""
    img_u8 = np.asarray(img_u8)
    out = np.empty_like(img_u8)
    for b in range(img_u8.shape[0]):
        x, seen_contrast = img_u8[b], False
        for op in np.asarray(ops[b]).tolist():
            if op == BRIGHTNESS:
                x = np_brightness(x, factors[b][0])
            elif op == CONTRAST and not seen_contrast:
                x, seen_contrast = np_contrast(x, factors[b][1]), True
            elif op == SATURATION:
                x = np_saturation(x, factors[b][2])
            elif op == HUE:
                x = np_hue(x, int(hue_shift[b]))
        out[b] = x
    return out
