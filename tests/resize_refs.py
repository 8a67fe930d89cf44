"""References, cases and size lists for the device resampler's tests (csrc/resize.hip,
csrc/resize_host.cpp): numpy only, imported by tests/test_resize_refs_cpu.py and tests/test_gpu_resize.py.

plan() restates the host planner's geometry (io_utils.clip_pixels' sizes and crop, Pillow's tap bounds);
window_coeffs() restates oracle/pil_resample.coeffs for the 224 coordinates of a tower window, vectorised over
the coordinates; window() runs the two integer passes over the window alone.  Everything is exact: the tests
that use these compare with equality."""
import math

import numpy as np

from oracle.pil_resample import vertical_first

PRECISION_BITS = 32 - 8 - 2
KMAX = 96  # kResizeKMax: taps per output coordinate the kernels hold
WIN = 224
FILTERS = ("bilinear", "bicubic")  # by geometry: 0 EfficientNet squash, 1 CLIP
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}

SWEEP = (1, 2, 3, 7, 113, 223, 224, 225, 227, 448, 449, 673)
SWEEP_PAIRS = [(w, h) for w in SWEEP for h in SWEEP]
TIES = (96, 160, 288, 352, 480, 672)
TIES_PAIRS = [p for t in TIES for p in ((t, t), (t, 224), (224, t))]
BUDGET = [(5264, 5264), (10528, 200), (200, 10528)]  # the last supported sizes: 95 taps
OVER = [(5265, 5265), (10529, 200), (200, 10529)]    # the first rejected sizes: 97 taps
# around Image.resize's vertical-first order (height > 100 * width and the height shrinks), in the squash (up to its
# 10528-row budget) and in CLIP (which shrinks the height only from a width of 225: 22501 rows at the least)
TALL = [(2, 223), (2, 225), (5, 500), (5, 501), (40, 4001), (105, 10528), (224, 22500), (225, 22500), (225, 22501)]


def _coef_sides():
    """(w, h, geom) jobs of the coefficient test: s -> 224 on both axes for s in 1..1024 in both filters (square
    images); CLIP's long axis (to int(224 * long / short), window offset (new_long - 224) // 2) for short sides
    1..512 with long side s + d, vertical for even s and horizontal for odd s; TIES and BUDGET in both
    geometries."""
    jobs = [(s, s, g) for s in range(1, 1025) for g in (0, 1)]
    for s in range(1, 513):
        for d in (0, 1, 3, 100, s):
            jobs.append((s, s + d, 1) if s % 2 == 0 else (s + d, s, 1))
    jobs += [(w, h, g) for w, h in TIES_PAIRS + BUDGET for g in (0, 1)]
    return list(dict.fromkeys(jobs))


COEF_SIDES = _coef_sides()


def _filter(name, x):
    """Pillow's bilinear_filter / bicubic_filter (a = -0.5) on an array, operation for operation."""
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def ksize(in_size, out_size, name):
    scale = float(in_size) / out_size
    return int(math.ceil(SUPPORT[name] * max(scale, 1.0))) * 2 + 1


def window_coeffs(in_size, out_size, first, name):
    """Bounds int64 [224][2] = (xmin, n) and fixed-point weights int64 [224][ksize] (zero at and past n) of the
    output coordinates first .. first + 223 of a resize from in_size to out_size (precompute_coeffs +
    normalize_coeffs_8bpc).  The weight sum accumulates tap by tap in ascending order, as Pillow's does."""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(first, first + WIN, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # astype truncates towards zero, as (int)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ks, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, _filter(name, ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(WIN)
    for t in range(ks):
        ww = ww + w[:, t]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(live & (ww != 0.0)[:, None], w / ww[:, None], w)
    kk = np.where(v < 0, (-0.5 + v * (1 << PRECISION_BITS)).astype(np.int64),
                  (0.5 + v * (1 << PRECISION_BITS)).astype(np.int64))
    return np.stack([xmin, n], 1), np.where(live, kk, 0)


def tap_range(in_size, out_size, xx, name):
    """[xmin, xmax) of output coordinate xx: one row of window_coeffs' bounds, as scalars."""
    scale = float(in_size) / out_size
    support = SUPPORT[name] * max(scale, 1.0)
    center = (xx + 0.5) * scale
    return max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)


def geometry(w, h, geom):
    """ow, oh, cx, cy: Pillow's resize output size and the tower window's offset in it."""
    if geom == 0 or (w, h) == (WIN, WIN):
        return WIN, WIN, 0, 0
    short, long_ = (w, h) if w <= h else (h, w)
    nl = int(224 * long_ / short)
    ow, oh = (WIN, nl) if w <= h else (nl, WIN)
    return ow, oh, (ow - WIN) // 2, (oh - WIN) // 2


def plan(w, h, geom):
    """(ow, oh, cx, cy, need_h, need_v, y0, y1, ksh, ksv, x0, x1) of the host planner, or None where a pass needs
    more than KMAX taps.  y0 .. y1 are the source rows the window's vertical taps read.  x0 .. x1 are 0, 0, except
    where Pillow runs the vertical pass first (oracle.pil_resample.vertical_first, both passes running): there
    they are the source columns the window's horizontal taps read."""
    name = FILTERS[geom]
    ow, oh, cx, cy = geometry(w, h, geom)
    need_h, need_v = int(ow != w), int(oh != h)
    ksh = ksize(w, ow, name) if need_h else 1
    ksv = ksize(h, oh, name) if need_v else 1
    if ksh > KMAX or ksv > KMAX:
        return None
    if need_v:  # = bv[0][0] and bv[223][0] + bv[223][1] of window_coeffs(h, oh, cy, name)'s bounds bv
        y0, y1 = tap_range(h, oh, cy, name)[0], tap_range(h, oh, cy + WIN - 1, name)[1]
    else:
        y0, y1 = cy, cy + WIN
    x0 = x1 = 0
    if need_h and need_v and vertical_first(w, h, oh):
        x0, x1 = tap_range(w, ow, cx, name)[0], tap_range(w, ow, cx + WIN - 1, name)[1]
    return ow, oh, cx, cy, need_h, need_v, y0, y1, ksh, ksv, x0, x1


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(src, bounds, kk):
    """acc[r][o][c] = 2^21 + sum_x src[r][xmin[o] + x][c] * kk[o][x] (int64, unclamped)."""
    acc = np.full((src.shape[0], WIN, src.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
    last = src.shape[1] - 1
    for t in range(int(bounds[:, 1].max())):
        col = np.minimum(bounds[:, 0] + t, last)  # a tap at or past n has weight 0
        acc += src[:, col, :] * kk[:, t][None, :, None]
    return acc


def window(img, geom, accs=None):
    """The tower window of a uint8 [h][w][>=3] image, computed over the window alone: the horizontal pass on source
    rows y0 .. y1 and the 224 window columns, then the vertical pass -- or, where Pillow runs the vertical pass
    first, that pass on source columns x0 .. x1 and the 224 window rows, then the horizontal one.  accs, a dict,
    receives the unclamped accumulators of the passes that ran ('h', 'v')."""
    img = np.asarray(img)[:, :, :3]
    h, w = img.shape[:2]
    name = FILTERS[geom]
    ow, oh, cx, cy, need_h, need_v, y0, y1, _, _, x0, x1 = plan(w, h, geom)
    accs = {} if accs is None else accs
    if x1 > 0:
        bv, kv = window_coeffs(h, oh, cy, name)
        accs["v"] = _pass(img[:, x0:x1].astype(np.int64).transpose(1, 0, 2), bv, kv)  # [column][window row][c]
        tmp = _clip8(accs["v"]).transpose(1, 0, 2)
        bh, kh = window_coeffs(w, ow, cx, name)
        accs["h"] = _pass(tmp.astype(np.int64), bh - np.array([x0, 0]), kh)
        return _clip8(accs["h"])
    if need_h:
        bh, kh = window_coeffs(w, ow, cx, name)
        accs["h"] = _pass(img[y0:y1].astype(np.int64), bh, kh)
        tmp = _clip8(accs["h"])
    else:
        tmp = img[y0:y1, cx:cx + WIN]
    if not need_v:
        return np.ascontiguousarray(tmp)
    bv, kv = window_coeffs(h, oh, cy, name)
    accs["v"] = _pass(tmp.astype(np.int64).transpose(1, 0, 2), bv - np.array([y0, 0]), kv)  # [column][window row][c]
    return np.ascontiguousarray(_clip8(accs["v"]).transpose(1, 0, 2))


# ---------------------------------------------------------------------------------------------- cases, all seeded
def random_image(w, h, seed=0):
    return np.random.default_rng([seed, w, h]).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def checker(w, h, period):
    """0/255 checkerboard of `period` pixels; channel c is shifted c pixels along x (period 1 has two phases
    only: channels 0 and 2 coincide there)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((((xx + c) // period + yy // period) & 1) * 255) for c in range(3)], -1).astype(np.uint8)


def impulses(w, h, seed=0):
    """Single pixels of 255 on 0: the four corners and seeded positions, in one seeded channel each."""
    g = np.random.default_rng([seed, w, h, 1])
    a = np.zeros((h, w, 3), np.uint8)
    k = max(4, (w * h) // 256)
    ys = np.concatenate([[0, 0, h - 1, h - 1], g.integers(0, h, k)])
    xs = np.concatenate([[0, w - 1, 0, w - 1], g.integers(0, w, k)])
    a[ys, xs, g.integers(0, 3, k + 4)] = 255
    return a


def step(w, h, vertical):
    """A 0/255 step at the middle: vertical = an edge between columns, else between rows; channel 1 inverted."""
    yy, xx = np.mgrid[0:h, 0:w]
    s = ((xx >= w // 2) if vertical else (yy >= h // 2)).astype(np.uint8) * 255
    return np.stack([s, 255 - s, s], -1)


CONTENT = {
    "random": lambda w, h: random_image(w, h),
    "checker1": lambda w, h: checker(w, h, 1),
    "checker2": lambda w, h: checker(w, h, 2),
    "impulses": lambda w, h: impulses(w, h),
    "vstep": lambda w, h: step(w, h, True),
    "hstep": lambda w, h: step(w, h, False),
}
STRUCTURED = [k for k in CONTENT if k != "random"]


def rgbx(img, seed=0):
    """The image with a random fourth byte per pixel (Pillow's in-memory layout; the resampler ignores it)."""
    h, w = img.shape[:2]
    x = np.random.default_rng([seed, w, h, 2]).integers(0, 256, size=(h, w, 1), dtype=np.uint8)
    return np.concatenate([img, x], -1)
