"""The EfficientNet deepfake classifier trained on the device (train_cifake_forensics.py:71-379).

The script fine-tunes a timm EfficientNet inside another model class and saves a timm-named state dict (:374) that
the inference constructor's fallback path applies to nothing.  Here the DEPLOYED classifier --
Dropout(0.2) then Linear(1280, 2) on the pooled row (misinfo_forensics.py:72-76) -- is trained on a frozen backbone,
and the file written is one ``MisinfoForensics(efficientnet_weights=...)`` loads:

* ``load_cifake_data``: the script's directory contract, balanced sample and 80 / 20 split.
* ``extract_image_features``: the pooled 1280-wide row of every image, once, through the HIP tower
  (``Engine.effnet_pooled``) -- and, for the training transform's RandomHorizontalFlip, the row of the mirrored
  window (``mmf_hflip_u8`` on the staged window, after the Pillow-exact resize: Resize, then the flip, :39-45).
  With ``jitter`` the rows of K colour-jittered views of every image: the script's ColorJitter(0.2, 0.2, 0.2, 0.1)
  on the staged window, byte-exact with torchvision's PIL backend (``mmf_color_jitter_u8``), no window leaving the
  device.  With ``jpeg`` the rows of K views saved as JPEGs at given qualities and loaded back, the reference's
  RandomJPEGCompression (misinformation_dataset.py:18-57), byte-exact with Pillow (``mmf_jpeg_roundtrip_u8``).
  With ``blur``, between those two, the reference's RandomApply([GaussianBlur((5, 9), (0.1, 5.0))], 0.3)
  (misinformation_dataset.py:104-125) in torchvision's float32 arithmetic (``mmf_gaussian_blur_u8``).
* ``jitter_params``: per view and image the order of the four operations, the three factors and the hue shift.
* ``blur_params`` / ``gaussian_kernel2d``: per view and image whether the blur fires and its sigma; torch's weights.
* ``jpeg_params``: per view and image the JPEG quality.
* ``plan``: per epoch the permutation, the flip draws and the dropout masks; with views, epoch e trains on view e % K.
* ``ClassifierTrainer``: one ``mmf_effcls_train_epoch`` and one ``mmf_effcls_eval`` call per epoch on the cached
  rows, a raw state dict on a strictly higher validation accuracy (:372-374), the best classifier put back into
  the detector.
* ``HeadStageTrainer`` (``train_cifake(unfreeze="head")``): one stage deeper -- features.8, the 1x1 conv
  320 -> 1280 with its BatchNorm's affine, trained jointly with the classifier (414,722 parameters) on cached trunk
  rows [N, 49, 320] (``extract_image_features(level="trunk")``, ``Engine.effnet_trunk``) by
  ``mmf_effhead_train_epoch`` / ``mmf_effhead_eval``.  The BatchNorm runs in eval mode, so a row does not depend on
  its minibatch and the trunk can be cached; the 16 MBConv blocks stay frozen.
* ``train_cifake`` / ``python -m mmf_amd.cifake_training``: the script's entry point.

Deviations, documented in DESIGN.md §7h.  The main one: a linear probe on a frozen backbone (with
``unfreeze="head"``: the head conv stage and the classifier, BatchNorm in eval mode), where the script
fine-tunes the whole backbone together with a 1538-d fusion head of another model class.  Further: the deployed
ImageNet normalisation (misinfo_forensics.py:249-253), not the script's CLIP mean / std; the flip comes from two
cached views, and ColorJitter from ``jitter_views`` cached views (0 by default: none; K = epochs gives every image a
fresh draw in every epoch, as the script's DataLoader does), GaussianBlur and RandomJPEGCompression -- which the
script does not apply, the reference's dataset transform does -- from ``blur_views`` and ``jpeg_views``; fp32, no
autocast / GradScaler; a seeded generator instead of the global RNG; file names sorted before the seeded shuffle
(os.listdir order is arbitrary); unreadable images dropped instead of fed as a blank tensor.
"""
from __future__ import annotations

import argparse
import functools
import os
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import io_utils
from . import weights
from . import training_common as TC
from .training_common import _black, pack_keep  # pack_keep here: bool [N, 1280] -> uint64 [N, 20]

BETAS, EPS, WEIGHT_DECAY = (0.9, 0.999), 1e-8, 0.0  # torch.optim.Adam defaults (train_cifake_forensics.py:334-337)
P_DROP = 0.2                                        # the classifier's Dropout (misinfo_forensics.py:73)
WIDTH = 1280
WORDS = WIDTH // 64
PARAM_KEYS = ("classifier.1.weight", "classifier.1.bias")
N_PARAMS = 2 * WIDTH + 2  # MMF_EFFCLS_PARAMS
TRUNK_CHANNELS, TRUNK_SHAPE = 320, (49, 320)  # what features.8 reads: 7 x 7 positions of 320 channels
HEAD_PARAM_KEYS = ("features.8.0.weight", "features.8.1.weight", "features.8.1.bias") + PARAM_KEYS
HEAD_N_PARAMS = WIDTH * TRUNK_CHANNELS + 2 * WIDTH + N_PARAMS  # MMF_EFFHEAD_PARAMS = 414722
BN_EPS = weights.BN_EPS
EXTENSIONS = (".jpg", ".jpeg", ".png")
DEFAULT_FILE = "efficientnet_cifake_best.pth"


# ---------------------------------------------------------------------------------------------
# the data set
# ---------------------------------------------------------------------------------------------
def _images_in(folder: str) -> List[str]:
    if not os.path.isdir(folder):
        return []
    out = []
    for name in sorted(os.listdir(folder)):
        path = os.path.join(folder, name)
        if os.path.isfile(path) and name.lower().endswith(EXTENSIONS):
            out.append(path)
    return out


def load_cifake_data(cifake_root: str, sample_per_label: int = 2500, seed: int = 42):
    """(train_paths, train_labels, val_paths, val_labels) of a CIFAKE tree (train_cifake_forensics.py:71-151):
    REAL images from test/REAL, FAKE images from train/FAKE and test/FAKE (.jpg / .jpeg / .png, any case); a
    balanced sample of min(sample_per_label, n_real, n_fake) per label, 0 = REAL and 1 = FAKE; shuffled by
    ``random.Random(seed)`` and split 80 / 20.  ValueError when either label has no image.  File names are sorted
    before the shuffles, so the result is a function of the tree and the seed alone."""
    real = _images_in(os.path.join(cifake_root, "test", "REAL"))
    fake = _images_in(os.path.join(cifake_root, "train", "FAKE")) + _images_in(os.path.join(cifake_root, "test", "FAKE"))
    if not real or not fake:
        raise ValueError(f"Insufficient data! REAL: {len(real)}, FAKE: {len(fake)}")
    rng = random.Random(seed)
    rng.shuffle(real)
    rng.shuffle(fake)
    n = min(int(sample_per_label), len(real), len(fake))
    rows = [(p, 0) for p in real[:n]] + [(p, 1) for p in fake[:n]]
    rng.shuffle(rows)
    cut = int(0.8 * len(rows))
    paths, labels = [p for p, _ in rows], [y for _, y in rows]
    return paths[:cut], labels[:cut], paths[cut:], labels[cut:]


# ---------------------------------------------------------------------------------------------
# cached features
# ---------------------------------------------------------------------------------------------
def jitter_params(N: int, views: int, seed: int, brightness: float = 0.2, contrast: float = 0.2,
                  saturation: float = 0.2, hue: float = 0.1):
    """ColorJitter.get_params for ``views`` views of N images -> (ops int32 [views, N, 4], factors float32
    [views, N, 3], hue_shift int32 [views, N]), the arguments of ``Engine.color_jitter`` per view.  From one
    ``torch.Generator().manual_seed(seed)``, in this order: the order of the four operations as the argsort of
    ``torch.rand(views, N, 4)`` (a uniform random permutation, as get_params' ``torch.randperm(4)``); the
    brightness, contrast and saturation factors uniform in [max(0, 1 - x), 1 + x] in float32; the hue factor
    uniform in [-hue, hue] in float64, turned into the H shift as adjust_hue does, ``uint8(hue_factor * 255)``:
    truncated toward zero, then mod 256.  A zero range leaves its operation out of the chain (-1), as
    torchvision's None does; its draw is still taken, so the other draws do not depend on it."""
    g = torch.Generator().manual_seed(int(seed))
    ops = torch.argsort(torch.rand(views, N, 4, generator=g), dim=-1).numpy().astype(np.int32)
    ranges = (float(brightness), float(contrast), float(saturation))
    factors = np.ones((views, N, 3), np.float32)
    for k, x in enumerate(ranges):
        if x < 0:
            raise ValueError(f"jitter_params: a negative range {x}")
        draw = torch.empty(views, N, dtype=torch.float32).uniform_(max(0.0, 1.0 - x), 1.0 + x, generator=g).numpy()
        if x > 0:
            factors[..., k] = draw
    if not 0 <= float(hue) <= 0.5:
        raise ValueError(f"jitter_params: hue must be in [0, 0.5], got {hue}")
    h = torch.empty(views, N, dtype=torch.float64).uniform_(-float(hue), float(hue), generator=g).numpy()
    hue_shift = (np.trunc(h * 255).astype(np.int64) % 256).astype(np.int32)
    for k, x in enumerate(ranges + (float(hue),)):
        if x == 0:
            ops[ops == k] = -1
    return ops, factors, hue_shift


def jpeg_params(N: int, views: int, seed: int, quality_range=(40, 80)) -> np.ndarray:
    """RandomJPEGCompression's draw for ``views`` views of N images -> int32 [views, N], the ``quality`` of
    ``Engine.jpeg_compress`` per view: uniform on the closed range, as the reference's ``random.randint(lo, hi)``.
    From a ``torch.Generator`` of its own, seeded by ``seed`` alone: ``jitter_params`` with the same seed draws what it
    drew without.  ValueError for a range outside 1..100 or reversed."""
    try:
        lo, hi = (int(v) for v in quality_range)
    except (TypeError, ValueError):
        raise ValueError(f"jpeg_params: quality_range must be (lo, hi), got {quality_range!r}") from None
    if not 1 <= lo <= hi <= 100:
        raise ValueError(f"jpeg_params: quality_range must satisfy 1 <= lo <= hi <= 100, got ({lo}, {hi})")
    if int(views) < 0 or int(N) < 0:
        raise ValueError(f"jpeg_params: N and views must be >= 0, got {N}, {views}")
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, (int(views), int(N)), generator=g).numpy().astype(np.int32)


BLUR_KERNEL_SIZE = (5, 9)  # the reference's GaussianBlur(kernel_size=(5, 9)): 5 wide, 9 high
BLUR_MAX_TAPS = 15         # kBlurMaxTaps


def _kernel_size(kernel_size, what: str) -> Tuple[int, int]:
    try:
        kx, ky = (int(v) for v in kernel_size)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: kernel_size must be (kx, ky), got {kernel_size!r}") from None
    if not all(1 <= k <= BLUR_MAX_TAPS and k % 2 for k in (kx, ky)):
        raise ValueError(f"{what}: kernel_size must be two odd numbers in 1..{BLUR_MAX_TAPS}, got ({kx}, {ky})")
    return kx, ky


def _kernel1d(k: int, sigma: float) -> torch.Tensor:
    """torchvision's _get_gaussian_kernel1d, in its own torch CPU operations."""
    lim = (k - 1) * 0.5
    x = torch.linspace(-lim, lim, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_kernel2d(sigma, kernel_size=BLUR_KERNEL_SIZE) -> np.ndarray:
    """The weights of torchvision's GaussianBlur for one sigma (both axes) -> float32 [ky, kx], or for an array of
    sigmas [...] -> [..., ky, kx]; ``kernel_size`` = (kx, ky), width first.  torchvision's own float32 operations on
    the CPU (linspace, exp of -0.5 (x / sigma)^2, the division by the sum, the outer product by ``torch.mm``), so
    the floats are torch's bit for bit and ``mmf_gaussian_blur_u8`` never evaluates an exp.  An array goes through
    the one-sigma computation element by element: torch's vectorised exp need not round as its scalar one does, and
    a window costs microseconds.  ValueError for a sigma that is not a positive finite number."""
    kx, ky = _kernel_size(kernel_size, "gaussian_kernel2d")
    s = np.asarray(sigma, dtype=np.float64)
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"gaussian_kernel2d: sigma must be positive and finite, got {sigma!r}")
    out = np.empty(s.shape + (ky, kx), np.float32)
    flat = out.reshape(-1, ky, kx)
    for n, v in enumerate(s.reshape(-1).tolist()):
        flat[n] = torch.mm(_kernel1d(ky, v)[:, None], _kernel1d(kx, v)[None, :]).numpy()
    return out


def blur_params(N: int, views: int, seed: int, p: float = 0.3, sigma=(0.1, 5.0)):
    """RandomApply([GaussianBlur(sigma=(lo, hi))], p)'s draws for ``views`` views of N images -> (apply bool
    [views, N], sigma float32 [views, N]), the ``apply`` and ``sigma`` of ``Engine.gaussian_blur`` per view.  From a
    ``torch.Generator`` of its own, seeded by ``seed`` alone, in this order: ``torch.rand(views, N) <= p`` as
    RandomApply tests it (torchvision skips when ``p < torch.rand(1)``), then the sigmas as GaussianBlur.get_params'
    ``torch.empty(...).uniform_(lo, hi)`` in float32 -- drawn for every image, applied or not, so the draws do not
    depend on p.  ``jitter_params`` and ``jpeg_params`` with the same seed draw what they drew without.  ValueError
    for p outside [0, 1] or a range that is not 0 < lo <= hi."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"blur_params: p must be in [0, 1], got {p}")
    try:
        lo, hi = (float(v) for v in sigma)
    except (TypeError, ValueError):
        raise ValueError(f"blur_params: sigma must be (lo, hi), got {sigma!r}") from None
    if not 0.0 < lo <= hi < float("inf"):
        raise ValueError(f"blur_params: sigma must satisfy 0 < lo <= hi, got ({lo}, {hi})")
    if int(views) < 0 or int(N) < 0:
        raise ValueError(f"blur_params: N and views must be >= 0, got {N}, {views}")
    g = torch.Generator().manual_seed(int(seed))
    apply = (torch.rand(int(views), int(N), generator=g) <= float(p)).numpy()
    s = torch.empty(int(views), int(N), dtype=torch.float32).uniform_(lo, hi, generator=g).numpy()
    return apply, s


def _blur_arg(blur, N: int):
    try:
        apply, sigma = (np.asarray(a) for a in blur)
    except (TypeError, ValueError):
        raise ValueError("blur: expected (apply, sigma)") from None
    if (apply.ndim != 2 or apply.shape[1] != N or apply.shape[0] < 1 or sigma.shape != apply.shape
            or apply.dtype != np.bool_ or sigma.dtype.kind != "f"):
        raise ValueError(f"blur: expected apply bool [K, {N}] and sigma float [K, {N}], K >= 1, got {apply.shape} "
                         f"{apply.dtype}, {sigma.shape} {sigma.dtype}")
    if sigma.size and not (np.isfinite(sigma).all() and (sigma > 0).all()):
        raise ValueError("blur: every sigma must be positive and finite")
    return apply, sigma.astype(np.float32)


def _jpeg_arg(jpeg, N: int) -> np.ndarray:
    q = np.asarray(jpeg)
    if q.ndim != 2 or q.shape[1] != N or q.shape[0] < 1 or q.dtype.kind not in "iu":
        raise ValueError(f"jpeg: expected int qualities [K, {N}], K >= 1, got {q.shape} {q.dtype}")
    if q.size and (q.min() < 1 or q.max() > 100):
        raise ValueError(f"jpeg: qualities must be in 1..100, got {q.min()}..{q.max()}")
    return q.astype(np.int32)


def extract_image_features(forensics, image_paths: Sequence, flip: bool = False, jitter=None, jpeg=None, blur=None,
                           level: str = "pooled"):
    """What the frozen backbone gives for every image -> (feats float32 [N, 1280], ok bool [N]), with ``flip`` also
    the rows of the mirrored windows: (feats, flipped float32 [N, 1280], ok).  In ``max_batch`` chunks: the images
    staged as analyze_pairs stages them (device JPEG decode where it applies, Pillow otherwise, the Pillow-exact
    squash to 224 x 224 on the device), the window mirrored on the device, both through ``Engine.effnet_pooled``.
    An image that cannot be read gives ok False and zero rows.

    ``jitter`` = (ops, factors, hue_shift) of ``jitter_params(N, views, ...)``: the rows become float32
    [views, N, 1280] (both of them with ``flip``), view v being the staged window after ``Engine.color_jitter``
    with draw v.  Every operation is per pixel or a whole-image mean, so jitter and flip commute exactly: the
    mirrored view is the mirror of the jittered window.  That holds for jitter only.

    ``jpeg`` = the int qualities [K, N] of ``jpeg_params(N, K, ...)``: view v is ``Engine.jpeg_compress`` of the
    window at jpeg[v] -- of the jittered window where ``jitter`` is given too, the reference's order (its K must be
    the same: ValueError otherwise).  The JPEG round trip does NOT commute with the mirror: the bias of the chroma
    downsampling alternates with the column's parity, and so does the upsampling's.  So with ``flip`` the mirrored
    row is that of ``jpeg_compress(hflip(window))``, mirrored first and compressed after as in the reference's
    Compose, not that of the mirrored compressed window.

    ``blur`` = (apply bool [K, N], sigma float [K, N]) of ``blur_params(N, K, ...)``: view v passes through
    ``Engine.gaussian_blur`` with draw v between the jitter and the JPEG round trip, the Compose's order (K must
    agree with the other two where they are given: ValueError otherwise).  The blur does not commute with the mirror
    bit for bit either: its taps are added left to right in a fixed order, and a float32 sum taken in the opposite
    order can round to the other side at a tie.  So with ``flip`` the mirrored row is that of
    ``gaussian_blur(hflip(window))``, mirrored first and blurred after, and the JPEG round trip follows.

    ``level`` = "trunk": the rows ``HeadStageTrainer`` reads instead, the last MBConv block's output [.., N, 49, 320]
    (``Engine.effnet_trunk``), through the same staging, flip, jitter, blur and JPEG path: only the final tower call
    differs.  They come back as float32 TENSORS ON THE ENGINE'S DEVICE, filled chunk by chunk -- 62,720 bytes per view
    and image, so 4,000 images x 2 flips x 10 views take 5.0 GB there -- and no more than one chunk of windows exists
    at a time.  Both results are views of one allocation laid out as the trainer's bank, so ``HeadStageTrainer.fit``
    trains on them in place; selecting rows out of them (an unreadable image dropped) makes a copy, and ``fit`` then
    builds its bank as a second one: twice the size at the peak."""
    if level not in ("pooled", "trunk"):
        raise ValueError(f"level must be 'pooled' or 'trunk', got {level!r}")
    trunk = level == "trunk"
    row = TRUNK_SHAPE if trunk else (WIDTH,)
    paths = list(image_paths)
    N = len(paths)
    if jpeg is not None:
        jpeg = _jpeg_arg(jpeg, N)
    if blur is not None:
        b_apply, b_sigma = _blur_arg(blur, N)
    counts = {}  # the K of each step that is given
    if jitter is not None:
        j_ops, j_fac, j_hue = (np.asarray(a) for a in jitter)
        views = j_ops.shape[0]
        if j_ops.shape != (views, N, 4) or j_fac.shape != (views, N, 3) or j_hue.shape != (views, N) or views < 1:
            raise ValueError(f"jitter: expected ops [K, {N}, 4], factors [K, {N}, 3], hue_shift [K, {N}], K >= 1, got "
                             f"{j_ops.shape}, {j_fac.shape}, {j_hue.shape}")
        counts["jitter"] = views
    if blur is not None:
        counts["blur"] = b_apply.shape[0]
    if jpeg is not None:
        counts["jpeg"] = jpeg.shape[0]
    if len(set(counts.values())) > 1:
        raise ValueError(" and ".join(f"{name} has {k} views" for name, k in counts.items()) + ": they must agree")
    plain = not counts
    views = 0 if plain else next(iter(counts.values()))
    shape = ((N,) if plain else (views, N)) + row
    if trunk:
        # ONE allocation in plan()'s bank order -- per view its rows, then its mirrored rows -- of which the two
        # results are views: HeadStageTrainer.fit recognises the layout and trains on it without a second copy
        base = torch.zeros((max(views, 1), 2 if flip else 1, N) + row, dtype=torch.float32,
                           device=forensics.engine.device)
        feats = base[0, 0] if plain else base[:, 0]
        flipped = (base[0, 1] if plain else base[:, 1]) if flip else None
    else:
        feats = np.zeros(shape, np.float32)
        flipped = np.zeros(shape, np.float32) if flip else None
    ok = np.ones(N, bool)
    cap = forensics.engine.max_batch
    chunks = [(a, min(a + cap, N)) for a in range(0, N, cap)]
    if chunks:
        forensics._ensure_jpeg_stager()
        forensics.detector.sync(("effnet",))

    def host_stage(a, b):
        try:
            return a, b, forensics._stage_images(paths[a:b])
        except Exception:  # noqa: BLE001  (a file of the chunk does not open: each on its own, marked where it fails)
            pils = []
            for i, p in enumerate(paths[a:b]):
                try:
                    pils.append(io_utils.to_pil(p))
                except Exception:  # noqa: BLE001
                    pils.append(_black())
                    ok[a + i] = False
            return a, b, forensics._stage_images(pils)

    def tower(eng, x):
        return eng.effnet_trunk(x) if trunk else eng.effnet_pooled(x).cpu().numpy()

    def after_flip(eng, x, v, a, b):
        """What follows the flip in the Compose for view v of images a .. b - 1 -- the blur, the JPEG round trip --
        and the tower."""
        if blur is not None:
            x = eng.gaussian_blur(x, b_sigma[v, a:b], b_apply[v, a:b])
        if jpeg is not None:
            x = eng.jpeg_compress(x, jpeg[v, a:b])
        return tower(eng, x)

    def device_part(staged):
        a, b, rgb = staged
        eff, _ = forensics._windows(*rgb)
        eng = forensics.engine
        if plain:
            feats[a:b] = tower(eng, eff)
            if flip:
                flipped[a:b] = tower(eng, eng.hflip(eff))
            return
        for v in range(views):
            win = eff if jitter is None else eng.color_jitter(eff, j_ops[v, a:b], j_fac[v, a:b], j_hue[v, a:b])
            feats[v, a:b] = after_flip(eng, win, v, a, b)
            if flip:
                flipped[v, a:b] = after_flip(eng, eng.hflip(win), v, a, b)

    if chunks:
        forensics._run_chunks(chunks, host_stage, device_part)
    bad = np.flatnonzero(~ok)  # (an index list: the same statement for an array and for a device tensor)
    for out in (feats, flipped):
        if out is not None and len(bad):
            if plain:
                out[bad] = 0
            else:
                out[:, bad] = 0
    if flip:
        return feats, flipped, ok
    return feats, ok


# ---------------------------------------------------------------------------------------------
# the epoch plan
# ---------------------------------------------------------------------------------------------
unpack_keep = functools.partial(TC.unpack_keep, width=WIDTH)  # uint64 [N, 20] -> bool [N, 1280]


def plan(N: int, batch_size: int, epochs: int, seed: int, flip: bool = True, views: int = 0):
    """Per epoch (perm int32 [N], keep uint64 [N, 20], flipped bool [N]) from one
    ``torch.Generator().manual_seed(seed)``: the DataLoader's shuffle as ``torch.randperm(N)``; with ``flip`` the
    RandomHorizontalFlip draws ``torch.rand(N) < 0.5`` indexed by data-set row (all False without); the dropout
    masks ``torch.rand(N, 1280) >= 0.2`` (row i = the row at position i of the epoch order).  ``perm`` holds the
    KERNEL's entries: row + N where the row is flipped, the mirrored view being rows N .. 2N - 1 of the bank.

    ``views`` = K > 0 colour-jittered views take no further draw: epoch e (from 0) trains on view e % K, and the
    bank is K blocks in view order -- with ``flip`` each block the view's rows, then its mirrored rows, the entry
    row + N (2 view + flipped); without, the entry row + N view."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for e in range(int(epochs)):
        order = torch.randperm(N, generator=g).numpy().astype(np.int64)
        flipped = (torch.rand(N, generator=g) < 0.5).numpy() if flip else np.zeros(N, bool)
        keep = pack_keep((torch.rand(N, WIDTH, generator=g) >= P_DROP).numpy())
        block = flipped[order].astype(np.int64)
        if views > 0:
            block = (2 * (e % views) + block) if flip else np.full(N, e % views, np.int64)
        out.append(((order + N * block).astype(np.int32), keep, flipped))
    return out


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
def _classifier(detector):
    return getattr(detector.efficientnet.classifier, "1")


def flatten_classifier(detector) -> torch.Tensor:
    """classifier.1.weight | classifier.1.bias of the detector's EfficientNet as one float32 [2562] tensor."""
    lin = _classifier(detector)
    flat = torch.cat([lin.weight.detach().reshape(-1).float(), lin.bias.detach().reshape(-1).float()])
    if flat.numel() != N_PARAMS:
        raise ValueError(f"a classifier of {flat.numel()} parameters, expected {N_PARAMS}")
    return flat


class ClassifierTrainer:
    """The training loop of train_cifake_forensics.py:351-376 on cached pooled rows: per epoch one training call and
    one validation call on the device.  ``fit`` ends with ONE re-pack of the detector's effnet component
    (``detector.sync``), which also re-runs the load-time precision calibration on the new classifier."""

    def __init__(self, forensics, batch_size: int = 16, epochs: int = 10, lr: float = 1e-4, seed: int = 0,
                 flip: bool = True, weight_decay: float = WEIGHT_DECAY, jitter_views: int = 0):
        if not 1 <= int(batch_size) <= 64:
            raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
        if int(jitter_views) < 0:
            raise ValueError(f"jitter_views must be >= 0, got {jitter_views}")
        self.jitter_views = int(jitter_views)
        self.forensics, self.batch_size, self.epochs = forensics, int(batch_size), int(epochs)
        self.lr, self.seed, self.flip, self.weight_decay = float(lr), int(seed), bool(flip), float(weight_decay)

    @staticmethod
    def _data(feats, labels, what):
        return TC.check_rows(what, (feats,), (WIDTH,), labels)

    def fit(self, train, train_labels, val, val_labels, checkpoint_path: Optional[str] = None,
            save_full_model: bool = False) -> List[dict]:
        """``train``: float32 [N, 1280], or with ``flip`` the pair (rows, rows of the mirrored windows); with
        ``jitter_views`` = K each of them float32 [K, N, 1280], as ``extract_image_features(jitter=...)`` returns."""
        f = self.forensics
        eng, det = f.engine, f.detector
        dev = eng.device
        K = self.jitter_views
        if self.flip and not (isinstance(train, (tuple, list)) and len(train) == 2):
            raise ValueError("flip=True needs train = (features, features of the mirrored windows)")
        parts = tuple(train) if self.flip else (train,)
        if K:
            parts = tuple(np.asarray(p) for p in parts)
            if any(p.ndim != 3 or p.shape[0] != K for p in parts):
                raise ValueError(f"jitter_views={K} needs training features [{K}, N, {WIDTH}], got "
                                 f"{[p.shape for p in parts]}")
        # the bank's blocks in plan()'s order: per view its rows, then (flip) its mirrored rows
        blocks = [p[v] if K else p for v in range(max(K, 1)) for p in parts]
        names = ("training", "mirrored training")
        blocks = [self._data(x, train_labels, names[i % len(parts)]) for i, x in enumerate(blocks)]
        yt = blocks[0][1]
        if len(blocks) == 1:
            bank, bank_labels = blocks[0]
        else:
            bank, bank_labels = np.concatenate([x for x, _ in blocks]), np.concatenate([yt] * len(blocks))
        xv, yv = self._data(val, val_labels, "validation")
        N, bs = len(yt), self.batch_size
        bank, bank_labels, xv, yv_d = (torch.from_numpy(a).to(dev) for a in (bank, bank_labels, xv, yv))
        params = flatten_classifier(det).to(dev).contiguous()
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        spe = -(-N // bs)
        history, best_acc, best, step0 = [], 0.0, None, 0
        for epoch, (perm, keep, _) in enumerate(plan(N, bs, self.epochs, self.seed, self.flip, K), 1):
            sl, sc = eng.effcls_train_epoch(bank, bank_labels, torch.from_numpy(perm).to(dev),
                                            torch.from_numpy(keep.view(np.int64)).to(dev), P_DROP, bs, self.lr, BETAS,
                                            EPS, self.weight_decay, step0, params, m, v)
            bl, lg = eng.effcls_eval(xv, yv_d, bs, params)
            step0 += spe
            # train_cifake_forensics.py:224, :270
            train_loss, train_acc, val_loss, val_acc, _ = TC.classifier_epoch_metrics(epoch, sl, sc, bl, lg, N, yv)
            history.append({"epoch": epoch, "train_loss": train_loss, "train_acc": train_acc, "val_loss": val_loss,
                            "val_acc": val_acc})
            if val_acc > best_acc:  # :372
                best_acc, best = val_acc, params.clone()
                if checkpoint_path:
                    torch.save(self._state(best, save_full_model), checkpoint_path)
        self.best_val_acc = best_acc
        self._install(best if best is not None else params)
        return history

    def _tensors(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        flat = flat.detach().cpu()
        return {PARAM_KEYS[0]: flat[:2 * WIDTH].reshape(2, WIDTH).clone(), PARAM_KEYS[1]: flat[2 * WIDTH:].clone()}

    def _state(self, flat: torch.Tensor, full: bool) -> Dict[str, torch.Tensor]:
        """A raw state dict in torchvision names, as the script saves a raw one (:374): the two classifier tensors,
        or (``full``) the whole detector.efficientnet.state_dict() with them."""
        cls = self._tensors(flat)
        if not full:
            return cls
        sd = {k: t.detach().cpu() for k, t in self.forensics.detector.efficientnet.state_dict().items()}
        sd.update(cls)
        return sd

    def _install(self, flat: torch.Tensor) -> None:
        """In-place copies bump the parameters' version counters; detector.sync() then re-packs the effnet component
        and re-runs check_effnet_precision, whose calibration depends on the classifier's logits."""
        det = self.forensics.detector
        lin, t = _classifier(det), self._tensors(flat)
        with torch.no_grad():
            lin.weight.copy_(t[PARAM_KEYS[0]])
            lin.bias.copy_(t[PARAM_KEYS[1]])
        det.sync(("effnet",))


# ---------------------------------------------------------------------------------------------
# the head conv stage, trained with the classifier
# ---------------------------------------------------------------------------------------------
def _head_stage(detector):
    stage = getattr(detector.efficientnet.features, "8")
    return getattr(stage, "0"), getattr(stage, "1")


def flatten_head_stage(detector) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(params float32 [414722], running_mean float32 [1280], running_var float32 [1280]) of the detector's
    EfficientNet: features.8.0.weight | features.8.1.weight | features.8.1.bias | classifier.1.weight |
    classifier.1.bias in state-dict order as one flat tensor, and the BatchNorm's statistics (copies)."""
    conv, bn = _head_stage(detector)
    lin = _classifier(detector)
    flat = torch.cat([t.detach().reshape(-1).float() for t in (conv.weight, bn.weight, bn.bias, lin.weight, lin.bias)])
    if flat.numel() != HEAD_N_PARAMS or tuple(conv.weight.shape[:2]) != (WIDTH, TRUNK_CHANNELS):
        raise ValueError(f"a head stage of {flat.numel()} parameters, expected {HEAD_N_PARAMS}")
    return flat, bn.running_mean.detach().float().clone(), bn.running_var.detach().float().clone()


class HeadStageTrainer(ClassifierTrainer):
    """ClassifierTrainer's loop one stage deeper: features.8 (the 1x1 conv and its BatchNorm's affine, in eval mode:
    the running statistics are read, never updated) is trained jointly with the classifier on cached trunk rows
    [.., N, 49, 320] (``extract_image_features(level="trunk")``), per epoch one ``mmf_effhead_train_epoch`` and one
    ``mmf_effhead_eval`` call.  The bank stays on the device: 49 x 320 x 4 = 62,720 bytes per view and image, so
    4,000 images x 2 flips x 10 views take 5.0 GB -- once, where the rows come from ``extract_image_features`` and
    are passed on whole (``_bank``); twice at the peak where they had to be copied together.  The best parameters are kept on a strictly higher validation
    accuracy; the checkpoint is a raw state dict of the five torchvision-named tensors."""

    @staticmethod
    def _data(feats, labels, what):
        """Trunk rows float32 [N, 49, 320] (a numpy array or a tensor on any device) and labels [N] of 0 / 1 -> the
        rows as a contiguous tensor, the labels int32."""
        x = feats if torch.is_tensor(feats) else torch.from_numpy(np.ascontiguousarray(np.asarray(feats, np.float32)))
        y = np.asarray(labels)
        if x.dim() != 3 or tuple(x.shape[1:]) != TRUNK_SHAPE or x.shape[0] < 1 or y.shape != (x.shape[0],):
            raise ValueError(f"{what} trunk rows {tuple(x.shape)} / labels {y.shape} must be [N, 49, 320] / [N], N >= 1")
        if x.dtype != torch.float32 or not bool(torch.isfinite(x).all()):
            raise ValueError(f"{what} trunk rows must be finite float32")
        if not np.isin(y, (0, 1)).all():
            raise ValueError(f"{what} labels must be 0 / 1")
        return x.contiguous(), y.astype(np.int32)

    def fit(self, train, train_labels, val, val_labels, checkpoint_path: Optional[str] = None,
            save_full_model: bool = False) -> List[dict]:
        """``train``: trunk rows [N, 49, 320], or with ``flip`` the pair (rows, rows of the mirrored windows); with
        ``jitter_views`` = K each of them [K, N, 49, 320], as ``extract_image_features(level="trunk")`` returns."""
        f = self.forensics
        eng, det = f.engine, f.detector
        dev = eng.device
        K = self.jitter_views
        if self.flip and not (isinstance(train, (tuple, list)) and len(train) == 2):
            raise ValueError("flip=True needs train = (trunk rows, trunk rows of the mirrored windows)")
        parts = tuple(train) if self.flip else (train,)
        if K and any(p.ndim != 4 or p.shape[0] != K for p in parts):
            raise ValueError(f"jitter_views={K} needs training trunk rows [{K}, N, 49, 320], got "
                             f"{[tuple(p.shape) for p in parts]}")
        # the bank's blocks in plan()'s order: per view its rows, then (flip) its mirrored rows
        blocks = [p[v] if K else p for v in range(max(K, 1)) for p in parts]
        names = ("training", "mirrored training")
        blocks = [self._data(x, train_labels, names[i % len(parts)]) for i, x in enumerate(blocks)]
        yt = blocks[0][1]
        bank = self._bank([x for x, _ in blocks], dev)
        bank_labels = torch.from_numpy(np.concatenate([yt] * len(blocks))).to(dev)
        xv, yv = self._data(val, val_labels, "validation")
        xv, yv_d = xv.to(dev), torch.from_numpy(yv).to(dev)
        N, bs = len(yt), self.batch_size
        params, mean, var = (t.to(dev).contiguous() for t in flatten_head_stage(det))
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        spe = -(-N // bs)
        history, best_acc, best, step0 = [], 0.0, None, 0
        for epoch, (perm, keep, _) in enumerate(plan(N, bs, self.epochs, self.seed, self.flip, K), 1):
            sl, sc = eng.effhead_train_epoch(bank, bank_labels, torch.from_numpy(perm).to(dev),
                                             torch.from_numpy(keep.view(np.int64)).to(dev), P_DROP, bs, mean, var,
                                             BN_EPS, self.lr, BETAS, EPS, self.weight_decay, step0, params, m, v)
            bl, lg = eng.effhead_eval(xv, yv_d, bs, params, mean, var, BN_EPS)
            step0 += spe
            train_loss, train_acc, val_loss, val_acc, _ = TC.classifier_epoch_metrics(epoch, sl, sc, bl, lg, N, yv)
            history.append({"epoch": epoch, "train_loss": train_loss, "train_acc": train_acc, "val_loss": val_loss,
                            "val_acc": val_acc})
            if val_acc > best_acc:
                best_acc, best = val_acc, params.clone()
                if checkpoint_path:
                    torch.save(self._state(best, save_full_model), checkpoint_path)
        self.best_val_acc = best_acc
        self._install(best if best is not None else params)
        return history

    @staticmethod
    def _bank(blocks, dev) -> torch.Tensor:
        """The blocks [N, 49, 320] as one bank [len(blocks) N, 49, 320] on the device.  Blocks that already lie there
        one behind the other in one allocation (what ``extract_image_features(level="trunk")`` returns) are taken as
        they are; anything else is copied together, the bank then existing beside the caller's tensors."""
        first, n = blocks[0], blocks[0].numel() * 4
        if first.device == dev and all(b.device == dev and b.untyped_storage().data_ptr() ==
                                       first.untyped_storage().data_ptr() and b.data_ptr() == first.data_ptr() + i * n
                                       for i, b in enumerate(blocks)):
            return torch.as_strided(first, (len(blocks) * first.shape[0],) + TRUNK_SHAPE, (49 * 320, 320, 1))
        return blocks[0].to(dev) if len(blocks) == 1 else torch.cat([b.to(dev) for b in blocks])

    def _tensors(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        flat = flat.detach().cpu()
        shapes = ((WIDTH, TRUNK_CHANNELS, 1, 1), (WIDTH,), (WIDTH,), (2, WIDTH), (2,))
        out, o = {}, 0
        for key, shape in zip(HEAD_PARAM_KEYS, shapes):
            n = int(np.prod(shape))
            out[key] = flat[o:o + n].reshape(shape).clone()
            o += n
        return out

    def _install(self, flat: torch.Tensor) -> None:
        """In-place copies, then ONE detector.sync: it re-folds the BatchNorm into the fp16 and fp32 head weights and
        re-runs check_effnet_precision on the new stage."""
        det = self.forensics.detector
        conv, bn = _head_stage(det)
        lin, t = _classifier(det), self._tensors(flat)
        with torch.no_grad():
            for dst, key in zip((conv.weight, bn.weight, bn.bias, lin.weight, lin.bias), HEAD_PARAM_KEYS):
                dst.copy_(t[key])
        det.sync(("effnet",))


# ---------------------------------------------------------------------------------------------
# the script's entry point
# ---------------------------------------------------------------------------------------------
def train_cifake(cifake_root: str, batch_size: int = 16, lr: float = 1e-4, epochs: int = 10,
                 sample_per_label: int = 2500, forensics=None, checkpoint_path: Optional[str] = DEFAULT_FILE, *,
                 device: str = "cuda", seed: int = 0, flip: bool = True, save_full_model: bool = False,
                 jitter_views: int = 0, jpeg_views: int = 0, jpeg_quality=(40, 80), blur_views: int = 0,
                 blur_p: float = 0.3, blur_sigma=(0.1, 5.0), unfreeze: str = "classifier"):
    """train_cifake_forensics.py:276-379: the CIFAKE tree's balanced sample and split, one feature extraction per
    split (two views of the training images with ``flip``; with ``jitter_views`` = K, K colour-jittered draws of
    each, from ``jitter_params(N, K, seed)``; with ``blur_views`` = K, K views blurred with probability ``blur_p``
    at a sigma drawn from ``blur_sigma``, ``blur_params(N, K, seed, blur_p, blur_sigma)``; with ``jpeg_views`` = K,
    K views saved as JPEGs at a quality drawn from the closed range ``jpeg_quality`` and loaded back,
    ``jpeg_params(N, K, seed, jpeg_quality)`` -- the ones that are non-zero must be equal, and view v is jittered
    first, blurred next and compressed last, the order of the reference dataset's Compose), unreadable images
    dropped and counted, then the trainer.  Returns the history.

    ``unfreeze`` = "classifier": the linear probe on cached pooled rows (``ClassifierTrainer``).  "head": features.8
    as well, on cached trunk rows (``HeadStageTrainer``; the rows stay on the device, 62,720 bytes per view and
    image)."""
    if unfreeze not in ("classifier", "head"):
        raise ValueError(f"unfreeze must be 'classifier' or 'head', got {unfreeze!r}")
    level = "trunk" if unfreeze == "head" else "pooled"
    jitter_views, blur_views, jpeg_views = int(jitter_views), int(blur_views), int(jpeg_views)
    if jitter_views < 0 or blur_views < 0 or jpeg_views < 0:
        raise ValueError(f"jitter_views, blur_views and jpeg_views must be >= 0, got {jitter_views}, {blur_views}, "
                         f"{jpeg_views}")
    if len({k for k in (jitter_views, blur_views, jpeg_views) if k}) > 1:
        raise ValueError(f"jitter_views={jitter_views}, blur_views={blur_views} and jpeg_views={jpeg_views}: the ones "
                         f"that are set must be equal")
    if jpeg_views:
        jpeg_params(0, 0, seed, jpeg_quality)  # the range checked before any file is read
    if blur_views:
        blur_params(0, 0, seed, blur_p, blur_sigma)
    views = jitter_views or blur_views or jpeg_views
    tr_p, tr_y, va_p, va_y = load_cifake_data(cifake_root, sample_per_label)
    print(f"Loaded {len(tr_p)} training samples ({tr_y.count(0)} REAL, {tr_y.count(1)} FAKE)")
    print(f"Loaded {len(va_p)} validation samples ({va_y.count(0)} REAL, {va_y.count(1)} FAKE)")
    if forensics is None:
        from .api import MisinfoForensics
        forensics = MisinfoForensics(device=device)
    jitter = jitter_params(len(tr_p), jitter_views, seed) if jitter_views else None
    jpeg = jpeg_params(len(tr_p), jpeg_views, seed, jpeg_quality) if jpeg_views else None
    blur = blur_params(len(tr_p), blur_views, seed, blur_p, blur_sigma) if blur_views else None
    out = extract_image_features(forensics, tr_p, flip=flip, jitter=jitter, jpeg=jpeg, blur=blur, level=level)
    ok_t = out[-1]
    xv, ok_v = extract_image_features(forensics, va_p, level=level)
    dropped = int((~ok_t).sum() + (~ok_v).sum())
    if dropped:
        print(f"Dropped {dropped} unreadable images")
    tr_y, va_y = np.asarray(tr_y)[ok_t], np.asarray(va_y)[ok_v]
    if level == "trunk":
        def readable(t, ok):  # device tensors [.., N, 49, 320]: nothing dropped (the usual case) makes no second copy
            return t if ok.all() else t[..., torch.from_numpy(np.flatnonzero(ok)).to(t.device), :, :]
        train = tuple(readable(o, ok_t) for o in out[:-1])
        train = train if flip else train[0]
        trainer = HeadStageTrainer(forensics, batch_size=batch_size, epochs=epochs, lr=lr, seed=seed, flip=flip,
                                   jitter_views=views)
        history = trainer.fit(train, tr_y, readable(xv, ok_v), va_y, checkpoint_path=checkpoint_path,
                              save_full_model=save_full_model)
    else:
        train = (out[0][..., ok_t, :], out[1][..., ok_t, :]) if flip else out[0][..., ok_t, :]
        trainer = ClassifierTrainer(forensics, batch_size=batch_size, epochs=epochs, lr=lr, seed=seed, flip=flip,
                                    jitter_views=views)
        history = trainer.fit(train, tr_y, xv[ok_v], va_y, checkpoint_path=checkpoint_path,
                              save_full_model=save_full_model)
    for h in history:
        print(f"Epoch {h['epoch']}/{epochs}  Train Loss: {h['train_loss']:.4f}, Train Acc: {h['train_acc']:.2f}%  "
              f"Val Loss: {h['val_loss']:.4f}, Val Acc: {h['val_acc']:.2f}%")
    print(f"Best validation accuracy: {trainer.best_val_acc:.2f}%")
    return history


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m mmf_amd.cifake_training",
                                 description="Train the EfficientNet deepfake classifier on cached pooled rows")
    ap.add_argument("--root", required=True, help="CIFAKE root (test/REAL, train/FAKE, test/FAKE)")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--samples-per-label", type=int, default=2500)
    ap.add_argument("--no-flip", action="store_true", help="train on the unmirrored view alone")
    ap.add_argument("--jitter-views", type=int, default=0, metavar="K",
                    help="ColorJitter(0.2, 0.2, 0.2, 0.1): K cached draws per image, epoch e trains on draw e %% K "
                         "(0: none; the number of epochs: a fresh draw per image and epoch, as the script)")
    ap.add_argument("--blur-views", type=int, default=0, metavar="K",
                    help="RandomApply([GaussianBlur((5, 9), sigma)], p): K cached views per image (0: none; the same "
                         "K as --jitter-views / --jpeg-views where those are set: after the jitter, before the JPEG)")
    ap.add_argument("--blur-p", type=float, default=0.3, metavar="P", help="the probability that a view is blurred")
    ap.add_argument("--blur-sigma", type=float, nargs=2, default=(0.1, 5.0), metavar=("LO", "HI"),
                    help="the range the blur's sigma is drawn from")
    ap.add_argument("--jpeg-views", type=int, default=0, metavar="K",
                    help="RandomJPEGCompression: K cached views per image saved as JPEGs and loaded back (0: none; "
                         "with --jitter-views the same K: jittered first, compressed after)")
    ap.add_argument("--jpeg-quality", type=int, nargs=2, default=(40, 80), metavar=("LO", "HI"),
                    help="the closed range the JPEG quality is drawn from")
    ap.add_argument("--unfreeze", choices=("classifier", "head"), default="classifier",
                    help="classifier: the linear probe on pooled rows; head: features.8 (1x1 conv + BatchNorm affine) "
                         "as well, on cached trunk rows kept on the device (62,720 bytes per view and image)")
    ap.add_argument("--checkpoint", default=DEFAULT_FILE)
    a = ap.parse_args(argv)
    train_cifake(a.root, batch_size=a.batch_size, lr=a.lr, epochs=a.epochs, sample_per_label=a.samples_per_label,
                 checkpoint_path=a.checkpoint, flip=not a.no_flip, jitter_views=a.jitter_views, jpeg_views=a.jpeg_views,
                 jpeg_quality=tuple(a.jpeg_quality), blur_views=a.blur_views, blur_p=a.blur_p,
                 blur_sigma=tuple(a.blur_sigma), unfreeze=a.unfreeze)


if __name__ == "__main__":
    main()
