"""Per-device engine: owns one libmmf_hip handle (weights, workspaces, Truth-Vault) and exposes
the five signals as batched tensor calls on torch device tensors (torch = device memory and
streams only; all arithmetic runs in the HIP kernels of libmmf_hip.so)."""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import hip, io_utils, precision
from .hip import check, ptr, stream_ptr

SCORE_KEYS = ("ai_score", "misinfo_score", "deepfake_score", "clip_similarity", "vault_discrepancy")
# the reference's error for a post with no modality (misinfo_forensics.py:793-794)
NO_INPUT_ERROR = "Provide at least one of: text, image_path, or video_path"


def _as_np(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu()
        return v.numpy() if v.dtype == torch.int64 else v.float().numpy()
    return np.asarray(v)


class Engine:
    """MI355X replica of the MisinfoForensics models on one device."""

    EFFNET_PRECISIONS = precision.EffnetGuard.CHOICES
    TEXT_PRECISIONS = precision.TextGuard.CHOICES

    def __init__(self, device: int = 0, detector_state=None, clip_state=None, eos_token_id: int = 49407,
                 max_batch: int = 256, max_text_len: int = 128, max_clip_len: int = 77,
                 effnet_precision: str = "auto", text_precision: str = "auto"):
        if effnet_precision not in self.EFFNET_PRECISIONS:
            raise ValueError(f"effnet_precision must be one of {self.EFFNET_PRECISIONS}, got {effnet_precision!r}")
        if text_precision not in self.TEXT_PRECISIONS:
            raise ValueError(f"text_precision must be one of {tuple(self.TEXT_PRECISIONS)}, got {text_precision!r}")
        self.lib = hip.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = ctypes.c_void_p()
        check(self.lib.mmf_create(device, ctypes.byref(h)), "mmf_create")
        self.h = h
        self.eos_token_id = eos_token_id
        # the precision policy (precision.py): an explicit choice, an MMF_TEXT_HILO / MMF_EFFNET_FP32
        # environment value under "auto", or a set_option of text_hilo / effnet_fp32 made after the engine's
        # own last write (the ledger records those) pins the tower against calibration and trap alike
        self.ledger = precision.OptionLedger(self)
        self.text_guard = precision.TextGuard(self, self.ledger, text_precision)
        self.effnet_guard = precision.EffnetGuard(self, self.ledger, effnet_precision)
        self.clip_guard = precision.ClipStreamGuard(self)
        self.vault_n = 0
        self._workspaces = {}
        if detector_state is not None:
            self.load_state(detector_state, "")
        if clip_state is not None:
            self.load_state(clip_state, "clip.")
        self.finalize()
        self.reserve(max_batch, max_text_len, max_clip_len)
        if clip_state is not None:
            self.check_clip_streams()
        self.calibrate(("text", "effnet") if detector_state is not None else ())

    # ------------------------------------------------------------------ weights
    def load_state(self, state: Dict, prefix: str = "") -> None:
        for name, v in state.items():
            a = _as_np(v)
            if a.dtype == np.int64:
                dt = 1
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                dt = 0
            shape = (ctypes.c_int64 * max(1, a.ndim))(*a.shape)
            check(self.lib.mmf_load_tensor(self.h, (prefix + name).encode(), dt, a.ndim, shape,
                                           a.ctypes.data_as(ctypes.c_void_p)), f"load {prefix + name}")

    def finalize(self) -> None:
        check(self.lib.mmf_finalize(self.h, int(self.eos_token_id)), "mmf_finalize")

    @property
    def ready(self) -> int:
        return self.lib.mmf_ready(self.h)

    # ------------------------------------------------------------------ precision guards
    # (delegations: precision.py holds the calibrations, the traps and what counts as a user pin)
    CLIP_STREAM_TOL = precision.ClipStreamGuard.TOL
    EFFNET_TOL = precision.EffnetGuard.TOL
    TEXT_TOL = precision.TextGuard.TOL
    text_precision = property(lambda self: self.text_guard.choice)
    effnet_precision = property(lambda self: self.effnet_guard.choice)
    text_check = property(lambda self: self.text_guard.check)
    effnet_check = property(lambda self: self.effnet_guard.check)
    clip_stream_check = property(lambda self: self.clip_guard.check)

    def calibrate(self, components=("effnet",)) -> None:
        """Load-time precision selection for re-packed components (called at construction and by
        the detector's sync after every re-pack: trained weights reach the engine through
        misinfo_forensics.py:175-186 / 285-303 after construction)."""
        if "text" in components and self.ready & 1:
            self.check_text_precision()
        if "effnet" in components and self.ready & 2:
            self.check_effnet_precision()

    def check_clip_streams(self, n: int = 8) -> dict:
        return self.clip_guard.calibrate(n)

    def check_text_precision(self, n: int = 64) -> dict:
        return self.text_guard.calibrate(n)

    def check_effnet_precision(self, n: int = 64) -> dict:
        return self.effnet_guard.calibrate(n)

    def clip_stream_overflow(self, *outputs) -> bool:
        return self.clip_guard.overflow(*outputs)

    def text_overflow(self, scores) -> bool:
        return self.text_guard.overflow(scores)

    def effnet_overflow(self, scores) -> bool:
        return self.effnet_guard.overflow(scores)

    def scores_overflow(self, scores5) -> bool:
        return precision.scores_overflow(self.text_guard, self.effnet_guard, self.clip_guard, scores5)

    # ------------------------------------------------------------------ options / accounting
    def set_option(self, name: str, value: int) -> None:
        """A/B switches of the library (include/mmf_hip.h: mmf_set_option)."""
        check(self.lib.mmf_set_option(self.h, name.encode(), int(value)), f"mmf_set_option({name})")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int()
        check(self.lib.mmf_get_option(self.h, name.encode(), ctypes.byref(v)), f"mmf_get_option({name})")
        return v.value

    @property
    def device_bytes(self) -> int:
        """Device memory owned by this handle (weights, workspaces, vault)."""
        return int(self.lib.mmf_device_bytes(self.h))

    def reserve(self, max_batch: int, max_text_len: int = 128, max_clip_len: int = 77) -> None:
        check(self.lib.mmf_reserve(self.h, max_batch, max_text_len, max_clip_len), "mmf_reserve")
        self.max_batch, self.max_text_len, self.max_clip_len = max_batch, max_text_len, max_clip_len

    # ------------------------------------------------------------------ vault
    def set_vault(self, embeddings: np.ndarray, title_ids=None, title_mask=None) -> None:
        """Rows normalised once, exactly as the reference does on every search call (numpy, in the
        vault's own dtype: io_utils.vault_unit_rows), then uploaded as float32."""
        v = np.ascontiguousarray(io_utils.vault_unit_rows(_as_np(embeddings)), dtype=np.float32)
        check(self.lib.mmf_set_vault_normalized(self.h, v.ctypes.data_as(ctypes.c_void_p), v.shape[0], v.shape[1]),
              "mmf_set_vault_normalized")
        self.vault_n = v.shape[0]
        if title_ids is not None:
            ids = self._i32(title_ids)
            mask = self._i32(title_mask)
            check(self.lib.mmf_set_vault_titles(self.h, ptr(ids), ptr(mask), ids.shape[0], ids.shape[1],
                                                stream_ptr()), "mmf_set_vault_titles")

    # ------------------------------------------------------------------ host-input geometry
    def resize_supported(self, width: int, height: int) -> bool:
        """Whether mmf_resize_pil's tap budget covers a width x height image (both geometries)."""
        return bool(self.lib.mmf_resize_supported(int(width), int(height)))

    def resize_images(self, images, effnet: bool = True, clip: bool = True):
        """Decoded uint8 images (HxWx3 RGB or HxWx4 RGBX numpy arrays -- all of one kind --, any
        sizes) -> device uint8 [B,224,224,3] EfficientNet squash-resize and CLIP shortest-edge +
        centre-crop windows, bit-exact with Pillow (mmf_resize_pil).  The images cross PCIe once,
        packed (threaded copies) into a pinned staging buffer."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        if not arrs:  # nothing to resample: empty outputs, no device call
            empty = [torch.empty((0, 224, 224, 3), dtype=torch.uint8, device=self.device) if k else None
                     for k in (effnet, clip)]
            return empty[0], empty[1]
        ps = arrs[0].shape[2]
        for a in arrs:
            if not (a.ndim == 3 and a.shape[2] == ps and ps in (3, 4)):
                raise ValueError(f"expected HxWx{ps} uint8, got {a.shape}")
        sizes = [a.nbytes for a in arrs]
        offs = np.zeros(len(arrs), np.int64)
        if arrs:
            offs[1:] = np.cumsum(sizes)[:-1]
        total = int(sum(sizes)) or 1
        if getattr(self, "_rs_host", None) is None or self._rs_host.numel() < total:
            self._rs_host = torch.empty(total, dtype=torch.uint8).pin_memory()
        host = self._rs_host.numpy()

        def pack(i):
            np.copyto(host[offs[i]:offs[i] + sizes[i]], arrs[i].reshape(-1))
        if total > (8 << 20) and len(arrs) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(16, len(arrs))) as ex:
                list(ex.map(pack, range(len(arrs))))
        else:
            for i in range(len(arrs)):
                pack(i)
        src = self._rs_host[:total].to(self.device, non_blocking=True)
        wh = np.array([[a.shape[1], a.shape[0]] for a in arrs], np.int32).reshape(-1)
        B = len(arrs)
        eff = torch.empty((B, 224, 224, 3), dtype=torch.uint8, device=self.device) if effnet else None
        clp = torch.empty((B, 224, 224, 3), dtype=torch.uint8, device=self.device) if clip else None
        check(self.lib.mmf_resize_pil(self.h, ptr(src), offs.ctypes.data_as(ctypes.c_void_p),
                                      wh.ctypes.data_as(ctypes.c_void_p), B, ps, ptr(eff), ptr(clp), stream_ptr()),
              "mmf_resize_pil")
        return eff, clp

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _tensor(x) -> torch.Tensor:
        # a read-only numpy view (an Arrow / PIL export, np.broadcast_to) is copied rather than
        # wrapped: torch cannot wrap non-writable memory without a UserWarning per process
        if isinstance(x, np.ndarray) and not x.flags.writeable:
            x = x.copy()
        return torch.as_tensor(x)

    def _i32(self, x) -> torch.Tensor:
        return self._tensor(x).to(self.device, torch.int32).contiguous()

    def _u8(self, x) -> torch.Tensor:
        t = self._tensor(x)
        if not (t.dtype == torch.uint8 and t.dim() == 4 and tuple(t.shape[1:]) == (224, 224, 3)):
            raise ValueError(f"images must be uint8 [B,224,224,3], got {tuple(t.shape)} {t.dtype}")
        return t.to(self.device).contiguous()

    def _f32(self, *shape) -> torch.Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ signals
    def text_forward(self, ids, mask):
        ids, mask = self._i32(ids), self._i32(mask)
        B, L = ids.shape
        ai, mi, sc = self._f32(B, 2), self._f32(B, 2), self._f32(B, 2)
        check(self.lib.mmf_text_forward(self.h, ptr(ids), ptr(mask), B, L, ptr(ai), ptr(mi), ptr(sc),
                                        stream_ptr()), "mmf_text_forward")
        return ai, mi, sc

    def text_pooled(self, ids, mask):
        """The rows the ai / misinfo heads read (mmf_text_pooled): last_hidden_state[:, 0, :] float32 [B, 768]
        on the device, by text_forward's launch sequence without the heads.  The run-time trap of the
        synchronous API paths (text_overflow): a non-finite row switches the tower, unless pinned, to the precise
        mode and the batch runs again."""
        ids, mask = self._i32(ids), self._i32(mask)
        B, L = ids.shape
        cls = self._f32(B, 768)

        def run():
            check(self.lib.mmf_text_pooled(self.h, ptr(ids), ptr(mask), B, L, ptr(cls), stream_ptr()),
                  "mmf_text_pooled")
            return cls
        return precision.rerun_if(self.text_overflow, run, lambda c: (c * 0).sum(1).cpu().numpy())  # 0 or NaN per row

    def effnet_forward(self, img):
        img = self._u8(img)
        B = img.shape[0]
        lg, sc = self._f32(B, 2), self._f32(B)
        check(self.lib.mmf_effnet_forward(self.h, ptr(img), B, ptr(lg), ptr(sc), stream_ptr()), "mmf_effnet_forward")
        return lg, sc

    def effnet_forward_f32(self, x):
        """Normalised fp32 NCHW input (detector.forward_image semantics)."""
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        if not (x.dim() == 4 and tuple(x.shape[1:]) == (3, 224, 224)):
            raise ValueError(f"expected [B,3,224,224], got {tuple(x.shape)}")
        B = x.shape[0]
        lg, sc = self._f32(B, 2), self._f32(B)
        check(self.lib.mmf_effnet_forward_f32(self.h, ptr(x), B, ptr(lg), ptr(sc), stream_ptr()),
              "mmf_effnet_forward_f32")
        return lg, sc

    def effnet_pooled(self, img):
        """The row the deepfake classifier reads (mmf_effnet_pooled): the global average of the 7x7 head output,
        float32 [B, 1280] on the device, by effnet_forward's launch sequence for the tower in use without the
        classifier.  The run-time trap of the synchronous API paths (effnet_overflow): a non-finite row switches
        the engine, unless pinned, to the fp32 tower and the batch runs again."""
        img = self._u8(img)
        B = img.shape[0]
        pooled = self._f32(B, 1280)

        def run():
            check(self.lib.mmf_effnet_pooled(self.h, ptr(img), B, ptr(pooled), stream_ptr()), "mmf_effnet_pooled")
            return pooled
        return precision.rerun_if(self.effnet_overflow, run, lambda p: (p * 0).sum(1).cpu().numpy())  # 0 or NaN per row

    def effnet_trunk(self, img):
        """What the head conv stage reads (mmf_effnet_trunk): the last MBConv block's output, float32 [B, 49, 320] on
        the device (positions row-major over 7 x 7, channels innermost), by effnet_forward's launch sequence for the
        tower in use without the head GEMM, the pool and the classifier.  The same run-time trap as effnet_pooled."""
        img = self._u8(img)
        B = img.shape[0]
        trunk = self._f32(B, 49, 320)

        def run():
            check(self.lib.mmf_effnet_trunk(self.h, ptr(img), B, ptr(trunk), stream_ptr()), "mmf_effnet_trunk")
            return trunk
        return precision.rerun_if(self.effnet_overflow, run, lambda t: (t * 0).sum((1, 2)).cpu().numpy())

    def hflip(self, img):
        """A staged uint8 [B, H, W, C] window mirrored left-right (mmf_hflip_u8) into a new device tensor."""
        t = self._tensor(img)
        if not (t.dtype == torch.uint8 and t.dim() == 4 and t.numel() > 0):
            raise ValueError(f"hflip: expected a non-empty uint8 [B, H, W, C] tensor, got {tuple(t.shape)} {t.dtype}")
        t = t.to(self.device).contiguous()
        out = torch.empty_like(t)
        B, H, Wd, C = t.shape
        check(self.lib.mmf_hflip_u8(ptr(t), ptr(out), B, H, Wd, C, stream_ptr()), "mmf_hflip_u8")
        return out

    def color_jitter(self, img, ops, factors, hue_shift):
        """torchvision's ColorJitter on staged uint8 [B, H, W, 3] windows (mmf_color_jitter_u8), byte-exact with its
        PIL backend, into a new device tensor.  Per image: ``ops`` int32 [B, 4] the operations in the order applied
        (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 skip), ``factors`` float32 [B, 3] (brightness, contrast,
        saturation), ``hue_shift`` int32 [B] what is added to H (0..255)."""
        t = self._tensor(img)
        if not (t.dtype == torch.uint8 and t.dim() == 4 and t.numel() > 0 and t.shape[3] == 3):
            raise ValueError(f"color_jitter: expected a non-empty uint8 [B, H, W, 3] tensor, got {tuple(t.shape)} "
                             f"{t.dtype}")
        t = t.to(self.device).contiguous()
        B, H, Wd, _ = t.shape
        ops = torch.as_tensor(ops, dtype=torch.int32).to(self.device).contiguous()
        factors = torch.as_tensor(factors, dtype=torch.float32).to(self.device).contiguous()
        hue_shift = torch.as_tensor(hue_shift, dtype=torch.int32).to(self.device).contiguous()
        if tuple(ops.shape) != (B, 4) or tuple(factors.shape) != (B, 3) or tuple(hue_shift.shape) != (B,):
            raise ValueError(f"color_jitter: expected ops [{B}, 4], factors [{B}, 3], hue_shift [{B}], got "
                             f"{tuple(ops.shape)}, {tuple(factors.shape)}, {tuple(hue_shift.shape)}")
        out = torch.empty_like(t)
        ws = torch.empty((B, hip.JITTER_CHUNKS), dtype=torch.int64, device=self.device)
        check(self.lib.mmf_color_jitter_u8(ptr(t), ptr(out), B, H, Wd, ptr(ops), ptr(factors), ptr(hue_shift), ptr(ws),
                                           stream_ptr()), "mmf_color_jitter_u8")
        return out

    def gaussian_blur(self, img, sigma, apply=None, kernel_size=(5, 9)):
        """torchvision's GaussianBlur on staged uint8 [B, H, W, 3] windows (mmf_gaussian_blur_u8), into a new device
        tensor: float32 sums with reflected borders, rounded half to even, as its tensor backend computes them for
        a PIL image -- in one fixed order of additions, so a byte can differ by one from torch's conv2d where the
        exact sum is within float32 rounding of a half.  ``sigma``: a float, or an array of length B (both axes
        share it); ``apply``: a bool array of length B, all True by default -- image b is copied unchanged where it
        is False (a RandomApply that did not fire); ``kernel_size`` = (kx, ky), width first, odd, 1..15.  The
        weights are torch's own, formed on the host (``cifake_training.gaussian_kernel2d``)."""
        from .cifake_training import _kernel_size, gaussian_kernel2d
        t = self._tensor(img)
        if not (t.dtype == torch.uint8 and t.dim() == 4 and t.numel() > 0 and t.shape[3] == 3):
            raise ValueError(f"gaussian_blur: expected a non-empty uint8 [B, H, W, 3] tensor, got {tuple(t.shape)} "
                             f"{t.dtype}")
        t = t.to(self.device).contiguous()
        B, H, Wd, _ = t.shape
        kx, ky = _kernel_size(kernel_size, "gaussian_blur")
        if Wd <= kx // 2 or H <= ky // 2:
            raise ValueError(f"gaussian_blur: a {kx} x {ky} window reflects only in images wider than {kx // 2} and "
                             f"higher than {ky // 2}, got {Wd} x {H}")
        s = np.asarray(sigma, dtype=np.float64)
        if s.ndim > 1 or (s.ndim == 1 and s.shape != (B,)):
            raise ValueError(f"gaussian_blur: sigma must be a float or an array of length {B}, got shape {s.shape}")
        s = np.broadcast_to(s, (B,))
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("gaussian_blur: every sigma must be positive and finite")
        on = np.ones(B, bool) if apply is None else np.asarray(apply)
        if on.shape != (B,) or on.dtype != np.bool_:
            raise ValueError(f"gaussian_blur: apply must be a bool array of length {B}, got {on.shape} {on.dtype}")
        weights = np.zeros((B, ky, kx), np.float32)  # images that are copied read none
        weights[on] = gaussian_kernel2d(s[on], (kx, ky))
        wd = torch.from_numpy(weights).to(self.device)
        ad = torch.from_numpy(on.astype(np.int32)).to(self.device)
        out = torch.empty_like(t)
        check(self.lib.mmf_gaussian_blur_u8(ptr(t), ptr(out), B, H, Wd, kx, ky, ptr(wd), ptr(ad), stream_ptr()),
              "mmf_gaussian_blur_u8")
        return out

    def jpeg_compress(self, img, quality):
        """The reference's RandomJPEGCompression at given qualities (misinformation_dataset.py:18-57) on staged uint8
        [B, H, W, 3] windows (mmf_jpeg_roundtrip_u8), into a new device tensor: byte-equal to
        ``Image.save(buf, format="JPEG", quality=q, optimize=False)``, reopen, ``convert("RGB")``.  ``quality``: an
        int, or an int array of length B; 1..100, or 0 for an unchanged copy.  An image the kernel flags as outside
        the decoder's exact range (none made from pixels has been seen to be) makes that round trip through Pillow
        on the host."""
        t = self._tensor(img)
        if not (t.dtype == torch.uint8 and t.dim() == 4 and t.numel() > 0 and t.shape[3] == 3):
            raise ValueError(f"jpeg_compress: expected a non-empty uint8 [B, H, W, 3] tensor, got {tuple(t.shape)} "
                             f"{t.dtype}")
        t = t.to(self.device).contiguous()
        B, H, Wd, _ = t.shape
        q = np.asarray(quality)
        if q.dtype.kind not in "iu" or q.ndim > 1:
            raise ValueError(f"jpeg_compress: quality must be an int or an int array of length {B}")
        q = np.broadcast_to(q, (B,)).astype(np.int32) if q.ndim == 0 else q.astype(np.int32)
        if q.shape != (B,) or q.min() < 0 or q.max() > 100:
            raise ValueError(f"jpeg_compress: quality must be {B} values in 0..100, got shape {q.shape}, "
                             f"range {q.min() if q.size else None}..{q.max() if q.size else None}")
        per_image = int(self.lib.mmf_jpeg_roundtrip_ws_bytes(H, Wd))
        if per_image <= 0:
            raise ValueError(f"jpeg_compress: unsupported image size {H} x {Wd}")
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(self.device)
        out = torch.empty_like(t)
        ws = torch.empty((B * per_image + 7) // 8, dtype=torch.int64, device=self.device)
        flags = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.mmf_jpeg_roundtrip_u8(ptr(t), ptr(out), B, H, Wd, ptr(qd), ptr(ws), ptr(flags), stream_ptr()),
              "mmf_jpeg_roundtrip_u8")
        flagged = np.flatnonzero(self._jpeg_flags(flags))
        if flagged.size:
            self._jpeg_host_redo(t, out, q, flagged)
        return out

    @staticmethod
    def _jpeg_flags(flags) -> np.ndarray:
        """mmf_jpeg_roundtrip_u8's flags on the host (the call's one synchronisation)."""
        return flags.cpu().numpy()

    @staticmethod
    def _jpeg_host_roundtrip(rgb: np.ndarray, quality: int) -> np.ndarray:
        """uint8 [H, W, 3] saved as a JPEG and loaded back by Pillow, as the reference does it."""
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, format="JPEG", quality=int(quality), optimize=False)
        buf.seek(0)
        im = Image.open(buf)
        im.load()
        return np.asarray(im.convert("RGB"))

    def _jpeg_host_redo(self, src, out, quality, flagged) -> None:
        """The images the kernel declined: their round trip on the host, written over out[i]."""
        for i in (int(v) for v in flagged):
            done = self._jpeg_host_roundtrip(src[i].cpu().numpy(), int(quality[i]))
            out[i].copy_(torch.from_numpy(np.array(done)))  # a copy: Pillow's buffer is read-only

    def clip_image(self, img):
        img = self._u8(img)
        e = self._f32(img.shape[0], 512)
        check(self.lib.mmf_clip_image(self.h, ptr(img), img.shape[0], ptr(e), stream_ptr()), "mmf_clip_image")
        return e

    def clip_text(self, ids, mask):
        ids, mask = self._i32(ids), self._i32(mask)
        e = self._f32(ids.shape[0], 512)
        check(self.lib.mmf_clip_text(self.h, ptr(ids), ptr(mask), ids.shape[0], ids.shape[1], ptr(e),
                                     stream_ptr()), "mmf_clip_text")
        return e

    def clip_consistency(self, img, ids, mask, out: Optional[dict] = None) -> dict:
        """analyze_consistency over a batch: {img_emb, txt_emb [B,512] unit, sim [B]} (one call,
        the CLIP text tower on a concurrent stream)."""
        img = self._u8(img)
        ids, mask = self._i32(ids), self._i32(mask)
        B = img.shape[0]
        if out is None:
            out = {"img_emb": self._f32(B, 512), "txt_emb": self._f32(B, 512), "sim": self._f32(B)}
        check(self.lib.mmf_clip_consistency(self.h, ptr(img), ptr(ids), ptr(mask), B, ids.shape[1],
                                            ptr(out["img_emb"]), ptr(out["txt_emb"]), ptr(out["sim"]), stream_ptr()),
              "mmf_clip_consistency")
        return out

    def clip_pooled(self, img, ids, mask):
        """The rows CLIPDetective's projection heads read (mmf_clip_pooled): (post_layernorm(CLS) float32
        [B, 768], final_layer_norm(EOS) float32 [B, 512]) on the device; ``img`` None or ``ids`` None skips
        that tower (its result is None).  The fp16-stream overflow trap of the synchronous API paths: a
        non-finite row switches the towers to fp32 streams and the batch runs again."""
        img = self._u8(img) if img is not None else None
        ids, mask = (self._i32(ids), self._i32(mask)) if ids is not None else (None, None)
        if img is None and ids is None:
            raise ValueError("clip_pooled: no input")
        B = img.shape[0] if img is not None else ids.shape[0]
        ip = self._f32(B, 768) if img is not None else None
        tp = self._f32(B, 512) if ids is not None else None

        def run():
            check(self.lib.mmf_clip_pooled(self.h, ptr(img), ptr(ids), ptr(mask), B, ids.shape[1] if ids is not None
                                           else 1, ptr(ip), ptr(tp), stream_ptr()), "mmf_clip_pooled")
            return ip, tp
        return precision.rerun_if(lambda rows: self.clip_stream_overflow(*rows), run)

    def set_clip_projections(self, visual=None, text=None) -> None:
        """Trained projection heads into the towers (mmf_set_clip_projections): float32 [512, 768] /
        [512, 512], rounded to fp16 on the device into the buffers clip_image / clip_text read; nothing is
        allocated."""
        def prep(w, cols):
            if w is None:
                return None
            t = torch.as_tensor(w, dtype=torch.float32).to(self.device).contiguous()
            if tuple(t.shape) != (512, cols):
                raise ValueError(f"projection must be [512, {cols}], got {tuple(t.shape)}")
            return t
        v, t = prep(visual, 768), prep(text, 512)
        check(self.lib.mmf_set_clip_projections(self.h, ptr(v), ptr(t), stream_ptr()), "mmf_set_clip_projections")
        torch.cuda.current_stream().synchronize()  # v / t may be temporaries

    CLIP_TRAIN_PARAMS = 655361  # MMF_CLIP_TRAIN_PARAMS: visual [512][768] | text [512][512] | logit_scale

    def _workspace(self, name: str, need: int) -> torch.Tensor:
        """The device byte buffer kept under ``name``, grown to at least ``need`` bytes."""
        ws = self._workspaces.get(name)
        if ws is None or ws.numel() < need:
            ws = self._workspaces[name] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=self.device)
        return ws

    @staticmethod
    def _nsteps(N: int, batch: int) -> int:
        return max(1, -(-N // max(1, int(batch))))

    def _check_tensors(self, what: str, tensors) -> None:
        """tensors: (name, tensor, dtype, elements, optional) of a trainer or eval call's device arguments."""
        for name, t, dt, n, optional in tensors:
            if t is None and optional:
                continue
            if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dt and t.is_contiguous()
                    and t.numel() == n):
                raise ValueError(f"{what}: {name} must be a contiguous {dt} tensor of {n} elements on {self.device}")

    def clip_train_epoch(self, img_feat, txt_feat, perm, batch: int, lr: float, betas, eps: float,
                         weight_decay: float, max_norm: float, step0: int, params, exp_avg, exp_avg_sq,
                         grad_out=None):
        """One epoch of projection-head training on cached pooled features (mmf_clip_train_epoch): device
        tensors img_feat float32 [N, 768], txt_feat float32 [N, 512], perm int32 [N]; params / exp_avg /
        exp_avg_sq float32 [655361], updated in place.  Returns (step_loss, step_gnorm) float32 [nsteps] on
        the device; nothing is synchronised."""
        N, P = int(perm.shape[0]), self.CLIP_TRAIN_PARAMS
        self._check_tensors("clip_train_epoch", (
            ("img_feat", img_feat, torch.float32, 768 * N, False), ("txt_feat", txt_feat, torch.float32, 512 * N, False),
            ("perm", perm, torch.int32, N, False), ("params", params, torch.float32, P, False),
            ("exp_avg", exp_avg, torch.float32, P, False), ("exp_avg_sq", exp_avg_sq, torch.float32, P, False),
            ("grad_out", grad_out, torch.float32, P, True)))
        nsteps = self._nsteps(N, batch)
        step_loss, step_gnorm = self._f32(nsteps), self._f32(nsteps)
        ws = self._workspace("clip_train", self.lib.mmf_clip_train_ws_bytes(int(batch)))
        check(self.lib.mmf_clip_train_epoch(ptr(img_feat), ptr(txt_feat), N, ptr(perm), int(batch), float(lr),
                                            float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                            float(max_norm), int(step0), ptr(params), ptr(exp_avg), ptr(exp_avg_sq),
                                            ptr(step_loss), ptr(step_gnorm), ptr(grad_out), ptr(ws), ws.numel(),
                                            stream_ptr()), "mmf_clip_train_epoch")
        return step_loss, step_gnorm

    def clip_contrastive_eval(self, img_feat, txt_feat, batch: int, params):
        """validate's forward on cached features (mmf_clip_contrastive_eval): consecutive batches in row
        order -> (batch_loss float32 [nbatches], row_cos float32 [N]) on the device."""
        N = int(img_feat.shape[0])
        self._check_tensors("clip_contrastive_eval", (
            ("img_feat", img_feat, torch.float32, 768 * N, False), ("txt_feat", txt_feat, torch.float32, 512 * N, False),
            ("params", params, torch.float32, self.CLIP_TRAIN_PARAMS, False)))
        nb = self._nsteps(N, batch)
        batch_loss, row_cos = self._f32(nb), self._f32(N)
        ws = self._workspace("clip_train", self.lib.mmf_clip_train_ws_bytes(int(batch)))
        check(self.lib.mmf_clip_contrastive_eval(ptr(img_feat), ptr(txt_feat), N, int(batch), ptr(params),
                                                 ptr(batch_loss), ptr(row_cos), ptr(ws), ws.numel(), stream_ptr()),
              "mmf_clip_contrastive_eval")
        return batch_loss, row_cos

    CLIP_TRIALS_MAX, CLIP_TRIAL_STRIDE = 16, 655364  # MMF_CLIP_TRIALS_MAX, MMF_CLIP_TRIAL_STRIDE

    def _trial_args(self, what: str, T: int, N: int, batch, active):
        """The host arrays of a trials call: (batch int32 [T], active int32 [T], the largest active step count)."""
        if not 1 <= T <= self.CLIP_TRIALS_MAX:
            raise ValueError(f"{what}: {T} trials, 1..{self.CLIP_TRIALS_MAX} fit one call")
        b = np.ascontiguousarray(np.asarray(batch, dtype=np.int32).reshape(-1))
        a = np.ones(T, np.int32) if active is None else np.ascontiguousarray(
            (np.asarray(active).reshape(-1) != 0).astype(np.int32))
        if b.shape != (T,) or a.shape != (T,):
            raise ValueError(f"{what}: batch and active must have {T} entries")
        most = max([self._nsteps(N, int(b[t])) for t in range(T) if a[t]], default=1)
        return b, a, most

    def clip_train_epoch_trials(self, img_feat, txt_feat, perm, batch, lr, betas, eps: float, weight_decay, max_norm,
                                step0, params, exp_avg, exp_avg_sq, active=None):
        """One epoch of T projection-head trainings side by side (mmf_clip_train_epoch_trials): img_feat /
        txt_feat as clip_train_epoch's, shared; perm int32 [T, N]; params / exp_avg / exp_avg_sq float32
        [T, 655364] (a trial's 655361 values first), updated in place; batch, lr, weight_decay, max_norm, step0,
        active: T host values each (active None: all).  Returns (step_loss, step_gnorm) float32 [T, S] on the
        device, S the largest active step count; a trial's row is NaN past its own steps, and all NaN when it is
        not active.  Nothing is synchronised."""
        T, N, S = int(params.shape[0]), int(img_feat.shape[0]), self.CLIP_TRIAL_STRIDE
        self._check_tensors("clip_train_epoch_trials", (
            ("img_feat", img_feat, torch.float32, 768 * N, False), ("txt_feat", txt_feat, torch.float32, 512 * N, False),
            ("perm", perm, torch.int32, T * N, False), ("params", params, torch.float32, T * S, False),
            ("exp_avg", exp_avg, torch.float32, T * S, False), ("exp_avg_sq", exp_avg_sq, torch.float32, T * S, False)))
        b, a, most = self._trial_args("clip_train_epoch_trials", T, N, batch, active)
        f64 = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (lr, weight_decay, max_norm)]
        s0 = np.ascontiguousarray(np.asarray(step0, dtype=np.int32).reshape(-1))
        if any(x.shape != (T,) for x in f64 + [s0]):
            raise ValueError(f"clip_train_epoch_trials: lr, weight_decay, max_norm and step0 must have {T} entries")
        step_loss = torch.full((T, most), float("nan"), dtype=torch.float32, device=self.device)
        step_gnorm = torch.full_like(step_loss, float("nan"))
        ws = self._workspace("clip_train", self.lib.mmf_clip_train_trials_ws_bytes(T, 64))
        check(self.lib.mmf_clip_train_epoch_trials(
            ptr(img_feat), ptr(txt_feat), N, T, ptr(perm), b.ctypes.data, f64[0].ctypes.data, f64[1].ctypes.data,
            f64[2].ctypes.data, s0.ctypes.data, a.ctypes.data, float(betas[0]), float(betas[1]), float(eps),
            ptr(params), ptr(exp_avg), ptr(exp_avg_sq), ptr(step_loss), ptr(step_gnorm), most, ptr(ws), ws.numel(),
            stream_ptr()), "mmf_clip_train_epoch_trials")
        return step_loss, step_gnorm

    def clip_contrastive_eval_trials(self, img_feat, txt_feat, batch, params, active=None):
        """validate's forward for T trials side by side (mmf_clip_contrastive_eval_trials): params float32
        [T, 655364]; batch, active: T host values each -> (batch_loss float32 [T, S], row_cos float32 [T, N]) on
        the device, S the largest active batch count; NaN where a trial wrote nothing."""
        T, N = int(params.shape[0]), int(img_feat.shape[0])
        self._check_tensors("clip_contrastive_eval_trials", (
            ("img_feat", img_feat, torch.float32, 768 * N, False), ("txt_feat", txt_feat, torch.float32, 512 * N, False),
            ("params", params, torch.float32, T * self.CLIP_TRIAL_STRIDE, False)))
        b, a, most = self._trial_args("clip_contrastive_eval_trials", T, N, batch, active)
        batch_loss = torch.full((T, most), float("nan"), dtype=torch.float32, device=self.device)
        row_cos = torch.full((T, N), float("nan"), dtype=torch.float32, device=self.device)
        ws = self._workspace("clip_train", self.lib.mmf_clip_train_trials_ws_bytes(T, 64))
        check(self.lib.mmf_clip_contrastive_eval_trials(
            ptr(img_feat), ptr(txt_feat), N, T, b.ctypes.data, a.ctypes.data, ptr(params), ptr(batch_loss),
            ptr(row_cos), most, ptr(ws), ws.numel(), stream_ptr()), "mmf_clip_contrastive_eval_trials")
        return batch_loss, row_cos

    HEAD_PARAMS = 197378  # MMF_HEAD_PARAMS: 0.weight [256][768] | 0.bias [256] | 3.weight [2][256] | 3.bias [2]

    def head_train_epoch(self, feat, labels, perm, keep, p_drop: float, batch: int, lr_steps, betas, eps: float,
                         weight_decay: float, max_norm: float, step0: int, params, exp_avg, exp_avg_sq,
                         grad_out=None):
        """One epoch of text-head training on cached CLS rows (mmf_head_train_epoch): device tensors feat
        float32 [N, 768], labels int32 [N], perm int32 [N], keep int64 [N, 4] (the uint64 masks' bits) or
        None; lr_steps: the nsteps learning rates (host); params / exp_avg / exp_avg_sq float32 [197378],
        updated in place.  Returns (step_loss float32, step_correct int32, step_gnorm float32) [nsteps] on the
        device; nothing is synchronised."""
        N, P = int(perm.shape[0]), self.HEAD_PARAMS
        self._check_tensors("head_train_epoch", (
            ("feat", feat, torch.float32, 768 * N, False), ("labels", labels, torch.int32, N, False),
            ("perm", perm, torch.int32, N, False), ("keep", keep, torch.int64, 4 * N, True),
            ("params", params, torch.float32, P, False), ("exp_avg", exp_avg, torch.float32, P, False),
            ("exp_avg_sq", exp_avg_sq, torch.float32, P, False), ("grad_out", grad_out, torch.float32, P, True)))
        nsteps = self._nsteps(N, batch)
        lrs = np.ascontiguousarray(np.asarray(lr_steps, dtype=np.float64).reshape(-1))
        if lrs.shape[0] != nsteps:
            raise ValueError(f"head_train_epoch: {lrs.shape[0]} learning rates for {nsteps} steps")
        step_loss, step_gnorm = self._f32(nsteps), self._f32(nsteps)
        step_correct = torch.empty(nsteps, dtype=torch.int32, device=self.device)
        ws = self._workspace("head_train", self.lib.mmf_head_train_ws_bytes(int(batch)))
        check(self.lib.mmf_head_train_epoch(ptr(feat), ptr(labels), N, ptr(perm), ptr(keep), float(p_drop), int(batch),
                                            lrs.ctypes.data_as(ctypes.c_void_p), float(betas[0]), float(betas[1]),
                                            float(eps), float(weight_decay), float(max_norm), int(step0), ptr(params),
                                            ptr(exp_avg), ptr(exp_avg_sq), ptr(step_loss), ptr(step_correct),
                                            ptr(step_gnorm), ptr(grad_out), ptr(ws), ws.numel(), stream_ptr()),
              "mmf_head_train_epoch")
        return step_loss, step_correct, step_gnorm

    def head_eval(self, feat, labels, batch: int, params):
        """validate's forward on cached CLS rows (mmf_head_eval): consecutive batches in row order ->
        (batch_loss float32 [nbatches], row_logits float32 [N, 2]) on the device."""
        N = int(labels.shape[0])
        self._check_tensors("head_eval", (
            ("feat", feat, torch.float32, 768 * N, False), ("labels", labels, torch.int32, N, False),
            ("params", params, torch.float32, self.HEAD_PARAMS, False)))
        nb = self._nsteps(N, batch)
        batch_loss, row_logits = self._f32(nb), self._f32(N, 2)
        ws = self._workspace("head_train", self.lib.mmf_head_train_ws_bytes(int(batch)))
        check(self.lib.mmf_head_eval(ptr(feat), ptr(labels), N, int(batch), ptr(params), ptr(batch_loss),
                                     ptr(row_logits), ptr(ws), ws.numel(), stream_ptr()), "mmf_head_eval")
        return batch_loss, row_logits

    EFFCLS_PARAMS = 2562  # MMF_EFFCLS_PARAMS: classifier.1.weight [2][1280] | classifier.1.bias [2]

    def effcls_train_epoch(self, feat, labels, perm, keep, p_drop: float, batch: int, lr: float, betas, eps: float,
                           weight_decay: float, step0: int, params, exp_avg, exp_avg_sq, grad_out=None):
        """One epoch of deepfake-classifier training in one launch (mmf_effcls_train_epoch): device tensors feat
        float32 [R, 1280] and labels int32 [R] (the row bank), perm int32 [N] (bank rows), keep int64 [N, 20] (the
        uint64 masks' bits) or None; params / exp_avg / exp_avg_sq float32 [2562], updated in place.  Returns
        (step_loss float32 [nsteps], step_correct int32 [nsteps]) on the device; nothing is synchronised."""
        R, N, P = int(labels.shape[0]), int(perm.shape[0]), self.EFFCLS_PARAMS
        self._check_tensors("effcls_train_epoch", (
            ("feat", feat, torch.float32, 1280 * R, False), ("labels", labels, torch.int32, R, False),
            ("perm", perm, torch.int32, N, False), ("keep", keep, torch.int64, 20 * N, True),
            ("params", params, torch.float32, P, False), ("exp_avg", exp_avg, torch.float32, P, False),
            ("exp_avg_sq", exp_avg_sq, torch.float32, P, False), ("grad_out", grad_out, torch.float32, P, True)))
        nsteps = self._nsteps(N, batch)
        step_loss = self._f32(nsteps)
        step_correct = torch.empty(nsteps, dtype=torch.int32, device=self.device)
        check(self.lib.mmf_effcls_train_epoch(ptr(feat), ptr(labels), R, ptr(perm), N, ptr(keep), float(p_drop),
                                              int(batch), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                              float(weight_decay), int(step0), ptr(params), ptr(exp_avg),
                                              ptr(exp_avg_sq), ptr(step_loss), ptr(step_correct), ptr(grad_out),
                                              stream_ptr()), "mmf_effcls_train_epoch")
        return step_loss, step_correct

    def effcls_eval(self, feat, labels, batch: int, params):
        """validate's forward on cached pooled rows (mmf_effcls_eval): consecutive batches in row order ->
        (batch_loss float32 [nbatches], row_logits float32 [R, 2]) on the device."""
        R = int(labels.shape[0])
        self._check_tensors("effcls_eval", (
            ("feat", feat, torch.float32, 1280 * R, False), ("labels", labels, torch.int32, R, False),
            ("params", params, torch.float32, self.EFFCLS_PARAMS, False)))
        nb = self._nsteps(R, batch)
        batch_loss, row_logits = self._f32(nb), self._f32(R, 2)
        check(self.lib.mmf_effcls_eval(ptr(feat), ptr(labels), R, int(batch), ptr(params), ptr(batch_loss),
                                       ptr(row_logits), stream_ptr()), "mmf_effcls_eval")
        return batch_loss, row_logits

    EFFHEAD_PARAMS = 414722  # MMF_EFFHEAD_PARAMS: features.8.0.weight | 8.1.weight | 8.1.bias | classifier.1.weight | .bias
    TRUNK_ROW = 49 * 320     # floats of one image's trunk rows

    def effhead_train_epoch(self, trunk, labels, perm, keep, p_drop: float, batch: int, bn_mean, bn_var, bn_eps: float,
                            lr: float, betas, eps: float, weight_decay: float, step0: int, params, exp_avg,
                            exp_avg_sq, grad_out=None):
        """One epoch of head-stage training (mmf_effhead_train_epoch): device tensors trunk float32 [R, 49, 320] and
        labels int32 [R] (the row bank), perm int32 [N] (bank rows), keep int64 [N, 20] (the uint64 masks' bits, on the
        pooled row) or None; bn_mean / bn_var float32 [1280], read only; params / exp_avg / exp_avg_sq float32
        [414722], updated in place.  Returns (step_loss float32 [nsteps], step_correct int32 [nsteps]) on the device;
        nothing is synchronised."""
        R, N, P = int(labels.shape[0]), int(perm.shape[0]), self.EFFHEAD_PARAMS
        self._check_tensors("effhead_train_epoch", (
            ("trunk", trunk, torch.float32, self.TRUNK_ROW * R, False), ("labels", labels, torch.int32, R, False),
            ("perm", perm, torch.int32, N, False), ("keep", keep, torch.int64, 20 * N, True),
            ("bn_mean", bn_mean, torch.float32, 1280, False), ("bn_var", bn_var, torch.float32, 1280, False),
            ("params", params, torch.float32, P, False), ("exp_avg", exp_avg, torch.float32, P, False),
            ("exp_avg_sq", exp_avg_sq, torch.float32, P, False), ("grad_out", grad_out, torch.float32, P, True)))
        nsteps = self._nsteps(N, batch)
        step_loss = self._f32(nsteps)
        step_correct = torch.empty(nsteps, dtype=torch.int32, device=self.device)
        ws = self._workspace("effhead_train", self.lib.mmf_effhead_ws_bytes(int(batch)))
        check(self.lib.mmf_effhead_train_epoch(ptr(trunk), ptr(labels), R, ptr(perm), N, ptr(keep), float(p_drop),
                                               int(batch), ptr(bn_mean), ptr(bn_var), float(bn_eps), float(lr),
                                               float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                               int(step0), ptr(params), ptr(exp_avg), ptr(exp_avg_sq), ptr(step_loss),
                                               ptr(step_correct), ptr(grad_out), ptr(ws), ws.numel(), stream_ptr()),
              "mmf_effhead_train_epoch")
        return step_loss, step_correct

    def effhead_eval(self, trunk, labels, batch: int, params, bn_mean, bn_var, bn_eps: float):
        """validate's forward on cached trunk rows (mmf_effhead_eval): consecutive batches in row order ->
        (batch_loss float32 [nbatches], row_logits float32 [R, 2]) on the device."""
        R = int(labels.shape[0])
        self._check_tensors("effhead_eval", (
            ("trunk", trunk, torch.float32, self.TRUNK_ROW * R, False), ("labels", labels, torch.int32, R, False),
            ("bn_mean", bn_mean, torch.float32, 1280, False), ("bn_var", bn_var, torch.float32, 1280, False),
            ("params", params, torch.float32, self.EFFHEAD_PARAMS, False)))
        nb = self._nsteps(R, batch)
        batch_loss, row_logits = self._f32(nb), self._f32(R, 2)
        ws = self._workspace("effhead_train", self.lib.mmf_effhead_ws_bytes(int(batch)))
        check(self.lib.mmf_effhead_eval(ptr(trunk), ptr(labels), R, int(batch), ptr(params), ptr(bn_mean), ptr(bn_var),
                                        float(bn_eps), ptr(batch_loss), ptr(row_logits), ptr(ws), ws.numel(),
                                        stream_ptr()), "mmf_effhead_eval")
        return batch_loss, row_logits

    def vault_topk(self, q_unit: torch.Tensor, k: int = 5, thresh: float = 0.85, text_emb=None):
        q = q_unit.contiguous()
        B = q.shape[0]
        sims, idx = self._f32(B, k), torch.empty((B, k), dtype=torch.int32, device=self.device)
        disc, tsim = self._f32(B), self._f32(B)
        check(self.lib.mmf_vault_topk(self.h, ptr(q), B, k, float(thresh), ptr(sims), ptr(idx), ptr(disc),
                                      ptr(text_emb), ptr(tsim), stream_ptr()), "mmf_vault_topk")
        return sims, idx, disc, tsim

    def search_rows(self, q_unit, bank, k: int = 5, thresh: float = 0.85, text_emb=None, title_bank=None,
                    nblocks: int = 0):
        """Top-k of unit queries [B, 512] over ANY device-resident bank [N, 512] of rows (used as they
        are: no renormalisation), by the fused similarity + top-k kernels (mmf_vault_search_rows: no
        [B, N] matrix; k in 1..8, slots past N hold index -1).  Returns (sims [B, k], idx [B, k], disc [B],
        tsim [B]) as vault_topk does; ``title_bank`` [N, 512] with ``text_emb`` [B, 512] gives tsim.
        ``nblocks``: vault partitions (0 = automatic; the result does not depend on it)."""
        q = torch.as_tensor(q_unit, dtype=torch.float32).to(self.device).contiguous()
        if not (torch.is_tensor(bank) and bank.is_cuda and bank.dtype == torch.float32 and bank.is_contiguous()):
            raise ValueError("bank must be a contiguous float32 tensor on the device")
        if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1]:
            raise ValueError(f"q_unit {tuple(q.shape)} and bank {tuple(bank.shape)} must be [B, D] and [N, D]")
        B, N, D = q.shape[0], bank.shape[0], bank.shape[1]
        ws = self._workspace("vault_search", self.lib.mmf_vault_search_ws_bytes(B, k, nblocks))
        sims, idx = self._f32(B, k), torch.empty((B, k), dtype=torch.int32, device=self.device)
        disc, tsim = self._f32(B), self._f32(B)
        if text_emb is not None:
            text_emb = torch.as_tensor(text_emb, dtype=torch.float32).to(self.device).contiguous()
        check(self.lib.mmf_vault_search_rows(ptr(q), ptr(bank), B, N, D, k, float(thresh), ptr(sims), ptr(idx),
                                             ptr(disc), 1, ptr(text_emb), ptr(title_bank), ptr(tsim), ptr(ws),
                                             ws.numel(), nblocks, stream_ptr()), "mmf_vault_search_rows")
        return sims, idx, disc, tsim

    def fusion(self, x5):
        x5 = torch.as_tensor(x5, dtype=torch.float32).to(self.device).contiguous()
        B = x5.shape[0]
        probs, conf = self._f32(B, 2), self._f32(B)
        verdict = torch.empty(B, dtype=torch.int32, device=self.device)
        rule = torch.empty(B, dtype=torch.int32, device=self.device)
        check(self.lib.mmf_fusion(self.h, ptr(x5), B, ptr(probs), ptr(verdict), ptr(conf), ptr(rule), stream_ptr()),
              "mmf_fusion")
        return probs, verdict, conf, rule

    FUSION_PARAMS = 2530  # MMF_FUSION_PARAMS: fusion_layer's parameters in state-dict order

    def fusion_train_epoch(self, scores5, labels, perm, keep, p_drop: float, batch: int, lr: float, betas,
                           eps: float, weight_decay: float, step0: int, params, exp_avg, exp_avg_sq,
                           grad_out=None):
        """One epoch of FusionJudge training in one launch (mmf_fusion_train_epoch): device tensors scores5
        float32 [N, 5], labels int32 [N], perm int32 [N], keep int64 [N] (the uint64 masks' bits) or None;
        params / exp_avg / exp_avg_sq float32 [2530], updated in place.  Returns (step_loss float32 [nsteps],
        step_correct int32 [nsteps]) on the device; nothing is synchronised."""
        N = int(labels.shape[0])
        P = self.FUSION_PARAMS
        self._check_tensors("fusion_train_epoch", (
            ("scores5", scores5, torch.float32, 5 * N, False), ("labels", labels, torch.int32, N, False),
            ("perm", perm, torch.int32, N, False), ("keep", keep, torch.int64, N, True),
            ("params", params, torch.float32, P, False), ("exp_avg", exp_avg, torch.float32, P, False),
            ("exp_avg_sq", exp_avg_sq, torch.float32, P, False), ("grad_out", grad_out, torch.float32, P, True)))
        nsteps = self._nsteps(N, batch)
        step_loss = self._f32(nsteps)
        step_correct = torch.empty(nsteps, dtype=torch.int32, device=self.device)
        check(self.lib.mmf_fusion_train_epoch(ptr(scores5), ptr(labels), N, ptr(perm), ptr(keep), float(p_drop),
                                              int(batch), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                              float(weight_decay), int(step0), ptr(params), ptr(exp_avg),
                                              ptr(exp_avg_sq), ptr(step_loss), ptr(step_correct), ptr(grad_out),
                                              stream_ptr()), "mmf_fusion_train_epoch")
        return step_loss, step_correct

    def analyze_batch(self, rob_ids, rob_mask, clip_ids, clip_mask, img, img_clip=None,
                      out: Optional[dict] = None) -> dict:
        """Text+image pairs through all five signals + fusion (misinfo_forensics.py:767-927)."""
        rob_ids, rob_mask = self._i32(rob_ids), self._i32(rob_mask)
        clip_ids, clip_mask = self._i32(clip_ids), self._i32(clip_mask)
        img = self._u8(img)
        img_clip = self._u8(img_clip) if img_clip is not None else None
        B = rob_ids.shape[0]
        if out is None:
            out = self.alloc_outputs(B)
        check(self.lib.mmf_analyze_batch(
            self.h, ptr(rob_ids), ptr(rob_mask), rob_ids.shape[1], ptr(clip_ids), ptr(clip_mask), clip_ids.shape[1],
            ptr(img), ptr(img_clip), B, ptr(out["scores"]), ptr(out["text_similarity"]), ptr(out["probs"]),
            ptr(out["verdict"]), ptr(out["confidence"]), ptr(out["rule"]), ptr(out["top_sims"]),
            ptr(out["top_idx"]), stream_ptr()), "mmf_analyze_batch")
        return out

    def mixed_plan(self, modality):
        """Host plan of a mixed batch (mmf_mixed_plan): modality per row (bit 0 text, bit 1 image) ->
        (row_map int32 [B, 3], (nT, nI, nC)).  A row without a modality raises the reference's
        ValueError (misinfo_forensics.py:793-794)."""
        m = np.asarray(modality.cpu() if isinstance(modality, torch.Tensor) else modality).reshape(-1)
        if m.size == 0:
            raise ValueError("empty batch")
        if (m == 0).any():
            raise ValueError(NO_INPUT_ERROR)
        if ((m < 0) | (m > 3)).any():
            raise ValueError("modality entries are 1 (text), 2 (image) or 3 (both)")
        m = np.ascontiguousarray(m, dtype=np.uint8)
        row_map = np.empty((m.size, 3), np.int32)
        counts = np.zeros(3, np.int32)
        check(self.lib.mmf_mixed_plan(m.ctypes.data_as(ctypes.c_void_p), m.size, row_map.ctypes.data_as(ctypes.c_void_p),
                                      counts.ctypes.data_as(ctypes.c_void_p)), "mmf_mixed_plan")
        return row_map, tuple(int(c) for c in counts)

    _PLAN_CACHE = 8  # device row maps kept (a serving loop repeats a few modality patterns)

    def _device_plan(self, modality):
        """mixed_plan with the row map on the device.  The upload of a small pageable array waits for
        the stream, so the last few plans are kept by their modality bytes: a repeated pattern costs
        no copy."""
        m = np.asarray(modality.cpu() if isinstance(modality, torch.Tensor) else modality).reshape(-1)
        key = m.astype(np.int64).tobytes()
        cache = self.__dict__.setdefault("_plans", {})
        hit = cache.pop(key, None)
        if hit is None:
            row_map, counts = self.mixed_plan(m)
            hit = (torch.from_numpy(row_map).to(self.device), counts)
            while len(cache) >= self._PLAN_CACHE:
                cache.pop(next(iter(cache)))
        cache[key] = hit  # (re-inserted last: the oldest entry is dropped first)
        return hit

    def analyze_mixed(self, modality, rob_ids, rob_mask, clip_ids, clip_mask, img, img_clip=None,
                      out: Optional[dict] = None) -> dict:
        """analyze_batch for posts with a text, an image or both (misinfo_forensics.py:790-899) in one
        launch sequence.  modality [B]: 1 text, 2 image, 3 both.  The inputs are COMPACT: rob_ids /
        rob_mask hold the nT text rows in batch order, img / img_clip the nI image rows, clip_ids /
        clip_mask the nC rows with both; a list without rows may be None.  Returns analyze_batch's
        dict of [B, ...] device tensors in batch order, absent signals 0 (top_idx -1) and the
        reference's single-modality verdict on the rows that are not pairs."""
        dmap, (nT, nI, nC) = self._device_plan(modality)
        B = dmap.shape[0]

        def rows(name, t, n):
            if n and (t is None or t.shape[0] != n):
                raise ValueError(f"{name}: expected {n} rows, got {None if t is None else t.shape[0]}")
            return t if n else None
        rob_ids = rows("rob_ids", self._i32(rob_ids) if nT else None, nT)
        rob_mask = rows("rob_mask", self._i32(rob_mask) if nT else None, nT)
        clip_ids = rows("clip_ids", self._i32(clip_ids) if nC else None, nC)
        clip_mask = rows("clip_mask", self._i32(clip_mask) if nC else None, nC)
        img = rows("img", self._u8(img) if nI else None, nI)
        img_clip = rows("img_clip", self._u8(img_clip), nI) if nI and img_clip is not None else None
        if out is None:
            out = self.alloc_outputs(B)
        check(self.lib.mmf_analyze_mixed(
            self.h, ptr(dmap), B, nT, nI, nC, ptr(rob_ids), ptr(rob_mask), rob_ids.shape[1] if nT else 0,
            ptr(clip_ids), ptr(clip_mask), clip_ids.shape[1] if nC else 0, ptr(img), ptr(img_clip),
            ptr(out["scores"]), ptr(out["text_similarity"]), ptr(out["probs"]), ptr(out["verdict"]),
            ptr(out["confidence"]), ptr(out["rule"]), ptr(out["top_sims"]), ptr(out["top_idx"]), stream_ptr()),
            "mmf_analyze_mixed")
        return out

    def alloc_outputs(self, B: int) -> dict:
        d = self.device
        return {"scores": self._f32(B, 5), "text_similarity": self._f32(B), "probs": self._f32(B, 2),
                "verdict": torch.empty(B, dtype=torch.int32, device=d), "confidence": self._f32(B),
                "rule": torch.empty(B, dtype=torch.int32, device=d), "top_sims": self._f32(B, 5),
                "top_idx": torch.empty((B, 5), dtype=torch.int32, device=d)}

    def host_pipeline(self, B: int, Lr: int, Lc: int = 77) -> "HostPipeline":
        return HostPipeline(self, B, Lr, Lc)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.mmf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class HostPipeline:
    """analyze_batch over batches that start in HOST memory (the boundary of analyze_pairs and of a
    serving loop): three device input slots (MMF_PIPE_SLOTS), H2D copies of batch i+1 on a copy stream while batch i
    computes on the current stream (ids int32 + uint8 images, ~38.6 MB per 256 pairs), results
    copied back into pinned host tensors.  Host inputs should be pinned (`torch.Tensor.pin_memory`)
    for the copies to run asynchronously."""

    _IN = ("rid", "rm", "cid", "cm", "img")

    def __init__(self, eng: Engine, B: int, Lr: int, Lc: int = 77, d2h_stream: Optional[bool] = None):
        self.eng, self.B = eng, B
        # result copies on a stream of their own (behind the batch's compute, beside the next batch's)
        # instead of in the compute stream; MMF_D2H_STREAM=0 restores the in-stream copies (A/B)
        if d2h_stream is None:
            d2h_stream = os.environ.get("MMF_D2H_STREAM", "1") != "0"
        self.d2h = torch.cuda.Stream(device=eng.device) if d2h_stream else None
        d = eng.device
        shapes = {"rid": ((B, Lr), torch.int32), "rm": ((B, Lr), torch.int32), "cid": ((B, Lc), torch.int32),
                  "cm": ((B, Lc), torch.int32), "img": ((B, 224, 224, 3), torch.uint8)}
        # input/output slots = batches in flight (MMF_PIPE_SLOTS, default 3): the copy of batch i+1 beside
        # the compute of batch i, and the host one more batch ahead.  With 2, a host hiccup longer than
        # one batch's compute left the device idle: bench headline 18,365 -> 18,562 pairs/s (3
        # interleaved processes), now level with the HBM-resident rate (profiles/r04_ab_pipe_slots.txt, git history at 168304c)
        self.n = max(2, int(os.environ.get("MMF_PIPE_SLOTS", "3")))
        self.slots = [{k: torch.empty(sh, dtype=dt, device=d) for k, (sh, dt) in shapes.items()} for _ in range(self.n)]
        self.outs = [eng.alloc_outputs(B) for _ in range(self.n)]
        self.host_out = [{k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in o.items()}
                         for o in self.outs]
        self.copy_stream = torch.cuda.Stream(device=d)
        self.ready = [torch.cuda.Event() for _ in range(self.n)]
        self.free = [torch.cuda.Event() for _ in range(self.n)]
        self.done = [torch.cuda.Event() for _ in range(self.n)]
        self.i = 0

    def submit(self, batch: Dict[str, torch.Tensor]) -> int:
        """Queue one host batch {rid, rm, cid, cm, img}; returns the slot whose results
        `result(slot)` returns once the batch has finished.  Never blocks on the device except
        when the slot is still in use by the batch submitted `n` calls earlier."""
        k = self.i % self.n
        main = torch.cuda.current_stream(self.eng.device)
        if self.i >= self.n:
            self.done[k].synchronize()  # the host copy of that slot's previous results is complete
        with torch.cuda.stream(self.copy_stream):
            if self.i >= self.n:
                self.copy_stream.wait_event(self.free[k])  # compute of batch i-n has read the slot
            for n in self._IN:
                self.slots[k][n].copy_(batch[n], non_blocking=True)
            self.ready[k].record(self.copy_stream)
        main.wait_event(self.ready[k])
        sl = self.slots[k]
        self.eng.analyze_batch(sl["rid"], sl["rm"], sl["cid"], sl["cm"], sl["img"], out=self.outs[k])
        self.free[k].record(main)
        if self.d2h is not None:
            with torch.cuda.stream(self.d2h):
                self.d2h.wait_event(self.free[k])
                for n, v in self.outs[k].items():
                    self.host_out[k][n].copy_(v, non_blocking=True)
                self.done[k].record(self.d2h)
        else:
            for n, v in self.outs[k].items():
                self.host_out[k][n].copy_(v, non_blocking=True)
            self.done[k].record(main)
        self.i += 1
        return k

    def result(self, slot: int) -> Dict[str, torch.Tensor]:
        self.done[slot].synchronize()
        return self.host_out[slot]
