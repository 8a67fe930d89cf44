"""Drop-in Python API mirroring the reference's plugin boundary:

* ``MultiModalMisinfoDetector`` (misinfo_forensics.py:43-108) — an ``nn.Module`` with the
  reference's state-dict layout; ``fusion_layer`` is a real trainable torch module (the
  train_fusion_judge.py loop runs unchanged on it), while ``forward_text`` / ``forward_image``
  execute on the HIP kernels of libmmf_hip.so.
* ``MisinfoForensics`` (misinfo_forensics.py:111-927) — same constructor keywords, methods and
  result dicts; every signal runs through the HIP engine.  ``analyze_batch`` is the batched
  tensor entry point the benchmark times.
* ``CLIPSimilarityEngine`` (clip_similarity_engine.py:13-174).

There is no CPU fallback: without a HIP device the constructors raise.
"""
from __future__ import annotations

import itertools
import math
import os
import warnings
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import xxhash

from . import explain, io_utils, weights as W
from .engine import Engine, NO_INPUT_ERROR, SCORE_KEYS
from .hip import MMFError
from .precision import rerun_if

_DEFAULT_CLIP_DIR = r"C:\Users\Lenovo\OneDrive\Desktop\hack\models\clip-vit-b32"


def _require_hip(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"mmf_amd runs only on a HIP device (MI355X); got device={device!r} and "
                           f"torch.cuda.is_available()={torch.cuda.is_available()}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


# ---------------------------------------------------------------------------------------------
# detector module (state-dict contract)
# ---------------------------------------------------------------------------------------------
def _param_tree(spec) -> nn.Module:
    """nn.Module tree whose state_dict keys are exactly the spec's names (no forward)."""
    root = nn.Module()
    for name, (shape, init) in spec.items():
        parts = name.split(".")
        mod = root
        for p in parts[:-1]:
            if not hasattr(mod, p) or not isinstance(getattr(mod, p), nn.Module):
                mod.add_module(p, nn.Module())
            mod = getattr(mod, p)
        leaf = parts[-1]
        if init[0] == "int_zero":
            mod.register_buffer(leaf, torch.zeros(shape, dtype=torch.int64))
        elif leaf in ("running_mean", "running_var"):
            mod.register_buffer(leaf, torch.zeros(shape))
        else:
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
    return root


# detector components as the engine packs them (mmf_finalize: one device weight group each)
_COMPONENTS: Tuple[Tuple[str, Tuple[str, ...]], ...] = (
    ("text", ("roberta", "ai_head", "misinfo_head")),  # RoBERTa + dual heads (ready bit 1)
    ("effnet", ("efficientnet",)),                     # EfficientNet-B0 (bit 2)
    ("fusion", ("fusion_layer",)),                     # FusionJudge (bit 16)
)
ALL_COMPONENTS = tuple(c for c, _ in _COMPONENTS)

# Process-wide count of parameter / buffer / submodule (re)registrations (torch's global module
# registration hooks): the detector's cached per-component tensor lists are rebuilt when it moves.
_REGISTRATIONS = [0]


def _count_registration(*_args):
    _REGISTRATIONS[0] += 1


for _reg in ("register_module_parameter_registration_hook", "register_module_buffer_registration_hook",
             "register_module_module_registration_hook"):
    getattr(torch.nn.modules.module, _reg)(_count_registration)


class MultiModalMisinfoDetector(nn.Module):
    """misinfo_forensics.py:43-108 with the same submodule names.  The encoders are parameter
    containers (their arithmetic is the HIP engine's); the heads and the fusion layer are real
    torch modules so training code keeps working.

    Weight changes after construction reach the device: ``detector.load_state_dict(...)``
    (train_fusion_judge.py:297), a head-level ``ai_head.load_state_dict(...)``
    (misinfo_forensics.py:274), ``.to()`` moves, optimizer steps on ``fusion_layer`` -- every
    in-place update bumps a tensor's version counter and every replacement changes its storage, so
    ``sync()`` (called before each device forward) compares a per-component fingerprint of
    (version, data_ptr) over all parameters and buffers and re-packs exactly the components that
    changed.  The tensor lists are cached (walking the module tree costs ~2 ms) and rebuilt whenever
    any module in the process registers a parameter, buffer or submodule (assignment of a new
    Parameter, ``load_state_dict(assign=True)``); an unchanged check costs ~0.2 ms."""

    def __init__(self, roberta_model_name: str = "roberta-base"):
        super().__init__()
        self.roberta = _param_tree(W.roberta_spec(""))
        hidden = W.ROBERTA["hidden"]
        self.ai_head = nn.Sequential(nn.Linear(hidden, 256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 2))
        self.misinfo_head = nn.Sequential(nn.Linear(hidden, 256), nn.ReLU(), nn.Dropout(0.3), nn.Linear(256, 2))
        self.efficientnet = _param_tree(W.effnet_spec(""))
        self.fusion_layer = nn.Sequential(nn.Linear(5, 64), nn.ReLU(), nn.Dropout(0.2), nn.Linear(64, 32),
                                          nn.ReLU(), nn.Linear(32, 2))
        for m in (self.ai_head, self.misinfo_head):
            for p in m.parameters():
                p.requires_grad_(False)
        self._engine: Optional[Engine] = None
        self._synced: Dict[str, tuple] = {}
        self._held: Dict[str, list] = {}  # storages of the packed state (see _fingerprint)
        self._tensors: Dict[str, list] = {}
        self._tensors_epoch = -1
        self._warned_inference = False
        self.uploads = {c: 0 for c in ALL_COMPONENTS}  # re-pack counts (observability, tests)

    def _apply(self, fn, *args, **kwargs):
        # .to() / .half() / .cuda() may replace parameter objects without a registration hook
        # firing: rebuild the cached tensor lists on the next fingerprint
        out = super()._apply(fn, *args, **kwargs)
        self._tensors_epoch = -1
        return out

    # -- HIP binding --------------------------------------------------------------------------
    def bind(self, engine: Engine) -> None:
        """Bind to a device engine and upload every component."""
        self._engine = engine
        self._synced = {}
        self.sync(force=True)

    def _eng(self) -> Engine:
        if self._engine is None:
            raise RuntimeError("detector is not bound to a HIP engine (construct it through MisinfoForensics)")
        return self._engine

    def _fingerprint(self, comp: str) -> tuple:
        """(version, address) per tensor.  The storages of the last packed state are held by
        ``sync`` (``_held``), so a replaced tensor -- ``.half()`` then ``.float()``, a move and back,
        any dtype or device change -- can never land on the address it had when it was packed: a
        replacement always changes the fingerprint (0.12 ms for the 573 tensors).  Inference
        tensors have no version counter; a component holding one is re-packed on every call
        (correct, slow; warned once)."""
        if self._tensors_epoch != _REGISTRATIONS[0]:
            self._tensors = {c: [t for m in mods for t in itertools.chain(getattr(self, m).parameters(),
                                                                            getattr(self, m).buffers())]
                             for c, mods in _COMPONENTS}
            self._tensors_epoch = _REGISTRATIONS[0]
        try:
            return tuple([(t._version, t.data_ptr()) for t in self._tensors[comp]])
        except RuntimeError:  # "Inference tensors do not track version counter"
            if not any(t.is_inference() for t in self._tensors[comp]):
                raise
            if not self._warned_inference:
                warnings.warn("detector holds inference-mode tensors (no version counter): their "
                              "components are re-packed before every device call")
                self._warned_inference = True
            return (object(),)  # never equal: always stale

    def stale_components(self, which: Sequence[str] = ALL_COMPONENTS) -> List[str]:
        """Components whose tensors changed since they were last packed on the device."""
        return [c for c, _ in _COMPONENTS if c in which and self._fingerprint(c) != self._synced.get(c)]

    def sync(self, which: Sequence[str] = ALL_COMPONENTS, force: bool = False) -> List[str]:
        """Re-pack the changed components (all of `which` if `force`) on the device engine; returns
        the names re-packed.  A component is staged whole (its packing fuses tensors: QKV, BN into
        the convs) and its previous device buffers are freed by mmf_finalize."""
        eng = self._eng()
        todo = []
        for c, mods in _COMPONENTS:
            if c not in which:
                continue
            fp = self._fingerprint(c)
            if force or fp != self._synced.get(c):
                todo.append((c, mods, fp))
        if not todo:
            return []
        for c, mods, _ in todo:
            sd = {}
            for m in mods:
                for k, v in getattr(self, m).state_dict().items():
                    sd[f"{m}.{k}"] = v.detach().cpu()  # device tensors (the detector lives on .device)
            eng.load_state(sd)
        eng.finalize()
        for c, _, fp in todo:
            self._synced[c] = fp
            self._held[c] = [t.untyped_storage() for t in self._tensors[c]]
            self.uploads[c] += 1
        names = [c for c, _, _ in todo]
        eng.calibrate(names)  # load-time precision selection of the re-packed towers
        return names

    def sync_fusion(self, force: bool = False) -> None:
        """Re-upload fusion_layer to the device engine after it was trained / reloaded."""
        self.sync(("fusion",), force=force)

    def sync_all(self) -> None:
        """Upload every detector tensor to the engine."""
        self.sync(force=True)

    # -- reference forward methods ------------------------------------------------------------
    def forward_text(self, input_ids, attention_mask):
        """misinfo_forensics.py:92-100 -> (ai_logits, misinfo_logits), on the HIP engine."""
        self.sync(("text",))
        ai, mi, _ = self._eng().text_forward(input_ids, attention_mask)
        return ai, mi

    def forward_image(self, image_tensor):
        """misinfo_forensics.py:102-104: normalised fp32 [B,3,224,224] -> logits [B,2] (HIP)."""
        self.sync(("effnet",))
        logits, _ = self._eng().effnet_forward_f32(image_tensor)
        return logits

    def forward_fusion(self, scores_tensor):
        """misinfo_forensics.py:106-108 (differentiable torch module, for fusion training)."""
        return self.fusion_layer(scores_tensor)


def _load_pretrained_states(clip_model_dir: str):
    """roberta-base and CLIP weights from the local HF cache / directory (no network)."""
    det, clip = None, None
    try:
        from transformers import RobertaModel
        m = RobertaModel.from_pretrained("roberta-base", local_files_only=True)
        det = {f"roberta.{k}": v for k, v in m.state_dict().items()}
    except Exception as e:  # noqa: BLE001
        warnings.warn(f"roberta-base weights not available locally ({type(e).__name__})")
    try:
        from transformers import CLIPModel
        m = CLIPModel.from_pretrained(clip_model_dir, local_files_only=True)
        clip = dict(m.state_dict())
    except Exception as e:  # noqa: BLE001
        warnings.warn(f"CLIP weights not available at {clip_model_dir!r} ({type(e).__name__})")
    return det, clip


CLIP_EOS_DEFAULT = 49407  # openai/clip-vit-base-patch32's text_config.eos_token_id


def clip_eos_token_id(clip_model_dir: Optional[str]) -> int:
    """The id the CLIP text tower pools at: `text_config.eos_token_id` of the CLIP config in
    `clip_model_dir` -- the value transformers' CLIPTextTransformer keys its pooling on (the first
    position holding it; the legacy id 2 means argmax(ids), handled by the device kernel too) --,
    overridden by MMF_CLIP_EOS_TOKEN_ID, 49407 when no config is available offline."""
    env = os.environ.get("MMF_CLIP_EOS_TOKEN_ID")
    if env:
        return int(env)
    if clip_model_dir:
        try:
            from transformers import CLIPConfig
            eos = CLIPConfig.from_pretrained(clip_model_dir, local_files_only=True).text_config.eos_token_id
            if eos is not None:
                return int(eos)
        except Exception:  # noqa: BLE001  (no local config: the published model's id)
            pass
    return CLIP_EOS_DEFAULT


def resolve_states(detector_state, clip_state, synthetic_seed: Optional[int], clip_model_dir: str,
                   loader=None):
    """Constructor weights: explicit states > synthetic seed > local pretrained files, each
    resolved on its own (an explicit detector_state is kept when only clip_state has to be found).
    ``loader(clip_model_dir) -> (roberta state | None, CLIP state | None)``."""
    if synthetic_seed is not None:
        if detector_state is None:
            detector_state = W.synthetic_detector_state(synthetic_seed)
        if clip_state is None:
            clip_state = W.synthetic_clip_state(synthetic_seed)
        return detector_state, clip_state
    if detector_state is not None and clip_state is not None:
        return detector_state, clip_state
    det_pre, clip_pre = (loader or _load_pretrained_states)(clip_model_dir)
    if detector_state is None:
        if det_pre is None:
            raise RuntimeError("no detector weights: roberta-base is not available locally; pass "
                               "detector_state= or synthetic_seed=")
        # heads, EfficientNet (weights=None in the reference: random init) and the fusion layer
        # start from the seeded synthetic init unless a checkpoint overrides them
        base = W.synthetic_detector_state(0)
        base.update({k: np.asarray(v) for k, v in det_pre.items() if k in base})
        detector_state = base
    if clip_state is None:
        if clip_pre is None:
            raise RuntimeError(f"no CLIP weights at {clip_model_dir!r}; pass clip_state= or synthetic_seed=")
        clip_state = clip_pre
    return detector_state, clip_state


# ---------------------------------------------------------------------------------------------
# MisinfoForensics
# ---------------------------------------------------------------------------------------------
def sample_video_frames(video_path: str, max_frames: int = 12, stride_seconds: float = 1.0) -> List:
    """Frame sampling of analyze_video (misinfo_forensics.py:501-548), verbatim semantics: OpenCV
    decode, fps fallback 25, stride = max(1, round(fps * max(0.1, stride_seconds))) frames, at most
    max_frames frames, BGR -> RGB PIL images.  Same errors as the reference."""
    try:
        import cv2
    except Exception as e:  # noqa: BLE001
        raise RuntimeError("opencv-python is required for video analysis. Install with: pip install "
                           "opencv-python") from e
    from PIL import Image
    cap = cv2.VideoCapture(video_path)
    if not cap.isOpened():
        raise RuntimeError(f"Could not open video: {video_path}")
    fps = cap.get(cv2.CAP_PROP_FPS)
    if not fps or fps <= 0:
        fps = 25.0
    frame_stride = max(1, int(round(fps * max(0.1, float(stride_seconds)))))
    frames, frame_idx = [], 0
    while len(frames) < max_frames:
        ok, frame = cap.read()
        if not ok:
            break
        if frame_idx % frame_stride != 0:
            frame_idx += 1
            continue
        frame_idx += 1
        frames.append(Image.fromarray(cv2.cvtColor(frame, cv2.COLOR_BGR2RGB)))
    cap.release()
    return frames


class MisinfoForensics:
    """misinfo_forensics.py:111-927 on the MI355X engine."""

    def __init__(self, fusion_weights: str = "forensics_master_final.pth",
                 ai_head_weights: str = "ai_head_best.pth",
                 misinfo_head_weights: str = "roberta_detective_best.pth",
                 efficientnet_weights: str = "efficientnet_cifake_best.pth",
                 clip_model_dir: str = _DEFAULT_CLIP_DIR,
                 clip_weights: str = "clip_detective_best.pth",
                 faiss_index_path: str = "guardian_embeddings.pkl",
                 gemini_api_key: Optional[str] = None,
                 device: str = "cuda",
                 *, roberta_tokenizer=None, clip_processor=None, detector_state=None, clip_state=None,
                 synthetic_seed: Optional[int] = None, max_batch: int = 256, max_text_len: int = 128,
                 effnet_precision: str = "auto", text_precision: str = "auto", verbose: bool = True):
        if effnet_precision not in Engine.EFFNET_PRECISIONS:
            raise ValueError(f"effnet_precision must be one of {Engine.EFFNET_PRECISIONS}, got {effnet_precision!r}")
        if text_precision not in Engine.TEXT_PRECISIONS:
            raise ValueError(f"text_precision must be one of {tuple(Engine.TEXT_PRECISIONS)}, got {text_precision!r}")
        self.device = _require_hip(device)
        self._verbose = verbose
        self._log(f"Using device: {self.device}")
        # Gemini (misinfo_forensics.py:147-165): a network service -> not available offline
        self.gemini_available = False
        self.gemini_api_key = gemini_api_key or os.getenv("GOOGLE_API_KEY")
        if self.gemini_api_key:
            self._log("⚠ Gemini client not available in this build. Using fallback explanations.")

        self._emb_cache = None  # (hash of the CLIP input window, its image embedding): _image_emb
        self.vit_passes = 0  # single-image ViT launches (observability, tests)
        self.reuse_image_embedding = True  # False: a ViT pass per call, as the reference (A/B)
        # analyze_pairs: JPEG bytes / files entropy-decoded on the host, reconstructed on the device
        # (jpeg.py; MMF_DEVICE_JPEG=0 or False here: Pillow decodes every image, A/B)
        self.device_jpeg = os.environ.get("MMF_DEVICE_JPEG", "1") != "0"
        self._jpeg = None
        self.roberta_tokenizer = roberta_tokenizer
        self.clip_processor = clip_processor
        if self.roberta_tokenizer is None:
            try:
                from transformers import RobertaTokenizer
                self.roberta_tokenizer = RobertaTokenizer.from_pretrained("roberta-base", local_files_only=True)
            except Exception:  # noqa: BLE001
                self._log("⚠ roberta-base tokenizer not available locally; pass roberta_tokenizer=")
        if self.clip_processor is None:
            try:
                from transformers import CLIPProcessor
                self.clip_processor = CLIPProcessor.from_pretrained(clip_model_dir, local_files_only=True)
            except Exception:  # noqa: BLE001
                self._log(f"⚠ CLIP processor not available at {clip_model_dir!r}; pass clip_processor=")

        detector_state, clip_state = resolve_states(detector_state, clip_state, synthetic_seed, clip_model_dir)
        # on the device like misinfo_forensics.py:172: train_fusion_judge.py:204-221 feeds CUDA
        # tensors to forward_fusion and checkpoints device tensors (:259-267)
        self.detector = MultiModalMisinfoDetector().to(self.device)
        self.detector.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in detector_state.items()},
                                      strict=False)
        # checkpoint overlays with the reference's strict=False semantics (quirks Q1-Q4)
        if os.path.exists(fusion_weights):
            self._log(f"\n🎯 Loading FINAL TRAINED MODEL from {fusion_weights}...")
            try:
                ck = torch.load(fusion_weights, map_location="cpu", weights_only=True)
                if "full_model_state_dict" not in ck:
                    raise KeyError("Missing full_model_state_dict")
                self.detector.load_state_dict(ck["full_model_state_dict"], strict=False)
            except Exception as e:  # noqa: BLE001
                self._log(f"  ⚠ Error loading fusion weights: {e}")
                self._load_individual_weights(ai_head_weights, misinfo_head_weights, efficientnet_weights,
                                              clip_weights)
        else:
            self._load_individual_weights(ai_head_weights, misinfo_head_weights, efficientnet_weights, clip_weights)
        self.detector.eval()

        self.clip_eos_token_id = clip_eos_token_id(clip_model_dir)
        # effnet_precision / text_precision "auto" (default): at every (re)load of the component the
        # engine measures its fast path against its precision fallback on seeded calibration inputs
        # and keeps the fallback when a score moves by more than 5e-4 (the fp32
        # EfficientNet tower; RoBERTa's precise mode, Engine.check_text_precision); the other values
        # pin the mode
        self.engine = Engine(self.device.index or 0, None, clip_state, eos_token_id=self.clip_eos_token_id,
                             max_batch=max_batch, max_text_len=max_text_len, effnet_precision=effnet_precision,
                             text_precision=text_precision)
        self.detector.bind(self.engine)  # uploads RoBERTa + heads, EfficientNet, FusionJudge
        self.clip_state = clip_state

        # ---- Truth-Vault (misinfo_forensics.py:214-246) ------------------------------------
        self.vault_loaded = False
        self.vault_embeddings, self.vault_metadata = None, None
        if faiss_index_path and os.path.exists(faiss_index_path):
            self._log(f"\nLoading Truth Vault from {faiss_index_path}...")
            emb, meta = io_utils.load_vault(faiss_index_path)
            if emb is None:
                self._log("  ⚠ Unknown database format")
            else:
                self.set_vault(emb, meta)
        else:
            self._log(f"⚠ Truth Vault not found: {faiss_index_path}")

    # ------------------------------------------------------------------ helpers
    def _log(self, msg: str) -> None:
        if self._verbose:
            print(msg)

    def _load_individual_weights(self, ai_head_weights, misinfo_head_weights, efficientnet_weights, clip_weights):
        """misinfo_forensics.py:260-317, including its silent no-op cases (quirks Q1-Q3)."""
        def _ld(path):
            return torch.load(path, map_location="cpu", weights_only=True)
        if os.path.exists(ai_head_weights):
            ck = _ld(ai_head_weights)
            st = {k.replace("ai_head.", ""): v for k, v in ck["model_state_dict"].items() if "ai_head" in k}
            self.detector.ai_head.load_state_dict(st, strict=False)
        if os.path.exists(misinfo_head_weights):
            ck = _ld(misinfo_head_weights)
            st = {k.replace("misinfo_head.", ""): v for k, v in ck["model_state_dict"].items() if "misinfo_head" in k}
            self.detector.misinfo_head.load_state_dict(st, strict=False)
        if os.path.exists(efficientnet_weights):
            ck = _ld(efficientnet_weights)
            if isinstance(ck, dict) and "model_state_dict" in ck:
                st = {k.replace("efficientnet.", ""): v for k, v in ck["model_state_dict"].items() if "efficientnet" in k}
                self.detector.efficientnet.load_state_dict(st, strict=False)
            else:
                try:
                    self.detector.efficientnet.load_state_dict(ck, strict=False)
                except RuntimeError:  # size mismatch (misinfo_forensics.py:299-303)
                    cls = {k: v for k, v in ck.items() if "classifier" in k}
                    if cls:
                        self.detector.efficientnet.classifier.load_state_dict(cls, strict=False)
        if os.path.exists(clip_weights):
            # Q1: the reference tries this before its CLIP model exists; the AttributeError is
            # swallowed, so fine-tuned CLIP weights never reach inference.  Reproduced.
            self._log("  ⚠ Could not load CLIP weights: 'MisinfoForensics' object has no attribute 'clip_model'")

    def set_vault(self, embeddings: np.ndarray, metadata: List[Dict]) -> None:
        """Load Truth-Vault rows (normalised once on the device) and pre-compute the CLIP text
        embeddings of their titles (the text_similarity operand, misinfo_forensics.py:467-484)."""
        self.vault_embeddings = np.asarray(embeddings)  # the file's dtype (float16 / float32)
        self.vault_metadata = metadata
        ids = mask = None
        if self.clip_processor is not None and metadata:
            seqs = io_utils.tokenize_clip(self.clip_processor, [m["title"] for m in metadata], truncation=True)
            ids, mask = io_utils.pad_ids(seqs, self.clip_eos_token_id, 77)
        self.engine.set_vault(self.vault_embeddings, ids, mask)
        self.vault_loaded = True
        self._log(f"  ✓ Loaded {len(metadata)} verified articles")

    def _rob_ids(self, text: str) -> np.ndarray:
        if self.roberta_tokenizer is None:
            raise RuntimeError("no RoBERTa tokenizer (pass roberta_tokenizer=)")
        ids = io_utils.tokenize_roberta(self.roberta_tokenizer, text)
        self._fit_text(len(ids))
        return np.asarray([ids], dtype=np.int32)

    def _fit_text(self, n_tokens: int) -> None:
        """The tokenizer truncates at 512 (misinfo_forensics.py:327-333); workspaces are reserved for
        `max_text_len` (128 by default) and grown to the full 512 the first time a longer text
        arrives, so every text the reference accepts runs on the device."""
        if n_tokens > self.engine.max_text_len:
            if n_tokens > 512:
                raise ValueError(f"text of {n_tokens} tokens: RoBERTa positions end at 512")
            self.engine.reserve(self.engine.max_batch, 512, self.engine.max_clip_len)

    def _clip_ids(self, texts: List[str], truncation: bool = False):
        if self.clip_processor is None:
            raise RuntimeError("no CLIP processor (pass clip_processor=)")
        seqs = io_utils.tokenize_clip(self.clip_processor, texts, truncation=truncation)
        if max(len(s) for s in seqs) > 77:
            raise ValueError("CLIP text longer than 77 tokens (the reference errors here too: "
                             "misinfo_forensics.py:386-391 does not truncate)")
        return io_utils.pad_ids(seqs, self.clip_eos_token_id)

    # ------------------------------------------------------------------ signals
    def analyze_text(self, text: str) -> Dict[str, float]:
        """misinfo_forensics.py:319-352."""
        ids = self._rob_ids(text)
        self.detector.sync(("text",))
        # (an overflowed fp16 branch output: once more in the precise mode)
        s = rerun_if(self.engine.text_overflow,
                     lambda: self.engine.text_forward(ids, np.ones_like(ids))[2].cpu().numpy())
        return {"ai_score": float(s[0, 0]), "misinfo_score": float(s[0, 1])}

    def analyze_image(self, image_path) -> Dict[str, float]:
        """misinfo_forensics.py:354-373."""
        px = io_utils.effnet_pixels(io_utils.to_pil(image_path))[None]
        self.detector.sync(("effnet",))
        # (an overflowed fp16 activation: once more on the fp32 tower)
        s = rerun_if(self.engine.effnet_overflow, lambda: self.engine.effnet_forward(px)[1].cpu().numpy())
        return {"deepfake_score": float(s[0])}

    def _image_emb(self, pil, check: bool = True) -> torch.Tensor:
        """CLIP image embedding [1,512] of one image.  analyze_consistency and search_vault both
        embed the image (quirk Q6: the reference runs the ViT twice per pair, misinfo_forensics.py:395,
        438; FusionTrainingDataset calls them back to back, train_fusion_judge.py:81-85): the last
        embedding is kept with a 128-bit hash of its 224x224 input window, and an identical window
        reuses it -- the same kernels on the same bytes, so the value is the one a second ViT pass
        would return.  check = False: the caller checks a value computed from the embedding for the
        fp16-stream overflow instead (analyze_consistency: its cosine)."""
        px = io_utils.clip_pixels(pil)
        key = xxhash.xxh3_128_digest(px.tobytes()) if self.reuse_image_embedding else None
        if key is not None and self._emb_cache is not None and self._emb_cache[0] == key:
            return self._emb_cache[1]

        def run():
            return self.engine.clip_image(px[None])
        emb = rerun_if(self.engine.clip_stream_overflow, run) if check else run()  # (once more on fp32 streams)
        self._emb_cache = (key, emb)
        self.vit_passes += 1
        return emb

    def analyze_consistency(self, text: str, image_path) -> Dict[str, float]:
        """misinfo_forensics.py:375-408."""
        ids, mask = self._clip_ids([text])
        pil = io_utils.to_pil(image_path)
        t = self.engine.clip_text(ids, mask)
        i = self._image_emb(pil, check=False)
        sim = float((t * i).sum().item())
        # the cosine is non-finite iff either embedding overflowed an fp16 stream: checked on the value
        # read back anyway (no isfinite launches); then both are re-run on fp32 streams.  (Not rerun_if: the
        # re-run differs from the first run -- it drops the cached embedding and checks the new one itself)
        if not math.isfinite(sim) and self.engine.clip_stream_overflow(np.array([sim])):
            self._emb_cache = None
            t = self.engine.clip_text(ids, mask)
            i = self._image_emb(pil)
            sim = float((t * i).sum().item())
        return {"clip_similarity": sim}

    def search_vault(self, image_path, user_caption: str = None, top_k: int = 5) -> Dict:
        """misinfo_forensics.py:410-491."""
        if not self.vault_loaded:
            return {"vault_discrepancy": 0.0, "matches": [], "vault_available": False, "text_similarity": 0.0}
        q = self._image_emb(io_utils.to_pil(image_path))
        temb = None
        if user_caption:
            ids, mask = self._clip_ids([user_caption], truncation=True)
            temb = rerun_if(self.engine.clip_stream_overflow, lambda: self.engine.clip_text(ids, mask))
        k = len(range(len(self.vault_metadata))[-top_k:])  # np.argsort(s)[-top_k:] keeps this many rows
        if k == 0:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")  # top_similarities[0]
        sims, idx, disc, tsim = self.engine.vault_topk(q, k, 0.85, temb)
        return self._vault_dict(sims.cpu().numpy()[0], idx.cpu().numpy()[0], float(disc.item()),
                                float(tsim.item()) if user_caption else 0.0)

    def _vault_dict(self, sims, idx, disc, tsim) -> Dict:
        matches = [{"similarity": float(s), "title": self.vault_metadata[int(i)]["title"],
                    "url": self.vault_metadata[int(i)].get("url", "N/A"),
                    "date": self.vault_metadata[int(i)].get("date", "N/A")} for s, i in zip(sims, idx) if i >= 0]
        return {"vault_discrepancy": disc, "matches": matches, "vault_available": True,
                "text_similarity": tsim if (matches and float(sims[0]) > 0.85) else 0.0}

    def analyze_video(self, video_path: str, text: Optional[str] = None, max_frames: int = 12,
                      stride_seconds: float = 1.0) -> Dict:
        """misinfo_forensics.py:493-573: frames sampled with OpenCV exactly as the reference does
        (sample_video_frames), then every per-frame signal for all frames in ONE batched launch
        sequence (analyze_frames) instead of 3 x F single-image passes."""
        frames = sample_video_frames(video_path, max_frames, stride_seconds)
        return self.analyze_frames(frames, text=text)

    def analyze_frames(self, frames: Sequence, text: Optional[str] = None) -> Dict:
        """The per-frame part of analyze_video (misinfo_forensics.py:540-573) over F frames (PIL
        images, paths or uint8 HWC arrays): EfficientNet, the CLIP image tower and the Truth-Vault
        top-5 run once over the F-frame batch; the caption's CLIP text embedding once.
        Aggregation as the reference: mean deepfake score, mean CLIP similarity (0.0 without
        text), and the vault result of the FIRST frame whose discrepancy strictly exceeds every
        earlier one (running best starts at 0.0)."""
        if len(frames) == 0:
            raise RuntimeError("No frames could be read from the video.")
        pils = [io_utils.to_pil(io_utils.Image.fromarray(f) if isinstance(f, np.ndarray) else f) for f in frames]
        eff = np.stack([io_utils.effnet_pixels(p) for p in pils])
        clp = np.stack([io_utils.clip_pixels(p) for p in pils])
        F = len(pils)
        self.detector.sync(("effnet",))
        cap = self.engine.max_batch  # frames beyond the reserved batch run as further launches

        def deepfake_scores():
            return torch.cat([self.engine.effnet_forward(eff[i:i + cap])[1] for i in range(0, F, cap)])

        def image_embs():
            return torch.cat([self.engine.clip_image(clp[i:i + cap]) for i in range(0, F, cap)])
        dsc = rerun_if(self.engine.effnet_overflow, deepfake_scores, lambda d: d.cpu().numpy())
        iemb = rerun_if(self.engine.clip_stream_overflow, image_embs)
        clip_mean = 0.0
        temb_vault = None
        if text:
            ids, mask = self._clip_ids([text])  # analyze_consistency: no truncation (Q8)
            temb = self.engine.clip_text(ids, mask)
            if self.engine.clip_stream_overflow(temb):  # (not rerun_if: the image tower runs again as well)
                temb = self.engine.clip_text(ids, mask)
                iemb = image_embs()
            # per-frame fp32 cosines (the reference's .item()), mean over python floats
            clip_mean = float(np.mean([float(v) for v in (iemb * temb).sum(1).cpu().numpy()]))
            tids, tmask = self._clip_ids([text], truncation=True)  # search_vault's caption
            temb_vault = temb if np.array_equal(tids, ids) else self.engine.clip_text(tids, tmask)
        best = {"vault_discrepancy": 0.0, "matches": [], "vault_available": self.vault_loaded, "text_similarity": 0.0}
        best_frame = None
        if self.vault_loaded:
            te = temb_vault.expand(F, -1).contiguous() if temb_vault is not None else None
            k = min(5, len(self.vault_metadata))
            parts = [self.engine.vault_topk(iemb[i:i + cap], k, 0.85, None if te is None else te[i:i + cap])
                     for i in range(0, F, cap)]
            sims, idx, disc, tsim = (torch.cat([p[j] for p in parts]).cpu().numpy() for j in range(4))
            for f in range(F):
                if float(disc[f]) > float(best["vault_discrepancy"]):
                    best = self._vault_dict(sims[f], idx[f], float(disc[f]), float(tsim[f]) if text else 0.0)
                    best_frame = pils[f]
        return {"deepfake_score": float(np.mean([float(v) for v in dsc.cpu().numpy()])),
                "clip_similarity": clip_mean,
                "vault_discrepancy": float(best.get("vault_discrepancy", 0.0)),
                "text_similarity": float(best.get("text_similarity", 0.0)),
                "vault_matches": best.get("matches", []), "best_frame": best_frame}

    def fusion_verdict(self, scores: Dict[str, float]) -> Dict:
        """misinfo_forensics.py:575-615 on the HIP fusion kernel."""
        self.detector.sync(("fusion",))
        x = np.array([[scores.get(k, 0.0) for k in SCORE_KEYS]], dtype=np.float32)
        probs, verdict, conf, _ = self.engine.fusion(x)
        p = probs.cpu().numpy()[0]
        return {"verdict": int(verdict.item()), "confidence": float(conf.item()),
                "fake_probability": float(p[1]), "real_probability": float(p[0])}

    def build_gemini_prompt(self, all_scores: Dict, vault_matches: list) -> str:
        return explain.gemini_prompt(all_scores, vault_matches)

    def generate_gemini_explanation(self, all_scores: Dict, vault_matches: list) -> str:
        """misinfo_forensics.py:695-740: Gemini is a network service -> rule-based fallback."""
        if not self.gemini_available:
            self._log("  ℹ Using fallback explanation (Gemini not available)")
        return self._generate_fallback_explanation(all_scores, vault_matches)

    def _generate_fallback_explanation(self, all_scores: Dict, vault_matches: list) -> str:
        return explain.fallback_explanation(all_scores, vault_matches)

    # ------------------------------------------------------------------ analyze
    def analyze(self, text: Optional[str] = None, image_path: Optional[str] = None,
                video_path: Optional[str] = None, verbose: bool = True) -> Dict:
        """misinfo_forensics.py:767-927 (same result dict)."""
        if not text and not image_path and not video_path:
            raise ValueError("Provide at least one of: text, image_path, or video_path")
        if text and image_path and not video_path:
            return self.analyze_pairs([text], [image_path])[0]  # the batched 5-signal path
        text_scores = {"ai_score": 0.0, "misinfo_score": 0.0}
        image_scores = {"deepfake_score": 0.0}
        cons = {"clip_similarity": 0.0}
        vault = {"vault_discrepancy": 0.0, "matches": [], "vault_available": self.vault_loaded,
                 "text_similarity": 0.0}
        if text:
            text_scores = self.analyze_text(text)
        if video_path:  # misinfo_forensics.py:812-829 (the video takes precedence over an image)
            vs = self.analyze_video(video_path, text=text)
            image_scores["deepfake_score"] = vs.get("deepfake_score", 0.0)
            cons["clip_similarity"] = vs.get("clip_similarity", 0.0)
            vault["vault_discrepancy"] = vs.get("vault_discrepancy", 0.0)
            vault["matches"] = vs.get("vault_matches", [])
            vault["text_similarity"] = vs.get("text_similarity", 0.0)
        elif image_path:
            image_scores = self.analyze_image(image_path)
            vault = self.search_vault(image_path, user_caption=text)
        all_scores = {**text_scores, **image_scores, **cons, "vault_discrepancy": vault["vault_discrepancy"],
                      "text_similarity": vault.get("text_similarity", 0.0)}
        if text and (image_path or video_path):  # use_fusion (misinfo_forensics.py:879-881)
            vr = self.fusion_verdict(all_scores)
        else:
            if text:
                fake = float(all_scores.get("misinfo_score", 0.0))
            else:
                fake = float(max(all_scores.get("deepfake_score", 0.0), all_scores.get("vault_discrepancy", 0.0)))
            fake = max(0.0, min(1.0, fake))
            label = 1 if fake > 0.5 else 0
            vr = {"verdict": label, "confidence": fake if label == 1 else 1.0 - fake,
                  "fake_probability": fake, "real_probability": 1.0 - fake}
        all_scores.update(vr)
        exp = self.generate_gemini_explanation(all_scores, vault["matches"])
        return {"verdict": vr["verdict"], "verdict_text": "FAKE" if vr["verdict"] == 1 else "REAL",
                "confidence": vr["confidence"], "scores": all_scores, "vault_matches": vault["matches"],
                "explanation": exp}

    def analyze_pairs(self, texts: List[str], images: List) -> List[Dict]:
        """Batched analyze() for text+image pairs: one analyze_batch launch sequence per
        `max_batch` pairs, then the reference's result dicts (one per pair, in order).  The host
        stage of chunk i + 1 (tokenisation, threaded image decode) runs on a helper thread while
        chunk i is resampled, analysed on the device and turned into dicts."""
        if len(texts) != len(images):
            raise ValueError(f"{len(texts)} texts vs {len(images)} images")
        cap = self.engine.max_batch
        chunks = [(i, min(i + cap, len(texts))) for i in range(0, len(texts), cap)]
        if not chunks:
            return []

        self._ensure_jpeg_stager()

        def host_stage(a, b):
            # (tokenising on a third thread while the images decode measured a tie for one chunk and
            # 33 % slower for four: DESIGN §6)
            rob = io_utils.tokenize_roberta_batch(self.roberta_tokenizer, texts[a:b])
            rid, rm = io_utils.pad_ids(rob, W.ROBERTA["pad_id"])
            cid, cm = self._clip_ids(list(texts[a:b]))
            return rid, rm, cid, cm, self._stage_images(images[a:b])

        res: List[Dict] = []

        def device_part(staged):
            rid, rm, cid, cm, rgb = staged
            self._fit_text(rid.shape[1])
            eff, clp = self._windows(*rgb)
            # run-time precision traps on the results already read back (no device launch: analyze()
            # at B = 1 -0.2 ms): a non-finite text score / deepfake score / clip_similarity (the cosine
            # of the two CLIP embeddings; a zero vault row's NaN stays in top_sims) means an fp16
            # stream overflowed -- that tower switches precision and the batch runs again
            out = rerun_if(self.engine.scores_overflow,
                           lambda: self.batch_to_host(self.analyze_batch(rid, rm, cid, cm, eff, clp)),
                           lambda o: o["scores"])
            res.extend(self.batch_to_dicts(out))

        self._run_chunks(chunks, host_stage, device_part)
        return res

    def _ensure_jpeg_stager(self) -> None:
        if self.device_jpeg and self._jpeg is None:
            from . import jpeg
            self._jpeg = jpeg.JpegStager()

    def _stage_images(self, images) -> Tuple:
        """Host stage of a chunk's images, the argument tuple of _windows.  JPEG bytes / files:
        entropy-decoded here, reconstructed on the device; everything else decoded by Pillow
        (pixels); the resampling to both towers' windows runs on the device."""
        st = None
        rest = list(range(len(images)))
        if self.device_jpeg:
            from . import jpeg
            st = self._jpeg.stage([jpeg.read_bytes(x) for x in images])
            done = set(st.index)
            rest = [i for i in rest if i not in done]
        rgb = io_utils.decode_rgb([images[i] for i in rest]) if rest else []
        return len(images), st, rest, rgb

    @staticmethod
    def _run_chunks(chunks, host_stage, device_part) -> None:
        """device_part(host_stage(a, b)) per chunk (a, b), in order; the host stage of chunk i + 1 on a
        helper thread while chunk i is on the device."""
        if len(chunks) == 1:  # nothing to overlap: no staging thread (analyze(): one pair per call)
            device_part(host_stage(*chunks[0]))
            return
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as ex:
            fut = ex.submit(host_stage, *chunks[0])
            for k in range(len(chunks)):
                staged = fut.result()
                if k + 1 < len(chunks):
                    fut = ex.submit(host_stage, *chunks[k + 1])
                device_part(staged)

    def analyze_many(self, texts: List[Optional[str]], images: List) -> List[Dict]:
        """Batched analyze() for a feed of posts where each has a text, an image or both: texts[i] /
        images[i] that is None or empty is absent (the reference's truthiness test,
        misinfo_forensics.py:793-811).  One analyze_mixed launch sequence per `max_batch` posts -- each
        tower runs only on the rows that have its modality -- then the reference's result dict per
        post, in order (rows without an image report no vault matches).  Chunking, the staging thread
        and the device JPEG decode / resampling of the images are analyze_pairs'.  A post with neither
        raises the reference's ValueError before anything is tokenised, decoded or launched."""
        if len(texts) != len(images):
            raise ValueError(f"{len(texts)} texts vs {len(images)} images")

        def present(x) -> bool:
            if x is None:
                return False
            return len(x) > 0 if isinstance(x, (str, bytes, bytearray)) else True
        mod = np.array([int(present(t)) | int(present(i)) << 1 for t, i in zip(texts, images)], np.uint8)
        if (mod == 0).any():
            raise ValueError(NO_INPUT_ERROR)
        cap = self.engine.max_batch
        chunks = [(i, min(i + cap, len(texts))) for i in range(0, len(texts), cap)]
        if not chunks:
            return []
        self._ensure_jpeg_stager()

        def host_stage(a, b):
            m = mod[a:b]
            tx = [texts[a + i] for i in np.flatnonzero(m & 1)]    # the text rows, in batch order
            both = [texts[a + i] for i in np.flatnonzero(m == 3)]  # the rows with both
            im = [images[a + i] for i in np.flatnonzero(m & 2)]    # the image rows
            rid = rm = cid = cm = None
            if tx:
                rob = io_utils.tokenize_roberta_batch(self.roberta_tokenizer, tx)
                rid, rm = io_utils.pad_ids(rob, W.ROBERTA["pad_id"])
            if both:
                cid, cm = self._clip_ids(both)
            return m, rid, rm, cid, cm, (self._stage_images(im) if im else None)

        res: List[Dict] = []

        def device_part(staged):
            m, rid, rm, cid, cm, rgb = staged
            if rid is not None:
                self._fit_text(rid.shape[1])
            eff, clp = self._windows(*rgb) if rgb is not None else (None, None)
            # the run-time precision traps of analyze_pairs on the scores read back (an absent signal's
            # 0 is finite)
            out = rerun_if(self.engine.scores_overflow,
                           lambda: self.batch_to_host(self.analyze_mixed(m, rid, rm, cid, cm, eff, clp)),
                           lambda o: o["scores"])
            res.extend(self.batch_to_dicts(out, modality=m))

        self._run_chunks(chunks, host_stage, device_part)
        return res

    def _windows(self, n: int, st, rest: List[int], rgb: List[np.ndarray]):
        """Both towers' windows of a chunk: device-decoded JPEGs (st) and Pillow-decoded pixels
        (rest, rgb) merged back into input order."""
        if st is None or not st.index:
            return self._resize(rgb)
        from . import jpeg
        e1, c1 = jpeg.device_windows(self.engine, self._jpeg, st)
        if not rest:
            return e1, c1
        eff = torch.empty((n, 224, 224, 3), dtype=torch.uint8, device=self.device)
        clp = torch.empty_like(eff)
        sel = torch.as_tensor(st.index, device=self.device)
        eff[sel], clp[sel] = e1, c1
        e2, c2 = self._resize(rgb)
        sel = torch.as_tensor(rest, device=self.device)
        eff[sel], clp[sel] = e2, c2
        return eff, clp

    def _resize(self, rgb: List[np.ndarray]):
        """Both towers' 224x224 windows of decoded images: Pillow-exact on the device
        (mmf_resize_pil); only images past its tap budget (a > 23x CLIP downscale, shortest side
        above ~5264 px) are resampled by Pillow on the host, the rest of the chunk stays on the
        device.  Any other device error propagates."""
        ok = [self.engine.resize_supported(a.shape[1], a.shape[0]) for a in rgb]
        if all(ok):
            return self.engine.resize_images(rgb)
        dev = self.device
        eff = torch.empty((len(rgb), 224, 224, 3), dtype=torch.uint8, device=dev)
        clp = torch.empty_like(eff)
        on_dev = [i for i, o in enumerate(ok) if o]
        on_host = [i for i, o in enumerate(ok) if not o]
        if on_dev:
            e, c = self.engine.resize_images([rgb[i] for i in on_dev])
            sel = torch.as_tensor(on_dev, device=dev)
            eff[sel], clp[sel] = e, c
        he, hc = io_utils.decode_batch([io_utils.Image.fromarray(np.ascontiguousarray(rgb[i][..., :3]))
                                        for i in on_host])
        sel = torch.as_tensor(on_host, device=dev)
        eff[sel], clp[sel] = torch.as_tensor(he).to(dev), torch.as_tensor(hc).to(dev)
        return eff, clp

    def analyze_batch(self, rob_ids, rob_mask, clip_ids, clip_mask, images_u8, clip_images_u8=None,
                      out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Tensor entry point (the benchmark's unit of work): pre-tokenised ids and uint8
        [B,224,224,3] images -> device tensors {scores [B,5], probs [B,2], verdict, confidence,
        rule, text_similarity, top_sims [B,5], top_idx [B,5]}."""
        self.detector.sync()
        return self.engine.analyze_batch(rob_ids, rob_mask, clip_ids, clip_mask, images_u8, clip_images_u8, out=out)

    def analyze_mixed(self, modality, rob_ids, rob_mask, clip_ids, clip_mask, images_u8, clip_images_u8=None,
                      out: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Tensor entry point for posts with a text, an image or both, next to analyze_batch:
        modality [B] (1 text, 2 image, 3 both) and COMPACT inputs -- ids of the text rows, uint8
        [nI,224,224,3] windows of the image rows, CLIP ids of the rows with both (a list without rows
        may be None) -> analyze_batch's dict of [B, ...] device tensors in batch order."""
        self.detector.sync()
        return self.engine.analyze_mixed(modality, rob_ids, rob_mask, clip_ids, clip_mask, images_u8, clip_images_u8,
                                         out=out)

    @staticmethod
    def batch_to_host(out: Dict[str, torch.Tensor]) -> Dict[str, np.ndarray]:
        return {k: v.cpu().numpy() for k, v in out.items()}

    def batch_to_dicts(self, out: Dict, modality=None) -> List[Dict]:
        """The reference's result dicts from analyze_batch's outputs (device tensors or their
        batch_to_host copies); modality (analyze_mixed's, per row): a row without an image reports no
        vault matches."""
        o = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
        res = []
        for b in range(o["scores"].shape[0]):
            s = o["scores"][b]
            searched = self.vault_loaded and (modality is None or int(modality[b]) & 2)
            vault = (self._vault_dict(o["top_sims"][b], o["top_idx"][b], float(s[4]), float(o["text_similarity"][b]))
                     if searched else {"vault_discrepancy": 0.0, "matches": [], "text_similarity": 0.0})
            all_scores = {"ai_score": float(s[0]), "misinfo_score": float(s[1]), "deepfake_score": float(s[2]),
                          "clip_similarity": float(s[3]), "vault_discrepancy": float(s[4]),
                          "text_similarity": float(vault.get("text_similarity", 0.0)),
                          "verdict": int(o["verdict"][b]), "confidence": float(o["confidence"][b]),
                          "fake_probability": float(o["probs"][b][1]), "real_probability": float(o["probs"][b][0])}
            exp = explain.fallback_explanation(all_scores, vault["matches"], int(o["rule"][b]))
            res.append({"verdict": all_scores["verdict"],
                        "verdict_text": "FAKE" if all_scores["verdict"] == 1 else "REAL",
                        "confidence": all_scores["confidence"], "scores": all_scores,
                        "vault_matches": vault["matches"], "explanation": exp})
        return res


# ---------------------------------------------------------------------------------------------
# CLIPSimilarityEngine
# ---------------------------------------------------------------------------------------------
class CLIPSimilarityEngine:
    """clip_similarity_engine.py:13-174 on the HIP CLIP towers."""

    def __init__(self, model_name="openai/clip-vit-base-patch32", threshold=0.25, *, processor=None,
                 clip_state=None, synthetic_seed: Optional[int] = None, device: str = "cuda"):
        print(f"Loading CLIP model: {model_name}...")
        try:
            self.device = str(_require_hip(device))
            if clip_state is None:
                if synthetic_seed is not None:
                    clip_state = W.synthetic_clip_state(synthetic_seed)
                else:
                    from transformers import CLIPModel
                    clip_state = dict(CLIPModel.from_pretrained(model_name, local_files_only=True).state_dict())
            if processor is None:
                from transformers import CLIPProcessor
                processor = CLIPProcessor.from_pretrained(model_name, local_files_only=True)
            self.processor = processor
            self.threshold = threshold
            self.model = Engine(torch.device(self.device).index or 0, None, clip_state, max_batch=64,
                                eos_token_id=clip_eos_token_id(model_name))
            print(f"Model loaded successfully on {self.device}")
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(f"Failed to load CLIP model: {str(e)}")

    def load_image(self, image_path):
        if not os.path.exists(image_path):
            raise FileNotFoundError(f"Image file not found: {image_path}")
        try:
            from PIL import Image
            image = Image.open(image_path)
            if image.mode != "RGB":
                image = image.convert("RGB")
            return image
        except Exception as e:  # noqa: BLE001
            raise ValueError(f"Failed to load image from {image_path}: {str(e)}")

    def calculate_similarity(self, image_path, text):
        try:
            image = self.load_image(image_path)
            if not text or not isinstance(text, str):
                raise ValueError("Text input must be a non-empty string")
            seqs = io_utils.tokenize_clip(self.processor, [text])
            ids, mask = io_utils.pad_ids(seqs, self.model.eos_token_id)
            px = io_utils.clip_pixels(image)[None]
            # (an overflowed fp16 stream: both towers once more on fp32 streams)
            t, i = rerun_if(lambda ti: self.model.clip_stream_overflow(*ti),
                            lambda: (self.model.clip_text(ids, mask), self.model.clip_image(px)))
            similarity = float((i * t).sum().item())
            label = "Match" if similarity >= self.threshold else "Mismatch"
            return similarity, label
        except (FileNotFoundError, ValueError):
            raise
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(f"Error calculating similarity: {str(e)}")

    def analyze_with_explanation(self, image_path, text):
        try:
            similarity, label = self.calculate_similarity(image_path, text)
            return {"image_path": image_path, "text": text, "similarity_score": round(similarity, 4),
                    "label": label, "explanation": self._generate_explanation(similarity, label)}
        except Exception as e:  # noqa: BLE001
            return {"image_path": image_path, "text": text, "error": str(e)}

    def _generate_explanation(self, similarity, label):
        return explain.clip_engine_explanation(similarity, label)
