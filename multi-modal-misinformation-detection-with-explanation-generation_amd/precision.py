"""The reduced-precision policy of the three guarded towers: fp16 or split RoBERTa, the fp16 EfficientNet
tower, fp16 CLIP residual streams.  Each tower is guarded twice: a load-time calibration measures the fast
mode against its fallback on seeded inputs and keeps the fast mode if it is within tolerance, and a run-time
trap switches the tower to the fallback for good when a value read back from it is non-finite (the caller
then runs the batch once more: rerun_if).

Pure host logic.  A guard reaches the engine only through get_option / set_option, max_batch /
max_text_len / max_clip_len, device (where the seeded inputs are put, once) and the forwards it measures
(text_forward, effnet_forward, clip_image, clip_text), so a stub without a device can stand in for it
(tests/test_precision_cpu.py).  The ledger and the guards hold the engine that owns them weakly: no reference
cycle keeps a dropped engine, and the device memory its __del__ frees, waiting for the cyclic collector."""
from __future__ import annotations

import itertools
import os
import weakref

import numpy as np
import torch


def all_finite(v) -> bool:
    """A host array is checked on the host (no device launch or extra synchronisation), a device tensor
    with torch.isfinite."""
    return bool(torch.isfinite(v).all()) if isinstance(v, torch.Tensor) else bool(np.isfinite(np.asarray(v)).all())


def rerun_if(trap, run, probe=None):
    """run(); if trap(probe(result)) -- trap(result) without a probe -- reports that a tower switched
    precision, run() once more.  Returns the last result."""
    result = run()
    if trap(result if probe is None else probe(result)):
        result = run()
    return result


class OptionLedger:
    """The options the engine itself wrote, so that a user's later set_option reads as a pin."""

    def __init__(self, engine):
        self.engine = weakref.proxy(engine)
        self.written = {}

    def write(self, name: str, value: int) -> None:
        """The engine writes the option and records the value."""
        self.engine.set_option(name, value)
        self.written[name] = int(value)

    def record(self, name: str) -> None:
        """The engine records the option's current value as its own, without writing."""
        self.written[name] = self.engine.get_option(name)

    def changed(self, name: str) -> bool:
        """True when the option was changed since the engine last wrote or recorded it (a user pin)."""
        return name in self.written and self.engine.get_option(name) != self.written[name]

    def last(self, name: str, default=None):
        """The value the engine last wrote or recorded for the option (default: it never did)."""
        return self.written.get(name, default)


class _PinnableGuard:
    """What the text and EfficientNet guards share: the user's precision choice and the pin predicate that
    both the calibration and the trap consult."""
    OPTION = ENV = None

    def __init__(self, engine, ledger: OptionLedger, choice: str):
        self.engine, self.ledger, self.check = weakref.proxy(engine), ledger, None
        # an environment value pins the tower under "auto": no calibration or trap overrides it
        self.choice = "pinned" if choice == "auto" and os.environ.get(self.ENV) else choice

    def pinned(self) -> bool:
        """The constructor's choice is not "auto", the tower's environment variable was set under "auto",
        or the user changed the option after the engine's last write."""
        return self.choice != "auto" or self.ledger.changed(self.OPTION)

    def _pinned_check(self, key: str) -> dict:
        self.check = {key: self.choice if self.choice != "auto" else "pinned", "calibrated": False}
        return self.check


# RoBERTa precise-mode GEMM kinds (option text_prec_mask: bit k = kind k on hi / lo activations, bit k + 4 =
# also on W_lo; kinds QKV, out-proj, FFN-1, FFN-2) and their relative GEMM cost (the K loop is 1x / 2x /
# 3x): the calibration keeps the cheapest mask within TextGuard.TOL of the full mode (255)
PREC_KIND_COST = (3, 1, 4, 4)
PREC_FULL = 255


def mask_cost(m: int) -> int:
    return sum(c * (1 + (m >> k & 1) + (m >> k & 1) * (m >> (k + 4) & 1)) for k, c in enumerate(PREC_KIND_COST))


def prec_masks():
    """Every operand mask below the full mode, cheapest first (3 levels per kind)."""
    ms = [sum((lv >= 1) << k | (lv == 2) << (k + 4) for k, lv in enumerate(lvls))
          for lvls in itertools.product((0, 1, 2), repeat=4)]
    return sorted((m for m in ms if m != PREC_FULL), key=lambda m: (mask_cost(m), m))


class TextGuard(_PinnableGuard):
    """RoBERTa: the fast layout (fp16 or split stream, from the LayerNorm bound) against the precise mode."""
    OPTION, ENV = "text_hilo", "MMF_TEXT_HILO"
    # choice -> option text_hilo (csrc/text_host.cpp run_text / run_text_precise): "auto" = the
    # LayerNorm-bound layout (-1) unless the calibration selects "precise"; the others pin the mode
    # ("fp16" / "split" also skip packing the precise weights)
    CHOICES = {"auto": -1, "fp16": 0, "split": 1, "precise": 2}
    # largest tolerated change of ai_score / misinfo_score between the fast layout and the precise mode on
    # the calibration texts (half the north-star bar)
    TOL = 5e-4

    def __init__(self, engine, ledger, choice="auto"):
        super().__init__(engine, ledger, choice)
        if self.choice != "pinned":
            ledger.write("text_hilo", self.CHOICES[choice])

    def calibrate(self, n: int = 64) -> dict:
        """Load-time selection of the text mode.  The fp16-operand design holds 1e-3 only while the
        LayerNorms do not amplify operand rounding: a checkpoint with one channel dominating every
        LayerNorm (gamma ~7: DESIGN.md §4) moves the scores by 1.6e-3 even on the split stream.  Unless the
        tower is pinned, on n seeded texts of 128 tokens:
          1. the fast layout against the full precise mode (fp32 stream / LayerNorm / attention, every GEMM
             on ~22-bit hi / lo operands); within TOL on every score -> the fast layout, and the precise
             weights are released (the run-time trap falls back to the precise mode on fp16 operands,
             which needs none of them);
          2. otherwise every cheaper operand mask (option text_prec_mask: which GEMM kinds read hi / lo
             operands, the rest fp16) against the full mode; the cheapest within TOL is selected and only
             its kinds' weights stay packed.
        A pinned tower (pinned()) is left alone.  Returns (and keeps as `check`) the result."""
        from . import synthetic as syn
        eng = self.engine
        if self.pinned():
            return self._pinned_check("mode")
        self.ledger.write("text_hilo", -1)
        n = max(1, n)
        L = min(128, eng.max_text_len)
        ids, mask = syn.roberta_ids(n, L, 6007, [L, L // 2, 17, 5])

        def scores():
            return torch.cat([eng.text_forward(ids[i:i + eng.max_batch], mask[i:i + eng.max_batch])[2].double()
                              for i in range(0, n, eng.max_batch)])

        def dist(a, b):
            return float((a - b).abs().max()) if all_finite(a) else float("inf")
        names = {0: "fp16", 1: "split", 2: "precise"}
        fast = scores()
        fast_mode = eng.get_option("text_hilo_effective")
        packed = eng.get_option("text_precise_packed")
        if packed != 15:  # (weights packed under a pinned layout: nothing to compare against)
            self.check = {"mode": names[fast_mode], "calibrated": False, "precise_packed": packed}
            return self.check
        eng.set_option("text_prec_mask", PREC_FULL)
        self.ledger.write("text_hilo", 2)
        full = scores()
        d = dist(fast, full)
        self.check = {"max_dscore": d, "fast_layout": names[fast_mode], "texts": n, "calibrated": True}
        if d <= self.TOL:
            self.ledger.write("text_hilo", -1)
            eng.set_option("text_precise_packed", 0)  # the +510 MB go when the mode is not used
            self.check["mode"] = names[fast_mode]
            return self.check
        tried = {}
        best = PREC_FULL
        for m in prec_masks():
            eng.set_option("text_prec_mask", m)
            tried[m] = dist(scores(), full)
            if tried[m] <= self.TOL:
                best = m
                break
        eng.set_option("text_prec_mask", best)
        eng.set_option("text_precise_packed", best & 15)
        self.check.update(mode="precise", prec_mask=best, mask_dscore=tried,
                          cost_vs_full=mask_cost(best) / mask_cost(PREC_FULL))
        return self.check

    def overflow(self, scores) -> bool:
        """Run-time overflow trap of the fast layouts.  The calibration bounds the drift on its seeded
        texts; an input whose branch output passes fp16's range (a token driving an FFN-2 row past 65504)
        turns that text's scores non-finite.  Given text scores the caller already read back: if a fast
        layout is selected and any is non-finite, the engine switches to the precise mode for good (fp32
        stream and branch outputs; hi / lo operands for the kinds still packed, fp16 for the rest) and
        returns True, and the caller re-runs the batch.  A pinned tower (pinned(): the calibration's own
        predicate) is left alone: nothing is written and its scores stay non-finite."""
        eng = self.engine
        if eng.get_option("text_hilo_effective") >= 2 or self.pinned() or all_finite(scores):
            return False
        packed = eng.get_option("text_precise_packed")
        eng.set_option("text_prec_mask", packed | packed << 4)
        self.ledger.write("text_hilo", 2)
        self.check = dict(self.check or {}, mode="precise", runtime_overflow=True,
                          prec_mask=eng.get_option("text_prec_mask"))
        return True


class EffnetGuard(_PinnableGuard):
    """EfficientNet: the fp16 tower against the fp32 tower."""
    OPTION, ENV = "effnet_fp32", "MMF_EFFNET_FP32"
    CHOICES = ("auto", "fp16", "fp32")
    # largest tolerated change of deepfake_score against the fp32 tower on the calibration images (half the
    # north-star bar; the ordinary draw measures ~1e-4 over 256)
    TOL = 5e-4

    def __init__(self, engine, ledger, choice="auto"):
        super().__init__(engine, ledger, choice)
        if self.choice == "auto":
            ledger.record("effnet_fp32")

    def calibrate(self, n: int = 64) -> dict:
        """Load-time guard of the fp16 tower.  A BN-conditioned tower is insensitive to fp16 activation
        storage; a chaotic one (logits of O(100): He-gain draws) amplifies it to O(0.1).
        Unless the tower is pinned, both towers run on n seeded calibration images; if any deepfake_score
        is non-finite or moves by more than TOL, the fp32 tower stays selected.  The choices "fp16" /
        "fp32" select their tower here without measuring; any other pin is left alone.  Returns (and keeps
        as `check`) the result."""
        from . import synthetic as syn
        eng = self.engine
        if self.pinned():
            if self.choice in ("fp16", "fp32"):
                eng.set_option("effnet_fp32", int(self.choice == "fp32"))
            return self._pinned_check("tower")
        n = max(1, n)
        imgs = torch.from_numpy(syn.images(n, 5003)).to(eng.device)

        def scores(fp32: int):
            self.ledger.write("effnet_fp32", fp32)
            return torch.cat([eng.effnet_forward(imgs[i:i + eng.max_batch])[1].double()
                              for i in range(0, n, eng.max_batch)])
        s16, s32 = scores(0), scores(1)
        finite = all_finite(s16)
        d = float((s16 - s32).abs().max()) if finite else float("inf")
        ok = finite and d <= self.TOL
        self.ledger.write("effnet_fp32", 0 if ok else 1)
        self.check = {"max_ddeepfake": d, "tower": "fp16" if ok else "fp32", "images": n, "calibrated": True}
        return self.check

    def overflow(self, scores) -> bool:
        """Run-time overflow trap of the fp16 tower: given deepfake scores the caller already read back, a
        non-finite one under the fp16 tower switches the engine to the fp32 tower for good and returns True
        (the caller re-runs the batch).  An image whose activation passes fp16's range (a saturated colour
        on a high-gain stem channel) is what the calibration on seeded images cannot see.  A pinned tower
        is left alone."""
        if self.engine.get_option("effnet_fp32") != 0 or self.pinned() or all_finite(scores):
            return False
        self.ledger.write("effnet_fp32", 1)
        self.check = dict(self.check or {}, tower="fp32", runtime_overflow=True)
        return True


class ClipStreamGuard:
    """CLIP: fp16 residual streams (option clip_res16) against fp32 streams.  No pin concept."""
    # largest tolerated change of an image-text cosine (the quantity clip_similarity and the vault scores
    # are made of) between fp16 and fp32 residual streams -- half of the north-star 1e-3 (the ordinary
    # synthetic draw measures 2.3e-4, an outlier-feature draw 1.3e-4)
    TOL = 5e-4

    def __init__(self, engine):
        self.engine, self.check = weakref.proxy(engine), None

    def calibrate(self, n: int = 8) -> dict:
        """Load-time guard of the fp16 streams.  The pre-LN stream is a running sum, so unlike RoBERTa's
        post-LN stream no LayerNorm parameter bounds it: trained weights with outlier features can push it
        past fp16's range (65504) or far enough up that its rounding matters.  A calibration forward
        measures it: both CLIP towers on n seeded images / captions with fp16 streams and again with fp32
        streams; if an embedding is non-finite or any of the n x n image-text cosines moves by more than
        TOL, the fp32 streams stay selected.  Returns (and keeps as `check`) the measured change."""
        from . import synthetic as syn
        eng = self.engine
        if eng.get_option("clip_res16") != 1:
            return self.check or {}
        n = max(1, min(n, eng.max_batch))
        imgs = torch.from_numpy(syn.images(n, 4099)).to(eng.device)
        ids, mask = syn.clip_ids(n, min(77, eng.max_clip_len), 4099)

        def cosines():
            e = eng.clip_image(imgs).double()
            t = eng.clip_text(ids, mask).double()
            return e, t, e @ t.T  # unit rows: cosines
        e16, t16, c16 = cosines()
        eng.set_option("clip_res16", 0)
        e32, t32, c32 = cosines()
        finite = all_finite(e16) and all_finite(t16)
        dcos = float((c16 - c32).abs().max()) if finite else float("inf")
        demb = float(max((e16 - e32).abs().max(), (t16 - t32).abs().max())) if finite else float("inf")
        ok = finite and dcos <= self.TOL
        if ok:
            eng.set_option("clip_res16", 1)
        self.check = {"max_dcos": dcos, "max_demb": demb, "fp16_streams": ok, "rows": n}
        return self.check

    def overflow(self, *outputs) -> bool:
        """Run-time overflow trap of the fp16 streams: the calibration measures 8 seeded inputs, so it
        bounds nothing for later ones.  An input that drives a stream past fp16's range turns the embedding
        non-finite, and clip_similarity / the vault scores with it.  The synchronous API paths (which read
        their results back anyway) pass their CLIP outputs here (device tensors, host arrays or None): if
        fp16 streams are selected and any value is non-finite, the engine switches to fp32 streams for good
        and returns True, and the caller re-runs the batch.  Drift short of overflow is what the
        calibration alone covers."""
        if self.engine.get_option("clip_res16") != 1 or all(all_finite(v) for v in outputs if v is not None):
            return False
        self.engine.set_option("clip_res16", 0)
        self.check = dict(self.check or {}, fp16_streams=False, runtime_overflow=True)
        return True


def scores_overflow(text: TextGuard, effnet: EffnetGuard, clip: ClipStreamGuard, scores5) -> bool:
    """All three run-time traps on an analyze_batch result read back to the host ([B, 5]: ai, misinfo,
    deepfake, clip_similarity, vault): True when any tower switched precision (the caller re-runs the batch
    once).  Every trap is consulted, also after the first fires."""
    s = np.asarray(scores5)
    if all_finite(s[:, :4]):  # (no trap fires on finite values: one host check instead of three and their option reads)
        return False
    hits = [text.overflow(s[:, :2]), effnet.overflow(s[:, 2]), clip.overflow(s[:, 3])]
    return any(hits)
