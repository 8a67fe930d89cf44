"""The precision policy (mmf_amd/precision.py) on a stub engine, no device: which states pin a tower, what
each calibration selects and writes for scripted scores, and what each run-time trap writes.  The stub is an
options dict behind get_option / set_option, forwards that return CPU tensors scripted on those options, and
a log of every option write and forward call."""
import numpy as np
import pytest
import torch

from mmf_amd import precision as P

NAN = float("nan")


@pytest.fixture(autouse=True)
def _no_env_pins(monkeypatch):
    monkeypatch.delenv("MMF_TEXT_HILO", raising=False)
    monkeypatch.delenv("MMF_EFFNET_FP32", raising=False)


class StubEngine:
    """text_score(mode, mask) / effnet_score(fp32) script the towers' scores (every row the same value);
    clip16 / clip32 = (image rows, text rows) the CLIP towers return under fp16 / fp32 streams."""
    max_batch, max_text_len, max_clip_len = 8, 128, 77
    device = torch.device("cpu")

    def __init__(self, layout=1, text_score=lambda mode, mask: 0.5, effnet_score=lambda fp32: 0.5,
                 clip16=None, clip32=None, **options):
        self.opts = dict(text_hilo=-1, text_prec_mask=P.PREC_FULL, text_precise_packed=15, effnet_fp32=0,
                         clip_res16=1)
        self.opts.update(options)
        self.layout, self.text_score, self.effnet_score = layout, text_score, effnet_score
        self.clip = {1: clip16, 0: clip32}
        self.log = []

    def get_option(self, name):
        if name == "text_hilo_effective":  # -1 = the layout from the LayerNorm bound
            return self.opts["text_hilo"] if self.opts["text_hilo"] >= 0 else self.layout
        return self.opts[name]

    def set_option(self, name, value):
        self.opts[name] = int(value)
        self.log.append(("set", name, int(value)))

    def text_forward(self, ids, mask):
        self.log.append(("text_forward", len(ids), self.get_option("text_hilo_effective"), self.opts["text_prec_mask"]))
        v = self.text_score(self.get_option("text_hilo_effective"), self.opts["text_prec_mask"])
        return None, None, torch.full((len(ids), 2), v, dtype=torch.float32)

    def effnet_forward(self, img):
        self.log.append(("effnet_forward", len(img), self.opts["effnet_fp32"]))
        return None, torch.full((len(img),), self.effnet_score(self.opts["effnet_fp32"]), dtype=torch.float32)

    def clip_image(self, img):
        self.log.append(("clip_image", len(img), self.opts["clip_res16"]))
        return self.clip[self.opts["clip_res16"]][0][:len(img)]

    def clip_text(self, ids, mask):
        self.log.append(("clip_text", len(ids), self.opts["clip_res16"]))
        return self.clip[self.opts["clip_res16"]][1][:len(ids)]

    def sets(self):
        return [e[1:] for e in self.log if e[0] == "set"]

    def forwards(self, name):
        return [e for e in self.log if e[0] == name]


class Rig:
    """The ledger and the three guards on one stub, built in the engine's order."""

    def __init__(self, stub, text="auto", effnet="auto"):
        self.stub = stub
        self.ledger = P.OptionLedger(stub)
        self.text = P.TextGuard(stub, self.ledger, text)
        self.effnet = P.EffnetGuard(stub, self.ledger, effnet)
        self.clip = P.ClipStreamGuard(stub)

    def scores_overflow(self, scores5):
        return P.scores_overflow(self.text, self.effnet, self.clip, scores5)


# ---------------------------------------------------------------------------------------------- 1. pin table
def _pinned_rigs(monkeypatch, tower, state):
    """(rig, the mode / tower value its calibration reports, the option writes that calibration makes)."""
    if state == "explicit":
        if tower == "text":
            return [(Rig(StubEngine(), text=c), c, []) for c in ("fp16", "split", "precise")]
        return [(Rig(StubEngine(), effnet=c), c, [("effnet_fp32", int(c == "fp32"))]) for c in ("fp16", "fp32")]
    if state == "env":
        monkeypatch.setenv("MMF_TEXT_HILO" if tower == "text" else "MMF_EFFNET_FP32", "1")
        return [(Rig(StubEngine()), "pinned", [])]
    rig = Rig(StubEngine(effnet_fp32=1))  # (the engine's own values: text_hilo -1 written, effnet_fp32 1 recorded)
    rig.stub.set_option(*(("text_hilo", 0) if tower == "text" else ("effnet_fp32", 0)))  # the user's, afterwards
    return [(rig, "pinned", [])]


def test_construction_writes():
    """An explicit text choice is written at construction, an EfficientNet one is not; "auto" EfficientNet
    only records the current value."""
    for choice, v in (("auto", -1), ("fp16", 0), ("split", 1), ("precise", 2)):
        rig = Rig(StubEngine(effnet_fp32=1), text=choice)
        assert rig.stub.sets() == [("text_hilo", v)] and rig.ledger.written == {"text_hilo": v, "effnet_fp32": 1}
        assert rig.text.choice == choice and rig.effnet.choice == "auto"
    for choice in ("fp16", "fp32"):
        rig = Rig(StubEngine(), effnet=choice)
        assert rig.stub.sets() == [("text_hilo", -1)] and rig.ledger.written == {"text_hilo": -1}
        assert rig.effnet.choice == choice


def test_construction_under_environment_pins(monkeypatch):
    monkeypatch.setenv("MMF_TEXT_HILO", "0")
    monkeypatch.setenv("MMF_EFFNET_FP32", "1")
    rig = Rig(StubEngine())
    assert rig.stub.sets() == [] and rig.ledger.written == {}
    assert rig.text.choice == "pinned" and rig.effnet.choice == "pinned"
    rig = Rig(StubEngine(), text="split", effnet="fp16")  # an explicit choice wins over the environment
    assert rig.stub.sets() == [("text_hilo", 1)] and rig.text.choice == "split" and rig.effnet.choice == "fp16"


@pytest.mark.parametrize("state", ["explicit", "env", "set_option"])
@pytest.mark.parametrize("tower", ["text", "effnet"])
def test_pinned_calibration_leaves_the_option(monkeypatch, tower, state):
    for rig, name, writes in _pinned_rigs(monkeypatch, tower, state):
        before = dict(rig.stub.opts)
        rig.stub.log.clear()
        guard = getattr(rig, tower)
        assert guard.pinned()
        check = guard.calibrate()
        assert check == {"mode" if tower == "text" else "tower": name, "calibrated": False} and guard.check is check
        assert rig.stub.sets() == writes  # (only explicit EfficientNet "fp16" / "fp32" writes: its tower)
        assert rig.stub.opts == dict(before, **dict(writes))
        assert not rig.stub.forwards("text_forward") and not rig.stub.forwards("effnet_forward")


@pytest.mark.parametrize("state", ["explicit", "env", "set_option"])
@pytest.mark.parametrize("tower", ["text", "effnet"])
def test_pinned_trap_leaves_the_tower(monkeypatch, tower, state):
    for rig, name, _ in _pinned_rigs(monkeypatch, tower, state):
        if name in ("precise", "fp32"):
            continue  # pinned to the fallback: no fast mode to trap
        guard = getattr(rig, tower)
        guard.calibrate()
        before, check = dict(rig.stub.opts), dict(guard.check)
        rig.stub.log.clear()
        assert guard.overflow(np.array([[0.5, NAN]]) if tower == "text" else np.array([NAN])) is False
        assert rig.stub.sets() == [] and rig.stub.opts == before and guard.check == check


def test_unpinned_traps_on_finite_values():
    rig = Rig(StubEngine())
    rig.stub.log.clear()
    assert rig.text.overflow(np.full((3, 2), 0.5)) is False
    assert rig.effnet.overflow(np.full(3, 0.5)) is False
    assert rig.clip.overflow(np.full(3, 0.5), None, torch.full((2, 4), 0.25)) is False
    assert rig.scores_overflow(np.full((3, 5), 0.5)) is False
    assert rig.stub.sets() == []


def test_unpinned_traps_already_on_the_fallback():
    rig = Rig(StubEngine(clip_res16=0))
    rig.ledger.write("text_hilo", 2)
    rig.ledger.write("effnet_fp32", 1)
    assert not rig.text.pinned() and not rig.effnet.pinned()
    rig.stub.log.clear()
    assert rig.text.overflow(np.array([[NAN, NAN]])) is False
    assert rig.effnet.overflow(np.array([NAN])) is False
    assert rig.clip.overflow(np.array([NAN])) is False
    assert rig.stub.sets() == [] and rig.clip.check is None


def test_text_trap_switches_to_the_precise_mode():
    rig = Rig(StubEngine())
    rig.text.calibrate(4)  # within tolerance: the fast layout, every precise weight released
    assert rig.stub.opts["text_precise_packed"] == 0 and not rig.text.pinned()
    earlier = dict(rig.text.check)
    rig.stub.opts["text_precise_packed"] = 5  # (kinds still packed: they keep their hi / lo operands)
    rig.stub.log.clear()
    assert rig.text.overflow(np.array([[0.5, 0.5], [NAN, 0.5]])) is True
    assert rig.stub.sets() == [("text_prec_mask", 5 | 5 << 4), ("text_hilo", 2)]
    assert rig.text.check == dict(earlier, mode="precise", runtime_overflow=True, prec_mask=85)
    assert not rig.text.pinned()  # the trap's own write is no user pin
    assert rig.text.overflow(np.array([[NAN, NAN]])) is False  # on the fallback now


def test_effnet_trap_switches_to_the_fp32_tower():
    rig = Rig(StubEngine())
    rig.effnet.calibrate(4)
    assert rig.stub.opts["effnet_fp32"] == 0
    earlier = dict(rig.effnet.check)
    rig.stub.log.clear()
    assert rig.effnet.overflow(np.array([0.5, float("inf")])) is True
    assert rig.stub.sets() == [("effnet_fp32", 1)]
    assert rig.effnet.check == dict(earlier, tower="fp32", runtime_overflow=True)
    assert not rig.effnet.pinned()
    assert rig.effnet.overflow(np.array([NAN])) is False


@pytest.mark.parametrize("outputs", [(np.array([0.5, NAN]),), (torch.ones(2, 4), torch.tensor([[1.0, NAN]])),
                                     (None, torch.tensor([NAN]))], ids=["host", "device_pair", "none_and_device"])
def test_clip_trap_switches_to_fp32_streams(outputs):
    rig = Rig(StubEngine())
    rig.clip.check = {"max_dcos": 1e-4, "max_demb": 2e-4, "fp16_streams": True, "rows": 8}
    assert rig.clip.overflow(*outputs) is True
    assert rig.stub.sets()[-1:] == [("clip_res16", 0)] and len(rig.stub.sets()) == 2  # (+ the constructor's text_hilo)
    assert rig.clip.check == {"max_dcos": 1e-4, "max_demb": 2e-4, "fp16_streams": False, "rows": 8,
                              "runtime_overflow": True}
    assert rig.clip.overflow(*outputs) is False


# ---------------------------------------------------------------------------------- 2. text calibration
def _text_script(fast, masks=None):
    """Scores: 0.5 in the full precise mode, 0.5 + fast on the fast layouts, 0.5 + masks.get(m, 1.0) under
    operand mask m."""
    def score(mode, mask):
        if mode < 2:
            return 0.5 + fast
        return 0.5 if mask == P.PREC_FULL else 0.5 + (masks or {}).get(mask, 1.0)
    return score


@pytest.mark.parametrize("layout", [0, 1])
def test_text_calibration_keeps_the_fast_layout(layout):
    rig = Rig(StubEngine(layout=layout, text_score=_text_script(P.TextGuard.TOL * 0.5)))
    rig.stub.log.clear()
    n = 20  # chunks of max_batch = 8: 8 + 8 + 4 rows per mode
    check = rig.text.calibrate(n)
    name = ("fp16", "split")[layout]
    assert check == {"max_dscore": pytest.approx(P.TextGuard.TOL * 0.5, rel=1e-3), "fast_layout": name, "texts": n,
                     "calibrated": True, "mode": name}
    assert rig.stub.sets() == [("text_hilo", -1), ("text_prec_mask", 255), ("text_hilo", 2), ("text_hilo", -1),
                               ("text_precise_packed", 0)]
    assert [e[1:] for e in rig.stub.forwards("text_forward")] == [(b, layout, 255) for b in (8, 8, 4)] + \
        [(b, 2, 255) for b in (8, 8, 4)]  # the fast layout, the full mode, and no mask
    assert not rig.text.pinned()


def test_text_calibration_walks_the_masks_to_the_first_within_tolerance():
    order = P.prec_masks()
    star = order[7]
    masks = {m: P.TextGuard.TOL * (0.5 if m in (star, order[9], order[30]) else 3.0) for m in order}
    rig = Rig(StubEngine(text_score=_text_script(P.TextGuard.TOL * 4, masks)))
    rig.stub.log.clear()
    check = rig.text.calibrate(8)
    assert check["mode"] == "precise" and check["calibrated"] and check["fast_layout"] == "split"
    assert check["max_dscore"] == pytest.approx(P.TextGuard.TOL * 4, rel=1e-3)
    assert check["prec_mask"] == star and list(check["mask_dscore"]) == order[:8]
    assert check["mask_dscore"][star] <= P.TextGuard.TOL < min(check["mask_dscore"][m] for m in order[:7])
    assert check["cost_vs_full"] == P.mask_cost(star) / P.mask_cost(P.PREC_FULL)
    assert [e[3] for e in rig.stub.forwards("text_forward")] == [255, 255] + order[:8]
    assert rig.stub.sets() == [("text_hilo", -1), ("text_prec_mask", 255), ("text_hilo", 2)] + \
        [("text_prec_mask", m) for m in order[:8]] + [("text_prec_mask", star), ("text_precise_packed", star & 15)]
    assert rig.stub.opts["text_hilo"] == 2 and not rig.text.pinned()


def test_text_calibration_keeps_the_full_mode_when_no_mask_holds():
    rig = Rig(StubEngine(text_score=_text_script(P.TextGuard.TOL * 4)))
    check = rig.text.calibrate(2)
    assert check["mode"] == "precise" and check["prec_mask"] == P.PREC_FULL and check["cost_vs_full"] == 1.0
    assert list(check["mask_dscore"]) == P.prec_masks()
    assert rig.stub.opts["text_prec_mask"] == 255 and rig.stub.opts["text_precise_packed"] == 15
    assert rig.stub.opts["text_hilo"] == 2


def test_text_calibration_counts_non_finite_fast_scores_as_infinitely_far():
    rig = Rig(StubEngine(text_score=_text_script(NAN, {0: 0.0})))
    check = rig.text.calibrate(2)
    assert check["max_dscore"] == float("inf") and check["mode"] == "precise" and check["prec_mask"] == 0
    assert rig.stub.opts["text_precise_packed"] == 0 and rig.stub.opts["text_hilo"] == 2


def test_text_calibration_without_every_precise_weight_packed():
    rig = Rig(StubEngine(layout=0, text_precise_packed=3))
    rig.stub.log.clear()
    check = rig.text.calibrate(8)
    assert check == {"mode": "fp16", "calibrated": False, "precise_packed": 3}
    assert len(rig.stub.forwards("text_forward")) == 1  # the fast layout's, then nothing more
    assert rig.stub.log[-1][0] == "text_forward" and rig.stub.sets() == [("text_hilo", -1)]


# -------------------------------------------------------------------------------- 3. EfficientNet calibration
@pytest.mark.parametrize("d16,tower", [(P.EffnetGuard.TOL * 0.5, "fp16"), (P.EffnetGuard.TOL * 2, "fp32"),
                                       (NAN, "fp32")], ids=["within", "outside", "non_finite"])
def test_effnet_calibration(d16, tower):
    rig = Rig(StubEngine(effnet_score=lambda fp32: 0.25 if fp32 else 0.25 + d16))
    rig.stub.log.clear()
    check = rig.effnet.calibrate(64)
    want = float("inf") if d16 != d16 else pytest.approx(d16, rel=1e-3)
    assert check == {"max_ddeepfake": want, "tower": tower, "images": 64, "calibrated": True}
    assert rig.stub.opts["effnet_fp32"] == int(tower == "fp32") and not rig.effnet.pinned()
    assert rig.stub.log == [("set", "effnet_fp32", 0)] + [("effnet_forward", 8, 0)] * 8 + \
        [("set", "effnet_fp32", 1)] + [("effnet_forward", 8, 1)] * 8 + [("set", "effnet_fp32", int(tower == "fp32"))]


# ------------------------------------------------------------------------------------- 4. CLIP stream check
def _unit_rows(seed, n=8, noise=0.0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 512, generator=g, dtype=torch.float64)
    v = v + noise * torch.randn(n, 512, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float()


@pytest.mark.parametrize("noise,ok", [(1e-4, True), (0.3, False), (None, False)], ids=["within", "outside", "non_finite"])
def test_clip_stream_check(noise, ok):
    c32 = (_unit_rows(1), _unit_rows(2))
    if noise is None:
        c16 = (_unit_rows(1), _unit_rows(2).clone())
        c16[1][3, 7] = NAN
    else:
        c16 = (_unit_rows(1, noise=noise), _unit_rows(2, noise=noise))
    rig = Rig(StubEngine(clip16=c16, clip32=c32))
    rig.stub.log.clear()
    check = rig.clip.calibrate(5)
    if noise is None:
        dcos = demb = float("inf")
    else:
        dcos = float((c16[0][:5].double() @ c16[1][:5].double().T - c32[0][:5].double() @ c32[1][:5].double().T).abs().max())
        demb = float(max((c16[0][:5].double() - c32[0][:5]).abs().max(), (c16[1][:5].double() - c32[1][:5]).abs().max()))
        assert (dcos <= P.ClipStreamGuard.TOL) == ok  # the script is on the side of the tolerance it claims
    assert check == {"max_dcos": dcos, "max_demb": demb, "fp16_streams": ok, "rows": 5} and rig.clip.check is check
    assert rig.stub.opts["clip_res16"] == int(ok)
    assert rig.stub.log == [("clip_image", 5, 1), ("clip_text", 5, 1), ("set", "clip_res16", 0), ("clip_image", 5, 0),
                            ("clip_text", 5, 0)] + ([("set", "clip_res16", 1)] if ok else [])


def test_clip_stream_check_caps_the_rows_at_max_batch():
    rig = Rig(StubEngine(clip16=(_unit_rows(1, 16), _unit_rows(2, 16)), clip32=(_unit_rows(1, 16), _unit_rows(2, 16))))
    assert rig.clip.calibrate(12)["rows"] == 8


def test_clip_stream_check_does_nothing_on_fp32_streams():
    rig = Rig(StubEngine(clip_res16=0))
    rig.stub.log.clear()
    assert rig.clip.calibrate() == {}
    rig.clip.check = {"max_dcos": 1.0, "max_demb": 1.0, "fp16_streams": False, "rows": 8}
    assert rig.clip.calibrate() is rig.clip.check
    assert rig.stub.log == []


# ----------------------------------------------------------------------------------------- 5. scores_overflow
def test_scores_overflow_consults_every_trap():
    rig = Rig(StubEngine())
    s = np.full((4, 5), 0.5, np.float32)
    s[1, 0] = s[2, 2] = NAN
    rig.stub.log.clear()
    assert rig.scores_overflow(s) is True
    assert rig.stub.sets() == [("text_prec_mask", 255), ("text_hilo", 2), ("effnet_fp32", 1)]
    assert rig.text.check["runtime_overflow"] and rig.effnet.check["runtime_overflow"] and rig.clip.check is None
    assert rig.scores_overflow(s) is False  # both towers are on their fallback
    s[:] = 0.5
    s[0, 3] = NAN
    assert rig.scores_overflow(s) is True and rig.stub.opts["clip_res16"] == 0 and rig.clip.check["runtime_overflow"]


# ------------------------------------------------------------------------------------------- engine lifetime
def test_guards_do_not_keep_their_engine_alive():
    """An engine frees its device memory in __del__: the ledger and the guards it owns must not hold it in a
    reference cycle, or the release would wait for the cyclic collector."""
    import gc
    freed = []

    class Owner(StubEngine):
        def __del__(self):
            freed.append(True)
    gc.collect()
    gc.disable()
    try:
        e = Owner()
        e.ledger = P.OptionLedger(e)
        e.text_guard, e.effnet_guard = P.TextGuard(e, e.ledger), P.EffnetGuard(e, e.ledger)
        e.clip_guard = P.ClipStreamGuard(e)
        e.text_guard.calibrate(2)
        assert P.scores_overflow(e.text_guard, e.effnet_guard, e.clip_guard, np.full((1, 5), NAN)) is True
        del e
        assert freed == [True]  # finalised by the reference count alone
    finally:
        gc.enable()
