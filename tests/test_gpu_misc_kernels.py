"""Per-kernel numerics of the closing fp32 kernels (csrc/misc.hip: the RoBERTa dual heads, the CLS copy, the
FusionJudge MLP with verdict / confidence / rule, the cosine rows, the finish of mmf_analyze_mixed) on a real
MI355X against the float64 references of tests/misc_refs.py, through the test-only entry points of
csrc/test_host.cpp.  Every output element is compared with the bounds derived there (certified against a float32
emulation in tests/test_misc_refs_cpu.py); copies, gathers, verdicts and rules must be exact.  Output buffers start
as NaN (integers: a sentinel), with canary columns where a row stride exceeds the row and a guard row behind."""
import numpy as np
import pytest
import torch

from tests import misc_refs as M
from tests.test_gpu_transformer_kernels import (EINVAL, NAN, _d, _nan, _p, _release, _run, _sp,  # noqa: F401
                                                _strided, _untouched, lib)

pytestmark = pytest.mark.gpu
SENTINEL = -77


def _close(got, ref, tol, what):
    """test_gpu_transformer_kernels._close with the ratio printed to three significant digits (the worst-case
    bounds of the long chains here leave ratios far below 0.001): every element within its bound, NaN fails."""
    err = (got.double().cpu() - ref).abs()
    ok = err <= tol
    ratio = (err / tol.clamp_min(1e-300)).nan_to_num(float("inf"))
    print(f"RATIO {what}: {float(ratio[ok].max()) if bool(ok.any()) else 0.0:.3g}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst {float(ratio.max()):.3g} x"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _dn(a):
    """Device copy of a numpy array (None stays None)."""
    return None if a is None else _d(_t(a))


def _ints(n):
    """[n + 1] int32 sentinels (the last one is a guard)."""
    return torch.full((n + 1,), SENTINEL, device="cuda", dtype=torch.int32)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    want = _t(want) if isinstance(want, np.ndarray) else want
    assert torch.equal(_bits(got), _bits(want)), f"{what}: not bit-identical"


def _all_nan(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


# ---- the RoBERTa dual heads ----
def _heads_call(lib, xd, row_stride, hw, B, score_stride, ovf=None, logits=True, scores=True):
    ai, mi = (_nan(B, 2), _nan(B, 2)) if logits else (None, None)
    sc = _nan(B, score_stride) if scores else None
    _run(lib.mmf_text_heads_f32(_p(xd), row_stride, *[_p(t) for t in hw], _p(ai), _p(mi), _p(sc), score_stride, _p(ovf),
                                B, _sp()))
    return ai, mi, sc


@pytest.mark.parametrize("regime", M.HEAD_REGIMES)
@pytest.mark.parametrize("B", M.ROWS)
@pytest.mark.parametrize("row_stride", [768, 3 * 768])
@pytest.mark.parametrize("score_stride", [2, 5])
def test_text_heads_vs_fp64(lib, B, regime, row_stride, score_stride):
    x, heads = M.heads_inputs(B, regime)
    xd = _strided(_t(x), row_stride)
    hw = [_dn(t) for h in ("ai", "mi") for t in heads[h]]
    ai, mi, sc = _heads_call(lib, xd, row_stride, hw, B, score_stride)
    _untouched(ai, B, 2, "ai logits")
    _untouched(mi, B, 2, "misinfo logits")
    _untouched(sc, B, 2, "scores")
    for col, (h, got) in enumerate((("ai", ai), ("mi", mi))):
        _, logits, e_l, score, e_s = M.heads_ref(x, *heads[h])
        _close(got[:B], _t(logits), _t(e_l), f"heads {regime} {h} logits")
        _close(sc[:B, col], _t(score), _t(e_s), f"heads {regime} {h} score")
    if regime == "trained":   # saturated: the ai scores that are 1 in float32 must be exactly 1
        one = _t(M.heads_ref(x, *heads["ai"])[3].astype(np.float32) == 1)
        assert bool((sc[:B, 0].cpu()[one] == 1).all())
    # logits-only and scores-only calls give the same bits
    ai2, mi2, _ = _heads_call(lib, xd, row_stride, hw, B, score_stride, scores=False)
    _same(ai2, ai, "logits-only ai")
    _same(mi2, mi, "logits-only misinfo")
    _, _, sc2 = _heads_call(lib, xd, row_stride, hw, B, score_stride, logits=False)
    _same(sc2[:B, :2], sc[:B, :2], "scores-only")
    _untouched(sc2, B, 2, "scores-only")


def test_text_heads_overflow_rows(lib):
    """A row with ovf != 0 gets NaN logits and scores in both heads; its neighbours in the same block keep the bits
    of the run without ovf."""
    B = 9
    x, heads = M.heads_inputs(B, "default")
    xd = _d(_t(x))
    hw = [_dn(t) for h in ("ai", "mi") for t in heads[h]]
    ovf = torch.zeros(B, dtype=torch.int32)
    ovf[1], ovf[6] = 1, 7
    clean = _heads_call(lib, xd, 768, hw, B, 2)
    got = _heads_call(lib, xd, 768, hw, B, 2, ovf=_d(ovf))
    bad = ovf != 0
    for g, c, what in zip(got, clean, ("ai logits", "misinfo logits", "scores")):
        assert bool(torch.isnan(g[:B].cpu()[bad]).all()), what
        _same(g[:B].cpu()[~bad], c[:B].cpu()[~bad], what)
        _untouched(g, B, 2, what)


def test_text_heads_rejects(lib):
    x, heads = M.heads_inputs(4, "default")
    xd = _d(_t(x))
    hw = [_p(_dn(t)) for h in ("ai", "mi") for t in heads[h]]
    ai, mi, sc = _nan(4, 2), _nan(4, 2), _nan(4, 2)
    f = lib.mmf_text_heads_f32
    assert f(_p(xd), 767, *hw, _p(ai), _p(mi), _p(sc), 2, None, 4, None) == EINVAL
    assert lib.mmf_last_error()
    assert f(_p(xd), 768, *hw, _p(ai), _p(mi), _p(sc), 1, None, 4, None) == EINVAL
    assert f(_p(xd), 768, *hw, None, None, None, 2, None, 4, None) == EINVAL
    assert f(None, 768, *hw, _p(ai), _p(mi), _p(sc), 2, None, 4, None) == EINVAL
    assert f(_p(xd), 768, *hw, _p(ai), _p(mi), _p(sc), 2, None, 0, None) == EINVAL
    for i in range(8):
        assert f(_p(xd), 768, *[None if j == i else w for j, w in enumerate(hw)], _p(ai), _p(mi), _p(sc), 2, None, 4,
                 None) == EINVAL
    torch.cuda.synchronize()
    assert _all_nan(ai, mi, sc)


@pytest.mark.parametrize("B", M.ROWS)
@pytest.mark.parametrize("row_stride", [768, 3 * 768])
def test_text_cls_rows_exact(lib, B, row_stride):
    x = M.heads_inputs(B, "default")[0]
    xd = _strided(_t(x), row_stride)
    out = _nan(B, 768)
    _run(lib.mmf_text_cls_rows_f32(_p(xd), row_stride, None, _p(out), B, _sp()))
    _same(out[:B], x, "cls rows")
    _untouched(out, B, 768, "cls rows")
    ovf = torch.zeros(B, dtype=torch.int32)
    ovf[B // 2] = 3
    out2 = _nan(B, 768)
    _run(lib.mmf_text_cls_rows_f32(_p(xd), row_stride, _p(_d(ovf)), _p(out2), B, _sp()))
    bad = ovf != 0
    assert bool(torch.isnan(out2[:B].cpu()[bad]).all())
    _same(out2[:B].cpu()[~bad], x[~bad.numpy()], "cls rows beside an overflowed one")
    _untouched(out2, B, 768, "cls rows with ovf")


def test_text_cls_rows_rejects(lib):
    xd = _d(_t(M.heads_inputs(4, "default")[0]))
    big = torch.zeros(4 * 772 + 8, device="cuda")
    out = _nan(4, 768)
    f = lib.mmf_text_cls_rows_f32
    assert f(_p(big) + 4, 772, None, _p(out), 4, None) == EINVAL          # misaligned x
    assert f(_p(big), 770, None, _p(out), 4, None) == EINVAL              # row_stride % 4 != 0
    assert f(_p(xd), 768, None, _p(out) + 4, 3, None) == EINVAL           # misaligned out
    assert f(_p(xd), 764, None, _p(out), 4, None) == EINVAL
    assert f(None, 768, None, _p(out), 4, None) == EINVAL
    assert f(_p(xd), 768, None, None, 4, None) == EINVAL
    assert f(_p(xd), 768, None, _p(out), 0, None) == EINVAL
    torch.cuda.synchronize()
    assert _all_nan(out)


# ---- FusionJudge ----
def _check_verdict(probs, verdict, conf, ref_probs, e, what):
    """verdict = p1 > 0.5 on the kernel's own probs, conf the selected probability bit for bit; and the reference's
    verdict on every row outside the band (the inputs have none inside: tests/test_misc_refs_cpu.py)."""
    p = probs.cpu()
    own = (p[:, 1] > 0.5).int()
    assert torch.equal(verdict.cpu(), own), f"{what}: verdict is not p1 > 0.5 of the returned probs"
    _same(conf, torch.where(own == 1, p[:, 1], p[:, 0]), what + " conf")
    band = M.verdict_band(ref_probs, e)
    assert int(band.sum()) == 0, f"{what}: {int(band.sum())} rows inside the verdict band"
    assert np.array_equal(own.numpy(), (ref_probs[:, 1] > 0.5).astype(np.int32)), f"{what}: verdict differs from fp64"


def _fusion_call(lib, x5, w, outputs=True):
    B = x5.shape[0]
    probs = _nan(B, 2)
    verdict, conf, rule = (_ints(B), _nan(B, 1), _ints(B)) if outputs else (None, None, None)
    _run(lib.mmf_fusion_raw_f32(_p(_dn(x5)), *[_p(_dn(t)) for t in w], _p(probs), _p(verdict), _p(conf), _p(rule), B,
                                _sp()))
    return probs, verdict, conf, rule


def _check_fusion(lib, x5, w, what):
    B = x5.shape[0]
    probs, verdict, conf, rule = _fusion_call(lib, x5, w)
    ref, e = M.fusion_ref(x5, *w)
    _close(probs[:B], _t(ref), _t(e), what + " probs")
    _untouched(probs, B, 2, what)
    for buf in (verdict, rule):
        assert int(buf[B]) == SENTINEL, f"{what}: wrote past the last row"
    _untouched(conf, B, 1, what + " conf")
    _check_verdict(probs[:B], verdict[:B], conf[:B, 0], ref, e, what)
    assert np.array_equal(rule[:B].cpu().numpy(), M.rule_ref(x5)), f"{what}: rule"
    probs2 = _fusion_call(lib, x5, w, outputs=False)[0]     # the nullable outputs left null
    _same(probs2, probs, what + " probs alone")
    return rule[:B].cpu().numpy()


@pytest.mark.parametrize("scale", [1.0, 10.0])
@pytest.mark.parametrize("B", M.ROWS)
def test_fusion_vs_fp64(lib, B, scale):
    _check_fusion(lib, M.fusion_inputs(B), M.fusion_weights(scale), f"fusion B={B} x{scale:g}")


@pytest.mark.parametrize("scale", [1.0, 10.0])
def test_fusion_threshold_rows(lib, scale):
    """Scores exactly on 0.7f / 0.3f and one float32 to either side: the rule must be the exact float32 cascade, and
    each of its six outcomes must have decided a row."""
    rule = _check_fusion(lib, M.threshold_rows(), M.fusion_weights(scale), f"fusion thresholds x{scale:g}")
    assert set(rule.tolist()) == {0, 1, 2, 3, 4, 5}


def test_fusion_exact_half(lib):
    """Equal output-layer rows and biases: p1 == 0.5 exactly, which is not above 0.5: verdict 0, conf = p0."""
    w = list(M.fusion_weights())
    w[4][1], w[5][1] = w[4][0], w[5][0]
    probs, verdict, conf, _ = _fusion_call(lib, M.fusion_inputs(5), w)
    assert bool((probs[:5] == 0.5).all()) and bool((verdict[:5] == 0).all()) and bool((conf[:5, 0] == 0.5).all())


def test_fusion_rejects(lib):
    x5, w = _dn(M.fusion_inputs(4)), [_p(_dn(t)) for t in M.fusion_weights()]
    probs = _nan(4, 2)
    f = lib.mmf_fusion_raw_f32
    assert f(None, *w, _p(probs), None, None, None, 4, None) == EINVAL
    assert f(_p(x5), *w, None, None, None, None, 4, None) == EINVAL
    assert f(_p(x5), *w, _p(probs), None, None, None, 0, None) == EINVAL
    for i in range(6):
        assert f(_p(x5), *[None if j == i else p for j, p in enumerate(w)], _p(probs), None, None, None, 4, None) == EINVAL
    torch.cuda.synchronize()
    assert _all_nan(probs)


# ---- cosine rows ----
def _rowdot(lib, a, c, ostride=1):
    B, C = a.shape
    out = _nan(B, ostride)
    _run(lib.mmf_rowdot_f32(_p(_dn(a)), _p(_dn(c)), _p(out), ostride, B, C, _sp()))
    return out


@pytest.mark.parametrize("ostride", [1, 5])
@pytest.mark.parametrize("C", M.ROWDOT_WIDTHS)
@pytest.mark.parametrize("B", M.ROWS)
def test_rowdot_vs_fp64(lib, B, C, ostride):
    a, c = M.rowdot_inputs(B, C)
    out = _rowdot(lib, a, c, ostride)
    ref, e = M.rowdot_ref(a, c)
    _close(out[:B, 0], _t(ref), _t(e), f"rowdot C={C}")
    _untouched(out, B, 1, "rowdot")


def test_rowdot_rejects(lib):
    a, c = (_dn(t) for t in M.rowdot_inputs(4, 64))
    out = _nan(4, 1)
    f = lib.mmf_rowdot_f32
    assert f(None, _p(c), _p(out), 1, 4, 64, None) == EINVAL
    assert f(_p(a), None, _p(out), 1, 4, 64, None) == EINVAL
    assert f(_p(a), _p(c), None, 1, 4, 64, None) == EINVAL
    assert f(_p(a), _p(c), _p(out), 0, 4, 64, None) == EINVAL
    assert f(_p(a), _p(c), _p(out), 1, 0, 64, None) == EINVAL
    assert f(_p(a), _p(c), _p(out), 1, 4, 0, None) == EINVAL
    torch.cuda.synchronize()
    assert _all_nan(out)


# ---- the finish of mmf_analyze_mixed ----
_MIXED_IN = ("text2", "deepfake", "v_emb", "t_emb", "c_sims", "c_idx", "c_disc", "title")


def _mixed_args(case, w, out, drop=()):
    """The flat argument list of mmf_mixed_finish_raw (MixedFinishArgs' order); `drop` names arguments passed null."""
    dev = {k: _dn(case[k]) for k in ("row_map",) + _MIXED_IN}
    dev.update({f"w{i}": (_dn(t) if w is not None else None) for i, t in enumerate(w or [None] * 6)})
    dev.update(out)
    g = lambda k: None if k in drop else _p(dev[k])  # noqa: E731
    return ([g("row_map"), case["B"], case["nT"], case["nI"], case["nC"]] + [g(k) for k in _MIXED_IN]
            + [float(case["thresh"])] + [g(f"w{i}") for i in range(6)]
            + [g(k) for k in ("scores5", "text_sim", "probs", "verdict", "conf", "rule", "top_sims", "top_idx")])


def _mixed_out(B):
    return dict(scores5=_nan(B, 5), text_sim=_nan(B, 1), probs=_nan(B, 2), verdict=_ints(B), conf=_nan(B, 1),
                rule=_ints(B), top_sims=_nan(B, 5), top_idx=torch.full((B + 1, 5), SENTINEL, device="cuda",
                                                                        dtype=torch.int32))


def _check_mixed(lib, case, w, what):
    B = case["B"]
    out = _mixed_out(B)
    _run(lib.mmf_mixed_finish_raw(*_mixed_args(case, w, out), _sp()))
    r = M.mixed_finish_ref(case)
    s5 = out["scores5"][:B].cpu()
    # exact gathers (or the absent convention 0 / -1), nothing past the last row
    for col in (0, 1, 2, 4):
        _same(s5[:, col], r["x"][:, col], f"{what} scores5[:, {col}]")
    _same(out["top_sims"][:B], r["top_sims"], what + " top_sims")
    _same(out["top_idx"][:B], r["top_idx"], what + " top_idx")
    for k in ("scores5", "text_sim", "probs", "conf", "top_sims"):
        assert bool(torch.isnan(out[k][B]).all()), f"{what}: {k} written past the last row"
    for k in ("verdict", "rule", "top_idx"):
        assert bool((out[k][B] == SENTINEL).all()), f"{what}: {k} written past the last row"
    # the cosines: within the rowdot bound (exactly 0 where there is none), and the bits of rowdot_kernel
    _close(s5[:, 3], _t(r["x3"]), _t(r["e3"]), what + " x[3]")
    _close(out["text_sim"][:B, 0], _t(r["text_sim"]), _t(r["e_text_sim"]), what + " text_sim")
    # the hit comparison on the pairs with titles: exactly 0 at the threshold (and for a NaN or an empty slot), a
    # cosine one float32 above it
    ts = out["text_sim"][:B, 0].cpu()
    for row, tag in enumerate(r["tags"]):
        if tag & {"top1_at_thresh", "top1_nan", "top1_empty"}:
            assert float(ts[row]) == 0.0, f"{what}: row {row} {sorted(tag)} is no hit, text_sim {float(ts[row])}"
        if tag & {"top1_ulp_above", "top1_hit"}:
            assert "text_sim" in tag and float(ts[row]) != 0.0, f"{what}: row {row} {sorted(tag)} is a hit"
    if r["x3_rows"]:
        rows, ii, ci = (list(v) for v in zip(*r["x3_rows"]))
        _same(s5[rows, 3], _rowdot(lib, case["v_emb"][ii], case["t_emb"][ci])[:len(rows), 0], what + " x[3] vs rowdot")
    if r["ts_rows"]:
        rows, ci, id1 = (list(v) for v in zip(*r["ts_rows"]))
        _same(out["text_sim"][rows, 0], _rowdot(lib, case["t_emb"][ci], case["title"][id1])[:len(rows), 0],
              what + " text_sim vs rowdot")
    # probs: the float64 MLP on the returned scores5 row for the pairs, the single-modality rule in exact float32
    x = s5.numpy()
    pairs = r["has_c"]
    ref_p, e = np.zeros((B, 2)), np.zeros((B, 2))
    if pairs.any():
        ref_p[pairs], e[pairs] = M.fusion_ref(x[pairs], *w)
    ref_p[~pairs] = M.single_modality_probs(x[~pairs], r["has_t"][~pairs])
    _close(out["probs"][:B], _t(ref_p), _t(e), what + " probs")
    _same(out["probs"][:B].cpu()[_t(~pairs)], ref_p[~pairs].astype(np.float32), what + " single-modality probs")
    _check_verdict(out["probs"][:B], out["verdict"][:B], out["conf"][:B, 0], ref_p, e, what)
    assert np.array_equal(out["rule"][:B].cpu().numpy(), M.rule_ref(x)), f"{what}: rule"
    return set().union(*r["tags"])


def test_mixed_finish_vs_reference(lib):
    """Every case of misc_refs.mixed_case (vault absent / present / with titles / no pairs at all, each B), plus the
    empty top-1 slot; at the end every branch of the kernel must have been taken by some row."""
    w = M.fusion_weights()
    seen = set()
    for variant in ("novault", "vault", "titles", "nopairs"):
        for B in M.ROWS:
            case = M.mixed_case(B, variant)
            ww = None if variant == "nopairs" else w   # nC == 0: the fusion weights are null and must not be read
            seen |= _check_mixed(lib, case, ww, f"mixed {variant} B={B}")
            if variant == "titles":
                seen |= _check_mixed(lib, M.mixed_case_empty_slot(case), ww, f"mixed {variant} empty slot B={B}")
    assert seen >= M.MIXED_BRANCHES, M.MIXED_BRANCHES - seen


def test_mixed_finish_nullable_outputs(lib):
    case, w = M.mixed_case(9, "titles"), M.fusion_weights()
    full, part = _mixed_out(9), _mixed_out(9)
    _run(lib.mmf_mixed_finish_raw(*_mixed_args(case, w, full), _sp()))
    drop = ("text_sim", "verdict", "conf", "rule", "top_sims", "top_idx")
    _run(lib.mmf_mixed_finish_raw(*_mixed_args(case, w, part, drop=drop), _sp()))
    _same(part["scores5"], full["scores5"], "scores5")
    _same(part["probs"], full["probs"], "probs")
    assert _all_nan(part["text_sim"], part["conf"], part["top_sims"])
    assert all(bool((part[k] == SENTINEL).all()) for k in ("verdict", "rule", "top_idx"))


def test_mixed_finish_rejects(lib):
    """Every null or absent-buffer condition of launch_mixed_finish is MMF_EINVAL with nothing written."""
    case, w = M.mixed_case(4, "titles"), M.fusion_weights()
    out = _mixed_out(4)
    f = lib.mmf_mixed_finish_raw
    for drop in ("row_map", "scores5", "probs", "text2", "deepfake", "v_emb", "t_emb", "w0", "w1", "w2", "w3", "w4",
                 "w5", "c_idx", "c_disc"):
        assert f(*_mixed_args(case, w, out, drop=(drop,)), None) == EINVAL, drop
        assert lib.mmf_last_error()
    for key, bad in (("B", 0), ("nT", -1), ("nI", -1), ("nC", -1)):
        assert f(*_mixed_args(dict(case, **{key: bad}), w, out), None) == EINVAL, key
    torch.cuda.synchronize()
    assert _all_nan(*(out[k] for k in ("scores5", "text_sim", "probs", "conf", "top_sims")))
    assert all(bool((out[k] == SENTINEL).all()) for k in ("verdict", "rule", "top_idx"))
