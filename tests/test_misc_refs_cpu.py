"""The bounds of tests/misc_refs.py, certified without a GPU: for every kernel of tests/test_gpu_misc_kernels.py,
at its shapes, a float32 emulation of the kernel's own operation order stays within half of the bound, and a planted
defect in the emulation puts more than half of the affected output elements outside the whole bound (exact
outputs: breaks equality).  The inputs of the verdict tests have no row whose reference p1 lies within the bound
of 0.5, so the GPU tests' verdict comparison never has to excuse a row.  Each test prints the emulation's worst
error / bound as a `RATIO emu <what>` line."""
import numpy as np
import pytest

from tests import misc_refs as M


def _under_half(emu, ref, e, what):
    err = np.abs(emu.astype(np.float64) - ref)
    ratio = float((err / np.maximum(e, 1e-300)).max())
    print(f"RATIO emu {what}: {ratio:.3g}")
    assert bool((err <= e / 2).all()), f"{what}: emulation at {ratio:.3f} of the bound"


def _caught(bad, ref, tol, what, affected=None):
    out = np.abs(bad.astype(np.float64) - ref) > tol
    if affected is not None:
        out = out[affected]
    assert out.size > 0, f"{what}: the defect affects nothing"
    frac = float(out.mean())
    assert frac > 0.5, f"{what}: only {frac:.2f} of the affected elements outside the bound"


# ---- heads ----
@pytest.mark.parametrize("regime", M.HEAD_REGIMES)
@pytest.mark.parametrize("B", M.ROWS)
def test_heads_bound(B, regime):
    x, heads = M.heads_inputs(B, regime)
    for h in ("ai", "mi"):
        _, logits, e_l, score, e_s = M.heads_ref(x, *heads[h])
        emu_l, emu_s = M.heads_emulate(x, *heads[h])
        _under_half(emu_l, logits, e_l, f"heads {regime} {h} logits")
        _under_half(emu_s, score, e_s, f"heads {regime} {h} score")


def test_heads_regimes_are_what_they_claim():
    x, heads = M.heads_inputs(9, "halfneg")
    pre = M.heads_ref(x, *heads["ai"])[0]
    assert 0.4 < float((pre < 0).mean()) < 0.6
    x, heads = M.heads_inputs(9, "trained")
    _, la, _, sa, _ = M.heads_ref(x, *heads["ai"])
    _, lm, _, sm, _ = M.heads_ref(x, *heads["mi"])
    assert float((la[:, 1] - la[:, 0]).max()) >= 20 and float((lm[:, 1] - lm[:, 0]).min()) <= -20
    assert bool((sa.astype(np.float32) == 1).any()) and float(sm.min()) < 1e-8


@pytest.mark.parametrize("defect", ["drop_slice", "bias_after_relu", "untransposed"])
def test_heads_logit_defects_are_caught(defect):
    for regime in ("default", "halfneg"):
        x, heads = M.heads_inputs(9, regime)
        _, logits, e_l, _, _ = M.heads_ref(x, *heads["ai"])
        _caught(M.heads_emulate(x, *heads["ai"], defect=defect)[0], logits, e_l, f"{defect} {regime}")


def test_heads_score_defects_are_caught():
    x, heads = M.heads_inputs(9, "default")
    ref = {h: M.heads_ref(x, *heads[h]) for h in heads}
    emu = {h: M.heads_emulate(x, *heads[h])[1] for h in heads}
    _caught(M.heads_emulate(x, *heads["ai"], defect="softmax0")[1], ref["ai"][3], ref["ai"][4], "softmax[:, 0]")
    _caught(emu["mi"], ref["ai"][3], ref["ai"][4], "ai / misinfo swapped (ai column)")
    _caught(emu["ai"], ref["mi"][3], ref["mi"][4], "ai / misinfo swapped (misinfo column)")


# ---- fusion ----
def _fusion_sets():
    for scale in (1.0, 10.0):
        w = M.fusion_weights(scale)
        for B in M.ROWS:
            yield f"B={B} x{scale:g}", M.fusion_inputs(B), w
        yield f"thresholds x{scale:g}", M.threshold_rows(), w


def test_fusion_bound_and_verdict_band():
    in_band = 0
    for what, x5, w in _fusion_sets():
        probs, e = M.fusion_ref(x5, *w)
        emu_p, emu_v, emu_c = M.fusion_emulate(x5, *w)
        _under_half(emu_p, probs, e, "fusion " + what)
        in_band += int(M.verdict_band(probs, e).sum())
        assert np.array_equal(emu_v, (probs[:, 1] > 0.5).astype(np.int32))
    assert in_band == 0, "a fusion input row lies inside the verdict band"


def test_fusion_defects_are_caught():
    for scale in (1.0, 10.0):
        w = M.fusion_weights(scale)
        x5 = np.concatenate([M.fusion_inputs(9), M.threshold_rows()])
        probs, e = M.fusion_ref(x5, *w)
        _caught(M.fusion_emulate(x5, *w, defect="w3_stride64")[0], probs, e, "w3 read with stride 64")
        _caught(M.fusion_emulate(x5, *w, defect="no_relu2")[0], probs, e, "second ReLU missing")
        good, bad = M.fusion_emulate(x5, *w), M.fusion_emulate(x5, *w, defect="conf_p1")
        real = good[1] == 0
        assert real.any() and not np.array_equal(good[2][real].view(np.int32), bad[2][real].view(np.int32))


def test_rule_cascade_and_its_defects():
    x = M.threshold_rows()
    rule = M.rule_ref(x)
    assert set(rule.tolist()) == {0, 1, 2, 3, 4, 5}
    # the rows that sit exactly on a threshold fall through; one float32 further they fire
    for slot, level in ((4, 0), (2, 1), (0, 2), (1, 3)):
        rows = [i for i in range(len(x)) if x[i, slot] in M.around(M.T07) and np.delete(x[i], slot).max() < 0.6]
        assert [int(rule[i]) for i in rows] == [5, 5, level]
    rows = [i for i in range(len(x)) if x[i, 3] in M.around(M.T03) and np.delete(x[i], 3).max() < 0.6]
    assert [int(rule[i]) for i in rows] == [4, 5, 5]
    for defect in ("x2_first", "ge07", "le03"):
        assert not np.array_equal(M.rule_ref(x, defect), rule), defect


def test_exact_half_row():
    """Equal output-layer rows and biases: both logits are the same float32, p1 == 0.5 exactly, verdict 0, conf p0."""
    w = list(M.fusion_weights())
    w[4][1], w[5][1] = w[4][0], w[5][0]
    p, v, c = M.fusion_emulate(M.fusion_inputs(4), *w)
    assert bool((p == np.float32(0.5)).all()) and not v.any() and bool((c == p[:, 0]).all())


# ---- rowdot ----
@pytest.mark.parametrize("C", M.ROWDOT_WIDTHS)
@pytest.mark.parametrize("B", M.ROWS)
def test_rowdot_bound(B, C):
    a, c = M.rowdot_inputs(B, C)
    ref, e = M.rowdot_ref(a, c)
    _under_half(M.rowdot_emulate(a, c), ref, e, f"rowdot C={C}")
    if B == 9:
        _caught(M.rowdot_emulate(a, c, defect="drop_last_pass"), ref, e, f"rowdot C={C} last pass dropped")


# ---- mixed finish ----
def test_mixed_cases_cover_every_branch_and_stay_out_of_the_band():
    seen, in_band = set(), 0
    w = M.fusion_weights()
    for variant in ("novault", "vault", "titles", "nopairs"):
        for B in M.ROWS:
            case = M.mixed_case(B, variant)
            cases = [case] + ([M.mixed_case_empty_slot(case)] if variant == "titles" else [])
            for c in cases:
                r = M.mixed_finish_ref(c)
                seen |= set().union(*r["tags"])
                if variant == "nopairs":
                    assert not r["has_c"].any()
                x = r["x"].copy()
                x[:, 3] = r["x3"].astype(np.float32)
                pairs = r["has_c"]
                if pairs.any():
                    probs, e = M.fusion_ref(x[pairs], *w)
                    in_band += int(M.verdict_band(probs, e).sum())
                single = M.single_modality_probs(x[~pairs], r["has_t"][~pairs])
                in_band += int((single[:, 1] == np.float32(0.5)).sum())
                # the cosines: emulation under half of the bound
                for row, ii, ci in r["x3_rows"]:
                    emu = M.rowdot_emulate(c["v_emb"][ii][None], c["t_emb"][ci][None])[0]
                    assert abs(float(emu) - r["x3"][row]) <= r["e3"][row] / 2
                for row, ci, id1 in r["ts_rows"]:
                    emu = M.rowdot_emulate(c["t_emb"][ci][None], c["title"][id1][None])[0]
                    assert abs(float(emu) - r["text_sim"][row]) <= r["e_text_sim"][row] / 2
    assert seen >= M.MIXED_BRANCHES, M.MIXED_BRANCHES - seen
    assert in_band == 0


def test_mixed_threshold_rows_decide_text_sim():
    """The top1_* tags sit on pair rows with vault and titles only, where `top1 > thresh` decides text_sim: the
    reference is exactly 0 at the threshold although the cosine a `>=` would write lies far outside the bound, and
    it is that cosine one float32 above the threshold."""
    at = above = 0
    for B in M.ROWS:
        c = M.mixed_case(B, "titles")
        r = M.mixed_finish_ref(c)
        for row, tag in enumerate(r["tags"]):
            if not any(t.startswith("top1_") for t in tag):
                continue
            ti, ii, ci = (int(v) for v in c["row_map"][row])
            assert r["has_c"][row] and "vault" in tag
            cos, e = (v[0] for v in M.rowdot_ref(c["t_emb"][ci][None], c["title"][int(c["c_idx"][ii, 0])][None]))
            if "top1_at_thresh" in tag:
                at += 1
                assert c["c_sims"][ii, 0] == c["thresh"] and r["text_sim"][row] == 0.0 and abs(cos) > 100 * e
            if "top1_ulp_above" in tag:
                above += 1
                assert r["text_sim"][row] == cos and abs(cos) > 100 * e
    assert at > 0 and above > 0
    for variant in ("novault", "vault", "nopairs"):   # without titles or pairs nothing carries a top1_* tag
        for B in M.ROWS:
            tags = set().union(*M.mixed_finish_ref(M.mixed_case(B, variant))["tags"])
            assert not any(t.startswith("top1_") for t in tags)
