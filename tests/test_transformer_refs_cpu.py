"""The bounds of tests/transformer_refs.py, certified without a GPU: for every kernel group of
tests/test_gpu_transformer_kernels.py, at its shapes, a float32 emulation of the operation (plain torch, with the kernel's
rounding points: fp16 P, fp16 stores, statistics of the stored stream) stays within half of the
arithmetic bound (an fp16 store: half of it plus the store's half-ulp), and a planted defect in the
emulation puts more than half of the affected output elements outside the whole bound (integer
outputs: breaks equality).  Groups that are another group's arithmetic on other rows or operands are
certified through it: layernorm_split3 through the LayerNorm bound (its `add` form), the attention epilogue through the L = 128
attention bound and the GEMM bound, the exact splits through test_hilo_split_is_exact.  Seeds are fixed
in transformer_refs."""
import pytest
import torch

from tests import transformer_refs as R


def _under_half(emu, ref, e, what, stored16=False):
    """emu (fp32, before any store) within e / 2; stored16: its fp16 rounding within e / 2 + the half-ulp."""
    err = (emu.double() - ref).abs()
    assert bool((err <= e / 2).all()), f"{what}: emulation at {float((err / e.clamp_min(1e-300)).max()):.3f} of the bound"
    if stored16:
        err = (emu.half().double() - ref).abs()
        assert bool((err <= R.store16(ref, e / 2)).all()), f"{what}: stored emulation outside e / 2 + half-ulp"


def _caught(bad, ref, tol, what, affected=None):
    """More than half of the affected elements of a defective result lie outside the bound."""
    out = (bad.double() - ref).abs() > tol
    if affected is not None:
        out = out[affected.expand_as(out)]
    assert out.numel() > 0, f"{what}: the defect affects nothing"
    frac = float(out.double().mean())
    assert frac > 0.5, f"{what}: only {frac:.2f} of the affected elements outside the bound"


# ---- LayerNorm family ----
@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("add,dominant", [(False, False), (True, False), (False, True)])
def test_layernorm_bound(rows, C, add, dominant):
    x = R.rows_input(rows, C, dominant=dominant)
    gam, bet = R.dominant_params(C) if dominant else R.ln_params(C)
    if add:
        a = R.rows_input(rows, C, 11) * 0.5
        sd = x.double() + a.double()
        ref, e = R.ln_ref(sd, gam, bet, e_x=R.U * sd.abs())
        x = x + a
    else:
        ref, e = R.ln_ref(x, gam, bet)
    _under_half(R.ln_emulate(x, gam, bet), ref, e, "LN", stored16=True)
    _caught(R.ln_emulate(x, gam, bet, defect="gamma_first").half(), ref, R.store16(ref, e), "LN gamma first")


def test_dominant_channel_bound_is_not_flat():
    """With one channel 100 times the rest and gamma 7 the bound follows the formula: the dominant channel's own
    element carries a bound tens of times the median one's (a flat figure would be wrong for one of them)."""
    x = R.rows_input(4, 768, dominant=True)
    gam, bet = R.dominant_params(768)
    _, e = R.ln_ref(x, gam, bet)
    assert float(e[:, 77].min()) > 20 * float(e.median())


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("rows", R.ROWS)
def test_add_ln_bound(rows, C):
    """s = x + y then LN(s), on the fp32 stream and on the fp16 one (LN of the stored, rounded s)."""
    x, y = R.rows_input(rows, C, 1), R.branch_input(rows, C)
    gam, bet = R.ln_params(C)
    s, e_s = R.add_ref(x, y)
    s32 = x + y.float()
    _under_half(s32, s, e_s, "s")
    ref, e = R.ln_ref(s, gam, bet, e_x=e_s / 2)
    _under_half(R.ln_emulate(s32, gam, bet), ref, e, "LN(s)", stored16=True)
    _caught(R.ln_emulate(s32, gam, bet, defect="gamma_first"), ref, e, "LN(s) gamma first")
    # fp16 stream: the stored s16 is the LN's operand
    x16 = x.half()
    s, e_s = R.add_ref(x16, y)
    s16 = (x16.float() + y.float()).half()
    _under_half(x16.float() + y.float(), s, e_s, "s16", stored16=True)
    ref, e = R.ln_ref(s16, gam, bet)
    _under_half(R.ln_emulate(s16.float(), gam, bet), ref, e, "LN(s16)", stored16=True)
    # split stream: s = (hi + lo) + y
    hi, lo = R.split_hilo(x)
    a = hi.double() + lo.double()
    s = a + y.double()
    ref, e = R.ln_ref(s, gam, bet, e_x=R.U * (a.abs() + s.abs()))
    emu = R.ln_emulate((hi.float() + lo.float()) + y.float(), gam, bet)
    _under_half(emu, ref, e, "LN(hi + lo + y)", stored16=True)
    h2, l2 = R.split_hilo(emu)
    assert bool(((h2.double() + l2.double() - ref).abs() <= R.hilo_sum_tol(ref, e / 2)).all())
    _caught(h2.double(), ref, R.hilo_sum_tol(ref, e), "hi alone against the hi + lo bound")


def test_hilo_split_is_exact():
    """hi + lo reproduces an fp32 value to 2^-22 relative; x - hi is exact in fp32 (what split_hilo relies on)."""
    x = R.rows_input(9, 768, 3)
    hi, lo = R.split_hilo(x)
    assert torch.equal((x.double() - hi.double()).float().double(), x.double() - hi.double())
    assert bool(((hi.double() + lo.double() - x.double()).abs() <= R.hilo_sum_tol(x.double(), torch.zeros(()))).all())


@pytest.mark.parametrize("C", R.WIDTHS)
def test_row_partial_bound(C):
    x = R.rows_input(9, C, 5).half()
    mean, e_m, m2, e_m2 = R.partial_ref(x)
    em, eq = R.partial_emulate(x.float())
    _under_half(em, mean, e_m, "mean")
    _under_half(eq, m2, e_m2, "M2")
    _caught(R.partial_emulate(x.float(), defect="uncentred")[1], m2, e_m2, "M2 about 0")


# ---- embeddings ----
def _pos_ids_loop(ids):
    out = torch.empty_like(ids, dtype=torch.int64)
    for b in range(ids.shape[0]):
        n = 0
        for t in range(ids.shape[1]):
            if int(ids[b, t]) != R.PAD:
                n += 1
                out[b, t] = n + R.PAD
            else:
                out[b, t] = R.PAD
    return out


@pytest.mark.parametrize("L", R.ROBERTA_L)
def test_roberta_embed_bound(L):
    ids = R.roberta_ids(L)
    assert torch.equal(R.roberta_pos_ids(ids), _pos_ids_loop(ids))
    assert bool((ids[0] != R.PAD).all()) and int(ids[1, 0]) == R.PAD and bool((ids[3] == R.PAD).all())
    word, pos, type0 = R.roberta_tables(L)
    gam, bet = R.ln_params(768)
    ref, e = R.roberta_ref(ids, word, pos, type0, gam, bet)
    emu = R.roberta_emulate(ids, word, pos, type0, gam, bet)
    _under_half(emu, ref, e, "embed", stored16=True)
    hi, lo = R.split_hilo(emu)
    assert bool(((hi.double() + lo.double() - ref).abs() <= R.hilo_sum_tol(ref, e / 2)).all())
    bad = R.roberta_emulate(ids, word, pos, type0, gam, bet, defect="pos_off_by_one")
    _caught(bad.half(), ref, R.store16(ref, e), "position id off by one", affected=(ids != R.PAD)[..., None])
    # any other position row falls outside the bound: the integer position id is visible in the output
    if L > 1:
        other, _ = R.roberta_ref(ids, word, pos, type0, gam, bet, pid=(R.roberta_pos_ids(ids) + 1).clamp_max(L + 1))
        _caught(other, ref, R.store16(ref, e), "neighbouring position row", affected=(R.roberta_pos_ids(ids) <= L)[..., None])


@pytest.mark.parametrize("L", R.CLIP_TEXT_L)
@pytest.mark.parametrize("x16", [False, True])
def test_clip_text_embed_bound(L, x16):
    ids, tok, pos = R.clip_text_inputs(2, L)
    gam, bet = R.ln_params(512)
    x, e_x = R.clip_text_x_ref(ids, tok, pos)
    emu = R.clip_text_x_emulate(ids, tok, pos)
    _under_half(emu, x, e_x, "x", stored16=x16)
    _caught(R.clip_text_x_emulate(ids, tok, pos, defect="pos_off_by_one"), x, R.store16(x, e_x), "position off by one")
    stored = emu.half().float() if x16 else emu
    if x16:
        ref, e = R.ln_ref(stored, gam, bet)
    else:
        ref, e = R.ln_ref(x, gam, bet, e_x=e_x / 2)
    _under_half(R.ln_emulate(stored, gam, bet), ref, e, "xb", stored16=True)
    _caught(R.ln_emulate(stored, gam, bet, defect="gamma_first").half(), ref, R.store16(ref, e), "xb gamma first")
    mean, e_m, m2, e_m2 = R.partial_ref(stored)
    em, eq = R.partial_emulate(stored)
    _under_half(em, mean, e_m, "st mean")
    _under_half(eq, m2, e_m2, "st M2")
    _caught(R.partial_emulate(stored, defect="uncentred")[1], m2, e_m2, "st M2 about 0")


@pytest.mark.parametrize("B", [1, 3])
def test_clip_vision_assemble_bound(B):
    patches, cls, pos = R.vision_inputs(B)
    pg, pb = R.ln_params(768, 2)
    g1, b1 = R.ln_params(768, 3)
    x, e_x = R.vision_x_ref(patches, cls, pos, B, pg, pb)
    emu = R.ln_emulate(R.vision_e(patches, cls, pos, B), pg, pb)
    _under_half(emu, x, e_x, "x", stored16=True)
    bad = R.ln_emulate(R.vision_e(patches, cls, pos, B, defect="cls_is_patch"), pg, pb)
    cls_rows = (torch.arange(B * 50) % 50 == 0)[:, None]
    _caught(bad, x, R.store16(x, e_x), "CLS row taken from the patches", affected=cls_rows)
    ref, e = R.ln_ref(x, g1, b1, e_x=e_x / 2)
    _under_half(R.ln_emulate(emu, g1, b1), ref, e, "xb (fp32 stream)", stored16=True)
    s16 = emu.half()
    ref, e = R.ln_ref(s16, g1, b1)
    _under_half(R.ln_emulate(s16.float(), g1, b1), ref, e, "xb (fp16 stream)", stored16=True)
    for stored in (emu, s16.float()):
        mean, e_m, m2, e_m2 = R.partial_ref(stored)
        em, eq = R.partial_emulate(stored)
        _under_half(em, mean, e_m, "st mean")
        _under_half(eq, m2, e_m2, "st M2")
        _caught(R.partial_emulate(stored, defect="uncentred")[1], m2, e_m2, "st M2 about 0")


@pytest.mark.parametrize("B", [1, 2])
def test_clip_im2col_bound(B):
    img = torch.randint(0, 256, (B, 224, 224, 3), generator=R._gen(B, 73), dtype=torch.uint8)
    ref, e = R.im2col_ref(img)
    _under_half(R.im2col_emulate(img), ref, e, "im2col", stored16=True)
    _caught(R.im2col_emulate(img, defect="swap_xy").half(), ref, R.store16(ref, e), "ky / kx exchanged")


# ---- pooling ----
@pytest.mark.parametrize("L", R.EOS_L)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("mode", ["eos", "argmax"])
def test_eos_index_reference(B, L, mode):
    ids = R.eos_inputs(B, L, mode)
    eos = R.EOS_ID if mode == "eos" else 2
    ref = R.eos_ref(ids, eos)
    assert torch.equal(R.eos_emulate(ids, eos), ref)
    if mode == "argmax" and B > 1:
        assert int(ref[0]) == 0 and int(ref[1]) == L - 1
    if mode == "eos" and B > 1:
        assert int(ref[0]) == 0 and not bool((ids[0] == eos).any())   # none: 0
    key = ids if mode == "argmax" else (ids == eos).int()
    tied = bool(((key == key.amax(1, keepdim=True)).sum(1) > 1)[key.amax(1) > 0].any())
    if tied:    # a row with its maximum / EOS at more than one place: the last one is another index
        assert not torch.equal(R.eos_emulate(ids, eos, defect="last"), ref)
    else:
        assert L < 64


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("B", [1, 5])
def test_l2norm_bound(B, C):
    x = R.rows_input(B, C, 7)
    ref, e = R.l2norm_ref(x)
    _under_half(R.l2norm_emulate(x), ref, e, "l2norm")
    _caught(R.l2norm_emulate(x, defect="mean_square"), ref, e, "mean instead of sum of squares")


@pytest.mark.parametrize("C", R.WIDTHS)
@pytest.mark.parametrize("L", [1, 7])
def test_gather_ln_bound(C, L):
    """The LayerNorm of the gathered rows; a gather that ignores idx (row b L) falls outside the bound."""
    B = 5
    x = R.rows_input(B * L, C, 12)
    gam, bet = R.ln_params(C)
    idx = R.gather_idx(B, L).long()
    ref, e = R.ln_ref(x[torch.arange(B) * L + idx], gam, bet)
    _under_half(R.ln_emulate(x[torch.arange(B) * L + idx], gam, bet), ref, e, "gather_ln", stored16=True)
    if L > 1:
        _caught(R.ln_emulate(x[torch.arange(B) * L], gam, bet).half(), ref, R.store16(ref, e), "idx ignored",
                affected=(idx != 0)[:, None])


# ---- attention ----
def _attn_case(B, L, H, mask, causal=False, qpos=None, p16=True, chunks=1, out16=True, seed=0, tail=False):
    qkv = R.attn_inputs(B, L, H, seed)
    D = H * 64
    q, k, v = (R.heads(qkv, B, L, H, o) for o in (0, D, 2 * D))
    if qpos is not None:
        q = q[:, :, :1]   # one query per sequence (its values are whatever row 0 holds)
    valid = R.attn_valid(mask, B, L, causal, qpos)
    ref, e = R.attn_ref(q, k, v, valid, p16, chunks)
    emu = R.attn_emulate(q, k, v, valid, p16)
    _under_half(emu, ref, e, f"attention L={L}", stored16=out16)
    tol = R.store16(ref, e) if out16 else e
    alive = valid.any(-1)[:, None, :, None]
    if bool(alive.any()):
        bad = R.attn_emulate(q, k, v, valid, p16, defect="drop_last_key")
        _caught(bad.half() if out16 else bad, ref, tol, f"dropped last key L={L}", affected=alive)
    if tail and L % 32 and L > 32:
        sees_tail = valid[..., L - L % 32:].any(-1)[:, None, :, None]
        if bool(sees_tail.any()):
            bad = R.attn_emulate(q, k, v, valid, p16, defect="v_tail")
            _caught(bad.half() if out16 else bad, ref, tol, f"V chunk tail omitted L={L}", affected=sees_tail)
    dead = ~valid.any(-1)
    if bool(dead.any()):
        assert bool((ref[dead[:, None].expand(-1, H, -1)] == 0).all()) and bool((e[dead[:, None].expand(-1, H, -1)] == 0).all())


@pytest.mark.parametrize("L", R.ATTN_SHORT_L + R.ATTN_LONG_L)
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_f16_bound(L, H, causal):
    chunks = R.long_chunks(L) if L > 128 else 1
    _attn_case(2, L, H, R.holes_mask(2, L), causal, chunks=chunks, tail=True)


@pytest.mark.parametrize("L", R.ATTN32_L)
def test_attention32_bound(L):
    chunks = -(-L // 32)
    _attn_case(2, L, 2, None, p16=False, chunks=chunks, out16=False, tail=True)
    m = R.holes_mask(2, L)
    if L > 32:
        m[0, :32] = 0   # a first chunk with no valid key, valid ones after
    _attn_case(2, L, 2, m, p16=False, chunks=chunks, out16=False, seed=1, tail=True)
    _attn_case(2, L, 2, R.holes_mask(2, L, dead=1), p16=False, chunks=chunks, out16=False, seed=2)


@pytest.mark.parametrize("L", R.Q1_L)
@pytest.mark.parametrize("B,H", R.Q1_BH)
def test_attention_q1_bound(L, B, H):
    for qp in (None, 0, L // 2, L - 1):
        qpos = None if qp is None else torch.full((B,), qp, dtype=torch.int32)
        if qpos is None:
            qpos_eff = torch.full((B,), L - 1, dtype=torch.int32)
        else:
            qpos_eff = qpos
        _attn_case(B, L, H, R.holes_mask(B, L, dead=B - 1 if B > 1 else None), qpos=qpos_eff, p16=False,
                   seed=3, tail=qp in (None, L - 1))


# ---- split-K ----
@pytest.mark.parametrize("M,N,K,act,bias,res,outs", R.splitk_cases())
def test_splitk_bound(M, N, K, act, bias, res, outs):
    A, W, bv, rv = R.gemm_inputs(M, N, K)
    S = K // 256
    b = bv if bias else None
    r = None if res == "none" else (rv if res == "res32" else rv.half())
    ref, e = R.gemm_ref(A, W, b, r, act, K // S + S + 4)
    emu = R.splitk_emulate(A, W, b, r, act, S)
    _under_half(emu, ref, e, "split-K", stored16=outs != "c32")
    bad = R.splitk_emulate(A, W, b, r, act, S, defect="skip_last_slice")
    affected = None if act != 4 else ((ref != 0) | (bad != 0))   # (ReLU: elements that are 0 either way show nothing)
    _caught(bad, ref, R.store16(ref, e) if outs == "c16" else e, "last K slice skipped", affected=affected)


def test_splitk_cases_cover_the_grid():
    cs = R.splitk_cases()
    assert {c[0] for c in cs} == set(R.SPLITK_M) and {c[1] for c in cs} == set(R.SPLITK_N)
    assert {c[2] for c in cs} == set(R.SPLITK_K) and {c[2] // 256 for c in cs} == {2, 3, 5, 6, 12}
    assert {c[3] for c in cs} == {0, 1, 2, 3, 4} and {c[4] for c in cs} == {True, False}
    assert {c[5] for c in cs} == set(R.RES_KINDS) and {c[6] for c in cs} == set(R.OUT_KINDS)


# ---- lazy-LN producer ----
@pytest.mark.parametrize("N", R.PRODUCER_N)
@pytest.mark.parametrize("K", R.PRODUCER_K)
@pytest.mark.parametrize("M", R.PRODUCER_M)
def test_ln_producer_bound(M, N, K):
    A, W, bias, res = R.gemm_inputs(M, N, K, 7)
    res = res.half()
    ref, e = R.gemm_ref(A, W, bias, res, 0, K + 4)
    emu = A.float() @ W.float().T + bias + res.float()
    _under_half(emu, ref, e, "stream", stored16=True)
    stored = emu.half()
    mean, e_m, m2, e_m2 = R.block_partials_ref(stored)
    em, eq = R.block_partials_emulate(stored.float())
    assert mean.shape == (M, -(-N // 96))
    _under_half(em, mean, e_m, "partial mean")
    _under_half(eq, m2, e_m2, "partial M2")
    if N % 96:
        bm, bq = R.block_partials_emulate(stored.float(), defect="tail_as_full")
        _caught(bm[:, -1], mean[:, -1], e_m[:, -1], "tail partial weighted as 96 columns (mean)")
        _caught(bq[:, -1], m2[:, -1], e_m2[:, -1], "tail partial weighted as 96 columns (M2)")


# ---- lazy-LN consumer ----
@pytest.mark.parametrize("M", R.CONSUMER_M)
@pytest.mark.parametrize("N", R.CONSUMER_N)
@pytest.mark.parametrize("K", R.CONSUMER_K)
@pytest.mark.parametrize("form", ["one", "blocks"])
def test_ln_consumer_bound(M, N, K, form):
    act = R.CONSUMER_ACT[K]
    tn = K if form == "one" else R.LN_TN
    s, Wp, u, c = R.consumer_inputs(M, N, K)
    pm, pq, e_pm, e_pq = R.supplied_partials(s, tn)
    ref, e = R.consumer_ref(s, Wp, u, c, act, tn, e_pm, e_pq)
    _under_half(R.consumer_emulate(s, Wp, u, c, act, pm, pq, tn), ref, e, "consumer", stored16=True)
    tol = R.store16(ref, e)
    live = None if act == 0 else (ref.abs() > 1e-3)    # (an activation's flat tail shows nothing)
    _caught(R.consumer_emulate(s, Wp, u, c, act, pm, pq, tn, defect="no_mean"), ref, tol, "mean u left out", affected=live)
    if K % tn:
        _caught(R.consumer_emulate(s, Wp, u, c, act, pm, pq, tn, defect="tail_as_full"), ref, tol,
                "tail partial weighted as 96 columns", affected=live)


def test_ln_chain_bound():
    """The producer's emulated stream and partials fed to the consumer, against the float64 LN of that stream."""
    M, Kp, C = 100, 192, 512
    A, W, bias, res = R.gemm_inputs(M, C, Kp, 7)
    stored = (A.float() @ W.float().T + bias + res.half().float()).half()
    pm, pq = R.block_partials_emulate(stored.float())
    _, e_pm, _, e_pq = R.block_partials_ref(stored)
    _, Wp, u, c = R.consumer_inputs(M, 200, C)
    ref, e = R.consumer_ref(stored, Wp, u, c, 1, R.LN_TN, e_pm, e_pq)
    _under_half(R.consumer_emulate(stored, Wp, u, c, 1, pm, pq, R.LN_TN), ref, e, "chain", stored16=True)
    _caught(R.consumer_emulate(stored, Wp, u, c, 1, pm, pq, R.LN_TN, defect="tail_as_full"), ref, R.store16(ref, e),
            "chain, tail partial weighted as 96 columns", affected=ref.abs() > 1e-3)
