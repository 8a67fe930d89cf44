"""The lazy-LayerNorm QKV consumer with the attention of its rows in the epilogue (csrc/gemm.hip epi 5, the CLIP
towers' option clip_qkv_attn) on a real MI355X, through the test-only entry mmf_gemm_f16_ln_attn.

A tile holds S = 256 // L whole sequences of L rows; W', u and c are interleaved per head (column 192 h + 64 part
+ d).  For every case:
  (a) ctx is bit-identical to the consumer GEMM on the same operands (256 x 192 tiles, forced gemm_config 10),
      de-interleaved, followed by mmf_attention_f16;
  (b) ctx is within the attention bound of float64 on the fp16 qkv that GEMM stored, for unmasked query rows (the
      bound of tests/transformer_refs.py attn_ref, as tests/test_gpu_transformer_kernels.py uses it for epi 3);
  (c) outputs start as NaN with canary columns and a guard row, and every operand carries NaN in its row padding
      and behind its last row: a stray write, or a read of padding that reaches a result, fails.
Shapes are the smallest that take each path: part of a tile, exactly one, one sequence more, two tiles and one;
every LK (32 / 64 / 96 / 128) at and around its edge; one and two heads; K = 192 (the minimum: three K-steps),
512, 768 with P = 2, 6, 8 partials per row."""
import pytest
import torch

from tests import transformer_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN = float("nan")
TN = R.LN_TN


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import mmf_amd.hip as hip
    return hip.load()


def _run(rc):
    import mmf_amd.hip as hip
    hip.check(rc)
    torch.cuda.synchronize()


def _sp():
    import mmf_amd.hip as hip
    return hip.stream_ptr()


def _padded(t, ld, extra_rows=2):
    """Device copy of host [rows][C] with row stride ld >= C and extra rows behind; every padding element NaN."""
    buf = torch.full((t.shape[0] + extra_rows, ld), NAN, device="cuda", dtype=t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t.cuda()
    return buf


def _vec(v):
    """[N] fp32 with the 256 entries of padding the launcher requires, NaN."""
    d = torch.full((v.numel() + 256,), NAN, device="cuda")
    d[:v.numel()] = v.cuda()
    return d


class Operands:
    """Device operands of one problem: s [M][K] (stride K + 8), W' [N][K] (stride K + 8), u, c, the partials of s over
    blocks of 96 columns (rows padded to 256 and 64 slots behind, NaN), the key mask."""

    def __init__(self, B, L, N, K, mask, seed=0, poison=None):
        self.B, self.L, self.N, self.K, self.M = B, L, N, K, B * L
        s, Wp, u, c = R.consumer_inputs(self.M, N, K, seed)
        if poison is not None:      # non-finite values in one sequence's rows
            s = s.clone()
            r0 = poison * L
            s[r0 + 1, 3] = float("inf")
            s[r0 + L // 2, K - 1] = NAN
            s[r0 + L - 1, 0] = -float("inf")
        pm, pq, _, _ = R.supplied_partials(s, TN)
        self.P = pm.shape[1]
        self.lda = self.ldw = K + 8
        self.s, self.W = _padded(s, self.lda), _padded(Wp, self.ldw)
        self.u, self.c = _vec(u), _vec(c)
        rows = -(-self.M // 256) * 256
        self.st = torch.full((rows * self.P + 64, 2), NAN, device="cuda")
        self.st[:self.M * self.P, 0], self.st[:self.M * self.P, 1] = pm.reshape(-1).cuda(), pq.reshape(-1).cuda()
        self.mask = mask
        self.md = None if mask is None else mask.contiguous().cuda()

    def _p(self, t):
        return None if t is None else t.data_ptr()

    def fused(self, lib, causal):
        """ctx [M][D] through the attention epilogue; canaries checked."""
        D = self.N // 3
        ctx = torch.full((self.M + 1, D + 4), NAN, device="cuda", dtype=torch.float16)
        _run(lib.mmf_gemm_f16_ln_attn(self.s.data_ptr(), self.lda, self.W.data_ptr(), self.ldw, self.c.data_ptr(),
                                      self.st.data_ptr(), self.P, TN, self.u.data_ptr(), R.EPS, self._p(self.md), self.L,
                                      causal, ctx.data_ptr(), D + 4, self.M, self.N, self.K, _sp()))
        assert bool(torch.isnan(ctx[:self.M, D:]).all()), "ctx: wrote into the row padding"
        assert bool(torch.isnan(ctx[self.M:]).all()), "ctx: wrote past the last row"
        return ctx[:self.M, :D]

    def unfused(self, lib, causal):
        """(qkv fp16 [M][3 D] de-interleaved as the consumer GEMM stored it, ctx [M][D] of mmf_attention_f16 on it)."""
        import mmf_amd.hip as hip
        M, N, D, H = self.M, self.N, self.N // 3, self.N // 192
        qkv_il = torch.full((M + 1, N), NAN, device="cuda", dtype=torch.float16)
        hip.set_process_option("gemm_config", 10)
        try:
            _run(lib.mmf_gemm_f16_ln_consumer(self.s.data_ptr(), self.lda, self.W.data_ptr(), self.ldw, self.c.data_ptr(),
                                              self.st.data_ptr(), self.P, TN, self.u.data_ptr(), R.EPS, qkv_il.data_ptr(),
                                              N, M, N, self.K, 0, _sp()))
        finally:
            hip.set_process_option("gemm_config", -1)
        assert bool(torch.isnan(qkv_il[M:]).all())
        # column h * 192 + part * 64 + d  ->  part * D + h * 64 + d
        qkv = qkv_il[:M].view(M, H, 3, 64).permute(0, 2, 1, 3).reshape(M, 3 * D).contiguous()
        out = torch.full((M + 1, D), NAN, device="cuda", dtype=torch.float16)
        _run(lib.mmf_attention_f16(qkv.data_ptr(), self._p(self.md), out.data_ptr(), self.B, self.L, H, causal, _sp()))
        assert bool(torch.isnan(out[M:]).all())
        return qkv, out[:M]


def _check(lib, B, L, causal, N=192, K=192, dead=None, with_mask=True):
    mask = R.holes_mask(B, L, dead=dead) if with_mask else None
    op = Operands(B, L, N, K, mask)
    ctx = op.fused(lib, causal)
    qkv, want = op.unfused(lib, causal)
    M, D, H = op.M, N // 3, N // 192
    assert torch.equal(R.bits16(ctx.cpu()), R.bits16(want.cpu())), "epilogue and consumer GEMM + attention differ"
    qh = qkv.cpu()
    ref, e = R.attn_ref(R.heads(qh, B, L, H, 0), R.heads(qh, B, L, H, D), R.heads(qh, B, L, H, 2 * D),
                        R.attn_valid(mask, B, L, bool(causal)), p16=True)
    ref, e = (t.permute(0, 2, 1, 3).reshape(M, D) for t in (ref, e))
    rows = torch.ones(M, dtype=torch.bool) if mask is None else (mask != 0).view(-1)
    err = (ctx.double().cpu() - ref).abs()[rows]
    tol = R.store16(ref, e)[rows]
    ratio = err / tol.clamp_min(1e-300)
    ok = err <= tol
    print(f"RATIO lazy-LN attention epilogue B={B} L={L} causal={causal} N={N} K={K}: "
          f"{float(ratio[ok].max()) if bool(ok.any()) else 0.0:.3f}")
    assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} elements outside the bound, worst {float(ratio.nan_to_num(float('inf')).max()):.3g} x"


@pytest.mark.parametrize("B", [1, 5, 6, 11])    # part of a tile, exactly one, a tile + one sequence, two tiles + one
def test_vit_shape(lib, B):
    """L = 50, not causal (LK 64, S = 5), no mask as the ViT runs it."""
    _check(lib, B, 50, 0, with_mask=False)


@pytest.mark.parametrize("B", [1, 3, 4, 7])
def test_text_shape(lib, B):
    """L = 77, causal (LK 96, S = 3), holes and ragged tails in the key mask; from B = 3 one sequence has every key
    masked."""
    _check(lib, B, 77, 1, dead=(1 if B > 1 else None))


@pytest.mark.parametrize("L", [17, 32, 33, 64, 65, 96, 128])
@pytest.mark.parametrize("causal", [0, 1])
def test_lk_and_s_edges(lib, L, causal):
    """Every LK at and around its edge, S = 15, 8, 7, 4, 3, 2, 2; B = S + 1: a full tile and one sequence."""
    _check(lib, 256 // L + 1, L, causal)


@pytest.mark.parametrize("N", [192, 384])
@pytest.mark.parametrize("K", [192, 512, 768])      # P = 2, 6 (the last block 32 columns), 8
@pytest.mark.parametrize("L,causal", [(50, 0), (77, 1)])
def test_heads_and_depth(lib, N, K, L, causal):
    _check(lib, 256 // L + 1, L, causal, N=N, K=K)


@pytest.mark.parametrize("L,causal,B,bad", [(50, 0, 6, 2), (77, 1, 4, 1), (32, 0, 9, 7)])
def test_sequences_are_isolated(lib, L, causal, B, bad):
    """inf and NaN in one sequence's rows (so in its statistics, q, k and v): every other sequence's ctx is
    bit-identical to the clean run -- a padded key of a neighbour must read zeros, not the poisoned rows."""
    mask = R.holes_mask(B, L)
    clean = Operands(B, L, 192, 192, mask).fused(lib, causal).cpu()
    dirty = Operands(B, L, 192, 192, mask, poison=bad).fused(lib, causal).cpu()
    keep = torch.ones(B * L, dtype=torch.bool)
    keep[bad * L:(bad + 1) * L] = False
    assert not bool(torch.isfinite(dirty[~keep].float()).all()), "the poisoned sequence came out finite"
    assert torch.equal(R.bits16(clean[keep]), R.bits16(dirty[keep])), "a sequence's ctx depends on another sequence's rows"


def test_rejects(lib):
    """What the epilogue does not take is EINVAL with the output still all NaN."""
    A, W = torch.zeros(512, 192, dtype=torch.float16, device="cuda"), torch.zeros(384, 192, dtype=torch.float16, device="cuda")
    v = torch.zeros(384 + 256, device="cuda")
    st = torch.zeros(512 * 8, 2, device="cuda")
    ctx = torch.full((513, 128), NAN, device="cuda", dtype=torch.float16)
    p = lambda t: None if t is None else t.data_ptr()

    def call(lda=192, ldw=192, bias=v, ln_in=st, P=2, ln_u=v, L=50, out=ctx, ldc=128, M=300, N=192, K=192):
        return lib.mmf_gemm_f16_ln_attn(p(A), lda, p(W), ldw, p(bias), p(ln_in), P, TN, p(ln_u), R.EPS, None, L, 0, p(out),
                                        ldc, M, N, K, None)

    assert call(L=129, M=258) == EINVAL         # L > 128
    assert call(L=8, M=296) == EINVAL           # more key-bias slots than the tile has
    assert call(M=310) == EINVAL                # not whole sequences
    assert call(N=200) == EINVAL                # not whole heads
    assert call(N=256) == EINVAL
    assert call(lda=128, ldw=128, K=128) == EINVAL      # K < 192
    assert call(P=1) == EINVAL                  # P tn < K
    assert call(P=9) == EINVAL
    assert call(ln_in=None) == EINVAL
    assert call(ln_u=None) == EINVAL
    assert call(bias=None) == EINVAL
    assert call(out=None) == EINVAL
    assert call(ldc=32) == EINVAL               # ldc < N / 3
    assert call(N=384, ldc=64) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx).all())
