// The RoBERTa tower's launch sequences: the fp16 / split-stream encoder (run_text) and the precise mode.
#include "handle.h"

namespace {

// RoBERTa precise mode (text_hilo = 2; precise.hip): fp32 stream, fp32 branch outputs, LayerNorm
// and attention, every GEMM on ~22-bit operands through the K-concatenated [hi | lo | hi] x
// [W_hi | W_hi | W_lo] product on the fp16 MFMA kernels.  All 12 layers run on every row; the heads
// read the CLS rows of the final stream.  DESIGN §4 states its cost.
int run_text_precise(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* ai, float* mi,
                     float* scores, int score_stride, hipStream_t s, float* cls) {
  Workspace& w = h->ws;
  const int M = B * L;
  const int pm = h->opt.text_prec_mask & 15;  // kinds on hi / lo activations: [A_hi | A_lo] x [W_hi | W_hi] (K = 2 in)
  const int pw = pm & (h->opt.text_prec_mask >> 4);  // ... of them also on W_lo: + A_hi x W_lo (K = 3 in)
  if (pm & ~h->r_precise)
    return fail(MMF_EINVAL, "text_hilo = 2: text_prec_mask %d needs precise-mode weights that are not packed (packed: %d; "
                            "re-load the text model with text_hilo -1 or 2)", pm, h->r_precise);
  if (!w.p32 || w.t32_rows < (size_t)M) return fail(MMF_EINVAL, "text_hilo = 2: precise workspaces not reserved");
  float* x = w.r_x;  // the fp32 residual stream [M][768]
  float* y = w.r_y;  // branch outputs / ctx [M][768]
  {
    ProfScope ps(h, s, PK_EMBED, 10.0 * M * 768, (double)M * 768 * (4 + 4 + 4));
    HIPCHK(launch_roberta_embed(ids, h->r_word, h->r_pos, h->r_type0, h->r_embln.g, h->r_embln.b, 1e-5f, nullptr,
                                w.r_xb, B, L, 768, 1, s, x));
  }
  // GEMM kind k on hi / lo operands (bit k of text_prec_mask): the K-concatenated weight, K = 3 in;
  // otherwise the fp16 weight against the hi third of the same operand rows (K = in): fp16 x fp16
  // products, fp32 accumulation and output.  split3 writes the lo / second hi thirds only for a
  // consumer that reads them.
  auto lin = [&](const f16_t* A, int lda, const Lin16& fast, const Lin16& prec, int kind) {
    if (!(pm >> kind & 1)) return gemm_args(A, lda, fast, M);
    GemmArgs g = gemm_args(A, lda, prec, M);
    if (!(pw >> kind & 1)) g.K = 2 * fast.in;  // the first two thirds of the concatenated rows
    return g;
  };
  HIPCHK(launch_split3(x, 768, w.s3, M, 768, s, pm & 1));
  for (int i = 0; i < 12; ++i) {
    const EncLayer& Ly = h->r_layers[i];
    GemmArgs g = with_ws(lin(w.s3, 2304, Ly.qkv, Ly.qkv3, 0), w.sk_text, w.sk_elems);
    g.c32 = w.p32;
    g.ldc = 2304;
    CHK(gemm(h, g, s));
    {
      ProfScope ps(h, s, PK_ATTN, 4.0 * B * 12 * (double)L * L * 64, (double)M * (2304 + 768) * 4);
      // ctx straight into the out-projection's operand rows (no fp32 ctx / split3 pass)
      HIPCHK(launch_attention32(w.p32, 2304, 768, 1536, mask, y, 768, B, L, 12, s, w.s3, pm >> 1 & 1));
    }
    g = with_ws(lin(w.s3, 2304, Ly.o, Ly.o3, 1), w.sk_text, w.sk_elems);
    g.c32 = y;
    CHK(gemm(h, g, s));
    {  // x = LN1(x + y) and FFN-1's operand rows of it, one pass
      ProfScope ps(h, s, PK_LN, 9.0 * M * 768, (double)M * 768 * 14);
      HIPCHK(launch_layernorm_split3(x, y, Ly.ln1.g, Ly.ln1.b, 1e-5f, w.s3, pm >> 2 & 1, M, 768, s));
    }
    g = with_ws(lin(w.s3, 2304, Ly.fc1, Ly.fc13, 2), w.sk_text, w.sk_elems);
    g.act = 1;  // GELU-erf
    // the hidden straight into FFN-2's operand rows (epilogue 4: hi | lo | hi, no fp32 hidden and
    // no split3 pass: -8 B of HBM traffic per hidden element); the fp32 + split3 path where the
    // persistent tiles do not apply (small batches)
    GemmArgs ge = g;
    ge.epi = 4;
    ge.split_lo = pm >> 3 & 1;
    ge.c16 = w.h3;
    ge.ldc = 9216;
    if (gemm_epi_ok(ge)) {
      CHK(gemm(h, ge, s));
    } else {
      g.c32 = w.p32;
      g.ldc = 3072;
      CHK(gemm(h, g, s));
      HIPCHK(launch_split3(w.p32, 3072, w.h3, M, 3072, s, pm >> 3 & 1));
    }
    g = with_ws(lin(w.h3, 9216, Ly.fc2, Ly.fc23, 3), w.sk_text, w.sk_elems);
    g.c32 = y;
    CHK(gemm(h, g, s));
    if (i < 11) {  // x = LN2(x + y) and the next layer's QKV operand rows of it
      ProfScope ps(h, s, PK_LN, 9.0 * M * 768, (double)M * 768 * 14);
      HIPCHK(launch_layernorm_split3(x, y, Ly.ln2.g, Ly.ln2.b, 1e-5f, w.s3, pm & 1, M, 768, s));
    } else {  // x = LN2(x + y) in fp32, in place (layernorm_kernel reads a row before writing it)
      ProfScope ps(h, s, PK_LN, 9.0 * M * 768, (double)M * 768 * 12);
      HIPCHK(launch_layernorm(x, 768, y, 768, Ly.ln2.g, Ly.ln2.b, 1e-5f, x, 768, nullptr, 0, M, 768, s));
    }
  }
  if (cls) {  // mmf_text_pooled: the CLS rows instead of the heads
    HIPCHK(launch_text_cls_rows(x, L * 768, nullptr, cls, B, s));
    return 0;
  }
  ProfScope ps(h, s, PK_HEADS, 2.0 * B * 2 * (768 * 256 + 256 * 2), (double)B * 768 * 4 + 2 * 768 * 256 * 4);
  HIPCHK(launch_text_heads(x, L * 768, h->h_w1a, h->h_b1a, h->h_w2a, h->h_b2a, h->h_w1m, h->h_b1m, h->h_w2m,
                           h->h_b2m, ai, mi, scores, score_stride, B, s));
  return 0;
}

}  // namespace

int run_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* ai, float* mi,
             float* scores, int score_stride, hipStream_t s, hipEvent_t heads_ev, float* cls) {
  Workspace& w = h->ws;
  const int hilo = text_mode(h);
  if (hilo >= 2) {
    CHK(run_text_precise(h, ids, mask, B, L, ai, mi, scores, score_stride, s, cls));
    if (heads_ev) HIPCHK(hipEventRecord(heads_ev, s));
    return 0;
  }
  uint16_t* rlo = hilo ? w.r_lo : nullptr;
  const int M = B * L;
  // overflow sentinel: a sequence whose fp16 stream or branch output leaves fp16's range gets NaN
  // scores (the masked softmax would hide it; engine.py's run-time trap then re-runs the batch in the
  // precise mode)
  int* ovf = w.r_ovf;
  HIPCHK(hipMemsetAsync(ovf, 0, (size_t)B * sizeof(int), s));
  {
    ProfScope ps(h, s, PK_EMBED, 10.0 * M * 768, (double)M * 768 * (4 + 4 + 2 + 2));
    HIPCHK(launch_roberta_embed(ids, h->r_word, h->r_pos, h->r_type0, h->r_embln.g, h->r_embln.b, 1e-5f, rlo,
                                w.r_xb, B, L, 768, 1, s, nullptr, ovf));
  }
  for (int i = 0; i < 12; ++i) {
    const EncLayer& Ly = h->r_layers[i];
    // last layer: only the CLS row feeds the heads (misinfo_forensics.py:95), so the rows below
    // run on B compact CLS rows (strided A / residual reads) instead of B*L rows
    const bool last = (i == 11);
    GemmArgs g;
    // (split-stream mode -- outlier-feature checkpoints, which sit at the parity bar: DESIGN §4 --
    // keeps the full last-layer attention, whose roundings were measured there)
    if (last && (h->opt.last_q1 & 1) && !rlo) {
      // ... and of its attention only the CLS queries are needed: K and V of every row (the fused
      // weight's rows 768..2303: 3 whole persistent rounds at M = 32768 instead of 4.5), Q of the
      // B CLS rows (skinny, split-K), one query per (sequence, head) (attention_q1_kernel) written
      // to the CLS rows of r_ctx
      g = with_ws(gemm_args(w.r_xb, 768, rows_of(Ly.qkv, 768, 1536), M), w.sk_text, w.sk_elems);
      g.c16 = w.r_qkv + 768;
      g.ldc = 2304;
      CHK(gemm(h, g, s));
      // Q of the CLS rows in fp32 (r_y is free until hilo_rows below); with the split stream the
      // lo word is added by a second skinny GEMM (q = Wq hi + bq + Wq lo: the ~22-bit row)
      const Lin16 qq = rows_of(Ly.qkv, 0, 768);
      float* qcls = w.r_y;
      g = with_ws(gemm_args(w.r_xb, L * 768, qq, B), w.sk_text, w.sk_elems);
      g.c32 = qcls;
      CHK(gemm(h, g, s));
      if (rlo) {
        g = with_ws(gemm_args(reinterpret_cast<const f16_t*>(rlo), L * 768, qq, B), w.sk_text, w.sk_elems);
        g.bias = nullptr;
        g.res32 = qcls;
        g.c32 = qcls;
        CHK(gemm(h, g, s));
      }
      ProfScope ps(h, s, PK_ATTN, 4.0 * B * 12 * (double)L * 64, (double)B * L * 768 * 2 * 2);
      HIPCHK(launch_attention_q1(qcls, 768, w.r_qkv, 2304, 768, 1536, mask, nullptr, w.r_ctx, L * 768, B, L, 12, s));
    } else if (h->opt.qkv_attn && L == 128 && M > 512) {
      // the attention of each (two sequences, head) tile inside the QKV GEMM's epilogue: ctx is
      // written directly (bit-identical to the two launches below, tests/test_gpu_parity.py)
      g = gemm_args(w.r_xb, 768, Ly.qkv_h, M);
      g.epi = 3;
      g.amask = mask;
      g.c16 = w.r_ctx;
      g.ldc = 768;
      CHK(gemm(h, g, s));
    } else {
      // (M <= 512, a single text or a few: split-K through the workspace, gemm_splitk_factor)
      g = with_ws(gemm_args(w.r_xb, 768, Ly.qkv, M), w.sk_text, w.sk_elems);
      g.c16 = w.r_qkv;
      CHK(gemm(h, g, s));
      CHK(attn(h, w.r_qkv, 2304, mask, w.r_ctx, 768, B, L, 12, 0, s));
    }
    if (!last) {
      // out-proj and FFN-2 write their fp16 branch output y; the residual add happens in fp32
      // inside add+LN (y lives in r_h, free until FFN-1, then in r_ctx, free after out-proj)
      f16_t* y = w.r_h;
      g = with_ws(gemm_args(w.r_ctx, 768, Ly.o, M), w.sk_text, w.sk_elems);
      g.c16 = y;
      CHK(gemm(h, g, s));
      CHK(add_ln_hilo(h, w.r_xb, rlo, 768, y, 768, Ly.ln1, M, s, ovf, L));
      g = with_ws(gemm_args(w.r_xb, 768, Ly.fc1, M), w.sk_text, w.sk_elems);
      g.act = 1;  // GELU-erf
      g.c16 = w.r_h;
      CHK(gemm(h, g, s));
      y = w.r_ctx;
      g = with_ws(gemm_args(w.r_h, 3072, Ly.fc2, M), w.sk_text, w.sk_elems);
      g.c16 = y;
      CHK(gemm(h, g, s));
      CHK(add_ln_hilo(h, w.r_xb, rlo, 768, y, 768, Ly.ln2, M, s, ovf, L));
      continue;
    }
    const int Mr = last ? B : M;            // rows after the attention
    const int rs = last ? L * 768 : 768;    // row stride of ctx at this point
    // the B CLS rows of the split residual stream, as fp32 (r_y, compact)
    HIPCHK(launch_hilo_rows(w.r_xb, rlo, rs, w.r_y, B, 768, s));
    g = with_ws(gemm_args(w.r_ctx, rs, Ly.o, Mr), w.sk_text, w.sk_elems);
    g.res32 = w.r_y;
    g.ldr = 768;
    g.c32 = w.r_y;
    CHK(gemm(h, g, s));
    CHK(lnorm(h, w.r_y, 768, Ly.ln1, last ? w.r_y : w.r_x, 768, w.r_xb, 768, Mr, 768, s));
    g = with_ws(gemm_args(w.r_xb, 768, Ly.fc1, Mr), w.sk_text, w.sk_elems);
    g.act = 1;  // GELU-erf
    g.c16 = w.r_h;
    CHK(gemm(h, g, s));
    g = with_ws(gemm_args(w.r_h, 3072, Ly.fc2, Mr), w.sk_text, w.sk_elems);
    g.res32 = last ? w.r_y : w.r_x;
    g.c32 = last ? w.r_x : w.r_y;
    CHK(gemm(h, g, s));
    CHK(lnorm(h, last ? w.r_x : w.r_y, 768, Ly.ln2, w.r_x, 768, w.r_xb, 768, Mr, 768, s));
  }
  // w.r_x now holds the B final CLS rows, compact
  if (cls) {  // mmf_text_pooled: the CLS rows instead of the heads
    HIPCHK(launch_text_cls_rows(w.r_x, 768, ovf, cls, B, s));
    return 0;
  }
  if (heads_ev) HIPCHK(hipEventRecord(heads_ev, s));
  ProfScope ps(h, s, PK_HEADS, 2.0 * B * 2 * (768 * 256 + 256 * 2), (double)B * 768 * 4 + 2 * 768 * 256 * 4);
  HIPCHK(launch_text_heads(w.r_x, 768, h->h_w1a, h->h_b1a, h->h_w2a, h->h_b2a, h->h_w1m, h->h_b1m, h->h_w2m,
                           h->h_b2m, ai, mi, scores, score_stride, B, s, ovf));
  return 0;
}
