// The launch sequences of the two CLIP towers (ViT-B/32 and the text transformer): embed, the shared
// pre-LN encoder (lazy or materialised LayerNorms), and the pooled-row tail.
#include "handle.h"

namespace {

// Lazy LayerNorm (option lazy_ln, gemm.hip): a row stream's statistics as partials
struct LnStats {
  float2* p = nullptr;  // [rows padded to 256][P]
  int P = 0, tn = 0;
};
// consumer: LN(s) W^T + b with the LN folded into (w', u, c) -- s = raw rows with statistics st
GemmArgs ln_consumer(const f16_t* s_rows, int ld, const Lin16& folded, const float* u, const LnStats& st, int M) {
  GemmArgs g = gemm_args(s_rows, ld, folded, M);
  g.epi = 1;
  g.ln_in = st.p;
  g.ln_in_P = st.P;
  g.ln_in_tn = st.tn;
  g.ln_u = u;
  g.ln_eps = 1e-5f;
  return g;
}
// producer: stream += A W^T + b in place; the new stream's statistics go to `out`
GemmArgs ln_producer(const Options& o, const f16_t* A, int lda, const Lin16& l, f16_t* stream, int M, float2* out,
                     LnStats* produced) {
  GemmArgs g = gemm_args(A, lda, l, M);
  apply_options(o, &g);  // the tile (so the partials' width) depends on options
  g.res16 = stream;
  g.c16 = stream;
  g.ln_out = out;
  g.ln_eps = 1e-5f;
  g.epi = 2;
  produced->p = out;
  produced->tn = gemm_ln_tn(g);
  produced->P = (l.out + produced->tn - 1) / produced->tn;
  return g;
}
// pre-LN CLIP encoder over x (residual stream, in place: fp32, or fp16 when opt.clip_res16) with
// xb = LN1_0(x) already computed
// Only one row per sequence is consumed after the last layer (CLS for the ViT, EOS for the text
// tower: TF clip:561-582, 650-651): the last layer's out-proj / MLP run on those B rows, gathered
// into compact buffers (xc fp32, ctxc fp16); on return xc holds them (before the final LN).
// independent of the batch size: rows must not change with the batch they run in (the lazy and
// materialised LayerNorms round differently), so sharding rows over GPUs keeps results bit-identical
// The exception is the latency regime: below kLazyMinRows rows (a ViT batch of <= 5 images, a text
// batch of <= 3 captions: analyze() one pair at a time) the 256-row lazy-LN tiles leave all but a
// few CUs idle (4-12 workgroups walking K = 768-3072: 20-37 us per GEMM at B = 1), so those batches
// run the materialised LayerNorms with split-K GEMMs; rows of batches >= 8 (the bench, shards) stay
// bit-identical across batch sizes (tests/test_gpu_parity.py), small batches match them to rounding.
constexpr int kLazyMinRows = 256;
bool clip_lazy(mmf_handle* h, int M) { return h->opt.lazy_ln && h->opt.clip_res16 && M >= kLazyMinRows; }

// One CLIP tower's encoder pass: its weights, workspaces and (lazy LN) the statistics of its stream
struct ClipEnc {
  EncLayer* layers;
  int H, I, heads;
  float* x;  // residual stream (fp32, or fp16 when opt.clip_res16: x16)
  f16_t *x16, *xb, *qkv, *ctx, *hid;
  const int32_t* mask;
  int causal, B, L, M;
  const int32_t* last_rows;
  float* xc;
  f16_t* ctxc;
  float* skws;
  size_t sk_elems;
  float2* const* st;
  bool lazy;
  LnStats cur;  // lazy LN: partials of the current stream
  int sti;      // which of the two partial buffers holds them
  bool qkv_attn;  // lazy LN: attention in the QKV consumer's epilogue (option clip_qkv_attn)
};
// option clip_qkv_attn for a tower: 1 = both, else a bitmask (2 ViT, 4 text tower)
bool clip_qkv_attn_on(const mmf_handle* h, int bit) { return h->opt.clip_qkv_attn == 1 || (h->opt.clip_qkv_attn & bit); }

ClipEnc vit_enc(mmf_handle* h, int B) {
  Workspace& w = h->ws;
  const int M = B * 50;
  return ClipEnc{h->v_layers, 768, 3072, 12, w.v_x, h->opt.clip_res16 ? reinterpret_cast<f16_t*>(w.v_x) : nullptr,
                 w.v_xb, w.v_qkv, w.v_ctx, w.v_h, nullptr, 0, B, 50, M, nullptr, w.v_xc, w.v_ctxc, w.sk_vit,
                 w.sk_elems, w.v_st, clip_lazy(h, M), LnStats{w.v_st[0], 1, 768}, 0, clip_qkv_attn_on(h, 2)};
}
ClipEnc text_enc(mmf_handle* h, const int32_t* mask, int B, int L) {
  Workspace& w = h->ws;
  const int M = B * L;
  return ClipEnc{h->t_layers, 512, 2048, 8, w.t_x, h->opt.clip_res16 ? reinterpret_cast<f16_t*>(w.t_x) : nullptr,
                 w.t_xb, w.t_qkv, w.t_ctx, w.t_h, mask, 1, B, L, M, w.t_eos, w.t_xc, w.t_ctxc, w.sk_ctext,
                 w.sk_elems, w.t_st, clip_lazy(h, M), LnStats{w.t_st[0], 1, 512}, 0, clip_qkv_attn_on(h, 4)};
}

// the four GEMMs of a lazy-LN layer (not the last): QKV and FFN-1 read the raw stream with LN1 / LN2
// folded (consumers), out-proj and FFN-2 add into the stream and write its next partials (producers)
GemmArgs lazy_qkv(ClipEnc& E, int i) {
  const EncLayer& Ly = E.layers[i];
  GemmArgs g = ln_consumer(E.x16, E.H, Ly.qkv_f, Ly.qkv_u, E.cur, E.M);
  g.c16 = E.qkv;
  return g;
}
// the same consumer on the per-head interleaved folded weights with the attention of its rows in the
// epilogue (gemm.hip epi 5): ctx straight from the stream, qkv never stored
GemmArgs lazy_qkv_attn(ClipEnc& E, int i) {
  const EncLayer& Ly = E.layers[i];
  GemmArgs g = ln_consumer(E.x16, E.H, Ly.qkv_fh, Ly.qkv_uh, E.cur, E.M);
  g.epi = 5;
  g.c16 = E.ctx;
  g.ldc = E.H;
  g.amask = E.mask;
  g.att_L = E.L;
  g.att_causal = E.causal;
  return g;
}
GemmArgs lazy_producer(mmf_handle* h, ClipEnc& E, const f16_t* A, int lda, const Lin16& l) {
  LnStats nxt;
  E.sti ^= 1;
  GemmArgs g = ln_producer(h->opt, A, lda, l, E.x16, E.M, E.st[E.sti], &nxt);
  E.cur = nxt;
  return g;
}
GemmArgs lazy_o(mmf_handle* h, ClipEnc& E, int i) { return lazy_producer(h, E, E.ctx, E.H, E.layers[i].o); }
GemmArgs lazy_fc1(ClipEnc& E, int i) {
  const EncLayer& Ly = E.layers[i];
  GemmArgs g = ln_consumer(E.x16, E.H, Ly.fc1_f, Ly.fc1_u, E.cur, E.M);
  g.act = 2;  // quick_gelu
  g.c16 = E.hid;
  return g;
}
GemmArgs lazy_fc2(mmf_handle* h, ClipEnc& E, int i) { return lazy_producer(h, E, E.hid, E.I, E.layers[i].fc2); }

// pre-LN CLIP encoder layers [i0, i1) over E.x (residual stream, in place: fp32, or fp16 when
// opt.clip_res16) with xb = LN1_0(x) already computed (materialised mode) or its statistics in
// st[0] (lazy mode)
int run_clip_encoder(mmf_handle* h, ClipEnc& E, int i0, int i1, hipStream_t s) {
  const int M = E.M, H = E.H, I = E.I, B = E.B, L = E.L;
  // lazy LN (gemm.hip; the caller's embedding wrote st[0] with the stream's statistics): the QKV /
  // FFN-1 GEMMs read the raw stream x16 with LN1 / LN2 folded, out-proj / FFN-2 add into it
  for (int i = i0; i < i1; ++i) {
    const EncLayer& Ly = E.layers[i];
    GemmArgs g;
    if (i == 11 && (h->opt.last_q1 & 2)) {
      // only the pooled rows' queries are needed in the last layer: their stream rows -> xc (fp32,
      // also the residual below), LN1 -> Q (skinny GEMM on the unfolded weights), K and V of every
      // row (the fused weight's rows H..3H; lazy consumer or materialised), one query per
      // (sequence, head) straight into the compact ctxc
      HIPCHK(launch_gather_rows2(nullptr, E.x16 ? nullptr : E.x, E.x16, E.last_rows, L, H, nullptr, E.xc, B, s));
      f16_t* xq = E.hid;                   // hid ([M][I] fp16) is free until FFN-1
      float* qc = reinterpret_cast<float*>(E.hid + (size_t)B * H);  // fp32 queries
      CHK(lnorm(h, E.xc, H, Ly.ln1, nullptr, 0, xq, H, B, H, s));
      g = with_ws(gemm_args(xq, H, rows_of(Ly.qkv, 0, H), B), E.skws, E.sk_elems);
      g.c32 = qc;
      CHK(gemm(h, g, s));
      // (the folded c and u are padded by 256 past 3H: the 256-column DMA stays in bounds)
      if (E.lazy) g = ln_consumer(E.x16, H, rows_of(Ly.qkv_f, H, 2 * H), Ly.qkv_u + H, E.cur, M);
      else g = with_ws(gemm_args(E.xb, H, rows_of(Ly.qkv, H, 2 * H), M), E.skws, E.sk_elems);
      g.c16 = E.qkv + H;
      g.ldc = 3 * H;
      CHK(gemm(h, g, s));
      {
        ProfScope ps(h, s, PK_ATTN, 4.0 * B * E.heads * (double)L * 64, (double)B * L * H * 2 * 2);
        HIPCHK(launch_attention_q1(qc, H, E.qkv, 3 * H, H, 2 * H, E.mask, E.causal ? E.last_rows : nullptr, E.ctxc, H,
                                   B, L, E.heads, s));
      }
    } else {
      bool fused = false;
      if (E.lazy && E.qkv_attn && L <= 128) {
        g = lazy_qkv_attn(E, i);
        fused = gemm_epi_ok(g);
      }
      if (fused) {
        CHK(gemm(h, g, s));
      } else {
        g = E.lazy ? lazy_qkv(E, i) : with_ws(gemm_args(E.xb, H, Ly.qkv, M), E.skws, E.sk_elems);
        if (!E.lazy) g.c16 = E.qkv;
        CHK(gemm(h, g, s));
        CHK(attn(h, E.qkv, 3 * H, E.mask, E.ctx, H, B, L, E.heads, E.causal, s));
      }
    }
    if (i == 11) {
      if (!(h->opt.last_q1 & 2))
        HIPCHK(launch_gather_rows2(E.ctx, E.x16 ? nullptr : E.x, E.x16, E.last_rows, L, H, E.ctxc, E.xc, B, s));
      g = with_ws(gemm_args(E.ctxc, H, Ly.o, B), E.skws, E.sk_elems);
      g.res32 = E.xc;
      g.c32 = E.xc;
      CHK(gemm(h, g, s));
      CHK(lnorm(h, E.xc, H, Ly.ln2, nullptr, 0, E.xb, H, B, H, s));
      g = with_ws(gemm_args(E.xb, H, Ly.fc1, B), E.skws, E.sk_elems);
      g.act = 2;  // quick_gelu
      g.c16 = E.hid;
      CHK(gemm(h, g, s));
      g = with_ws(gemm_args(E.hid, I, Ly.fc2, B), E.skws, E.sk_elems);
      g.res32 = E.xc;
      g.c32 = E.xc;
      CHK(gemm(h, g, s));
      break;
    }
    if (E.lazy) {
      CHK(gemm(h, lazy_o(h, E, i), s));
      CHK(gemm(h, lazy_fc1(E, i), s));
      CHK(gemm(h, lazy_fc2(h, E, i), s));
      continue;
    }
    // out-proj / FFN-2 write their fp16 branch output y (out-proj into `hid`, free until FFN-1;
    // FFN-2 into `ctx`, free after out-proj); add+LN adds it to the fp32 residual stream x in place
    // (skinny M <= 512: split-K through the tower's workspace, gemm_splitk_factor)
    // layer i + 1 < 12 always holds here (layer 11 takes the compact branch above)
    auto add = [&](const f16_t* y, const LNp& ln) {
      return E.x16 ? add_ln(h, E.x16, H, y, H, ln, E.xb, H, M, H, s)
                   : add_ln(h, E.x, H, y, H, ln, E.x, nullptr, E.xb, H, M, H, s);
    };
    g = with_ws(gemm_args(E.ctx, H, Ly.o, M), E.skws, E.sk_elems);
    g.c16 = E.hid;
    CHK(gemm(h, g, s));
    CHK(add(E.hid, Ly.ln2));
    g = with_ws(gemm_args(E.xb, H, Ly.fc1, M), E.skws, E.sk_elems);
    g.act = 2;  // quick_gelu
    g.c16 = E.hid;
    CHK(gemm(h, g, s));
    g = with_ws(gemm_args(E.hid, I, Ly.fc2, M), E.skws, E.sk_elems);
    g.c16 = E.ctx;
    CHK(gemm(h, g, s));
    CHK(add(E.ctx, E.layers[i + 1].ln1));
  }
  return 0;
}

int clip_image_embed(mmf_handle* h, const uint8_t* img, int B, hipStream_t s) {
  Workspace& w = h->ws;
  {
    ProfScope ps(h, s, PK_IM2COL, 2.0 * B * 49 * 3072, (double)B * 49 * 3072 * (1 + 2));
    HIPCHK(launch_clip_im2col(img, w.v_col, B, s));
  }
  const Lin16 pe{h->v_patch_w, nullptr, 768, 3072};
  GemmArgs g = gemm_args(w.v_col, 3072, pe, B * 49);
  g.c32 = w.v_patch;
  CHK(gemm(h, g, s));
  ProfScope ps(h, s, PK_EMBED, 16.0 * B * 50 * 768, (double)B * 50 * 768 * (4 + 4 + 2));
  HIPCHK(launch_clip_vision_assemble(w.v_patch, h->v_cls, h->v_pos, h->v_pre.g, h->v_pre.b, h->v_layers[0].ln1.g,
                                     h->v_layers[0].ln1.b, 1e-5f, h->opt.clip_res16 ? nullptr : w.v_x,
                                     h->opt.clip_res16 ? reinterpret_cast<f16_t*>(w.v_x) : nullptr, w.v_xb,
                                     clip_lazy(h, B * 50) ? w.v_st[0] : nullptr, B, s));
  return 0;
}

int clip_text_embed(mmf_handle* h, const int32_t* ids, int B, int L, hipStream_t s) {
  Workspace& w = h->ws;
  {
    ProfScope ps(h, s, PK_EMBED, 10.0 * B * L * 512, (double)B * L * 512 * (4 + 4 + 4 + 2));
    HIPCHK(launch_clip_text_embed(ids, h->t_tok, h->t_pos, h->t_layers[0].ln1.g, h->t_layers[0].ln1.b, 1e-5f,
                                  h->opt.clip_res16 ? nullptr : w.t_x,
                                  h->opt.clip_res16 ? reinterpret_cast<f16_t*>(w.t_x) : nullptr, w.t_xb,
                                  clip_lazy(h, B * L) ? w.t_st[0] : nullptr, B, L, 512, s));
  }
  HIPCHK(launch_eos_index(ids, w.t_eos, B, L, h->eos_id, s));
  return 0;
}

// the pooled rows xc -> final LayerNorm (fp16 `pooled`) -> projection [512][in] -> unit-norm emb [B][512]
int clip_tail(mmf_handle* h, const float* xc, const LNp& ln, f16_t* pooled, f16_t* proj, int in, float* sk, int B,
              float* emb, hipStream_t s) {
  HIPCHK(launch_gather_ln(xc, nullptr, 1, ln.g, ln.b, 1e-5f, pooled, nullptr, B, in, s));
  const Lin16 pj{proj, nullptr, 512, in};
  GemmArgs g = with_ws(gemm_args(pooled, in, pj, B), sk, h->ws.sk_elems);
  g.c32 = emb;
  CHK(gemm(h, g, s));
  HIPCHK(launch_l2norm(emb, B, 512, s));
  return 0;
}

}  // namespace

int run_clip_image(mmf_handle* h, const uint8_t* img, int B, float* emb, hipStream_t s) {
  CHK(clip_image_embed(h, img, B, s));
  ClipEnc E = vit_enc(h, B);
  CHK(run_clip_encoder(h, E, 0, 12, s));
  const Workspace& w = h->ws;
  return clip_tail(h, w.v_xc, h->v_post, w.v_cls, h->v_proj, 768, w.sk_vit, B, emb, s);
}

int run_clip_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* emb, hipStream_t s) {
  CHK(clip_text_embed(h, ids, B, L, s));
  ClipEnc E = text_enc(h, mask, B, L);
  CHK(run_clip_encoder(h, E, 0, 12, s));
  const Workspace& w = h->ws;
  return clip_tail(h, w.t_xc, h->t_final, w.t_pool, h->t_proj, 512, w.sk_ctext, B, emb, s);
}

// The towers up to clip_tail's LayerNorm, its fp32 leg alone: what the projection heads read
// (train_clip_detective.py:119-122 with the encoders frozen, :89-99)
int run_clip_image_pooled(mmf_handle* h, const uint8_t* img, int B, float* pooled, hipStream_t s) {
  CHK(clip_image_embed(h, img, B, s));
  ClipEnc E = vit_enc(h, B);
  CHK(run_clip_encoder(h, E, 0, 12, s));
  HIPCHK(launch_gather_ln(h->ws.v_xc, nullptr, 1, h->v_post.g, h->v_post.b, 1e-5f, nullptr, pooled, B, 768, s));
  return 0;
}

int run_clip_text_pooled(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* pooled,
                         hipStream_t s) {
  CHK(clip_text_embed(h, ids, B, L, s));
  ClipEnc E = text_enc(h, mask, B, L);
  CHK(run_clip_encoder(h, E, 0, 12, s));
  HIPCHK(launch_gather_ln(h->ws.t_xc, nullptr, 1, h->t_final.g, h->t_final.b, 1e-5f, nullptr, pooled, B, 512, s));
  return 0;
}
