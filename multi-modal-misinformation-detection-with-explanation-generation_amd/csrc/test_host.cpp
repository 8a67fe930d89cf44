// Test-only entry points: the transformer towers' row kernels (norm.hip), the precise-mode kernels
// (precise.hip), the one-query attention (attention.hip), the split-K skinny GEMM, the lazy-LN consumer and
// producer epilogues and the QKV GEMM's attention epilogue (gemm.hip) on raw device operands (include/mmf_hip.h;
// tests/test_gpu_transformer_kernels.py), the plain GEMM with independent strides (tests/test_gpu_gemm_kernels.py),
// the closing fp32 kernels (misc.hip; tests/test_gpu_misc_kernels.py) and the vault's similarity, top-k and
// candidate-sort stages (vault.hip; tests/test_gpu_vault_kernels.py).  No handle.  Null, shape and alignment
// checks run on the host before anything is launched; what a launcher does not support -- its own
// hipErrorInvalidValue included -- is MMF_EINVAL with nothing written.
#include "handle.h"

namespace {

// a launcher's hipErrorInvalidValue is its "unsupported shape" answer; anything else is a HIP failure
int test_launch_rc(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  if (e == hipErrorInvalidValue) return fail(MMF_EINVAL, "%s: unsupported shape", what);
  return fail(MMF_EIO, "%s: %s", what, hipGetErrorString(e));
}

// the row kernels read and write rows as float4 / 4 x fp16: row strides in whole groups of 4
bool ld4(int ld, int C) { return ld >= C && (ld & 3) == 0; }

}  // namespace

extern "C" {

int mmf_layernorm_f32(const float* x, int ldx, const float* add, int ldadd, const float* g, const float* b, float eps,
                      float* y32, int ldy32, void* y16, int ldy16, int rows, int C, void* stream) {
  if (!x || !g || !b || (!y32 && !y16)) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0 || C <= 0 || !ld4(ldx, C) || (add && !ld4(ldadd, C)) || (y32 && !ld4(ldy32, C)) ||
      (y16 && !ld4(ldy16, C)))
    return fail(MMF_EINVAL, "layernorm: bad shape (rows=%d C=%d ldx=%d ldadd=%d ldy32=%d ldy16=%d)", rows, C, ldx,
                ldadd, ldy32, ldy16);
  return test_launch_rc(launch_layernorm(x, ldx, add, ldadd, g, b, eps, y32, ldy32, (f16_t*)y16, ldy16, rows, C,
                                         (hipStream_t)stream),
                        "layernorm");
}

int mmf_add_ln_f32(const float* x, int ldx, const void* y, int ldy, const float* g, const float* b, float eps,
                   float* s32, float* o32, void* o16, int ldo, int rows, int C, void* stream) {
  if (!x || !y || !g || !b || !o16) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0 || C <= 0 || !ld4(ldx, C) || !ld4(ldy, C) || !ld4(ldo, C))
    return fail(MMF_EINVAL, "add_ln: bad shape (rows=%d C=%d ldx=%d ldy=%d ldo=%d)", rows, C, ldx, ldy, ldo);
  return test_launch_rc(launch_add_ln(x, ldx, (const f16_t*)y, ldy, g, b, eps, s32, o32, (f16_t*)o16, ldo, rows, C,
                                      (hipStream_t)stream),
                        "add_ln");
}

int mmf_add_ln_f16(const void* x16, int ldx, const void* y, int ldy, const float* g, const float* b, float eps,
                   void* s16, void* o16, int ldo, int rows, int C, void* stream) {
  if (!x16 || !y || !g || !b || !o16) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0 || C <= 0 || !ld4(ldx, C) || !ld4(ldy, C) || !ld4(ldo, C))
    return fail(MMF_EINVAL, "add_ln: bad shape (rows=%d C=%d ldx=%d ldy=%d ldo=%d)", rows, C, ldx, ldy, ldo);
  return test_launch_rc(launch_add_ln((const f16_t*)x16, ldx, (const f16_t*)y, ldy, g, b, eps, (f16_t*)s16,
                                      (f16_t*)o16, ldo, rows, C, (hipStream_t)stream),
                        "add_ln (fp16 stream)");
}

int mmf_add_ln_hilo_f16(void* hi, void* lo, int ld, const void* y, int ldy, const float* g, const float* b, float eps,
                        int rows, int C, int32_t* ovf, int L, void* stream) {
  if (!hi || !y || !g || !b) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0 || C <= 0 || ld < C || ldy < C)
    return fail(MMF_EINVAL, "add_ln_hilo: bad shape (rows=%d C=%d ld=%d ldy=%d)", rows, C, ld, ldy);
  return test_launch_rc(launch_add_ln_hilo((f16_t*)hi, (uint16_t*)lo, ld, (const f16_t*)y, ldy, g, b, eps, rows, C,
                                           (hipStream_t)stream, ovf, L),
                        "add_ln_hilo");
}

int mmf_hilo_rows_f32(const void* hi, const void* lo, int row_stride, float* out, int B, int C, void* stream) {
  if (!hi || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || C <= 0 || row_stride < C)
    return fail(MMF_EINVAL, "hilo_rows: bad shape (B=%d C=%d row_stride=%d)", B, C, row_stride);
  return test_launch_rc(
      launch_hilo_rows((const f16_t*)hi, (const uint16_t*)lo, row_stride, out, B, C, (hipStream_t)stream), "hilo_rows");
}

int mmf_layernorm_split3_f32(float* x, const float* add, const float* g, const float* b, float eps, void* s3,
                             int with_lo, int rows, int C, void* stream) {
  if (!x || !add || !g || !b || !s3) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0) return fail(MMF_EINVAL, "layernorm_split3: bad shape (rows=%d)", rows);
  return test_launch_rc(launch_layernorm_split3(x, add, g, b, eps, (f16_t*)s3, with_lo, rows, C, (hipStream_t)stream),
                        "layernorm_split3");
}

int mmf_roberta_embed_f32(const int32_t* ids, const float* word, const float* pos, const float* type0, const float* g,
                          const float* b, float eps, void* xlo, void* xb, float* x32, int32_t* ovf, int B, int L, int H,
                          int pad_id, void* stream) {
  if (!ids || !word || !pos || !type0 || !g || !b || (!xb && !x32)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || L <= 0 || pad_id < 0)
    return fail(MMF_EINVAL, "roberta_embed: bad shape (B=%d L=%d pad_id=%d)", B, L, pad_id);
  return test_launch_rc(launch_roberta_embed(ids, word, pos, type0, g, b, eps, (uint16_t*)xlo, (f16_t*)xb, B, L, H,
                                             pad_id, (hipStream_t)stream, x32, ovf),
                        "roberta_embed");
}

int mmf_clip_text_embed_f32(const int32_t* ids, const float* tok, const float* pos, const float* g, const float* b,
                            float eps, float* x, void* x16, void* xb, void* st, int B, int L, int H, void* stream) {
  if (!ids || !tok || !pos || !g || !b || (!xb && !st)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || L <= 0) return fail(MMF_EINVAL, "clip_text_embed: bad shape (B=%d L=%d)", B, L);
  return test_launch_rc(launch_clip_text_embed(ids, tok, pos, g, b, eps, x, (f16_t*)x16, (f16_t*)xb, (float2*)st, B, L,
                                               H, (hipStream_t)stream),
                        "clip_text_embed");
}

int mmf_clip_vision_assemble_f32(const float* patches, const float* cls, const float* pos, const float* pre_g,
                                 const float* pre_b, const float* ln1_g, const float* ln1_b, float eps, float* x,
                                 void* x16, void* xb, void* st, int B, void* stream) {
  if (!patches || !cls || !pos || !pre_g || !pre_b || !ln1_g || !ln1_b || (!xb && !st))
    return fail(MMF_EINVAL, "null argument");
  if (B <= 0) return fail(MMF_EINVAL, "clip_vision_assemble: bad batch %d", B);
  return test_launch_rc(launch_clip_vision_assemble(patches, cls, pos, pre_g, pre_b, ln1_g, ln1_b, eps, x, (f16_t*)x16,
                                                    (f16_t*)xb, (float2*)st, B, (hipStream_t)stream),
                        "clip_vision_assemble");
}

int mmf_clip_im2col_f16(const uint8_t* img, void* A, int B, void* stream) {
  if (!img || !A) return fail(MMF_EINVAL, "null argument");
  if (B <= 0) return fail(MMF_EINVAL, "clip_im2col: bad batch %d", B);
  return test_launch_rc(launch_clip_im2col(img, (f16_t*)A, B, (hipStream_t)stream), "clip_im2col");
}

int mmf_eos_index_i32(const int32_t* ids, int32_t* out, int B, int L, int eos_id, void* stream) {
  if (!ids || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || L <= 0) return fail(MMF_EINVAL, "eos_index: bad shape (B=%d L=%d)", B, L);
  return test_launch_rc(launch_eos_index(ids, out, B, L, eos_id, (hipStream_t)stream), "eos_index");
}

int mmf_gather_ln_f32(const float* x, const int32_t* idx, int L, const float* g, const float* b, float eps, void* out16,
                      float* out32, int B, int C, void* stream) {
  if (!x || !g || !b || (!out16 && !out32)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || L <= 0) return fail(MMF_EINVAL, "gather_ln: bad shape (B=%d L=%d)", B, L);
  return test_launch_rc(launch_gather_ln(x, idx, L, g, b, eps, (f16_t*)out16, out32, B, C, (hipStream_t)stream),
                        "gather_ln");
}

int mmf_gather_rows2(const void* a16, const float* a32, const void* a32h, const int32_t* idx, int L, int C, void* o16,
                     float* o32, int B, void* stream) {
  if (!o32 || (a16 && !o16)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || B > 65535 || L <= 0 || C <= 0) return fail(MMF_EINVAL, "gather_rows2: bad shape (B=%d L=%d C=%d)", B, L, C);
  return test_launch_rc(launch_gather_rows2((const f16_t*)a16, a32, (const f16_t*)a32h, idx, L, C, (f16_t*)o16, o32, B,
                                            (hipStream_t)stream),
                        "gather_rows2");
}

int mmf_l2norm_f32(float* x, int B, int C, void* stream) {
  if (!x) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || C <= 0 || (C & 63)) return fail(MMF_EINVAL, "l2norm: bad shape (B=%d C=%d)", B, C);
  return test_launch_rc(launch_l2norm(x, B, C, (hipStream_t)stream), "l2norm");
}

int mmf_split3_f32(const float* x, int ldx, void* out, int rows, int C, int with_lo, void* stream) {
  if (!x || !out) return fail(MMF_EINVAL, "null argument");
  if (rows <= 0 || C <= 0 || ldx < C) return fail(MMF_EINVAL, "split3: bad shape (rows=%d C=%d ldx=%d)", rows, C, ldx);
  return test_launch_rc(launch_split3(x, ldx, (f16_t*)out, rows, C, (hipStream_t)stream, with_lo), "split3");
}

int mmf_attention32_f32(const float* qkv, int ld, int koff, int voff, const int32_t* mask, float* out, int ldo,
                        void* out3, int with_lo, int B, int L, int H, void* stream) {
  if (!qkv || !out == !out3) return fail(MMF_EINVAL, "attention32: qkv and exactly one of out / out3");
  if (B <= 0 || L <= 0 || H <= 0 || (long)B * H > 65535 || koff < 0 || voff < 0 || ld < koff + H * 64 ||
      ld < voff + H * 64 || (out && ldo < H * 64))
    return fail(MMF_EINVAL, "attention32: bad shape (B=%d L=%d H=%d ld=%d koff=%d voff=%d ldo=%d)", B, L, H, ld, koff,
                voff, ldo);
  return test_launch_rc(launch_attention32(qkv, ld, koff, voff, mask, out, out ? ldo : 4, B, L, H, (hipStream_t)stream,
                                           (f16_t*)out3, with_lo),
                        "attention32");
}

int mmf_attention_q1_f16(const float* q, int ldq, const void* qkv, int ld, int koff, int voff, const int32_t* mask,
                         const int32_t* qpos, void* out, int ldo, int B, int L, int H, void* stream) {
  if (!q || !qkv || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || L <= 0 || H <= 0 || koff < 0 || voff < 0 || ldq < H * 64 || ld < koff + H * 64 || ld < voff + H * 64 ||
      ldo < H * 64)
    return fail(MMF_EINVAL, "attention_q1: bad shape (B=%d L=%d H=%d ldq=%d ld=%d koff=%d voff=%d ldo=%d)", B, L, H, ldq,
                ld, koff, voff, ldo);
  return test_launch_rc(launch_attention_q1(q, ldq, (const f16_t*)qkv, ld, koff, voff, mask, qpos, (f16_t*)out, ldo, B,
                                            L, H, (hipStream_t)stream),
                        "attention_q1");
}

// mmf_gemm_f16 with the split-K workspace of the skinny-M path and either residual kind
static GemmArgs splitk_args(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res32,
                            const void* res16, float* c32, void* c16, int ldc, int M, int N, int K, int act) {
  GemmArgs g{};
  g.A = (const f16_t*)A;
  g.lda = lda;
  g.W = (const f16_t*)W;
  g.ldw = ldw;
  g.bias = bias;
  g.res32 = res32;
  g.res16 = (const f16_t*)res16;
  g.ldr = ldc;
  g.c32 = c32;
  g.c16 = (f16_t*)c16;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  g.act = act;
  apply_options(process_options(), &g);
  return g;
}

int mmf_gemm_splitk_factor(int M, int N, int K, int ldc) {
  if (M <= 0 || N <= 0 || K <= 0 || ldc < N) return fail(MMF_EINVAL, "gemm_splitk_factor: bad shape");
  return gemm_splitk_factor(splitk_args(nullptr, K, nullptr, K, nullptr, nullptr, nullptr, nullptr, nullptr, ldc, M, N, K, 0));
}

int mmf_gemm_f16_splitk(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res32,
                        const void* res16, float* c32, void* c16, int ldc, int M, int N, int K, int act, float* ws,
                        int64_t ws_elems, void* stream) {
  if (!A || !W || (!c32 && !c16)) return fail(MMF_EINVAL, "null argument");
  if (res32 && res16) return fail(MMF_EINVAL, "gemm: at most one of res32 / res16");
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || ws_elems < 0 || act < 0 || act > 4)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d act=%d)", M, N, K, lda, ldw, ldc, act);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, res32, res16, c32, c16, ldc, M, N, K, act);
  g.ws = ws;
  g.ws_elems = ws ? (size_t)ws_elems : 0;
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm");
}

// the epilogue-0 GEMM with every operand and stride independent (tests/test_gpu_gemm_kernels.py): no split-K
// workspace; *config_out = the instantiation launch_gemm runs for exactly these arguments
int mmf_gemm_f16_raw(const void* A, int lda, const void* W, int ldw, const float* bias, const float* res32,
                     const void* res16, int ldr, const float* ascale, int rows_per_batch, float* c32, void* c16,
                     int ldc, int M, int N, int K, int act, int* config_out, void* stream) {
  if (!A || !W || (!c32 && !c16)) return fail(MMF_EINVAL, "null argument");
  if (res32 && res16) return fail(MMF_EINVAL, "gemm: at most one of res32 / res16");
  if (ascale && rows_per_batch <= 0) return fail(MMF_EINVAL, "rows_per_batch must be > 0 with ascale");
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || act < 0 || act > 4)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d act=%d)", M, N, K, lda, ldw, ldc, act);
  if ((res32 || res16) && (ldr < N || (ldr & 3))) return fail(MMF_EINVAL, "gemm: bad residual stride %d (N=%d)", ldr, N);
  if ((K & 7) || (N & 3) || (lda & 7) || (ldw & 7) || (ldc & 3))
    return fail(MMF_EINVAL, "gemm: unsupported shape (N=%d K=%d lda=%d ldw=%d ldc=%d)", N, K, lda, ldw, ldc);
  for (const void* p : {A, W, (const void*)bias, (const void*)res32, res16, (const void*)ascale, (const void*)c32,
                        (const void*)c16})
    if ((uintptr_t)p & 15) return fail(MMF_EINVAL, "gemm: operand %p is not 16-byte aligned", p);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, res32, res16, c32, c16, ldc, M, N, K, act);
  g.ldr = (res32 || res16) ? ldr : 0;
  g.ascale = ascale;
  g.rows_per_batch = rows_per_batch;
  if (config_out) *config_out = gemm_config(g);
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm");
}

int mmf_gemm_f16_ln_consumer(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_in,
                             int P, int tn, const float* ln_u, float eps, void* c16, int ldc, int M, int N, int K,
                             int act, void* stream) {
  if (!A || !W || !bias || !ln_in || !ln_u || !c16) return fail(MMF_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || act < 0 || act > 2)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d act=%d)", M, N, K, lda, ldw, ldc, act);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, nullptr, nullptr, nullptr, c16, ldc, M, N, K, act);
  g.ldr = 0;
  g.epi = 1;
  g.ln_in = (const float2*)ln_in;
  g.ln_in_P = P;
  g.ln_in_tn = tn;
  g.ln_u = ln_u;
  g.ln_eps = eps;
  if (!gemm_epi_ok(g))
    return fail(MMF_EINVAL, "lazy-LN consumer epilogue not applicable (M=%d N=%d K=%d P=%d tn=%d)", M, N, K, P, tn);
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm (lazy-LN consumer)");
}

int mmf_gemm_f16_attn(const void* A, int lda, const void* W, int ldw, const float* bias, const int32_t* amask, void* ctx,
                      int ldc, int M, int N, int K, void* stream) {
  if (!A || !W || !bias || !ctx) return fail(MMF_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d lda=%d ldw=%d)", M, N, K, lda, ldw);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, nullptr, nullptr, nullptr, ctx, ldc, M, N, K, 0);
  g.ldr = 0;
  g.epi = 3;
  g.amask = amask;
  if (!gemm_epi_ok(g))
    return fail(MMF_EINVAL, "attention epilogue not applicable (M=%d N=%d K=%d ldc=%d)", M, N, K, ldc);
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm (attention epilogue)");
}

int mmf_gemm_f16_ln_attn(const void* A, int lda, const void* W, int ldw, const float* bias, const void* ln_in, int P,
                         int tn, const float* ln_u, float eps, const int32_t* amask, int L, int causal, void* ctx,
                         int ldc, int M, int N, int K, void* stream) {
  if (!A || !W || !bias || !ln_in || !ln_u || !ctx) return fail(MMF_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || L <= 0 || lda < K || ldw < K)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d L=%d lda=%d ldw=%d)", M, N, K, L, lda, ldw);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, nullptr, nullptr, nullptr, ctx, ldc, M, N, K, 0);
  g.ldr = 0;
  g.epi = 5;
  g.ln_in = (const float2*)ln_in;
  g.ln_in_P = P;
  g.ln_in_tn = tn;
  g.ln_u = ln_u;
  g.ln_eps = eps;
  g.amask = amask;
  g.att_L = L;
  g.att_causal = causal ? 1 : 0;
  if (!gemm_epi_ok(g))
    return fail(MMF_EINVAL, "lazy-LN attention epilogue not applicable (M=%d N=%d K=%d L=%d P=%d tn=%d ldc=%d)", M, N, K, L,
                P, tn, ldc);
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm (lazy-LN consumer + attention epilogue)");
}

int mmf_gemm_ln_tn(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return fail(MMF_EINVAL, "gemm_ln_tn: bad shape");
  GemmArgs g = splitk_args(nullptr, K, nullptr, K, nullptr, nullptr, nullptr, nullptr, nullptr, N, M, N, K, 0);
  g.epi = 2;
  return gemm_ln_tn(g);
}

int mmf_gemm_f16_ln_producer(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res16,
                             void* c16, int ldc, void* ln_out, int M, int N, int K, void* stream) {
  if (!A || !W || !res16 || !c16 || !ln_out) return fail(MMF_EINVAL, "null argument");
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N)
    return fail(MMF_EINVAL, "gemm: bad shape (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d)", M, N, K, lda, ldw, ldc);
  GemmArgs g = splitk_args(A, lda, W, ldw, bias, nullptr, res16, nullptr, c16, ldc, M, N, K, 0);
  g.epi = 2;
  g.ln_out = (float2*)ln_out;
  if (!gemm_epi_ok(g))
    return fail(MMF_EINVAL, "lazy-LN producer epilogue not applicable (M=%d N=%d K=%d ldc=%d)", M, N, K, ldc);
  return test_launch_rc(launch_gemm(g, (hipStream_t)stream), "gemm (lazy-LN producer)");
}

}  // extern "C"

// ---- the closing fp32 kernels (misc.hip) and the vault's stages (vault.hip) on raw operands
// (tests/test_gpu_misc_kernels.py, tests/test_gpu_vault_kernels.py) ----
namespace {

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

VaultOut vault_out(float thresh, float* sims, int32_t* idx, float* disc, int disc_stride, const float* temb,
                   const float* title, int D, float* tsim) {
  VaultOut o{};
  o.thresh = thresh;
  o.sims = sims;
  o.idx = idx;
  o.disc = disc;
  o.disc_stride = disc_stride;
  o.temb = temb;
  o.title = title;
  o.D = D;
  o.tsim = tsim;
  return o;
}

// what every VaultOut needs whichever kernel fills it
bool vault_out_ok(const VaultOut& o) {
  if (!o.sims && !o.idx && !o.disc && !o.tsim) return false;
  if (o.disc && o.disc_stride < 1) return false;
  if (o.tsim && o.temb && o.title && o.D < 1) return false;
  return true;
}

}  // namespace

extern "C" {

int mmf_text_heads_f32(const float* x, int row_stride, const float* w1a_t, const float* b1a, const float* w2a,
                       const float* b2a, const float* w1m_t, const float* b1m, const float* w2m, const float* b2m,
                       float* ai_logits, float* mi_logits, float* scores, int score_stride, const int32_t* ovf, int B,
                       void* stream) {
  if (!x || !w1a_t || !b1a || !w2a || !b2a || !w1m_t || !b1m || !w2m || !b2m) return fail(MMF_EINVAL, "null argument");
  if (!ai_logits && !mi_logits && !scores) return fail(MMF_EINVAL, "text_heads: no output");
  if (B <= 0 || row_stride < 768 || (scores && score_stride < 2))
    return fail(MMF_EINVAL, "text_heads: bad shape (B=%d row_stride=%d score_stride=%d)", B, row_stride, score_stride);
  return test_launch_rc(launch_text_heads(x, row_stride, w1a_t, b1a, w2a, b2a, w1m_t, b1m, w2m, b2m, ai_logits,
                                          mi_logits, scores, score_stride, B, (hipStream_t)stream, ovf),
                        "text_heads");
}

int mmf_text_cls_rows_f32(const float* x, int row_stride, const int32_t* ovf, float* out, int B, void* stream) {
  if (!x || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || row_stride < 768 || (row_stride & 3) || !al16(x) || !al16(out))
    return fail(MMF_EINVAL, "text_cls_rows: bad shape or alignment (B=%d row_stride=%d)", B, row_stride);
  return test_launch_rc(launch_text_cls_rows(x, row_stride, ovf, out, B, (hipStream_t)stream), "text_cls_rows");
}

int mmf_fusion_raw_f32(const float* x5, const float* w0, const float* b0, const float* w3, const float* b3,
                       const float* w5, const float* b5, float* probs, int32_t* verdict, float* conf, int32_t* rule,
                       int B, void* stream) {
  if (!x5 || !w0 || !b0 || !w3 || !b3 || !w5 || !b5 || !probs) return fail(MMF_EINVAL, "null argument");
  if (B <= 0) return fail(MMF_EINVAL, "fusion: bad batch %d", B);
  return test_launch_rc(launch_fusion(x5, w0, b0, w3, b3, w5, b5, probs, verdict, conf, rule, B, (hipStream_t)stream),
                        "fusion");
}

int mmf_rowdot_f32(const float* a, const float* c, float* out, int ostride, int B, int C, void* stream) {
  if (!a || !c || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || C <= 0 || ostride < 1) return fail(MMF_EINVAL, "rowdot: bad shape (B=%d C=%d ostride=%d)", B, C, ostride);
  return test_launch_rc(launch_rowdot(a, c, out, ostride, B, C, (hipStream_t)stream), "rowdot");
}

int mmf_mixed_finish_raw(const int32_t* row_map, int B, int nT, int nI, int nC, const float* text2,
                         const float* deepfake, const float* v_emb, const float* t_emb, const float* c_sims,
                         const int32_t* c_idx, const float* c_disc, const float* title, float thresh, const float* w0,
                         const float* b0, const float* w3, const float* b3, const float* w5, const float* b5,
                         float* scores5, float* text_sim, float* probs, int32_t* verdict, float* conf, int32_t* rule,
                         float* top_sims, int32_t* top_idx, void* stream) {
  if (nT < 0 || nI < 0 || nC < 0) return fail(MMF_EINVAL, "mixed_finish: bad list sizes (nT=%d nI=%d nC=%d)", nT, nI, nC);
  MixedFinishArgs a{};
  a.row_map = row_map;
  a.B = B; a.nT = nT; a.nI = nI; a.nC = nC;
  a.text2 = text2;
  a.deepfake = deepfake;
  a.v_emb = v_emb;
  a.t_emb = t_emb;
  a.c_sims = c_sims;
  a.c_idx = c_idx;
  a.c_disc = c_disc;
  a.title = title;
  a.thresh = thresh;
  a.w0 = w0; a.b0 = b0; a.w3 = w3; a.b3 = b3; a.w5 = w5; a.b5 = b5;
  a.scores5 = scores5; a.text_sim = text_sim; a.probs = probs;
  a.verdict = verdict; a.conf = conf; a.rule = rule;
  a.top_sims = top_sims; a.top_idx = top_idx;
  return test_launch_rc(launch_mixed_finish(a, (hipStream_t)stream), "mixed_finish");
}

int mmf_vault_sims_f32(const float* q, const float* v, float* S, int B, int N, int D, int ref, void* stream) {
  if (!q || !v || !S) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || N <= 0 || D <= 0 || (D & 63)) return fail(MMF_EINVAL, "vault_sims: bad shape (B=%d N=%d D=%d)", B, N, D);
  if (!al16(q) || !al16(v) || !al16(S)) return fail(MMF_EINVAL, "vault_sims: operands must be 16-byte aligned");
  return test_launch_rc(launch_vault_sims(q, v, S, B, N, D, (hipStream_t)stream, ref), "vault_sims");
}

int mmf_vault_topk_f32(const float* S, int B, int N, int k, float thresh, float* sims, int32_t* idx, float* disc,
                       int disc_stride, const float* temb, const float* title, int D, float* tsim, int ref,
                       void* stream) {
  if (!S) return fail(MMF_EINVAL, "null argument");
  const VaultOut o = vault_out(thresh, sims, idx, disc, disc_stride, temb, title, D, tsim);
  if (B <= 0 || N <= 0 || k <= 0 || !vault_out_ok(o))
    return fail(MMF_EINVAL, "vault_topk: bad shape or no output (B=%d N=%d k=%d disc_stride=%d D=%d)", B, N, k,
                disc_stride, D);
  return test_launch_rc(launch_vault_topk(S, B, N, k, o, (hipStream_t)stream, ref), "vault_topk");
}

// the JPEG round trip's block arithmetic on raw sample blocks (jpeg_encode.hip; tests/test_gpu_jpeg_roundtrip.py).
// The operands are read back and checked here first -- a synchronous call: 32-bit arithmetic holds for
// |sample| <= 1024 and table entries 1..255
int mmf_jpeg_block_roundtrip_raw(const int16_t* blocks, const uint8_t* table, int n, int16_t* coefs, uint8_t* samples,
                                 int32_t* outside, void* stream) {
  if (!blocks || !table || !coefs || !samples || !outside) return fail(MMF_EINVAL, "null argument");
  if (n < 1 || n > (1 << 20)) return fail(MMF_EINVAL, "jpeg_block_roundtrip: n=%d (1..2^20)", n);
  if (((uintptr_t)blocks | (uintptr_t)coefs) & 1 || (uintptr_t)outside & 3)
    return fail(MMF_EINVAL, "jpeg_block_roundtrip: blocks and coefs must be 2-byte aligned, outside 4-byte");
  std::vector<int16_t> host((size_t)n * 64);
  uint8_t tab[64];
  HIPCHK(hipMemcpyAsync(host.data(), blocks, host.size() * sizeof(int16_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipMemcpyAsync(tab, table, sizeof(tab), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int16_t v : host)
    if (v < -1024 || v > 1024) return fail(MMF_EINVAL, "jpeg_block_roundtrip: sample %d outside +-1024", (int)v);
  for (uint8_t t : tab)
    if (t == 0) return fail(MMF_EINVAL, "jpeg_block_roundtrip: a zero table entry");
  return test_launch_rc(launch_jpeg_block_roundtrip(blocks, table, n, coefs, samples, outside, (hipStream_t)stream),
                        "jpeg_block_roundtrip");
}

int mmf_vault_sort_cand_f32(const float* cs, const int32_t* cidx, int chunks, int chunk_rows, int B, int k,
                            float thresh, float* sims, int32_t* idx, float* disc, int disc_stride, const float* temb,
                            const float* title, int D, float* tsim, void* stream) {
  if (!cs || !cidx) return fail(MMF_EINVAL, "null argument");
  const VaultOut o = vault_out(thresh, sims, idx, disc, disc_stride, temb, title, D, tsim);
  if (B <= 0 || chunks <= 0 || chunk_rows <= 0 || k <= 0 || (long long)chunks * k > 16384 || !vault_out_ok(o))
    return fail(MMF_EINVAL, "vault_sort_cand: bad shape or no output (chunks=%d chunk_rows=%d B=%d k=%d)", chunks,
                chunk_rows, B, k);
  return test_launch_rc(launch_vault_sort_cand(cs, cidx, chunks, chunk_rows, B, k, o, (hipStream_t)stream),
                        "vault_sort_cand");
}

}  // extern "C"
