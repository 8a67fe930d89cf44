// Host-side launchers of the gfx950 kernels (implemented in *.hip).  All enqueue on `stream`
// and return hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t f16_t;

struct GemmArgs {
  const f16_t* A;  int lda;     // activations [M][K] fp16
  const f16_t* W;  int ldw;     // weights [N][K] fp16 (PyTorch Linear layout)
  const float* bias;             // [N] or null
  const float* res32;            // fp32 residual [M][N] (ldr) or null
  const f16_t* res16;           // fp16 residual [M][N] (ldr) or null
  int ldr;
  float* c32;                    // fp32 out [M][N] (ldc) or null
  f16_t* c16;                   // fp16 out [M][N] (ldc) or null
  int ldc;
  const float* ascale;           // per-(batch, k) fp32 scale of A (SE excitation) or null
  int rows_per_batch;            // rows of A per batch item when ascale != null
  int M, N, K, act;
  int force_cfg;                 // 0 = automatic tile choice, c + 1 = instantiation c (A/B option)
  int no_splitk;                 // 1 = never split K on the skinny-M path (A/B option)
  int group_m;                   // persistent-tile order: 0 row-major, g > 0 grouped by g row panels
  float* ws;                     // split-K partials workspace (skinny-M GEMMs) or null
  size_t ws_elems;               // its capacity in floats
  // Lazy LayerNorm (option lazy_ln; gemm.hip).  A row's LN statistics travel as P partials
  // (mean_p, M2_p) over consecutive column blocks of tn columns ([rows][P] float2, buffers padded
  // to whole 256-row blocks), combined with Chan's formula by the reader.
  int epi;                       // 0 plain; 1 A = raw rows s: out = r (acc - mean u) + bias (LN folded
                                 // into W, bias padded by 256); 2 out = acc + bias + res16 (in
                                 // place allowed), partials of out written
  const float2* ln_in;           // epi 1: partials of A's rows
  int ln_in_P, ln_in_tn;         //   their count per row and column-block width
  const float* ln_u;             // epi 1: [N] sum_k W[n][k] (padded to N + 256)
  float2* ln_out;                // epi 2: partials of the output rows, [rows][ceil(N / tn_out)]
  float ln_eps;
  // epi 3 (RoBERTa, L = 128, option qkv_attn): W / bias are the fused QKV with rows interleaved per
  // head ([q_h; k_h; v_h] = 192 rows for head h), so a 256 x 192 tile holds q, k and v of one head
  // for two whole sequences; the epilogue runs their attention and writes ctx [M][ldc] (c16, head h
  // at columns 64 h) instead of qkv.  amask: key-padding mask int32 [M / 128][128] (1 keep) or null
  const int32_t* amask;
  // epi 4 (RoBERTa precise mode, FFN-1): out = act(acc + bias) written as the next GEMM's split
  // operand row: c16[m * ldc + n] = hi, and with split_lo also [+ N] = lo = fp16(out - hi), [+ 2N] = hi
  // (ldc >= 3N), so the fp32 hidden and its split3 pass are never formed
  int split_lo;
  // epi 5 (CLIP towers, option clip_qkv_attn): the lazy-LN consumer of epi 1 on a QKV weight whose folded
  // (W', u, c) rows are interleaved per head as for epi 3, with the attention of the tile's
  // floor(256 / att_L) whole sequences of att_L rows (16 .. 128) in its epilogue: row panel tm starts at
  // row tm * floor(256 / att_L) * att_L, ctx [M][ldc] goes to c16 and qkv is never stored.  amask:
  // int32 [M / att_L][att_L] (1 keep) or null; att_causal: key j of a sequence is visible to queries >= j
  int att_L, att_causal;
};
// whether launch_gemm accepts a (epi != 0) epilogue for these arguments (the host falls back to
// the plain path otherwise)
bool gemm_epi_ok(const GemmArgs& a);
// epi 2: the column-block width (= P partials per row of ceil(N / tn)) launch_gemm will use
int gemm_ln_tn(const GemmArgs& a);
// split-K factor the skinny-M (M <= 512) GEMM path uses for this (K) -- independent of M, so
// results stay batch-invariant; 1 = no split.  Workspace need: splitk_factor * M * N floats.
int gemm_splitk_factor(const GemmArgs& a);
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
int gemm_config(const GemmArgs& a);          // which instantiation launch_gemm picks
constexpr int kGemmConfigs = 17;  // numbering of the tile instantiations (0 .. 16; gemm.hip config_exists)
const char* gemm_config_name(int c);
// streaming 1x1-convolution kernel (pointwise.hip), picked by launch_gemm when applicable
bool pw_applicable(const GemmArgs& a);
hipError_t launch_pw(const GemmArgs& a, hipStream_t s);

// LayerNorm over rows of width C (multiple of 256): y = LN(x [+ add]) * g + b.
// x/add fp32 with row strides; writes fp32 y32 and/or fp16 y16.
hipError_t launch_layernorm(const float* x, int ldx, const float* add, int ldadd, const float* g, const float* b,
                            float eps, float* y32, int ldy32, f16_t* y16, int ldy16, int rows, int C,
                            hipStream_t s);

// Residual add + LayerNorm: s = x (fp32, row stride ldx) + y (fp16 GEMM output, ldy); optionally
// s32 = s, o32 = LN(s) (both with stride ldx; may alias x); o16 = LN(s) fp16 (ldo).  C in {512, 768}.
hipError_t launch_add_ln(const float* x, int ldx, const f16_t* y, int ldy, const float* g, const float* b, float eps,
                         float* s32, float* o32, f16_t* o16, int ldo, int rows, int C, hipStream_t s);
// the same with an fp16 residual stream (pre-LN CLIP, option clip_res16): s16 = s (may alias x)
hipError_t launch_add_ln(const f16_t* x, int ldx, const f16_t* y, int ldy, const float* g, const float* b, float eps,
                         f16_t* s16, f16_t* o16, int ldo, int rows, int C, hipStream_t s);

// Fused multi-head attention, head_dim 64, L <= 128: qkv fp16 [B*L][ldqkv] with q at col h*64,
// k at D + h*64, v at 2D + h*64 (D = H*64); mask int32 [B][L] (1 keep) or null; out fp16 [B*L][ldo].
// one query per sequence over the sequence's keys (the compact last encoder layer): q [B][ldq] fp32, out
// row b at out + b * ldo; qpos (nullable) = the query's position per sequence for a causal mask
hipError_t launch_attention_q1(const float* q, int ldq, const f16_t* qkv, int ld, int koff, int voff,
                               const int32_t* mask, const int32_t* qpos, f16_t* out, int ldo, int B, int L, int H,
                               hipStream_t s);
hipError_t launch_attention(const f16_t* qkv, int ldqkv, const int32_t* mask, f16_t* out, int ldo, int B,
                            int L, int H, int causal, hipStream_t s);

// RoBERTa embeddings + LayerNorm -> the split stream xb (hi) + xlo (lo, nullable) [B*L][H] fp16, or,
// with x32 non-null, the fp32 stream only (precise mode)
hipError_t launch_roberta_embed(const int32_t* ids, const float* word, const float* pos, const float* type0,
                                const float* g, const float* b, float eps, uint16_t* xlo, f16_t* xb, int B, int L,
                                int H, int pad_id, hipStream_t s, float* x32 = nullptr, int* ovf = nullptr);
// ovf (nullable, [B] int32): the overflow sentinel of the fp16 / split stream -- a row whose
// LayerNorm statistics are non-finite sets ovf[sequence] = 1 (embeddings and add+LN); the text heads
// then return NaN for that sequence (capi.cpp run_text)
// RoBERTa precise mode (precise.hip, option text_hilo = 2): fp32 rows -> [hi | lo | hi] fp16 rows of 3C
// (the K-concatenated GEMM operand), and fp32 attention over an fp32 qkv (q at h*64, k at koff + h*64,
// v at voff + h*64; key-padding mask int32 [B][L] or null) -> fp32 out [B*L][ldo]
// with_lo = 0: only the hi third is written (a consumer on fp16 operands)
hipError_t launch_split3(const float* x, int ldx, f16_t* out, int rows, int C, hipStream_t s, int with_lo = 1);
// out3 (nullable): ctx written as the next GEMM's operand rows [hi | lo | hi] (ld 3 * H * 64; with_lo = 0: hi
// alone) instead of fp32 rows to out
hipError_t launch_attention32(const float* qkv, int ld, int koff, int voff, const int32_t* mask, float* out, int ldo,
                              int B, int L, int H, hipStream_t s, f16_t* out3 = nullptr, int with_lo = 1);
// precise mode: x = LN(x + add) in place [rows][768] fp32, and s3 = [hi | lo | hi] rows of it (with_lo = 0: hi only)
hipError_t launch_layernorm_split3(float* x, const float* add, const float* g, const float* b, float eps, f16_t* s3,
                                   int with_lo, int rows, int C, hipStream_t s);
// RoBERTa post-LN residual stream split as hi = fp16(x) (also the GEMM operand), lo = fp16(x - hi)
hipError_t launch_add_ln_hilo(f16_t* hi, uint16_t* lo, int ld, const f16_t* y, int ldy, const float* g,
                              const float* b, float eps, int rows, int C, hipStream_t s, int* ovf = nullptr, int L = 0);
hipError_t launch_hilo_rows(const f16_t* hi, const uint16_t* lo, int row_stride, float* out, int B, int C,
                            hipStream_t s);
// CLIP text embeddings (tok + pos) -> x fp32 (or x16 fp16: exactly one non-null), then LN1 of layer 0
// -> xb fp16
hipError_t launch_clip_text_embed(const int32_t* ids, const float* tok, const float* pos, const float* g,
                                  const float* b, float eps, float* x, f16_t* x16, f16_t* xb, float2* st, int B, int L,
                                  int H, hipStream_t s);
// (lazy LN, st != null: st[row] = (mean, M2) of the stored stream instead of xb)
// CLIP patch im2col with normalisation: img uint8 [B,224,224,3] -> A fp16 [B*49][3072]
hipError_t launch_clip_im2col(const uint8_t* img, f16_t* A, int B, hipStream_t s);
// CLIP vision: x = preLN(cat(cls, patches) + pos) -> x fp32 [B*50][768] (or x16 fp16: exactly one
// non-null), xb = LN1(x) fp16
hipError_t launch_clip_vision_assemble(const float* patches, const float* cls, const float* pos,
                                       const float* pre_g, const float* pre_b, const float* ln1_g,
                                       const float* ln1_b, float eps, float* x, f16_t* x16, f16_t* xb, float2* st,
                                       int B, hipStream_t s);

// EOS index per row (first == eos_id, or argmax when eos_id == 2)
hipError_t launch_eos_index(const int32_t* ids, int32_t* out, int B, int L, int eos_id, hipStream_t s);
// gather rows: out fp16 [B][C] = LN(x[row_index(b)]) where row_index = b*L + (idx ? idx[b] : 0)
hipError_t launch_gather_ln(const float* x, const int32_t* idx, int L, const float* g, const float* b, float eps,
                            f16_t* out, float* out32, int B, int C, hipStream_t s);
// compact copies of rows b*L + (idx ? idx[b] : 0) of a fp16 (a16, nullable: then o16 is not written) and
// an fp32 (a32, or fp16 a32h: exactly one non-null) [.,C] buffer; o32 is fp32 either way
hipError_t launch_gather_rows2(const f16_t* a16, const float* a32, const f16_t* a32h, const int32_t* idx, int L,
                               int C, f16_t* o16, float* o32, int B, hipStream_t s);
// L2-normalise rows of fp32 [B][C] in place (C multiple of 64)
hipError_t launch_l2norm(float* x, int B, int C, hipStream_t s);
// two 768->256->2 heads (fp32) from CLS rows x[b*L*768]; writes logits and softmax[:,1] scores
hipError_t launch_text_heads(const float* x, int row_stride, const float* w1a, const float* b1a,
                             const float* w2a, const float* b2a, const float* w1m, const float* b1m,
                             const float* w2m, const float* b2m, float* ai_logits, float* mi_logits,
                             float* scores, int score_stride, int B, hipStream_t s, const int* ovf = nullptr);
// fusion MLP 5->64->32->2 (+ verdict, confidence, explanation rule)
hipError_t launch_fusion(const float* x5, const float* w0, const float* b0, const float* w3, const float* b3,
                         const float* w5, const float* b5, float* probs, int32_t* verdict, float* conf,
                         int32_t* rule, int B, hipStream_t s);
// one epoch of FusionJudge training (forward, cross-entropy, backward, AdamW per minibatch) in one launch by one
// workgroup (fusion_train.hip; include/mmf_hip.h mmf_fusion_train_epoch); hipErrorInvalidValue on a bad N / batch /
// p_drop with nothing launched
hipError_t launch_fusion_train_epoch(const float* scores5, const int32_t* labels, int N, const int32_t* perm,
                                     const uint64_t* keep, float p_drop, int batch, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, int step0, float* params,
                                     float* exp_avg, float* exp_avg_sq, float* step_loss, int32_t* step_correct,
                                     float* grad_out, hipStream_t s);
// CLIPDetective's projection heads on cached pooled features (clip_train.hip; include/mmf_hip.h
// mmf_clip_train_epoch / mmf_clip_contrastive_eval): six launches per minibatch (three for the eval), ws of
// clip_train_ws_bytes(batch) bytes (0 for a batch outside 1..64); hipErrorInvalidValue on a bad N / batch with
// nothing launched
constexpr int kClipTrainParams = 655361;  // visual [512][768] | text [512][512] | logit_scale
size_t clip_train_ws_bytes(int batch);
hipError_t launch_clip_train_epoch(const float* img_feat, const float* txt_feat, int N, const int32_t* perm, int batch,
                                   double lr, double beta1, double beta2, double eps, double weight_decay,
                                   double max_norm, int step0, float* params, float* exp_avg, float* exp_avg_sq,
                                   float* step_loss, float* step_gnorm, float* grad_out, float* ws, hipStream_t s);
hipError_t launch_clip_contrastive_eval(const float* img_feat, const float* txt_feat, int N, int batch,
                                        const float* params, float* batch_loss, float* row_cos, float* ws,
                                        hipStream_t s);
// The same for `trials` independent trainings side by side in the same launches (include/mmf_hip.h
// mmf_clip_train_epoch_trials / mmf_clip_contrastive_eval_trials): params / exp_avg / exp_avg_sq
// [trials][kClipTrialStride], perm [trials][N], step_loss / step_gnorm [trials][max_nsteps], batch_loss
// [trials][max_nb], row_cos [trials][N], ws of clip_train_trials_ws_bytes(trials, 64) bytes (0 for trials outside
// 1..kClipTrialsMax).  batch, lr, weight_decay, max_norm, step0, active are HOST arrays [trials] read at enqueue time
// (active NULL: every trial).  grad_out (NULL but for the single-trial call): trial 0's last clipped gradient.
// hipErrorInvalidValue with nothing launched: trials, N or an active trial's batch out of range, max_nsteps /
// max_nb below an active trial's step count.
constexpr int kClipTrialsMax = 16;
constexpr int kClipTrialStride = 655364;  // kClipTrainParams rounded up to 4 floats: every slice 16-byte aligned
size_t clip_train_trials_ws_bytes(int trials, int batch_max);
hipError_t launch_clip_train_epoch_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                          const int32_t* perm, const int32_t* batch, const double* lr,
                                          const double* weight_decay, const double* max_norm, const int32_t* step0,
                                          const int32_t* active, double beta1, double beta2, double eps, float* params,
                                          float* exp_avg, float* exp_avg_sq, float* step_loss, float* step_gnorm,
                                          int max_nsteps, float* grad_out, float* ws, hipStream_t s);
hipError_t launch_clip_contrastive_eval_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                               const int32_t* batch, const int32_t* active, const float* params,
                                               float* batch_loss, float* row_cos, int max_nb, float* ws,
                                               hipStream_t s);
// a RoBERTa text head (Linear(768,256)-ReLU-Dropout-Linear(256,2)) on cached CLS rows (head_train.hip;
// include/mmf_hip.h mmf_head_train_epoch / mmf_head_eval): four launches per minibatch (two for the eval), ws of
// head_train_ws_bytes(batch) bytes (0 for a batch outside 1..64); lr_steps is a HOST array read at enqueue time;
// hipErrorInvalidValue on a bad N / batch / p_drop with nothing launched
constexpr int kHeadTrainParams = 197378;  // 0.weight [256][768] | 0.bias [256] | 3.weight [2][256] | 3.bias [2]
size_t head_train_ws_bytes(int batch);
hipError_t launch_head_train_epoch(const float* feat, const int32_t* labels, int N, const int32_t* perm,
                                   const uint64_t* keep, float p_drop, int batch, const double* lr_steps, double beta1,
                                   double beta2, double eps, double weight_decay, double max_norm, int step0,
                                   float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                                   int32_t* step_correct, float* step_gnorm, float* grad_out, float* ws, hipStream_t s);
hipError_t launch_head_eval(const float* feat, const int32_t* labels, int N, int batch, const float* params,
                            float* batch_loss, float* row_logits, float* ws, hipStream_t s);
// the deployed EfficientNet classifier (Dropout(0.2)-Linear(1280,2)) on cached pooled rows (effnet_train.hip;
// include/mmf_hip.h mmf_effcls_train_epoch / mmf_effcls_eval): one launch per epoch by one workgroup, parameters and
// moments in registers; the eval one workgroup per batch; hipErrorInvalidValue on a bad R / N / batch / p_drop with
// nothing launched
constexpr int kEffClsParams = 2562;  // classifier.1.weight [2][1280] | classifier.1.bias [2]
hipError_t launch_effcls_train_epoch(const float* feat, const int32_t* labels, int R, const int32_t* perm, int N,
                                     const uint64_t* keep, float p_drop, int batch, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, int step0, float* params,
                                     float* exp_avg, float* exp_avg_sq, float* step_loss, int32_t* step_correct,
                                     float* grad_out, hipStream_t s);
hipError_t launch_effcls_eval(const float* feat, const int32_t* labels, int R, int batch, const float* params,
                              float* batch_loss, float* row_logits, hipStream_t s);
// EfficientNet's head conv stage (features.8: 1x1 conv, eval-mode BatchNorm, SiLU) trained with the classifier on
// cached trunk rows [R][49][320] (effhead_train.hip; include/mmf_hip.h mmf_effhead_train_epoch / mmf_effhead_eval):
// three launches per optimizer step (forward, classifier step, owner-per-tile backward with Adam in the epilogue), two
// per eval batch; ws holds effhead_ws_bytes(batch) bytes (0 for a batch outside 1..64); hipErrorInvalidValue on a bad
// R / N / batch / p_drop with nothing launched
constexpr int kEffHeadParams = 414722;  // W [1280][320] | gamma [1280] | beta [1280] | Wc [2][1280] | bc [2]
size_t effhead_ws_bytes(int batch);
hipError_t launch_effhead_train_epoch(const float* trunk, const int32_t* labels, int R, const int32_t* perm, int N,
                                      const uint64_t* keep, float p_drop, int batch, const float* bn_mean,
                                      const float* bn_var, double bn_eps, double lr, double beta1, double beta2,
                                      double eps, double weight_decay, int step0, float* params, float* exp_avg,
                                      float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* grad_out,
                                      float* ws, hipStream_t s);
hipError_t launch_effhead_eval(const float* trunk, const int32_t* labels, int R, int batch, const float* params,
                               const float* bn_mean, const float* bn_var, double bn_eps, float* batch_loss,
                               float* row_logits, float* ws, hipStream_t s);
// dst[b][y][x][c] = src[b][y][W - 1 - x][c] (uint8; mmf_hflip_u8)
hipError_t launch_hflip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, hipStream_t s);
// ColorJitter on uint8 [B][H][W][3], byte-exact with torchvision's PIL backend (jitter.hip; include/mmf_hip.h
// mmf_color_jitter_u8): two launches, grid (chunks <= kJitterChunks, B); ws uint64 [B][kJitterChunks] holds the
// chunks' sums of L for the contrast mean; hipErrorInvalidValue on a bad shape with nothing launched
constexpr int kJitterChunks = 256;                   // MMF_JITTER_CHUNKS
constexpr int kJitterMaxBatch = 65535;               // the grid's y extent
constexpr size_t kJitterMaxPixels = (size_t)1 << 40; // per image: 255 * pixels stays exact in a double (< 2^53)
hipError_t launch_color_jitter_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ops,
                                  const float* factors, const int32_t* hue_shift, uint64_t* ws, hipStream_t s);
// GaussianBlur on uint8 [B][H][W][3] with reflected borders (blur.hip; include/mmf_hip.h mmf_gaussian_blur_u8): one
// launch, grid (tiles of kBlurTileRows rows x kBlurTileBytes row bytes, B), weights float32 [B][KY][KX], image b
// copied where apply[b] == 0; (5, 9) compiled with constant taps, every other odd size up to kBlurMaxTaps with
// run-time ones; hipErrorInvalidValue on a bad shape or size with nothing launched
constexpr int kBlurTileRows = 32;
constexpr int kBlurTileBytes = 256;                  // of a row's 3 * W
constexpr int kBlurMaxTaps = 15;
constexpr int kBlurMaxBatch = 65535;                 // the grid's y extent
constexpr size_t kBlurMaxPixels = (size_t)1 << 30;   // per image: the tiles stay below 2^31, a row's bytes below 2^32
hipError_t launch_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int KX, int KY,
                                   const float* weights, const int32_t* apply, hipStream_t s);
// A JPEG save-and-reload round trip on uint8 [B][H][W][3], byte-exact with Pillow (jpeg_encode.hip; include/mmf_hip.h
// mmf_jpeg_roundtrip_u8): flags cleared, then two launches, grid (blocks or pixels, B); ws of
// jpeg_roundtrip_ws_bytes(H, W) bytes per image (0 for a bad shape) holds the sample planes; hipErrorInvalidValue on
// a bad shape with nothing launched
constexpr int kJpegEncMaxBatch = 65535;                // the grid's y extent
constexpr size_t kJpegEncMaxPixels = (size_t)1 << 30;  // per image: pixel and block indices stay ints
size_t jpeg_roundtrip_ws_bytes(int H, int W);
hipError_t launch_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* quality,
                                    uint8_t* ws, int32_t* flags, hipStream_t s);
// the round trip's block arithmetic on n raw level-shifted sample blocks [n][64] (|sample| <= 1024: the caller's
// check) and one table of 64 bytes: quantised coefficients, range-limited samples, 1 where the block left the
// exact range (mmf_jpeg_block_roundtrip_raw)
hipError_t launch_jpeg_block_roundtrip(const int16_t* blocks, const uint8_t* table, int n, int16_t* coefs,
                                       uint8_t* samples, int32_t* outside, hipStream_t s);
// the CLS rows the text heads read: out fp32 [B][768] = x[b * row_stride ..]; a sequence with ovf[b] != 0 (nullable)
// gets a NaN row, as launch_text_heads gives it NaN logits
hipError_t launch_text_cls_rows(const float* x, int row_stride, const int* ovf, float* out, int B, hipStream_t s);
// dst fp16 [n] = round-to-nearest-even of src fp32 [n] (n a multiple of 4, 16-byte aligned)
hipError_t launch_f32_to_f16(const float* src, f16_t* dst, size_t n, hipStream_t s);
// mmf_analyze_mixed's last kernel: per batch row, the row's compact tower results gathered through
// row_map [B][3] (position of the row in the text / image / both lists; anything outside [0, n) is
// absent), the CLIP cosine and the caption-title cosine of the "both" rows, the vault outputs scattered
// (or the no-image convention: 0, 0, -1), the FusionJudge MLP for the "both" rows and the reference's
// single-modality verdict for the rest (misinfo_forensics.py:879-899), the rule cascade for all
struct MixedFinishArgs {
  const int32_t* row_map;
  int B, nT, nI, nC;
  const float* text2;    // [nT][2] ai, misinfo
  const float* deepfake; // [nI]
  const float* v_emb;    // [nI][512] unit image embeddings
  const float* t_emb;    // [nC][512] unit caption embeddings
  const float* c_sims;   // [nI][5] vault top-5 (null: no vault set)
  const int32_t* c_idx;  // [nI][5]
  const float* c_disc;   // [nI]
  const float* title;    // [N][512] unit title embeddings or null
  float thresh;
  const float *w0, *b0, *w3, *b3, *w5, *b5;  // fusion layer (read only when nC > 0)
  float *scores5, *text_sim, *probs;         // [B][5], [B] (nullable), [B][2]
  int32_t* verdict; float* conf; int32_t* rule;  // [B] each, nullable
  float* top_sims; int32_t* top_idx;             // [B][5] each, nullable
};
hipError_t launch_mixed_finish(const MixedFinishArgs& a, hipStream_t s);
// cosine of unit rows: out[b*ostride] = dot(a[b], c[b])
hipError_t launch_rowdot(const float* a, const float* c, float* out, int ostride, int B, int C, hipStream_t s);
// vault (vault.hip): S[B][N] = Q[B][D] . V[N][D]^T (fp32)
hipError_t launch_vault_sims(const float* q, const float* v, float* S, int B, int N, int D, hipStream_t s, int ref = 0);
// What a vault search writes for its B query rows (every pointer nullable), the same whichever kernel
// path served it; passed to the kernels by value, as MixedFinishArgs.
struct VaultOut {
  float thresh;        // a hit: the top-1 similarity is above it (a NaN is not)
  float* sims;         // [B][k] similarities, descending (NaN rows first); slots past N hold -inf
  int32_t* idx;        // [B][k] their vault rows; slots past N hold -1
  float* disc;         // disc[b * disc_stride] = the top-1 similarity of a hit, else 0
  int disc_stride;
  const float* temb;   // [B][D] unit caption embeddings  } both non-null: tsim[b] = the cosine of the
  const float* title;  // [N][D] unit title embeddings    } caption and a hit's top-1 title, else 0
  int D;
  float* tsim;         // [B]
};
hipError_t launch_vault_topk(const float* S, int B, int N, int k, const VaultOut& out, hipStream_t s, int ref = 0);
// the same result without S (option vault_fused, mmf_vault_search_rows): out.D = 512, k in 1..8; ws holds
// vault_search_ws_bytes(B, k, nblocks) bytes of per-block candidates; nblocks 0 = vault_search_blocks' choice
int vault_search_blocks(int B, int N, int nblocks);
size_t vault_search_ws_bytes(int B, int k, int nblocks);
hipError_t launch_vault_search(const float* q, const float* v, int B, int N, int k, const VaultOut& out, void* ws,
                               int nblocks, hipStream_t s);
// final ranking of [chunks][B][k] per-chunk top-k results (launch_vault_topk outputs with chunk-local
// indices, chunk c = vault rows c * chunk_rows ..): chunks * k <= 16384
hipError_t launch_vault_sort_cand(const float* cs, const int32_t* cidx, int chunks, int chunk_rows, int B, int k,
                                  const VaultOut& out, hipStream_t s);

// EfficientNet-B0 pieces (NHWC fp16 activations)
hipError_t launch_effnet_stem(const uint8_t* img, const float* w, const float* bias, f16_t* out, int B,
                              hipStream_t s);
hipError_t launch_effnet_stem_f32(const float* x_nchw, const float* w, const float* bias, f16_t* out, int B,
                                  hipStream_t s);
// stem fused into the stage-1 depthwise conv (3x3 s1, 32 channels at 112^2) + its SE pool partials;
// exactly one of img (uint8 HWC) / xf32 (normalised fp32 NCHW) is non-null
hipError_t launch_effnet_stem_dw(const uint8_t* img, const float* xf32, const float* ws, const float* bs,
                                 const float* wd, const float* bd, f16_t* out, float* pool_part, int B,
                                 int* nchunks_out, hipStream_t s);
// flags: bit 0 = compile-time tile geometries where one exists (runtime-geometry kernels otherwise),
// bit 3 = 32-channel groups for C in {480, 672, 1152} (option dw_cw32)
hipError_t launch_dwconv(const f16_t* in, const float* w, const float* bias, f16_t* out, float* pool_part,
                         int B, int H, int W, int C, int k, int stride, int* nchunks_out, hipStream_t s, int ct = 1);
hipError_t launch_se(const float* pool_part, int nchunks, float inv_hw, const float* w1, const float* b1,
                     const float* w2, const float* b2, float* scale, int B, int C, int Csq, hipStream_t s,
                     bool precise = false);  // precise: the fc1 SiLU in silu_precise form (fp32 tower)
hipError_t launch_gap_classifier(const f16_t* x, int HW, int C, const float* w, const float* b, float* logits,
                                 float* score, int score_stride, int B, hipStream_t s);
// the classifier's input row alone (mmf_effnet_pooled): pooled fp32 [B][C] = the ascending-pixel sum * (1 / HW)
hipError_t launch_gap_pooled(const f16_t* x, int HW, int C, float* pooled, int B, hipStream_t s);
// n fp16 values (a multiple of 8, both pointers 16-byte aligned) converted exactly to fp32 (mmf_effnet_trunk)
hipError_t launch_f16_rows_to_f32(const f16_t* x, float* out, size_t n, hipStream_t s);
hipError_t launch_fill_strided(float* p, int stride, int B, float v, hipStream_t s);
// fused MBConv front: expand 1x1 (we fp16 [C][cin], be fp32, BN folded) + SiLU computed per input
// tile into LDS, then the depthwise conv of launch_dwconv (same outputs, same pool partials)
bool expand_dw_applicable(int cin, int cexp, int k);
hipError_t launch_expand_dw(const f16_t* x, int cin, const f16_t* we, const float* be, const float* w,
                            const float* bias, f16_t* out, float* pool_part, int B, int H, int W, int C, int k,
                            int stride, int* nchunks_out, hipStream_t s, int ct = 1);
// number of pool-partial chunks launch_dwconv uses for an output of Ho x Wo with C channels
int dwconv_nchunks(int H, int W, int C, int stride);
// JPEG reconstruction (jpeg.hip): islow IDCT per block, then fancy upsampling + YCbCr -> RGBX per pixel
hipError_t launch_jpeg_reconstruct(const uint8_t* packed, const uint32_t* block_off, const int64_t* pk_off,
                                   const uint16_t* qt, const int64_t* coef_blocks, const int32_t* infos,
                                   const int64_t* out_offsets, int B, int max_blocks, int max_pixels, uint8_t* samples,
                                   uint8_t* out, hipStream_t s);

// Pillow-exact resampling of decoded images to the towers' 224 x 224 windows (resize.hip)
constexpr int kResizeKMax = 96;  // taps per output coordinate (bicubic support 2 x scale <= 47)
struct ResizeJob {
  long long src_off;  // byte offset of the source image (uint8 HWC RGB) in the source buffer
  int w, h;           // source size
  int ow, oh;         // Pillow resize output size (before the crop)
  int cx, cy;         // window offset in the resize output (centre crop; 0 for the squash)
  int filt;           // 0 bilinear, 1 bicubic
  int need_h, need_v; // Pillow runs the pass (size changes on that axis)
  int y0, y1;         // source rows the window's vertical taps read
  int ksh, ksv;       // taps per coordinate, horizontal / vertical
  long long tmp_off;  // byte offset of this job's [y1 - y0][224][3] first-pass rows
  int coef_off;       // int32 offset of [224][ksh] then [224][ksv] coefficients
  int ps;             // source bytes per pixel: 3 (RGB) or 4 (RGBX, Pillow's in-memory layout)
  int x0, x1;         // x1 > 0: the vertical pass runs first (Image.resize's order for a source over 100 times as
                      // tall as wide whose height shrinks), over the source columns the window's horizontal taps
                      // read; tmp is then [x1 - x0][224][3]
};
// the coefficient launch of launch_resize_pil alone: coef int32 [sum 224 * (ksh + ksv)] at each job's coef_off,
// bounds int32 [njobs][2][224][2] = (xmin, n) per job, axis (0 horizontal, 1 vertical) and window coordinate
hipError_t launch_resize_coef(const ResizeJob* jobs, int njobs, int32_t* coef, int32_t* bounds, hipStream_t s);
hipError_t launch_resize_pil(const uint8_t* src, const ResizeJob* jobs, int njobs, int max_rows, int32_t* coef,
                             int32_t* bounds, uint8_t* tmp, uint8_t* const* outs, hipStream_t s);

// fp32 EfficientNet tower (option effnet_fp32, effnet_f32.hip): NHWC fp32 activations
hipError_t launch_effnet_stem32(const uint8_t* img, const float* x_nchw, const float* w, const float* bias,
                                float* out, int B, hipStream_t s);
// which kernel launch_pw32 runs for a shape and a pw32_mfma mode: pw32_kernel (VALU), pw32m_kernel<D>, or
// pw32r_kernel<NF, D> over column tiles of NC; PW32_NONE = a shape no kernel takes (N, K % 4 != 0, ...)
enum { PW32_NONE = -1, PW32_VALU = 0, PW32_MFMA = 1, PW32_ROWS = 2 };
struct Pw32Variant {
  int kind, D, NF, NC;
};
Pw32Variant pw32_variant(int M, int N, int K, int mfma);
// C[M][N] = act((A .* ascale[m / rows_per_image]) W^T + bias) (+ res); W fp32 [N][K]; N, K % 4 == 0
hipError_t launch_pw32(const float* A, const float* W, const float* bias, const float* ascale, int rows_per_image,
                       const float* res, float* C, int M, int N, int K, int act, hipStream_t s, int mfma = 1);
// w tap-major [k*k][C]
hipError_t launch_dw32(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int C,
                       int k, int stride, hipStream_t s);
// part[b][j][c] = sum over pixel chunk j of nchunks (the SE's pool partials)
hipError_t launch_sum32(const float* x, int B, int HW, int C, int nchunks, float* part, hipStream_t s);
hipError_t launch_gap32(const float* x, int HW, int C, const float* w, const float* b, float* logits, float* score,
                        int score_stride, int B, hipStream_t s);
hipError_t launch_gap32_pooled(const float* x, int HW, int C, float* pooled, int B, hipStream_t s);
