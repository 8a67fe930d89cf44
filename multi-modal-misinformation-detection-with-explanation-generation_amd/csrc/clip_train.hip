// Training of CLIPDetective's projection heads on cached pooled features (train_clip_detective.py:129-166,
// 203-225, 236-273): visual_projection [512][768], text_projection [512][512] and logit_scale, fp32 master
// weights, every minibatch as a short chain of six ordinary launches on the caller's stream:
//   1. clip_project    one workgroup per (16 outputs, tower): the (clamped) permutation entries' feature rows are
//                      copied into the workspace; e = P W^T, thread (j, r) one ascending-k fmaf chain over LDS tiles
//      clip_normalise  one workgroup per (row, tower): the row norm (a fixed tree over 512 squares), e / norm
//   2. clip_logits     ONE workgroup: cos[i][j] = I_i . T_j (ascending-k chains on unit rows read from L2),
//                      logits = exp(logit_scale) cos, both softmaxes (ascending chains), the loss, dL/dlogits
//                      and dL/dlogit_scale
//   3. clip_embgrad    one workgroup per (row, tower): dL/d(unit row) as an ascending chain over the other
//                      tower's rows, pulled back through e / |e|
//   4. clip_wgrad      dW = dE^T P: a thread owns 4 consecutive elements of the flat gradient, each an
//                      ascending-row chain; the block's sum of squares by a fixed tree over its 1,024 elements
//   5. clip_adamw      every block re-derives the total norm from the 640 block sums in one fixed order, then
//                      clip_grad_norm_'s coefficient and torch.optim.AdamW on its 1,024 elements
// Stream order is the only synchronisation: no grid barrier, no cooperative launch, no flag, no atomics.  Every
// reduction has a fixed order, so results are bit-reproducible and do not depend on how an epoch is split into
// launches; the step-dependent Adam scalars are computed in double from the step number alone (as fusion_train.hip).
//
// Trials.  Every launch carries a trial dimension in blockIdx.z: T independent trainings (a hyperparameter study)
// share the six launches of a step.  Per-trial state is stacked (params / moments [T][kClipTrialStride], perm [T][N],
// one workspace image per trial, outputs [T][row stride]); a trial's batch size, step count, max_norm and that
// step's Adam scalars travel by value in the kernel arguments (ClipTrials).  Trials differ in batch size and so in
// steps per epoch: a workgroup whose trial has no minibatch st, or whose row lies past its trial's rows, returns at
// its very top -- a test on blockIdx and the arguments alone, uniform over the workgroup -- and touches nothing.
// The single-trial entry points are T = 1 through the same kernel bodies (instantiated for one trial: ClipTrials
// below), and no workgroup reads another trial's slice, so a trial's bits do not depend on its neighbours.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "train_common.h"

namespace {

constexpr int CT_D = 512;                    // embedding width
constexpr int CT_KV = 768, CT_KT = 512;      // pooled widths: ViT, text tower
constexpr int CT_NV = CT_D * CT_KV;          // 393,216
constexpr int CT_NT = CT_D * CT_KT;          // 262,144
constexpr int CT_NW = CT_NV + CT_NT;         // 655,360: logit_scale follows
constexpr int CT_BMAX = 64;                  // rows of a minibatch
constexpr int CT_BLK = 1024;                 // elements of a wgrad / adamw block
constexpr int CT_NBLK = CT_NW / CT_BLK;      // 640
static_assert(CT_NV % CT_BLK == 0 && CT_NW % CT_BLK == 0, "a block stays inside one projection");
static_assert(CT_NW + 1 == kClipTrainParams, "flat parameter layout");
static_assert(kClipTrialStride >= kClipTrainParams && kClipTrialStride % 4 == 0, "a trial's slice stays 16-byte aligned");

// workspace image, in floats (every region 16-byte aligned); strides are those of CT_BMAX rows whatever the batch
constexpr size_t W_PB = 0;                                   // [2][64][768] the minibatch's feature rows
constexpr size_t W_EH = W_PB + 2 * CT_BMAX * CT_KV;          // [2][64][512] unit embeddings
constexpr size_t W_NRM = W_EH + 2 * CT_BMAX * CT_D;          // [2][64]      |e|
constexpr size_t W_DL = W_NRM + 2 * CT_BMAX;                 // [64][64]     dL/dlogits
constexpr size_t W_SC = W_DL + CT_BMAX * CT_BMAX;            // [4]          exp(logit_scale), dL/dlogit_scale
constexpr size_t W_DE = W_SC + 4;                            // [2][64][512] dL/de
constexpr size_t W_PART = W_DE + 2 * CT_BMAX * CT_D;         // [640]        per-block sums of squares
constexpr size_t W_G = W_PART + CT_NBLK;                     // [655,360 + 4] the unclipped gradient
constexpr size_t W_END = W_G + CT_NW + 4;
static_assert(W_END % 4 == 0, "a trial's workspace image stays 16-byte aligned");

// What a workgroup knows of its trial, by value in the kernel arguments.  nsteps: the trial's minibatches in this
// call (0: the trial takes no part); A: the scalars of the step being launched (training only).
struct ClipTrial {
  int batch, nsteps;
  float max_norm;
  AdamScalars A;
};
// TM: the trials an instantiation holds.  TM = 1 (the single-trial entry points, and a study of one) knows its
// trial at compile time, and its grids are that trial's own, so it has no idle workgroups and no test for them: it
// reads its trial with the other arguments, as the kernels did before they had trials.  With more, a workgroup first
// fetches t[blockIdx.z] and decides whether it has work, dependent scalar loads in front of every kernel (measured
// through the single-trial call: 0.2 to 0.3 us per launch).
template <int TM>
struct ClipTrials {
  ClipTrial t[TM];
};
template <int TM>
MMF_DEV int trial_index() { return TM == 1 ? 0 : (int)blockIdx.z; }
// rows of minibatch st of a trial, 0 where it has none
MMF_DEV int trial_rows(const ClipTrial& t, int st, int N) { return st < t.nsteps ? min(t.batch, N - st * t.batch) : 0; }

// ---- 1a. e = P W^T: grid (32 blocks of 16 outputs, 2 towers), 256 threads = 16 outputs x 16 rows ----
// K runs in tiles of 256 staged in LDS by coalesced 16-byte loads (W rows are 2-3 KB apart: a thread walking its
// own row from global memory would touch 64 cache lines per wave instruction); thread (j, r) carries its chain
// across the tiles, so the order is the ascending-k one whatever the tiling.  Rows run in groups of 16.
constexpr int PJ_J = 16, PJ_R = 16, PJ_KT = 256;
constexpr int PJ_LD = PJ_KT + 4;  // 65 x 16 bytes per row: 16 rows read as float4 fall into 16 different bank groups
static_assert(CT_KV % PJ_KT == 0 && CT_KT % PJ_KT == 0 && CT_D % PJ_J == 0, "projection tiles");
// grid z: the trial (its perm row, parameter slice and workspace image)
template <int TM>
__global__ __launch_bounds__(256) void clip_project_kernel(const float* img_feat, const float* txt_feat, int N,
                                                           const int32_t* perm, int st, ClipTrials<TM> T,
                                                           const float* params, float* ws) {
  const int z = trial_index<TM>(), rows = trial_rows(T.t[z], st, N);
  if (TM > 1 && rows == 0) return;
  __shared__ __attribute__((aligned(16))) float Ws[PJ_J * PJ_LD], Ps[PJ_R * PJ_LD];
  __shared__ int srcs[CT_BMAX];
  const int jb = blockIdx.x, tw = blockIdx.y, tid = threadIdx.x;
  const int K = tw ? CT_KT : CT_KV, pos0 = st * T.t[z].batch;
  if (perm) perm += (size_t)z * N;
  params += (size_t)z * kClipTrialStride;
  ws += (size_t)z * W_END;
  if (tid < rows) srcs[tid] = perm ? min(max(perm[pos0 + tid], 0), N - 1) : pos0 + tid;
  __syncthreads();
  const float* feat = tw ? txt_feat : img_feat;
  const float* W = params + (tw ? CT_NV : 0) + (size_t)jb * PJ_J * K;
  float* pb = ws + W_PB + (size_t)tw * CT_BMAX * CT_KV;
  float* E = ws + W_EH + (size_t)tw * CT_BMAX * CT_D;
  const int j = tid >> 4, rr = tid & 15;
  for (int r0 = 0; r0 < rows; r0 += PJ_R) {
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += PJ_KT) {
      float4 wv[4], pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // element tid + 256 u of a [16][64 x float4] tile
        const int e4 = tid + 256 * u, row = e4 >> 6, c = (e4 & 63) * 4;
        wv[u] = *reinterpret_cast<const float4*>(W + (size_t)row * K + k0 + c);
        const int r = r0 + row;
        pv[u] = r < rows ? *reinterpret_cast<const float4*>(feat + (size_t)srcs[r] * K + k0 + c)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();  // the previous tile's readers are done
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e4 = tid + 256 * u, row = e4 >> 6, c = (e4 & 63) * 4;
        *reinterpret_cast<float4*>(Ws + row * PJ_LD + c) = wv[u];
        *reinterpret_cast<float4*>(Ps + row * PJ_LD + c) = pv[u];
        if (jb == 0 && r0 + row < rows)  // the minibatch's rows, for clip_wgrad
          *reinterpret_cast<float4*>(pb + (size_t)(r0 + row) * CT_KV + k0 + c) = pv[u];
      }
      __syncthreads();
#pragma unroll 8
      for (int c = 0; c < PJ_KT; c += 4) {
        const float4 w = *reinterpret_cast<const float4*>(Ws + j * PJ_LD + c);
        const float4 q = *reinterpret_cast<const float4*>(Ps + rr * PJ_LD + c);
        acc = fmaf(q.x, w.x, acc); acc = fmaf(q.y, w.y, acc); acc = fmaf(q.z, w.z, acc); acc = fmaf(q.w, w.w, acc);
      }
    }
    if (r0 + rr < rows) E[(size_t)(r0 + rr) * CT_D + jb * PJ_J + j] = acc;
  }
}

// ---- 1b. the row norm (a fixed tree over 512 squares) and e / norm, in place: grid (rows, 2), 256 threads ----
template <int TM>
__global__ __launch_bounds__(256) void clip_normalise_kernel(int N, int st, ClipTrials<TM> T, float* ws) {
  const int z = trial_index<TM>();
  if (TM > 1 && (int)blockIdx.x >= trial_rows(T.t[z], st, N)) return;
  __shared__ float red[256];
  const int r = blockIdx.x, tw = blockIdx.y, tid = threadIdx.x;
  ws += (size_t)z * W_END;
  float* eh = ws + W_EH + ((size_t)tw * CT_BMAX + r) * CT_D;
  const float e0 = eh[tid], e1 = eh[tid + 256];
  const float nrm = sqrtf(block_tree_sum(fmaf(e1, e1, e0 * e0), red, tid));
  eh[tid] = e0 / nrm;  // no epsilon, as the reference: a zero row gives NaN
  eh[tid + 256] = e1 / nrm;
  if (tid == 0) ws[W_NRM + tw * CT_BMAX + r] = nrm;
}

// ascending-k chain of two unit rows
MMF_DEV float dot512(const float* a, const float* b) {
  float s = 0.f;
  for (int k = 0; k < CT_D; k += 16) {
    float4 x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = *reinterpret_cast<const float4*>(a + k + 4 * u);
      y[u] = *reinterpret_cast<const float4*>(b + k + 4 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s = fmaf(x[u].x, y[u].x, s); s = fmaf(x[u].y, y[u].y, s); s = fmaf(x[u].z, y[u].z, s); s = fmaf(x[u].w, y[u].w, s);
    }
  }
  return s;
}

// ---- 2. logits, both softmaxes, loss, dL/dlogits, dL/dlogit_scale: ONE workgroup of 256 threads per trial ----
// train: D and the scalars go to the workspace; else row_cos[i] = cos[i][i] (row_cos [T][N]).  loss_out [T][ostride].
template <int TM>
__global__ __launch_bounds__(256) void clip_logits_kernel(int N, int st, ClipTrials<TM> T, const float* params, float* ws,
                                                          float* loss_out, int ostride, float* row_cos, int train) {
  const int z = trial_index<TM>(), rows = trial_rows(T.t[z], st, N);
  if (TM > 1 && rows == 0) return;
  params += (size_t)z * kClipTrialStride;
  ws += (size_t)z * W_END;
  loss_out += (size_t)z * ostride + st;
  if (!train) row_cos += (size_t)z * N + (size_t)st * T.t[z].batch;
  __shared__ float L[CT_BMAX * CT_BMAX];        // logits [i][j] (image row i, text row j)
  __shared__ float DL[CT_BMAX * CT_BMAX];       // dL/dlogits
  __shared__ float mx[2 * CT_BMAX], sm[2 * CT_BMAX], part[CT_BMAX];
  const int tid = threadIdx.x, B = rows;
  const float scale = expf(params[CT_NW]);
  const float* EI = ws + W_EH;
  const float* ET = ws + W_EH + (size_t)CT_BMAX * CT_D;
  for (int idx = tid; idx < B * B; idx += 256) {
    const int i = idx / B, j = idx - i * B;
    const float c = dot512(EI + (size_t)i * CT_D, ET + (size_t)j * CT_D);
    if (!train && i == j) row_cos[i] = c;
    L[i * CT_BMAX + j] = scale * c;
  }
  __syncthreads();
  // thread t < B: the softmax of image row t over the texts; B <= t < 2B: of text row t - B over the images
  if (tid < 2 * B) {
    const int r = tid < B ? tid : tid - B;
    const int ld = tid < B ? 1 : CT_BMAX, base = tid < B ? r * CT_BMAX : r;
    float m = L[base];
    for (int q = 1; q < B; ++q) m = fmaxf(m, L[base + q * ld]);
    float s = 0.f;
    for (int q = 0; q < B; ++q) s += expf(L[base + q * ld] - m);
    mx[tid] = m;
    sm[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {  // the two cross-entropies against the diagonal, ascending rows
    float li = 0.f, lt = 0.f;
    for (int r = 0; r < B; ++r) {
      const float d = L[r * CT_BMAX + r];
      li += (mx[r] + logf(sm[r])) - d;
      lt += (mx[B + r] + logf(sm[B + r])) - d;
    }
    const float invB = 1.0f / (float)B;
    *loss_out = (li * invB + lt * invB) * 0.5f;
  }
  if (!train) return;
  // dL/dlogits[i][j] = (softmax_i[j] + softmax_j[i] - 2 [i == j]) / (2 B)
  const float h = 0.5f / (float)B;
  float* D = ws + W_DL;
  for (int idx = tid; idx < B * B; idx += 256) {
    const int i = idx / B, j = idx - i * B;
    const float l = L[i * CT_BMAX + j];
    const float pi = expf(l - mx[i]) / sm[i], pt = expf(l - mx[B + j]) / sm[B + j];
    const float d = ((pi + pt) - (i == j ? 2.f : 0.f)) * h;
    DL[i * CT_BMAX + j] = d;
    D[i * CT_BMAX + j] = d;
  }
  __syncthreads();
  // dL/dlogit_scale = sum_ij D[i][j] logits[i][j]: thread i its row ascending, thread 0 the rows ascending
  if (tid < B) {
    float s = 0.f;
    for (int j = 0; j < B; ++j) s = fmaf(DL[tid * CT_BMAX + j], L[tid * CT_BMAX + j], s);
    part[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < B; ++i) s += part[i];
    ws[W_SC] = scale;
    ws[W_SC + 1] = s;
  }
}

// ---- 3. dL/de of one row: grid (rows, 2), 128 threads (4 columns each) ----
template <int TM>
__global__ __launch_bounds__(128) void clip_embgrad_kernel(int N, int st, ClipTrials<TM> T, float* ws) {
  const int z = trial_index<TM>(), rows = trial_rows(T.t[z], st, N);
  if (TM > 1 && (int)blockIdx.x >= rows) return;
  ws += (size_t)z * W_END;
  __shared__ float coef[CT_BMAX];
  __shared__ __attribute__((aligned(16))) float dy[CT_D], y[CT_D];
  __shared__ float dots;
  const int r = blockIdx.x, tw = blockIdx.y, tid = threadIdx.x;
  const float scale = ws[W_SC];
  const float* D = ws + W_DL;
  // d logits[i][j] / d cos = scale: image row r pairs with text rows q through D[r][q], text row r through D[q][r]
  if (tid < rows) coef[tid] = scale * (tw ? D[tid * CT_BMAX + r] : D[r * CT_BMAX + tid]);
  const float* other = ws + W_EH + (size_t)(tw ? 0 : CT_BMAX) * CT_D;
  const float4 own = *reinterpret_cast<const float4*>(ws + W_EH + ((size_t)tw * CT_BMAX + r) * CT_D + tid * 4);
  __syncthreads();
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  int q = 0;
  for (; q + 4 <= rows; q += 4) {
    float4 o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = *reinterpret_cast<const float4*>(other + (size_t)(q + u) * CT_D + tid * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float c = coef[q + u];
      g.x = fmaf(c, o[u].x, g.x); g.y = fmaf(c, o[u].y, g.y); g.z = fmaf(c, o[u].z, g.z); g.w = fmaf(c, o[u].w, g.w);
    }
  }
  for (; q < rows; ++q) {
    const float4 o = *reinterpret_cast<const float4*>(other + (size_t)q * CT_D + tid * 4);
    const float c = coef[q];
    g.x = fmaf(c, o.x, g.x); g.y = fmaf(c, o.y, g.y); g.z = fmaf(c, o.z, g.z); g.w = fmaf(c, o.w, g.w);
  }
  *reinterpret_cast<float4*>(dy + tid * 4) = g;
  *reinterpret_cast<float4*>(y + tid * 4) = own;
  __syncthreads();
  if (tid == 0) {  // y . dy, ascending
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < CT_D; ++k) s = fmaf(y[k], dy[k], s);
    dots = s;
  }
  __syncthreads();
  // y = e / n  =>  de = (dy - y (y . dy)) / n
  const float s = dots, n = ws[W_NRM + tw * CT_BMAX + r];
  float4 de;
  de.x = (g.x - own.x * s) / n;
  de.y = (g.y - own.y * s) / n;
  de.z = (g.z - own.z * s) / n;
  de.w = (g.w - own.w * s) / n;
  *reinterpret_cast<float4*>(ws + W_DE + ((size_t)tw * CT_BMAX + r) * CT_D + tid * 4) = de;
}

// ---- 4. dW[j][k] = sum_r de[r][j] P[r][k]: 640 blocks of 256 threads, 4 consecutive k per thread ----
template <int TM>
__global__ __launch_bounds__(256) void clip_wgrad_kernel(int N, int st, ClipTrials<TM> T, float* ws) {
  const int z = trial_index<TM>(), rows = trial_rows(T.t[z], st, N);
  if (TM > 1 && rows == 0) return;
  ws += (size_t)z * W_END;
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int flat = blockIdx.x * CT_BLK + tid * 4;
  const int tw = flat >= CT_NV;
  const int K = tw ? CT_KT : CT_KV;
  const int local = flat - (tw ? CT_NV : 0);
  const int j = local / K, k = local - j * K;
  const float* de = ws + W_DE + (size_t)tw * CT_BMAX * CT_D + j;
  const float* pb = ws + W_PB + (size_t)tw * CT_BMAX * CT_KV + k;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  int r = 0;
  for (; r + 4 <= rows; r += 4) {
    float d[4];
    float4 p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      d[u] = de[(size_t)(r + u) * CT_D];
      p[u] = *reinterpret_cast<const float4*>(pb + (size_t)(r + u) * CT_KV);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      g.x = fmaf(d[u], p[u].x, g.x); g.y = fmaf(d[u], p[u].y, g.y); g.z = fmaf(d[u], p[u].z, g.z); g.w = fmaf(d[u], p[u].w, g.w);
    }
  }
  for (; r < rows; ++r) {
    const float d = de[(size_t)r * CT_D];
    const float4 p = *reinterpret_cast<const float4*>(pb + (size_t)r * CT_KV);
    g.x = fmaf(d, p.x, g.x); g.y = fmaf(d, p.y, g.y); g.z = fmaf(d, p.z, g.z); g.w = fmaf(d, p.w, g.w);
  }
  *reinterpret_cast<float4*>(ws + W_G + flat) = g;
  const float sq = fmaf(g.w, g.w, fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)));
  const float tot = block_tree_sum(sq, red, tid);
  if (tid == 0) ws[W_PART + blockIdx.x] = tot;
}

// ---- 5. total norm, clip coefficient, AdamW: 640 blocks of 256 threads ----
// gnorm_out [T][ostride]; grad_out (the single-trial call's, else NULL): trial 0's clipped gradient
template <int TM>
__global__ __launch_bounds__(256) void clip_adamw_kernel(int st, ClipTrials<TM> T, float* params, float* exp_avg,
                                                         float* exp_avg_sq, const float* ws, float* gnorm_out,
                                                         int ostride, float* grad_out) {
  const int z = trial_index<TM>();
  if (TM > 1 && st >= T.t[z].nsteps) return;
  const AdamScalars A = T.t[z].A;
  const float max_norm = T.t[z].max_norm;
  params += (size_t)z * kClipTrialStride;
  exp_avg += (size_t)z * kClipTrialStride;
  exp_avg_sq += (size_t)z * kClipTrialStride;
  ws += (size_t)z * W_END;
  gnorm_out += (size_t)z * ostride + st;
  if (z) grad_out = nullptr;
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int flat = blockIdx.x * CT_BLK + tid * 4;
  // this block's operands first: their loads overlap the norm
  float4 g = *reinterpret_cast<const float4*>(ws + W_G + flat);
  float4 p = *reinterpret_cast<const float4*>(params + flat);
  float4 m = *reinterpret_cast<const float4*>(exp_avg + flat);
  float4 v = *reinterpret_cast<const float4*>(exp_avg_sq + flat);
  // the 640 block sums: thread t its three (t, t + 256, t + 512) ascending, then the fixed tree, then logit_scale's
  float s = ws[W_PART + tid];
  s += ws[W_PART + tid + 256];
  if (tid + 512 < CT_NBLK) s += ws[W_PART + tid + 512];
  const float gs = ws[W_SC + 1];
  const float norm = sqrtf(fmaf(gs, gs, block_tree_sum(s, red, tid)));
  const float c = fminf(max_norm / (norm + 1e-6f), 1.0f);  // clip_grad_norm_: clamped at 1, always applied
  g.x *= c; g.y *= c; g.z *= c; g.w *= c;
  adamw_update(A, g.x, p.x, m.x, v.x);
  adamw_update(A, g.y, p.y, m.y, v.y);
  adamw_update(A, g.z, p.z, m.z, v.z);
  adamw_update(A, g.w, p.w, m.w, v.w);
  *reinterpret_cast<float4*>(params + flat) = p;
  *reinterpret_cast<float4*>(exp_avg + flat) = m;
  *reinterpret_cast<float4*>(exp_avg_sq + flat) = v;
  if (grad_out) *reinterpret_cast<float4*>(grad_out + flat) = g;
  if (blockIdx.x == 0 && tid == 0) {  // logit_scale, and the step's norm
    float ps = params[CT_NW], ms = exp_avg[CT_NW], vs = exp_avg_sq[CT_NW];
    const float gc = gs * c;
    adamw_update(A, gc, ps, ms, vs);
    params[CT_NW] = ps;
    exp_avg[CT_NW] = ms;
    exp_avg_sq[CT_NW] = vs;
    if (grad_out) grad_out[CT_NW] = gc;
    *gnorm_out = norm;
  }
}

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float* src, f16_t* dst, int n4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = *reinterpret_cast<const float4*>(src + (size_t)i * 4);
  *reinterpret_cast<uint2*>(dst + (size_t)i * 4) = make_uint2(pack2h(v.x, v.y), pack2h(v.z, v.w));
}

}  // namespace

size_t clip_train_ws_bytes(int batch) { return (batch < 1 || batch > CT_BMAX) ? 0 : W_END * sizeof(float); }
size_t clip_train_trials_ws_bytes(int trials, int batch_max) {
  return (trials < 1 || trials > kClipTrialsMax) ? 0 : (size_t)trials * clip_train_ws_bytes(batch_max);
}

namespace {
// The trials' step counts for N rows (0 for a trial that is not active; active NULL: all are) into T; the largest
// of them, or -1 on a trial count, N or an active trial's batch out of range.
template <int TM>
int plan_trials(int N, int trials, const int32_t* batch, const int32_t* active, ClipTrials<TM>& T) {
  if (N < 1 || trials < 1 || trials > TM) return -1;
  T = ClipTrials<TM>{};
  int most = 0;
  for (int t = 0; t < trials; ++t) {
    if (active && !active[t]) continue;
    if (batch[t] < 1 || batch[t] > CT_BMAX) return -1;
    T.t[t].batch = batch[t];
    T.t[t].nsteps = (N + batch[t] - 1) / batch[t];
    most = std::max(most, T.t[t].nsteps);
  }
  return most;
}
// the largest minibatch st among the trials that have one: what the row grids are sized by
template <int TM>
int most_rows(const ClipTrials<TM>& T, int trials, int st, int N) {
  int rows = 0;
  for (int t = 0; t < trials; ++t)
    if (st < T.t[t].nsteps) rows = std::max(rows, std::min(T.t[t].batch, N - st * T.t[t].batch));
  return rows;
}

template <int TM>
hipError_t train_epoch_trials(const float* img_feat, const float* txt_feat, int N, int trials, const int32_t* perm,
                              const int32_t* batch, const double* lr, const double* weight_decay,
                              const double* max_norm, const int32_t* step0, const int32_t* active, double beta1,
                              double beta2, double eps, float* params, float* exp_avg, float* exp_avg_sq,
                              float* step_loss, float* step_gnorm, int max_nsteps, float* grad_out, float* ws,
                              hipStream_t s) {
  ClipTrials<TM> T;
  const int most = plan_trials(N, trials, batch, active, T);
  if (most < 0 || most > max_nsteps) return hipErrorInvalidValue;
  for (int t = 0; t < trials; ++t) T.t[t].max_norm = (float)max_norm[t];
  for (int st = 0; st < most; ++st) {
    for (int t = 0; t < trials; ++t)
      if (st < T.t[t].nsteps) T.t[t].A = adam_scalars(lr[t], beta1, beta2, eps, weight_decay[t], step0[t] + st + 1);
    const int rows = most_rows(T, trials, st, N);
    hipLaunchKernelGGL(clip_project_kernel<TM>, dim3(CT_D / PJ_J, 2, trials), dim3(256), 0, s, img_feat, txt_feat, N,
                       perm, st, T, params, ws);
    hipLaunchKernelGGL(clip_normalise_kernel<TM>, dim3(rows, 2, trials), dim3(256), 0, s, N, st, T, ws);
    hipLaunchKernelGGL(clip_logits_kernel<TM>, dim3(1, 1, trials), dim3(256), 0, s, N, st, T, params, ws, step_loss,
                       max_nsteps, nullptr, 1);
    hipLaunchKernelGGL(clip_embgrad_kernel<TM>, dim3(rows, 2, trials), dim3(128), 0, s, N, st, T, ws);
    hipLaunchKernelGGL(clip_wgrad_kernel<TM>, dim3(CT_NBLK, 1, trials), dim3(256), 0, s, N, st, T, ws);
    hipLaunchKernelGGL(clip_adamw_kernel<TM>, dim3(CT_NBLK, 1, trials), dim3(256), 0, s, st, T, params, exp_avg,
                       exp_avg_sq, ws, step_gnorm, max_nsteps, st == most - 1 ? grad_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int TM>
hipError_t contrastive_eval_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                   const int32_t* batch, const int32_t* active, const float* params, float* batch_loss,
                                   float* row_cos, int max_nb, float* ws, hipStream_t s) {
  ClipTrials<TM> T;
  const int most = plan_trials(N, trials, batch, active, T);
  if (most < 0 || most > max_nb) return hipErrorInvalidValue;
  for (int b = 0; b < most; ++b) {
    hipLaunchKernelGGL(clip_project_kernel<TM>, dim3(CT_D / PJ_J, 2, trials), dim3(256), 0, s, img_feat, txt_feat, N,
                       (const int32_t*)nullptr, b, T, params, ws);
    hipLaunchKernelGGL(clip_normalise_kernel<TM>, dim3(most_rows(T, trials, b, N), 2, trials), dim3(256), 0, s, N, b, T,
                       ws);
    hipLaunchKernelGGL(clip_logits_kernel<TM>, dim3(1, 1, trials), dim3(256), 0, s, N, b, T, params, ws, batch_loss,
                       max_nb, row_cos, 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

hipError_t launch_clip_train_epoch_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                          const int32_t* perm, const int32_t* batch, const double* lr,
                                          const double* weight_decay, const double* max_norm, const int32_t* step0,
                                          const int32_t* active, double beta1, double beta2, double eps, float* params,
                                          float* exp_avg, float* exp_avg_sq, float* step_loss, float* step_gnorm,
                                          int max_nsteps, float* grad_out, float* ws, hipStream_t s) {
  const auto run = trials == 1 ? train_epoch_trials<1> : train_epoch_trials<kClipTrialsMax>;
  return run(img_feat, txt_feat, N, trials, perm, batch, lr, weight_decay, max_norm, step0, active, beta1, beta2, eps,
             params, exp_avg, exp_avg_sq, step_loss, step_gnorm, max_nsteps, grad_out, ws, s);
}

hipError_t launch_clip_train_epoch(const float* img_feat, const float* txt_feat, int N, const int32_t* perm, int batch,
                                   double lr, double beta1, double beta2, double eps, double weight_decay,
                                   double max_norm, int step0, float* params, float* exp_avg, float* exp_avg_sq,
                                   float* step_loss, float* step_gnorm, float* grad_out, float* ws, hipStream_t s) {
  if (N < 1 || batch < 1 || batch > CT_BMAX) return hipErrorInvalidValue;
  const int32_t b = batch, s0 = step0;
  return launch_clip_train_epoch_trials(img_feat, txt_feat, N, 1, perm, &b, &lr, &weight_decay, &max_norm, &s0, nullptr,
                                        beta1, beta2, eps, params, exp_avg, exp_avg_sq, step_loss, step_gnorm,
                                        (N + batch - 1) / batch, grad_out, ws, s);
}

hipError_t launch_clip_contrastive_eval_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                               const int32_t* batch, const int32_t* active, const float* params,
                                               float* batch_loss, float* row_cos, int max_nb, float* ws,
                                               hipStream_t s) {
  const auto run = trials == 1 ? contrastive_eval_trials<1> : contrastive_eval_trials<kClipTrialsMax>;
  return run(img_feat, txt_feat, N, trials, batch, active, params, batch_loss, row_cos, max_nb, ws, s);
}

hipError_t launch_clip_contrastive_eval(const float* img_feat, const float* txt_feat, int N, int batch,
                                        const float* params, float* batch_loss, float* row_cos, float* ws,
                                        hipStream_t s) {
  if (N < 1 || batch < 1 || batch > CT_BMAX) return hipErrorInvalidValue;
  const int32_t b = batch;
  return launch_clip_contrastive_eval_trials(img_feat, txt_feat, N, 1, &b, nullptr, params, batch_loss, row_cos,
                                             (N + batch - 1) / batch, ws, s);
}

hipError_t launch_f32_to_f16(const float* src, f16_t* dst, size_t n, hipStream_t s) {
  if (n % 4) return hipErrorInvalidValue;
  const int n4 = (int)(n / 4);
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, src, dst, n4);
  return hipGetLastError();
}
