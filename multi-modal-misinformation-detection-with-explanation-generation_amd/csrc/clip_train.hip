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

// ---- 1a. e = P W^T: grid (32 blocks of 16 outputs, 2 towers), 256 threads = 16 outputs x 16 rows ----
// K runs in tiles of 256 staged in LDS by coalesced 16-byte loads (W rows are 2-3 KB apart: a thread walking its
// own row from global memory would touch 64 cache lines per wave instruction); thread (j, r) carries its chain
// across the tiles, so the order is the ascending-k one whatever the tiling.  Rows run in groups of 16.
constexpr int PJ_J = 16, PJ_R = 16, PJ_KT = 256;
constexpr int PJ_LD = PJ_KT + 4;  // 65 x 16 bytes per row: 16 rows read as float4 fall into 16 different bank groups
static_assert(CT_KV % PJ_KT == 0 && CT_KT % PJ_KT == 0 && CT_D % PJ_J == 0, "projection tiles");
__global__ __launch_bounds__(256) void clip_project_kernel(const float* img_feat, const float* txt_feat, int N,
                                                           const int32_t* perm, int pos0, int rows,
                                                           const float* params, float* ws) {
  __shared__ __attribute__((aligned(16))) float Ws[PJ_J * PJ_LD], Ps[PJ_R * PJ_LD];
  __shared__ int srcs[CT_BMAX];
  const int jb = blockIdx.x, tw = blockIdx.y, tid = threadIdx.x;
  const int K = tw ? CT_KT : CT_KV;
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
__global__ __launch_bounds__(256) void clip_normalise_kernel(float* ws) {
  __shared__ float red[256];
  const int r = blockIdx.x, tw = blockIdx.y, tid = threadIdx.x;
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

// ---- 2. logits, both softmaxes, loss, dL/dlogits, dL/dlogit_scale: ONE workgroup of 256 threads ----
// train: D and the scalars go to the workspace; else row_cos[i] = cos[i][i]
__global__ __launch_bounds__(256) void clip_logits_kernel(int rows, const float* params, float* ws, float* loss_out,
                                                          float* row_cos, int train) {
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
    const int st = tid < B ? 1 : CT_BMAX, base = tid < B ? r * CT_BMAX : r;
    float m = L[base];
    for (int q = 1; q < B; ++q) m = fmaxf(m, L[base + q * st]);
    float s = 0.f;
    for (int q = 0; q < B; ++q) s += expf(L[base + q * st] - m);
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
__global__ __launch_bounds__(128) void clip_embgrad_kernel(int rows, float* ws) {
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
__global__ __launch_bounds__(256) void clip_wgrad_kernel(int rows, float* ws) {
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
__global__ __launch_bounds__(256) void clip_adamw_kernel(AdamScalars A, float max_norm, float* params, float* exp_avg,
                                                         float* exp_avg_sq, const float* ws, float* gnorm_out,
                                                         float* grad_out) {
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

hipError_t launch_clip_train_epoch(const float* img_feat, const float* txt_feat, int N, const int32_t* perm, int batch,
                                   double lr, double beta1, double beta2, double eps, double weight_decay,
                                   double max_norm, int step0, float* params, float* exp_avg, float* exp_avg_sq,
                                   float* step_loss, float* step_gnorm, float* grad_out, float* ws, hipStream_t s) {
  if (N < 1 || batch < 1 || batch > CT_BMAX) return hipErrorInvalidValue;
  const int nsteps = (N + batch - 1) / batch;
  for (int st = 0; st < nsteps; ++st) {
    const int pos0 = st * batch, rows = std::min(batch, N - pos0);
    const AdamScalars A = adam_scalars(lr, beta1, beta2, eps, weight_decay, step0 + st + 1);
    hipLaunchKernelGGL(clip_project_kernel, dim3(CT_D / PJ_J, 2), dim3(256), 0, s, img_feat, txt_feat, N, perm, pos0,
                       rows, params, ws);
    hipLaunchKernelGGL(clip_normalise_kernel, dim3(rows, 2), dim3(256), 0, s, ws);
    hipLaunchKernelGGL(clip_logits_kernel, dim3(1), dim3(256), 0, s, rows, params, ws, step_loss + st, nullptr, 1);
    hipLaunchKernelGGL(clip_embgrad_kernel, dim3(rows, 2), dim3(128), 0, s, rows, ws);
    hipLaunchKernelGGL(clip_wgrad_kernel, dim3(CT_NBLK), dim3(256), 0, s, rows, ws);
    hipLaunchKernelGGL(clip_adamw_kernel, dim3(CT_NBLK), dim3(256), 0, s, A, (float)max_norm, params, exp_avg,
                       exp_avg_sq, ws, step_gnorm + st, st == nsteps - 1 ? grad_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_clip_contrastive_eval(const float* img_feat, const float* txt_feat, int N, int batch,
                                        const float* params, float* batch_loss, float* row_cos, float* ws,
                                        hipStream_t s) {
  if (N < 1 || batch < 1 || batch > CT_BMAX) return hipErrorInvalidValue;
  const int nb = (N + batch - 1) / batch;
  for (int b = 0; b < nb; ++b) {
    const int pos0 = b * batch, rows = std::min(batch, N - pos0);
    hipLaunchKernelGGL(clip_project_kernel, dim3(CT_D / PJ_J, 2), dim3(256), 0, s, img_feat, txt_feat, N, nullptr, pos0,
                       rows, params, ws);
    hipLaunchKernelGGL(clip_normalise_kernel, dim3(rows, 2), dim3(256), 0, s, ws);
    hipLaunchKernelGGL(clip_logits_kernel, dim3(1), dim3(256), 0, s, rows, params, ws, batch_loss + b, row_cos + pos0,
                       0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_f32_to_f16(const float* src, f16_t* dst, size_t n, hipStream_t s) {
  if (n % 4) return hipErrorInvalidValue;
  const int n4 = (int)(n / 4);
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, src, dst, n4);
  return hipGetLastError();
}
