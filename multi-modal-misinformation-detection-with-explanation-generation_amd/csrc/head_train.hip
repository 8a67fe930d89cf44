// Training of a RoBERTa text head (ai_head / misinfo_head: Linear(768,256)-ReLU-Dropout(0.3)-Linear(256,2),
// misinfo_forensics.py:57-69) on cached CLS rows (train_ai_head.py:206-255 the loop body, :258-296 validate), fp32
// master weights flat in state-dict order -- 0.weight [256][768] | 0.bias [256] | 3.weight [2][256] | 3.bias [2] --
// every minibatch as a chain of four ordinary launches on the caller's stream:
//   1. head_pre    one workgroup per 16 hidden units: the (clamped) permutation entries' feature rows are copied
//                  into the workspace; pre[r][j] = (X_r . W1_j) + b1[j], thread (j, r) one ascending-k fmaf chain
//                  from 0 over LDS tiles of 256, the bias added last
//   2. head_mid    ONE workgroup, thread j = hidden unit j: h = pre > 0 ? pre * scale : 0 where kept, else 0;
//                  logits[r][o] = (ascending-j fmaf chain from 0 of h[r][j] W2[o][j]) + b2[o] by thread (r, o);
//                  thread r the row's cross-entropy m + log(exp(l0 - m) + exp(l1 - m)) - l[label], its argmax (a tie
//                  is class 0) and dlogits = (softmax - onehot) / rows; thread 0 the loss (ascending rows, divided
//                  by rows) and the count; then thread j: dpre[r][j] = (dl[r][0] W2[0][j] + dl[r][1] W2[1][j]) * mask,
//                  db1[j] = ascending-r sum of dpre, dW2[o][j] = ascending-r fmaf chain of dl[r][o] h[r][j], thread
//                  o < 2 db2[o] = ascending-r sum of dl; the tail's sum of squares: thread j's
//                  fma(dW2[1][j]^2 + fma(dW2[0][j]^2 + db1[j]^2)) through the fixed tree over 256, then db2[0]^2 and
//                  db2[1]^2 added in that order
//   3. head_wgrad  dW1 = dpre^T X: a thread owns 4 consecutive elements of the flat gradient, each an ascending-row
//                  fmaf chain; the block's sum of squares by the fixed tree over its 1,024 elements
//   4. head_adamw  every block re-derives the total norm in one order -- thread t < 192 holds block sum t, the fixed
//                  tree over 256, plus the tail's sum, square root --, then clip_grad_norm_'s coefficient and
//                  torch.optim.AdamW on its 1,024 elements (block 192: the 770 tail elements)
// The fixed tree: 256 values, strides 128, 64, ..., 1, red[t] += red[t + s].  Stream order is the only
// synchronisation: no grid barrier, no cooperative launch, no flag, no atomics.  Every reduction has a fixed order
// that depends on the minibatch's row count alone, so results are bit-reproducible and do not depend on the batch
// argument or on how an epoch is split into launches; the step-dependent Adam scalars are computed in double from
// the step number and the step's learning rate alone (as clip_train.hip).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "train_common.h"

namespace {

constexpr int HT_K = 768, HT_H = 256;        // CLS width, hidden units
constexpr int HT_NW1 = HT_H * HT_K;          // 196,608
constexpr int HT_B1 = HT_NW1;                // 0.bias
constexpr int HT_W2 = HT_B1 + HT_H;          // 3.weight [2][256]
constexpr int HT_B2 = HT_W2 + 2 * HT_H;      // 3.bias
constexpr int HT_TAIL = HT_H + 2 * HT_H + 2; // 770 elements after 0.weight
constexpr int HT_BMAX = 64;                  // rows of a minibatch
constexpr int HT_BLK = 1024;                 // elements of a wgrad / adamw block
constexpr int HT_NBLK = HT_NW1 / HT_BLK;     // 192
static_assert(HT_NW1 % HT_BLK == 0 && HT_NBLK <= 256, "block sums fit one tree");
static_assert(HT_B2 + 2 == kHeadTrainParams, "flat parameter layout");

// workspace image, in floats (every region 16-byte aligned); strides are those of HT_BMAX rows whatever the batch
constexpr size_t W_X = 0;                                  // [64][768] the minibatch's feature rows
constexpr size_t W_PRE = W_X + HT_BMAX * HT_K;             // [64][256] pre-activations
constexpr size_t W_DP = W_PRE + HT_BMAX * HT_H;            // [64][256] dL/dpre
constexpr size_t W_PART = W_DP + HT_BMAX * HT_H;           // [192 + 1 (+3)] per-block sums of squares, the tail's
constexpr size_t W_G = W_PART + HT_NBLK + 4;               // [197,378 (+2)] the unclipped gradient
constexpr size_t W_END = W_G + kHeadTrainParams + 2;

// ---- 1. pre = X W1^T + b1: 16 blocks of 16 hidden units, 256 threads = 16 units x 16 rows ----
// K runs in tiles of 256 staged in LDS by coalesced 16-byte loads (W1 rows are 3 KB apart: a thread walking its own
// row from global memory would touch 64 cache lines per wave instruction); thread (j, r) carries its chain across
// the tiles, so the order is the ascending-k one whatever the tiling.  Rows run in groups of 16.
constexpr int PJ_J = 16, PJ_R = 16, PJ_KT = 256;
constexpr int PJ_LD = PJ_KT + 4;  // 65 x 16 bytes per row: 16 rows read as float4 fall into 16 different bank groups
static_assert(HT_K % PJ_KT == 0 && HT_H % PJ_J == 0, "tiles");
__global__ __launch_bounds__(256) void head_pre_kernel(const float* feat, int N, const int32_t* perm, int pos0, int rows,
                                                       const float* params, float* ws) {
  __shared__ __attribute__((aligned(16))) float Ws[PJ_J * PJ_LD], Ps[PJ_R * PJ_LD];
  __shared__ int srcs[HT_BMAX];
  const int jb = blockIdx.x, tid = threadIdx.x;
  if (tid < rows) srcs[tid] = perm ? min(max(perm[pos0 + tid], 0), N - 1) : pos0 + tid;
  __syncthreads();
  const float* W = params + (size_t)jb * PJ_J * HT_K;
  float* xb = ws + W_X;
  const int j = tid >> 4, rr = tid & 15;
  const float bias = params[HT_B1 + jb * PJ_J + j];
  for (int r0 = 0; r0 < rows; r0 += PJ_R) {
    float acc = 0.f;
    for (int k0 = 0; k0 < HT_K; k0 += PJ_KT) {
      float4 wv[4], pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // element tid + 256 u of a [16][64 x float4] tile
        const int e4 = tid + 256 * u, row = e4 >> 6, c = (e4 & 63) * 4;
        wv[u] = *reinterpret_cast<const float4*>(W + (size_t)row * HT_K + k0 + c);
        const int r = r0 + row;
        pv[u] = r < rows ? *reinterpret_cast<const float4*>(feat + (size_t)srcs[r] * HT_K + k0 + c)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();  // the previous tile's readers are done
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e4 = tid + 256 * u, row = e4 >> 6, c = (e4 & 63) * 4;
        *reinterpret_cast<float4*>(Ws + row * PJ_LD + c) = wv[u];
        *reinterpret_cast<float4*>(Ps + row * PJ_LD + c) = pv[u];
        if (jb == 0 && r0 + row < rows)  // the minibatch's rows, for head_wgrad
          *reinterpret_cast<float4*>(xb + (size_t)(r0 + row) * HT_K + k0 + c) = pv[u];
      }
      __syncthreads();
#pragma unroll 8
      for (int c = 0; c < PJ_KT; c += 4) {
        const float4 w = *reinterpret_cast<const float4*>(Ws + j * PJ_LD + c);
        const float4 q = *reinterpret_cast<const float4*>(Ps + rr * PJ_LD + c);
        acc = fmaf(q.x, w.x, acc); acc = fmaf(q.y, w.y, acc); acc = fmaf(q.z, w.z, acc); acc = fmaf(q.w, w.w, acc);
      }
    }
    if (r0 + rr < rows) ws[W_PRE + (size_t)(r0 + rr) * HT_H + jb * PJ_J + j] = acc + bias;
  }
}

// ---- 2. everything between pre and dpre: ONE workgroup of 256 threads (thread j = hidden unit j) ----
// train: keep (nullable) / scale give the dropout mask of the rows at positions pos0 .. of the epoch order; the tail
// gradient, its sum of squares and dpre go to the workspace.  Else: no dropout, row_logits [rows][2] is written.
constexpr int MD_R = 32;          // rows of h staged at a time
constexpr int MD_LD = HT_H + 4;
__global__ __launch_bounds__(256) void head_mid_kernel(const int32_t* labels, int N, const int32_t* perm, int pos0,
                                                       int rows, const uint64_t* keep, float scale,
                                                       const float* params, float* ws, float* loss_out,
                                                       int32_t* correct_out, float* row_logits, int train) {
  __shared__ __attribute__((aligned(16))) float hs[MD_R * MD_LD];
  __shared__ __attribute__((aligned(16))) float w2s[2 * HT_H];
  __shared__ float lg[HT_BMAX * 2], dl[HT_BMAX * 2], rloss[HT_BMAX], red[256];
  __shared__ int lab[HT_BMAX], hit[HT_BMAX];
  const int tid = threadIdx.x;
  const float w20 = params[HT_W2 + tid], w21 = params[HT_W2 + HT_H + tid];
  w2s[tid] = w20;
  w2s[HT_H + tid] = w21;
  if (tid < rows) {
    const int src = perm ? min(max(perm[pos0 + tid], 0), N - 1) : pos0 + tid;
    lab[tid] = labels[src] & 1;
  }
  const float* pre = ws + W_PRE + tid;
  // bit r of km: hidden unit tid of row r is kept
  uint64_t km = ~0ull;
  if (keep) {
    km = 0;
    for (int r = 0; r < rows; ++r)
      km |= (keep[(size_t)(pos0 + r) * 4 + (tid >> 6)] >> (tid & 63) & 1ull) << r;
  }
  const float sc = keep ? scale : 1.0f;
  for (int r0 = 0; r0 < rows; r0 += MD_R) {
    const int nr = min(MD_R, rows - r0);
    __syncthreads();  // the previous group's readers are done (and w2s / lab are written)
    for (int r = 0; r < nr; ++r) {
      const float a = pre[(size_t)(r0 + r) * HT_H];
      hs[r * MD_LD + tid] = (a > 0.f && (km >> (r0 + r) & 1ull)) ? a * sc : 0.f;
    }
    __syncthreads();
    if (tid < 2 * nr) {  // thread (r, o): the ascending-j chain
      const int r = tid >> 1, o = tid & 1;
      float acc = 0.f;
#pragma unroll 8
      for (int c = 0; c < HT_H; c += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(hs + r * MD_LD + c);
        const float4 wv = *reinterpret_cast<const float4*>(w2s + o * HT_H + c);
        acc = fmaf(hv.x, wv.x, acc); acc = fmaf(hv.y, wv.y, acc); acc = fmaf(hv.z, wv.z, acc); acc = fmaf(hv.w, wv.w, acc);
      }
      lg[(r0 + r) * 2 + o] = acc + params[HT_B2 + o];
    }
  }
  __syncthreads();
  if (tid < rows) {
    const float l0 = lg[tid * 2], l1 = lg[tid * 2 + 1];
    const CeRow o = ce_row(l0, l1, lab[tid]);
    rloss[tid] = o.loss;
    hit[tid] = o.hit;
    const float inv = 1.0f / (float)rows;
    dl[tid * 2] = o.d0 * inv;
    dl[tid * 2 + 1] = o.d1 * inv;
    if (!train) {
      row_logits[(size_t)tid * 2] = l0;
      row_logits[(size_t)tid * 2 + 1] = l1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    int c = 0;
    for (int r = 0; r < rows; ++r) {
      s += rloss[r];
      c += hit[r];
    }
    *loss_out = s / (float)rows;
    if (correct_out) *correct_out = c;
  }
  if (!train) return;
  float* dp = ws + W_DP + tid;
  float db1 = 0.f, g20 = 0.f, g21 = 0.f;
  for (int r = 0; r < rows; ++r) {
    const float a = pre[(size_t)r * HT_H];
    const bool live = a > 0.f && (km >> r & 1ull);
    const float h = live ? a * sc : 0.f;
    const float d0 = dl[r * 2], d1 = dl[r * 2 + 1];
    const float dh = fmaf(d1, w21, d0 * w20);
    const float d = live ? dh * sc : 0.f;
    dp[(size_t)r * HT_H] = d;
    db1 += d;
    g20 = fmaf(d0, h, g20);
    g21 = fmaf(d1, h, g21);
  }
  float* G = ws + W_G;
  G[HT_B1 + tid] = db1;
  G[HT_W2 + tid] = g20;
  G[HT_W2 + HT_H + tid] = g21;
  float tot = block_tree_sum(fmaf(g21, g21, fmaf(g20, g20, db1 * db1)), red, tid);
  if (tid == 0) {
    float b0 = 0.f, b1 = 0.f;
    for (int r = 0; r < rows; ++r) {
      b0 += dl[r * 2];
      b1 += dl[r * 2 + 1];
    }
    G[HT_B2] = b0;
    G[HT_B2 + 1] = b1;
    tot = fmaf(b0, b0, tot);
    tot = fmaf(b1, b1, tot);
    ws[W_PART + HT_NBLK] = tot;
  }
}

// ---- 3. dW1[j][k] = sum_r dpre[r][j] X[r][k]: 192 blocks of 256 threads, 4 consecutive k per thread ----
__global__ __launch_bounds__(256) void head_wgrad_kernel(int rows, float* ws) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int flat = blockIdx.x * HT_BLK + tid * 4;
  const int j = flat / HT_K, k = flat - j * HT_K;
  const float* dpre = ws + W_DP + j;
  const float* xb = ws + W_X + k;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  int r = 0;
  for (; r + 4 <= rows; r += 4) {
    float d[4];
    float4 p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      d[u] = dpre[(size_t)(r + u) * HT_H];
      p[u] = *reinterpret_cast<const float4*>(xb + (size_t)(r + u) * HT_K);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      g.x = fmaf(d[u], p[u].x, g.x); g.y = fmaf(d[u], p[u].y, g.y); g.z = fmaf(d[u], p[u].z, g.z); g.w = fmaf(d[u], p[u].w, g.w);
    }
  }
  for (; r < rows; ++r) {
    const float d = dpre[(size_t)r * HT_H];
    const float4 p = *reinterpret_cast<const float4*>(xb + (size_t)r * HT_K);
    g.x = fmaf(d, p.x, g.x); g.y = fmaf(d, p.y, g.y); g.z = fmaf(d, p.z, g.z); g.w = fmaf(d, p.w, g.w);
  }
  *reinterpret_cast<float4*>(ws + W_G + flat) = g;
  const float sq = fmaf(g.w, g.w, fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)));
  const float tot = block_tree_sum(sq, red, tid);
  if (tid == 0) ws[W_PART + blockIdx.x] = tot;
}

// ---- 4. total norm, clip coefficient, AdamW: 192 blocks of 1,024 elements + 1 block for the 770 tail elements ----
__global__ __launch_bounds__(256) void head_adamw_kernel(AdamScalars A, float max_norm, float* params, float* exp_avg,
                                                         float* exp_avg_sq, const float* ws, float* gnorm_out,
                                                         float* grad_out) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const bool tail = blockIdx.x == HT_NBLK;
  const int flat = blockIdx.x * HT_BLK + tid * 4;
  float4 g, p, m, v;
  if (!tail) {  // this block's operands first: their loads overlap the norm
    g = *reinterpret_cast<const float4*>(ws + W_G + flat);
    p = *reinterpret_cast<const float4*>(params + flat);
    m = *reinterpret_cast<const float4*>(exp_avg + flat);
    v = *reinterpret_cast<const float4*>(exp_avg_sq + flat);
  }
  const float s = tid < HT_NBLK ? ws[W_PART + tid] : 0.f;
  const float norm = sqrtf(block_tree_sum(s, red, tid) + ws[W_PART + HT_NBLK]);
  const float c = fminf(max_norm / (norm + 1e-6f), 1.0f);  // clip_grad_norm_: clamped at 1, always applied
  if (!tail) {
    g.x *= c; g.y *= c; g.z *= c; g.w *= c;
    adamw_update(A, g.x, p.x, m.x, v.x);
    adamw_update(A, g.y, p.y, m.y, v.y);
    adamw_update(A, g.z, p.z, m.z, v.z);
    adamw_update(A, g.w, p.w, m.w, v.w);
    *reinterpret_cast<float4*>(params + flat) = p;
    *reinterpret_cast<float4*>(exp_avg + flat) = m;
    *reinterpret_cast<float4*>(exp_avg_sq + flat) = v;
    if (grad_out) *reinterpret_cast<float4*>(grad_out + flat) = g;
    return;
  }
  for (int i = HT_NW1 + tid; i < kHeadTrainParams; i += 256) {
    float ps = params[i], ms = exp_avg[i], vs = exp_avg_sq[i];
    const float gc = ws[W_G + i] * c;
    adamw_update(A, gc, ps, ms, vs);
    params[i] = ps;
    exp_avg[i] = ms;
    exp_avg_sq[i] = vs;
    if (grad_out) grad_out[i] = gc;
  }
  if (tid == 0) *gnorm_out = norm;
}

}  // namespace

size_t head_train_ws_bytes(int batch) { return (batch < 1 || batch > HT_BMAX) ? 0 : W_END * sizeof(float); }

hipError_t launch_head_train_epoch(const float* feat, const int32_t* labels, int N, const int32_t* perm,
                                   const uint64_t* keep, float p_drop, int batch, const double* lr_steps, double beta1,
                                   double beta2, double eps, double weight_decay, double max_norm, int step0,
                                   float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                                   int32_t* step_correct, float* step_gnorm, float* grad_out, float* ws, hipStream_t s) {
  if (N < 1 || batch < 1 || batch > HT_BMAX || !(p_drop >= 0.f && p_drop < 1.f)) return hipErrorInvalidValue;
  const int nsteps = (N + batch - 1) / batch;
  const float scale = (float)(1.0 / (1.0 - (double)p_drop));
  for (int st = 0; st < nsteps; ++st) {
    const int pos0 = st * batch, rows = std::min(batch, N - pos0);
    const AdamScalars A = adam_scalars(lr_steps[st], beta1, beta2, eps, weight_decay, step0 + st + 1);
    hipLaunchKernelGGL(head_pre_kernel, dim3(HT_H / PJ_J), dim3(256), 0, s, feat, N, perm, pos0, rows, params, ws);
    hipLaunchKernelGGL(head_mid_kernel, dim3(1), dim3(256), 0, s, labels, N, perm, pos0, rows, keep, scale, params, ws,
                       step_loss + st, step_correct + st, (float*)nullptr, 1);
    hipLaunchKernelGGL(head_wgrad_kernel, dim3(HT_NBLK), dim3(256), 0, s, rows, ws);
    hipLaunchKernelGGL(head_adamw_kernel, dim3(HT_NBLK + 1), dim3(256), 0, s, A, (float)max_norm, params,
                       exp_avg, exp_avg_sq, ws, step_gnorm + st, st == nsteps - 1 ? grad_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_head_eval(const float* feat, const int32_t* labels, int N, int batch, const float* params,
                            float* batch_loss, float* row_logits, float* ws, hipStream_t s) {
  if (N < 1 || batch < 1 || batch > HT_BMAX) return hipErrorInvalidValue;
  const int nb = (N + batch - 1) / batch;
  for (int b = 0; b < nb; ++b) {
    const int pos0 = b * batch, rows = std::min(batch, N - pos0);
    hipLaunchKernelGGL(head_pre_kernel, dim3(HT_H / PJ_J), dim3(256), 0, s, feat, N, (const int32_t*)nullptr, pos0, rows,
                       params, ws);
    hipLaunchKernelGGL(head_mid_kernel, dim3(1), dim3(256), 0, s, labels, N, (const int32_t*)nullptr, pos0, rows,
                       (const uint64_t*)nullptr, 1.0f, params, ws, batch_loss + b, (int32_t*)nullptr,
                       row_logits + (size_t)pos0 * 2, 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
