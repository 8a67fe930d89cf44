// EfficientNet's head conv stage -- features.8 = Conv2d(320, 1280, 1, bias=False) + BatchNorm2d(1280) (eval mode)
// + SiLU -- trained jointly with the deployed classifier (Dropout(0.2) then Linear(1280, 2) on the pooled row) on
// cached trunk rows x [R][49][320] (mmf_effnet_trunk): include/mmf_hip.h mmf_effhead_train_epoch / mmf_effhead_eval.
// The running statistics are inputs and never written; no gradient with respect to the trunk is formed.
//
// Parameters: ONE flat fp32 vector of kEffHeadParams entries in state-dict order,
//   W [1280][320] | gamma [1280] | beta [1280] | Wc [2][1280] | bc [2].
// Three launches per optimizer step, in stream order, no host synchronisation and no atomics, flags or spin-waits:
//
//   1. effhead_forward_kernel, grid (20 channel tiles of 64, n images), 256 threads.  The row tile is ONE image: its 49
//      positions padded with zero rows to 64, so that no image straddles a tile and the pool needs no cross-tile sum.
//      z = x W^T on v_mfma_f32_32x32x2_f32 (wave w: rows 32 (w & 1) .., channels 32 (w >> 1) ..; K = 320 from LDS in
//      five chunks of 64): per output ONE fmaf chain over k = 0 .. 319 ascending, from 0.  s_c = gamma_c /
//      sqrtf(var_c + eps), t_c = fmaf(-mean_c, s_c, beta_c) from the current parameters; y = fmaf(s_c, z, t_c);
//      a = silu_precise(y).  z goes to the workspace (the backward recomputes y from it bit for bit, and needs z itself
//      for gamma), a into LDS, and thread c < 64 adds the 49 positions of its channel in ascending order from 0 and
//      multiplies by fp32(1 / 49): pooled[r][c].  The image-0 workgroups also leave s and t in the workspace: the
//      backward reads them there, since gamma and beta are updated by one of its own workgroups.
//
//   2. effhead_cls_kernel, ONE workgroup of 256 threads: effnet_train.hip's classifier step on the n pooled rows.
//      xd = keep ? pooled * scale : 0.  Thread t owns columns t + 256 k, k = 0 .. 4, of both classes: its partial
//      logit is the fmaf chain over k ascending from 0; the 256 partials go through wave_sum's xor butterfly (offsets
//      32 .. 1), then ((wave0 + wave1) + wave2) + wave3, then the bias.  ce_row per row; loss and correct count are
//      ascending-row sums by thread 0; the classifier's gradients are ascending-row fmaf chains by the owning thread,
//      which also applies Adam.  dpooled[r][c] = mult * fmaf(dl1, Wc[1][c], dl0 * Wc[0][c]) with the weights from
//      BEFORE the update, mult = scale, 0 or (no keep) 1.
//
//   3. effhead_backward_kernel, grid (10 k tiles of 32, 20 channel tiles of 64) = 200 owners, 256 threads.  An owner
//      walks ALL M = 49 n rows in ascending order, 32 at a time: dy[m][c] = (dpooled[r][c] * fp32(1 / 49)) *
//      (sig * (1 + y * (1 - sig))), sig = 1 / (1 + expf(-y)), staged in LDS with the trunk rows' 32 columns; then
//      dW[c][k] += (dy * s_c) x[m][k] on v_mfma_f32_16x16x4_f32 (wave w: channels 16 w .., two accumulators for
//      the two halves of the k tile): per output ONE fmaf chain over m = 0 .. M - 1 ascending, from 0 -- never split
//      across waves or workgroups.  The owner applies Adam to its tile in the epilogue; the gradient goes to memory
//      only as grad_out on the last minibatch.  The k-tile-0 owners also keep, in thread c < 64, dbeta_c += dy and
//      dgamma_c = fmaf(dy, (z - mean_c) / sqrtf(var_c + eps), dgamma_c) over the same rows ascending, and apply Adam
//      to gamma and beta.  Rows past M in the last chunk are zeros; fmaf(0, 0, acc) leaves acc unchanged.
//
// All arithmetic is fp32; the Adam scalars of a step are computed in double from the step number alone and rounded
// once (train_common.h), so a step's bits do not depend on which call ran it.  Every order above depends on the
// minibatch's row count alone: two launches of the same call give identical bits.  mmf_effhead_eval runs launch 1
// (without storing z) and the forward half of launch 2 without dropout, per batch; a row's logits do not depend on the
// batch it is evaluated in, since every row tile is one image.
#include "common.h"
#include "kernels.h"
#include "train_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int EH_K = 320, EH_C = 1280, EH_HW = 49, EH_EB = 64;
constexpr int EH_OFF_G = EH_C * EH_K, EH_OFF_B = EH_OFF_G + EH_C, EH_OFF_WC = EH_OFF_B + EH_C,
              EH_OFF_BC = EH_OFF_WC + 2 * EH_C;
static_assert(EH_OFF_BC + 2 == kEffHeadParams, "effhead_train: parameter count");
constexpr int EH_KT = EH_C / 256;        // 5 columns per thread of the classifier
constexpr int EH_SLOTS = 2 * EH_KT + 1;  // 10 weights + (threads 0, 1) a bias
constexpr int EH_KC = 64;                // forward: k per LDS chunk
constexpr int EH_LD = EH_KC + 1;         // LDS row stride, floats
constexpr int EH_MC = 32;                // backward: rows per chunk
constexpr float EH_INV_HW = 1.0f / 49.0f;

// workspace, in floats: z [batch * 49][1280] | pooled [batch][1280] | dpooled [batch][1280] | s [1280] | t [1280]
struct EhWs {
  float *z, *pooled, *dpooled, *s, *t;
};
__host__ __device__ inline EhWs eh_ws(float* ws, int batch) {
  EhWs w;
  w.z = ws;
  w.pooled = w.z + (size_t)batch * EH_HW * EH_C;
  w.dpooled = w.pooled + (size_t)batch * EH_C;
  w.s = w.dpooled + (size_t)batch * EH_C;
  w.t = w.s + EH_C;
  return w;
}

// the bank row of image r of the minibatch: perm's entry clamped into [0, R) (training), or row0 + r (eval: perm NULL)
MMF_DEV int eh_src(const int32_t* perm, int pos0, int r, int R) {
  return perm ? min(max(perm[pos0 + r], 0), R - 1) : pos0 + r;
}

// ---- 1. forward: one image x 64 channels per workgroup ----
__global__ __launch_bounds__(256) void effhead_forward_kernel(const float* __restrict__ trunk, int R,
                                                              const int32_t* __restrict__ perm, int pos0,
                                                              const float* __restrict__ params,
                                                              const float* __restrict__ bn_mean,
                                                              const float* __restrict__ bn_var, float bn_eps,
                                                              float* __restrict__ z_out, float* __restrict__ pooled,
                                                              float* __restrict__ s_out, float* __restrict__ t_out) {
  __shared__ float sx[64 * EH_LD], sw[64 * EH_LD];  // [row][k] and [channel][k] of the chunk; then a [row][channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64, r = blockIdx.y;
  const float* x = trunk + (size_t)eh_src(perm, pos0, r, R) * EH_HW * EH_K;
  const int row0 = 32 * (wave & 1), col0 = 32 * (wave >> 1);
  const int li = lane & 31, lh = lane >> 5;
  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < EH_K; k0 += EH_KC) {
    __syncthreads();  // the previous chunk's readers are done
    for (int e = tid; e < 64 * EH_KC; e += 256) {
      const int row = e / EH_KC, k = e % EH_KC;
      sx[row * EH_LD + k] = row < EH_HW ? x[(size_t)row * EH_K + k0 + k] : 0.f;
      sw[row * EH_LD + k] = params[(size_t)(c0 + row) * EH_K + k0 + k];
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < EH_KC; k += 2) {
      const float a = sx[(row0 + li) * EH_LD + k + lh];  // A[i = lane & 31][k = lane >> 5]
      const float b = sw[(col0 + li) * EH_LD + k + lh];  // B[k = lane >> 5][j = lane & 31] = W[channel j][k]
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  __syncthreads();
  // C: column lane & 31, row (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  const int c = c0 + col0 + li;
  const float s = params[EH_OFF_G + c] / sqrtf(bn_var[c] + bn_eps);
  const float t = fmaf(-bn_mean[c], s, params[EH_OFF_B + c]);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = row0 + (i & 3) + 8 * (i >> 2) + 4 * lh;
    if (row < EH_HW) {
      const float z = acc[i];
      if (z_out) z_out[((size_t)r * EH_HW + row) * EH_C + c] = z;
      sx[row * EH_LD + col0 + li] = silu_precise(fmaf(s, z, t));
    }
  }
  if (r == 0 && s_out && row0 == 0 && lh == 0) {
    s_out[c] = s;
    t_out[c] = t;
  }
  __syncthreads();
  if (tid < 64) {
    float sum = 0.f;
    for (int p = 0; p < EH_HW; ++p) sum += sx[p * EH_LD + tid];
    pooled[(size_t)r * EH_C + c0 + tid] = sum * EH_INV_HW;
  }
}

// ---- 2. the classifier step on the pooled rows (TRAIN), or validate's forward (!TRAIN) ----
struct EhClsArgs {
  const float* pooled; const int32_t* labels; int R; const int32_t* perm; int pos0; int rows;
  const uint64_t* keep; float scale;
  AdamScalars ad; float wd; int decay;
  float *params, *exp_avg, *exp_avg_sq, *dpooled, *loss_out; int32_t* correct_out; float *grad_out, *row_logits;
};

// slot q of thread tid in the flat parameter vector (effnet_train.hip's ownership)
MMF_DEV int eh_cls_index(int q, int tid) {
  return q < 2 * EH_KT ? EH_OFF_WC + (q / EH_KT) * EH_C + tid + 256 * (q % EH_KT) : EH_OFF_BC + tid;
}
MMF_DEV bool eh_cls_live(int q, int tid) { return q < 2 * EH_KT || tid < 2; }

// thread tid's five dropout multipliers of the row at epoch position pos: scale, 0, or (no keep) 1
MMF_DEV void eh_mult(const EhClsArgs& A, int pos, int tid, float (&mu)[EH_KT]) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < EH_KT; ++k) {
    // column tid + 256 k = 64-bit word wave + 4 k, bit lane
    mu[k] = !A.keep ? 1.0f : (((A.keep[(size_t)pos * (EH_C / 64) + wave + 4 * k] >> lane) & 1ull) ? A.scale : 0.f);
  }
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void effhead_cls_kernel(EhClsArgs A) {
  __shared__ float s_red[4][EH_EB][2];
  __shared__ float s_dl[EH_EB][2], s_loss[EH_EB], s_cor[EH_EB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float pv[EH_SLOTS];
#pragma unroll
  for (int q = 0; q < EH_SLOTS; ++q) pv[q] = eh_cls_live(q, tid) ? A.params[eh_cls_index(q, tid)] : 0.f;
  for (int r = 0; r < A.rows; ++r) {
    float mu[EH_KT];
    eh_mult(A, A.pos0 + r, tid, mu);
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int k = 0; k < EH_KT; ++k) {
      const float x = A.pooled[(size_t)r * EH_C + tid + 256 * k];
      const float xd = A.keep ? (mu[k] != 0.f ? x * mu[k] : 0.f) : x;
      p0 = fmaf(pv[k], xd, p0);
      p1 = fmaf(pv[EH_KT + k], xd, p1);
    }
    p0 = wave_sum(p0);
    p1 = wave_sum(p1);
    if (lane == 0) { s_red[wave][r][0] = p0; s_red[wave][r][1] = p1; }
  }
  __syncthreads();
  if (tid < A.rows) {
    const int r = tid;
    const float l0 = (((s_red[0][r][0] + s_red[1][r][0]) + s_red[2][r][0]) + s_red[3][r][0]) + A.params[EH_OFF_BC];
    const float l1 = (((s_red[0][r][1] + s_red[1][r][1]) + s_red[2][r][1]) + s_red[3][r][1]) + A.params[EH_OFF_BC + 1];
    const CeRow o = ce_row(l0, l1, A.labels[eh_src(A.perm, A.pos0, r, A.R)] & 1);
    const float inv_rows = 1.0f / (float)A.rows;
    s_loss[r] = o.loss;
    s_cor[r] = o.hit ? 1.f : 0.f;
    s_dl[r][0] = o.d0 * inv_rows;
    s_dl[r][1] = o.d1 * inv_rows;
    if (!TRAIN) {
      A.row_logits[(size_t)(A.pos0 + r) * 2] = l0;
      A.row_logits[(size_t)(A.pos0 + r) * 2 + 1] = l1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float loss_sum = 0.f, cor_sum = 0.f;
    for (int r = 0; r < A.rows; ++r) { loss_sum += s_loss[r]; cor_sum += s_cor[r]; }
    *A.loss_out = loss_sum * (1.0f / (float)A.rows);
    if (TRAIN) *A.correct_out = (int32_t)cor_sum;
  }
  if (!TRAIN) return;
  float g[EH_SLOTS];
#pragma unroll
  for (int q = 0; q < EH_SLOTS; ++q) g[q] = 0.f;
  for (int r = 0; r < A.rows; ++r) {
    float mu[EH_KT];
    eh_mult(A, A.pos0 + r, tid, mu);
    const float d0 = s_dl[r][0], d1 = s_dl[r][1];
#pragma unroll
    for (int k = 0; k < EH_KT; ++k) {
      const float x = A.pooled[(size_t)r * EH_C + tid + 256 * k];
      const float xd = A.keep ? (mu[k] != 0.f ? x * mu[k] : 0.f) : x;
      g[k] = fmaf(d0, xd, g[k]);
      g[EH_KT + k] = fmaf(d1, xd, g[EH_KT + k]);
      const float dp = fmaf(d1, pv[EH_KT + k], d0 * pv[k]);
      A.dpooled[(size_t)r * EH_C + tid + 256 * k] = A.keep ? (mu[k] != 0.f ? dp * mu[k] : 0.f) : dp;
    }
    g[2 * EH_KT] += (tid & 1) ? d1 : d0;
  }
#pragma unroll
  for (int q = 0; q < EH_SLOTS; ++q) {
    if (eh_cls_live(q, tid)) {
      const int p = eh_cls_index(q, tid);
      float pq = pv[q], m = A.exp_avg[p], v = A.exp_avg_sq[p];
      adam_update(A.ad, A.decay ? fmaf(A.wd, pq, g[q]) : g[q], pq, m, v);
      A.params[p] = pq;
      A.exp_avg[p] = m;
      A.exp_avg_sq[p] = v;
      if (A.grad_out) A.grad_out[p] = g[q];
    }
  }
}

// ---- 3. backward: one owner per 64 channel x 32 k tile of dW ----
struct EhBwdArgs {
  const float* trunk; int R; const int32_t* perm; int pos0; int rows;
  const float *z, *dpooled, *s, *t, *bn_mean, *bn_var; float bn_eps;
  AdamScalars ad; float wd; int decay;
  float *params, *exp_avg, *exp_avg_sq, *grad_out;
};

MMF_DEV void eh_adam_at(const EhBwdArgs& A, int p, float g) {
  float pq = A.params[p], m = A.exp_avg[p], v = A.exp_avg_sq[p];
  adam_update(A.ad, A.decay ? fmaf(A.wd, pq, g) : g, pq, m, v);
  A.params[p] = pq;
  A.exp_avg[p] = m;
  A.exp_avg_sq[p] = v;
  if (A.grad_out) A.grad_out[p] = g;
}

__global__ __launch_bounds__(256) void effhead_backward_kernel(EhBwdArgs A) {
  __shared__ float s_dy[EH_MC][64 + 1], s_xh[EH_MC][64 + 1], s_x[EH_MC][32 + 1];
  __shared__ int s_src[EH_EB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * 32, c0 = blockIdx.y * 64;
  const bool bn_owner = blockIdx.x == 0;
  const int M = A.rows * EH_HW;
  if (tid < A.rows) s_src[tid] = eh_src(A.perm, A.pos0, tid, A.R);
  // the stage: channel cs of rows (tid >> 6) + 4 j; trunk element (row tid >> 3 .., k 4 (tid & 7) ..)
  const int cs = tid & 63;
  const float sc = A.s[c0 + cs], tc = A.t[c0 + cs];
  const float mean = A.bn_mean[c0 + cs], sd = sqrtf(A.bn_var[c0 + cs] + A.bn_eps);
  // the MFMA operands: A[i = lane & 15][k = lane >> 4] = dy[row][channel] * s, B[k = lane >> 4][j = lane & 15] = x[row][k]
  const int ml = lane & 15, mk = lane >> 4;
  const float sa = A.s[c0 + 16 * wave + ml];
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float dgamma = 0.f, dbeta = 0.f;
  __syncthreads();
  for (int m0 = 0; m0 < M; m0 += EH_MC) {
#pragma unroll
    for (int j = 0; j < EH_MC / 4; ++j) {
      const int row = (tid >> 6) + 4 * j, m = m0 + row;
      float dy = 0.f, xh = 0.f;
      if (m < M) {
        const int r = m / EH_HW;
        const float z = A.z[(size_t)m * EH_C + c0 + cs];
        const float y = fmaf(sc, z, tc);
        const float sig = 1.0f / (1.0f + expf(-y));
        dy = (A.dpooled[(size_t)r * EH_C + c0 + cs] * EH_INV_HW) * (sig * (1.0f + y * (1.0f - sig)));
        if (bn_owner) xh = (z - mean) / sd;
      }
      s_dy[row][cs] = dy;
      if (bn_owner) s_xh[row][cs] = xh;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j, row = e >> 5, k = e & 31, m = m0 + row;
      float x = 0.f;
      if (m < M) {
        const int r = m / EH_HW, p = m - r * EH_HW;
        x = A.trunk[((size_t)s_src[r] * EH_HW + p) * EH_K + k0 + k];
      }
      s_x[row][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EH_MC; q += 4) {
      const float a = s_dy[q + mk][16 * wave + ml] * sa;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_x[q + mk][ml], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_x[q + mk][16 + ml], acc1, 0, 0, 0);
    }
    if (bn_owner && tid < 64) {
      const int nr = min(EH_MC, M - m0);
      for (int row = 0; row < nr; ++row) {
        const float dy = s_dy[row][tid];
        dbeta += dy;
        dgamma = fmaf(dy, s_xh[row][tid], dgamma);
      }
    }
    __syncthreads();
  }
  // C: column lane & 15 (k), row 4 (lane >> 4) + i (channel)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + 16 * wave + 4 * mk + i;
    eh_adam_at(A, c * EH_K + k0 + ml, acc0[i]);
    eh_adam_at(A, c * EH_K + k0 + 16 + ml, acc1[i]);
  }
  if (bn_owner && tid < 64) {
    eh_adam_at(A, EH_OFF_G + c0 + tid, dgamma);
    eh_adam_at(A, EH_OFF_B + c0 + tid, dbeta);
  }
}

}  // namespace

size_t effhead_ws_bytes(int batch) {
  if (batch < 1 || batch > EH_EB) return 0;
  return sizeof(float) * ((size_t)batch * EH_HW * EH_C + 2 * (size_t)batch * EH_C + 2 * EH_C);
}

hipError_t launch_effhead_train_epoch(const float* trunk, const int32_t* labels, int R, const int32_t* perm, int N,
                                      const uint64_t* keep, float p_drop, int batch, const float* bn_mean,
                                      const float* bn_var, double bn_eps, double lr, double beta1, double beta2,
                                      double eps, double weight_decay, int step0, float* params, float* exp_avg,
                                      float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* grad_out,
                                      float* ws, hipStream_t s) {
  if (R < 1 || N < 1 || batch < 1 || batch > EH_EB || !(p_drop >= 0.f && p_drop < 1.f)) return hipErrorInvalidValue;
  const EhWs w = eh_ws(ws, batch);
  const float scale = keep ? (float)(1.0 / (1.0 - (double)p_drop)) : 1.0f;
  const int nsteps = (N + batch - 1) / batch;
  for (int st = 0; st < nsteps; ++st) {
    const int pos0 = st * batch, rows = std::min(batch, N - pos0);
    const AdamScalars ad = adam_scalars(lr, beta1, beta2, eps, weight_decay, step0 + st + 1);
    float* gout = st == nsteps - 1 ? grad_out : nullptr;
    hipLaunchKernelGGL(effhead_forward_kernel, dim3(EH_C / 64, rows), dim3(256), 0, s, trunk, R, perm, pos0, params,
                       bn_mean, bn_var, (float)bn_eps, w.z, w.pooled, w.s, w.t);
    EhClsArgs c{w.pooled, labels, R, perm, pos0, rows, keep, scale, ad, (float)weight_decay, weight_decay != 0.0,
                params, exp_avg, exp_avg_sq, w.dpooled, step_loss + st, step_correct + st, gout, nullptr};
    hipLaunchKernelGGL(effhead_cls_kernel<true>, dim3(1), dim3(256), 0, s, c);
    EhBwdArgs b{trunk, R, perm, pos0, rows, w.z, w.dpooled, w.s, w.t, bn_mean, bn_var, (float)bn_eps, ad,
                (float)weight_decay, weight_decay != 0.0, params, exp_avg, exp_avg_sq, gout};
    hipLaunchKernelGGL(effhead_backward_kernel, dim3(EH_K / 32, EH_C / 64), dim3(256), 0, s, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_effhead_eval(const float* trunk, const int32_t* labels, int R, int batch, const float* params,
                               const float* bn_mean, const float* bn_var, double bn_eps, float* batch_loss,
                               float* row_logits, float* ws, hipStream_t s) {
  if (R < 1 || batch < 1 || batch > EH_EB) return hipErrorInvalidValue;
  const EhWs w = eh_ws(ws, batch);
  int b = 0;
  for (int r0 = 0; r0 < R; r0 += batch, ++b) {
    const int rows = std::min(batch, R - r0);
    hipLaunchKernelGGL(effhead_forward_kernel, dim3(EH_C / 64, rows), dim3(256), 0, s, trunk, R,
                       (const int32_t*)nullptr, r0, params, bn_mean, bn_var, (float)bn_eps, (float*)nullptr, w.pooled,
                       (float*)nullptr, (float*)nullptr);
    EhClsArgs c{w.pooled, labels, R, nullptr, r0, rows, nullptr, 1.0f, AdamScalars{}, 0.f, 0,
                const_cast<float*>(params), nullptr, nullptr, nullptr, batch_loss + b, nullptr, nullptr, row_logits};
    hipLaunchKernelGGL(effhead_cls_kernel<false>, dim3(1), dim3(256), 0, s, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
