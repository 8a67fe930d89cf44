// One epoch of FusionJudge training in one launch (train_fusion_judge.py:213-233 per minibatch):
// Linear(5,64)-ReLU-Dropout-Linear(64,32)-ReLU-Linear(32,2), mean cross-entropy, backward and
// torch.optim.AdamW, for every minibatch of the epoch.  The steps depend on each other, so ONE
// workgroup of 256 threads walks them all; the 2,530 parameters stay in LDS (the image fusion_mlp
// reads, W3 rows padded to 65), and each parameter has an owner thread (parameter p: thread p % 256,
// slot p / 256) that keeps its value, both Adam moments and its gradient sum in registers for the
// whole launch.  Per step only the scores, labels, the permutation and the masks are read: thread r of
// wave 0 fetches row r of a chunk -- its permutation entry two chunks ahead, its scores, label and
// mask one chunk ahead -- so no step waits for a dependent pair of global loads.
//
// All arithmetic is fp32 (the reference's fp16 autocast + GradScaler is the identity unless something
// overflows: DESIGN.md); the step-dependent Adam scalars are computed in double from the step number
// alone, so a step's bits do not depend on which launch ran it.  Every reduction has a fixed order:
// dot products are ascending-index fmaf chains from the bias (fusion_mlp's convention), sums over
// the rows of a minibatch are ascending-row chains by ONE thread (the parameter's owner; thread 0
// for the loss).  A minibatch runs in chunks of 64 rows whose activations live in LDS; the owners'
// chains continue across chunks, so the chunking does not change the order.
#include "common.h"
#include "kernels.h"
#include "train_common.h"

namespace {

constexpr int FT_P = 2530;                   // parameters, state-dict order
constexpr int FT_SLOTS = (FT_P + 255) / 256;  // 10 owned parameters per thread
constexpr int FT_RC = 64;                    // rows of a minibatch resident at a time

// LDS image, in floats
constexpr int O_W0 = 0;                // [64][5]
constexpr int O_B0 = O_W0 + 320;       // [64]
constexpr int O_W3 = O_B0 + 64;        // [32][65]
constexpr int O_B3 = O_W3 + 32 * 65;   // [32]
constexpr int O_W5 = O_B3 + 32;        // [2][32]
constexpr int O_B5 = O_W5 + 64;        // [2]
constexpr int O_ONE = O_B5 + 2;        // 1.0f: the second factor of a bias's gradient sum
constexpr int O_X = O_ONE + 2;         // [RC][5]   gathered scores
constexpr int O_A1 = O_X + FT_RC * 5;  // [RC][64]  dropout(relu(z1))
constexpr int O_DZ1 = O_A1 + FT_RC * 64;  // [RC][64] dL/dz1
constexpr int O_H2 = O_DZ1 + FT_RC * 64;  // [RC][32] relu(z2)
constexpr int O_DZ2 = O_H2 + FT_RC * 32;  // [RC][32] dL/dz2
constexpr int O_DL = O_DZ2 + FT_RC * 32;  // [RC][2]  dL/dlogits
constexpr int O_LOSS = O_DL + FT_RC * 2;  // [RC]
constexpr int O_COR = O_LOSS + FT_RC;     // [RC]     1.0f where argmax == label
constexpr int O_LAB = O_COR + FT_RC;      // [RC]     the row's label (int bits)
constexpr int O_KEEP = O_LAB + FT_RC;     // [RC][2]  the row's keep mask (low, high word bits)
constexpr int FT_LDS = O_KEEP + FT_RC * 2;  // 15,620 floats = 62,480 bytes
static_assert(FT_LDS * 4 <= 64 * 1024, "fusion_train: LDS image past 64 KiB");

// where parameter p lives in the LDS image, and its gradient as sum_r S[a + r * sa] * S[b + r * sb]
struct FtSlot { int loc, a, sa, b, sb; };
MMF_DEV FtSlot ft_slot(int p) {
  if (p < 320) return {O_W0 + p, O_DZ1 + p / 5, 64, O_X + p % 5, 5};
  if (p < 384) return {O_B0 + (p - 320), O_DZ1 + (p - 320), 64, O_ONE, 0};
  if (p < 2432) { const int q = p - 384, k = q >> 6, i = q & 63; return {O_W3 + k * 65 + i, O_DZ2 + k, 32, O_A1 + i, 64}; }
  if (p < 2464) return {O_B3 + (p - 2432), O_DZ2 + (p - 2432), 32, O_ONE, 0};
  if (p < 2528) { const int q = p - 2464; return {O_W5 + q, O_DL + (q >> 5), 2, O_H2 + (q & 31), 32}; }
  if (p < FT_P) return {O_B5 + (p - 2528), O_DL + (p - 2528), 2, O_ONE, 0};
  return {O_ONE, O_ONE, 0, O_ONE, 0};  // no parameter: reads 1.0f, stores nothing
}

struct FtArgs {
  const float* scores5; const int32_t* labels; int N;
  const int32_t* perm; const uint64_t* keep; float scale; int batch;
  double lr, beta1, beta2, eps, wd; int step0;
  float *params, *exp_avg, *exp_avg_sq, *step_loss; int32_t* step_correct; float* grad_out;
};

// one row's inputs, fetched ahead of the chunk that uses them
struct FtRow { float x[5]; int lab; uint32_t klo, khi; };

// the (clamped) permutation entry at pos, -1 for pos -1
MMF_DEV int ft_src(const FtArgs& A, int pos) { return pos < 0 ? -1 : min(max(A.perm[pos], 0), A.N - 1); }
MMF_DEV void ft_fetch(const FtArgs& A, int src, int pos, FtRow& d) {
  if (src < 0) return;
#pragma unroll
  for (int i = 0; i < 5; ++i) d.x[i] = A.scores5[(size_t)src * 5 + i];
  d.lab = A.labels[src] != 0;
  const uint64_t kb = A.keep ? A.keep[pos] : ~0ull;
  d.klo = (uint32_t)kb;
  d.khi = (uint32_t)(kb >> 32);
}

__global__ __launch_bounds__(256) void fusion_train_epoch_kernel(FtArgs A) {
  __shared__ float S[FT_LDS];
  const int tid = threadIdx.x;
  FtSlot sl[FT_SLOTS];
  float pv[FT_SLOTS], mv[FT_SLOTS], vv[FT_SLOTS], g[FT_SLOTS];
#pragma unroll
  for (int s = 0; s < FT_SLOTS; ++s) {
    const int p = tid + 256 * s;
    sl[s] = ft_slot(p);
    const bool live = p < FT_P;
    pv[s] = live ? A.params[p] : 0.f;
    mv[s] = live ? A.exp_avg[p] : 0.f;
    vv[s] = live ? A.exp_avg_sq[p] : 0.f;
    g[s] = 0.f;
  }
  if (tid == 0) S[O_ONE] = 1.0f;
#pragma unroll
  for (int s = 0; s < FT_SLOTS; ++s)
    if (tid + 256 * s < FT_P) S[sl[s].loc] = pv[s];

  const int nsteps = (A.N + A.batch - 1) / A.batch;
  const EpochWalk<FT_RC> wk{A.N, A.batch, nsteps};
  // wave 0, thread r: row r of the current chunk in `row`, the next chunk's permutation entry in `src1`
  FtRow row = {};
  int src1 = -1, pos1 = -1;
  if (tid < FT_RC) {
    const Chunk first{0, 0};
    const int pos = wk.pos(first, tid);
    ft_fetch(A, ft_src(A, pos), pos, row);
    pos1 = wk.pos(wk.next(first), tid);
    src1 = ft_src(A, pos1);
  }
  for (int st = 0; st < nsteps; ++st) {
    const int pos0 = st * A.batch;
    const int rows = min(A.batch, A.N - pos0);
    const float inv_rows = 1.0f / (float)rows;
    float loss_sum = 0.f, cor_sum = 0.f;  // thread 0
#pragma unroll
    for (int s = 0; s < FT_SLOTS; ++s) g[s] = 0.f;

    for (int c0 = 0; c0 < rows; c0 += FT_RC) {
      const int nr = min(FT_RC, rows - c0);
      __syncthreads();  // the previous chunk's / step's readers of S are done; the new parameters are visible
      if (tid < FT_RC) {
        // this chunk's rows to LDS; then the next chunk's rows and the permutation entries of the one after it
        if (tid < nr) {
#pragma unroll
          for (int i = 0; i < 5; ++i) S[O_X + tid * 5 + i] = row.x[i];
          S[O_LAB + tid] = __int_as_float(row.lab);
          S[O_KEEP + tid * 2] = __uint_as_float(row.klo);
          S[O_KEEP + tid * 2 + 1] = __uint_as_float(row.khi);
        }
        const Chunk nxt = wk.next(Chunk{st, c0});
        ft_fetch(A, src1, pos1, row);
        pos1 = wk.pos(wk.next(nxt), tid);
        src1 = ft_src(A, pos1);
      }
      __syncthreads();
      // Linear(5,64) + ReLU + Dropout: item (row r, unit j)
      for (int idx = tid; idx < nr * 64; idx += 256) {
        const int r = idx >> 6, j = idx & 63;
        const uint32_t kw = __float_as_uint(S[O_KEEP + r * 2 + (j >> 5)]);
        float a = S[O_B0 + j];
#pragma unroll
        for (int i = 0; i < 5; ++i) a = fmaf(S[O_W0 + j * 5 + i], S[O_X + r * 5 + i], a);
        a = fmaxf(a, 0.f);
        S[O_A1 + idx] = ((kw >> (j & 31)) & 1) ? a * A.scale : 0.f;
      }
      __syncthreads();
      // Linear(64,32) + ReLU: item (row r, unit k)
      for (int idx = tid; idx < nr * 32; idx += 256) {
        const int r = idx >> 5, k = idx & 31;
        float a = S[O_B3 + k];
#pragma unroll 16
        for (int i = 0; i < 64; ++i) a = fmaf(S[O_W3 + k * 65 + i], S[O_A1 + r * 64 + i], a);
        S[O_H2 + idx] = fmaxf(a, 0.f);
      }
      __syncthreads();
      // Linear(32,2), cross-entropy of the row and dL/dlogits = (softmax - onehot) / rows: thread r
      if (tid < nr) {
        const int r = tid;
        const int lab = __float_as_int(S[O_LAB + r]);
        float l0 = S[O_B5], l1 = S[O_B5 + 1];
        for (int o = 0; o < 32; ++o) {
          l0 = fmaf(S[O_W5 + o], S[O_H2 + r * 32 + o], l0);
          l1 = fmaf(S[O_W5 + 32 + o], S[O_H2 + r * 32 + o], l1);
        }
        const CeRow o = ce_row(l0, l1, lab);
        S[O_LOSS + r] = o.loss;
        S[O_COR + r] = o.hit ? 1.f : 0.f;
        S[O_DL + r * 2] = o.d0 * inv_rows;
        S[O_DL + r * 2 + 1] = o.d1 * inv_rows;
      }
      __syncthreads();
      // dL/dz2 = (dlogits W5) * [h2 > 0]: item (row r, unit k)
      for (int idx = tid; idx < nr * 32; idx += 256) {
        const int r = idx >> 5, k = idx & 31;
        float d = S[O_DL + r * 2] * S[O_W5 + k];
        d = fmaf(S[O_DL + r * 2 + 1], S[O_W5 + 32 + k], d);
        S[O_DZ2 + idx] = S[O_H2 + idx] > 0.f ? d : 0.f;
      }
      __syncthreads();
      // dL/dz1 = (dz2 W3) * scale * [a1 > 0] (a1 > 0: the unit was kept and its ReLU passed): item (r, i)
      for (int idx = tid; idx < nr * 64; idx += 256) {
        const int r = idx >> 6, i = idx & 63;
        float d = 0.f;
#pragma unroll 16
        for (int k = 0; k < 32; ++k) d = fmaf(S[O_DZ2 + r * 32 + k], S[O_W3 + k * 65 + i], d);
        S[O_DZ1 + idx] = S[O_A1 + idx] > 0.f ? d * A.scale : 0.f;
      }
      __syncthreads();
      // the owners' gradient sums over the chunk's rows, ascending
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
#pragma unroll
        for (int s = 0; s < FT_SLOTS; ++s) g[s] = fmaf(S[sl[s].a + r * sl[s].sa], S[sl[s].b + r * sl[s].sb], g[s]);
      }
      if (tid == 0)
        for (int r = 0; r < nr; ++r) { loss_sum += S[O_LOSS + r]; cor_sum += S[O_COR + r]; }
    }

    // AdamW (torch.optim.AdamW, single-tensor form), bias correction by the global step
    const AdamScalars ad = adam_scalars(A.lr, A.beta1, A.beta2, A.eps, A.wd, A.step0 + st + 1);
    // (no barrier: since the last one every thread reads activations only, never the parameters)
#pragma unroll
    for (int s = 0; s < FT_SLOTS; ++s) {
      adamw_update(ad, g[s], pv[s], mv[s], vv[s]);
      if (tid + 256 * s < FT_P) S[sl[s].loc] = pv[s];
    }
    if (tid == 0) {
      A.step_loss[st] = loss_sum * inv_rows;
      A.step_correct[st] = (int32_t)cor_sum;
    }
  }
#pragma unroll
  for (int s = 0; s < FT_SLOTS; ++s) {
    const int p = tid + 256 * s;
    if (p < FT_P) {
      A.params[p] = pv[s];
      A.exp_avg[p] = mv[s];
      A.exp_avg_sq[p] = vv[s];
      if (A.grad_out) A.grad_out[p] = g[s];
    }
  }
}

}  // namespace

hipError_t launch_fusion_train_epoch(const float* scores5, const int32_t* labels, int N, const int32_t* perm,
                                     const uint64_t* keep, float p_drop, int batch, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, int step0, float* params,
                                     float* exp_avg, float* exp_avg_sq, float* step_loss, int32_t* step_correct,
                                     float* grad_out, hipStream_t s) {
  if (N < 1 || batch < 1 || batch > 256 || !(p_drop >= 0.f && p_drop < 1.f)) return hipErrorInvalidValue;
  FtArgs a{scores5, labels, N, perm, keep, keep ? 1.0f / (1.0f - p_drop) : 1.0f, batch, lr, beta1, beta2, eps,
           weight_decay, step0, params, exp_avg, exp_avg_sq, step_loss, step_correct, grad_out};
  hipLaunchKernelGGL(fusion_train_epoch_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}
