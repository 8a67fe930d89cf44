// The deployed EfficientNet deepfake classifier -- Dropout(0.2) then Linear(1280, 2) on the pooled row
// (misinfo_forensics.py:72-76) -- trained on cached pooled rows: one epoch in one launch
// (train_cifake_forensics.py:187-216 per minibatch, stated for the frozen backbone): xd = x * keep * scale,
// logits = xd W^T + b, mean cross-entropy, backward to both tensors and torch.optim.Adam (L2 weight decay added to
// the gradient, not decoupled), for every minibatch of the epoch.  The steps depend on each other, so ONE workgroup
// of 256 threads walks them all.  Thread t owns columns t, t + 256, ..., t + 1024 of both classes (threads 0 and 1
// also bias 0 and 1): 11 parameters, their Adam moments and their gradient sums stay in registers for the whole
// launch; only the two biases are mirrored in LDS, for the threads that finish a row's logits.
//
// A minibatch is walked in chunks of 16 rows.  Thread t reads its five values of each row straight from global
// memory (a wave's load is a contiguous 256-byte run per k), and the 32-bit mask words that hold their keep bits.  The
// rows of the NEXT chunk are fetched raw, and the permutation entries of the chunk after it, before the current
// chunk is reduced; the dropout mask is applied when a chunk's turn comes.  So no step waits for a dependent pair
// of global loads, and nothing waits for a load right after issuing it.
//
// All arithmetic is fp32; the step-dependent Adam scalars are computed in double from the step number alone and
// rounded once, so a step's bits do not depend on which launch ran it.  Every reduction has a fixed order:
//   * a thread's partial logit of (row, class) is the fmaf chain over its columns k = 0 .. 4 ascending, from 0;
//   * the 256 partials go through ONE tree: the xor butterfly of wave_sum inside each wave (offsets 32, 16, ..., 1),
//     then ((wave0 + wave1) + wave2) + wave3, and the bias is added last;
//   * a row's loss is (m + logf(e0 + e1)) - logit[label], m = max of the two logits;
//   * sums over the rows of a minibatch (gradients by the parameter's owner, loss and correct count by thread 0) are
//     ascending-row chains that continue across chunks, so the chunking does not change the order.
// The order depends on the minibatch's row count alone.  mmf_effcls_eval runs the same forward without dropout, one
// workgroup per batch.  Loop bounds come from N and batch only; no flags, spin-waits or atomics.
#include "common.h"
#include "kernels.h"
#include "train_common.h"

namespace {

constexpr int EC_K = 1280;         // the pooled row
constexpr int EC_P = 2 * EC_K + 2;  // classifier.1.weight [2][1280] | classifier.1.bias [2]
constexpr int EC_KT = EC_K / 256;  // 5 columns per thread
constexpr int EC_RC = 16;          // rows of a minibatch in registers at a time
constexpr int EC_SLOTS = 2 * EC_KT + 1;  // 10 weights + (threads 0, 1) a bias
constexpr int EC_EB = 64;          // the largest batch
static_assert(kEffClsParams == EC_P, "effnet_train: parameter count");

struct EcArgs {
  const float* feat; const int32_t* labels; int R;
  const int32_t* perm; int N; const uint64_t* keep; float scale; int batch;
  double lr, beta1, beta2, eps, wd; int step0;
  float *params, *exp_avg, *exp_avg_sq, *step_loss; int32_t* step_correct; float* grad_out;
};

using EcWalk = EpochWalk<EC_RC>;

// the raw permutation entry at pos (0 for pos -1), and the clamped bank row it names (-1 for pos -1): two steps, so
// that the entry can be loaded a chunk before anything reads it
MMF_DEV int ec_entry(const EcArgs& A, int pos) { return pos < 0 ? 0 : A.perm[pos]; }
MMF_DEV int ec_src(const EcArgs& A, int pos, int entry) { return pos < 0 ? -1 : min(max(entry, 0), A.R - 1); }

// index of slot q of thread tid in the flat parameter vector
MMF_DEV int ec_index(int q, int tid) {
  return q < 2 * EC_KT ? (q / EC_KT) * EC_K + tid + 256 * (q % EC_KT) : 2 * EC_K + tid;
}
MMF_DEV bool ec_live(int q, int tid) { return q < 2 * EC_KT || tid < 2; }

// thread tid's five columns of the rows of chunk c (bank rows src[]) and the 32-bit mask words that hold their keep
// bits, both RAW: nothing here reads a loaded value, so the loads stay in flight until ec_apply
MMF_DEV void ec_fetch(const EcArgs& A, EcWalk wk, Chunk c, const int (&src)[EC_RC], int tid,
                      float (&x)[EC_RC][EC_KT], uint32_t (&kw)[EC_RC][EC_KT]) {
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t* keep32 = reinterpret_cast<const uint32_t*>(A.keep);
#pragma unroll
  for (int r = 0; r < EC_RC; ++r) {
    if (src[r] >= 0) {
      const float* row = A.feat + (size_t)src[r] * EC_K + tid;
#pragma unroll
      for (int k = 0; k < EC_KT; ++k) x[r][k] = row[256 * k];
      if (A.keep) {
        // column tid + 256 k = 64-bit word wave + 4 k, bit lane = 32-bit word 2 (wave + 4 k) + lane / 32, bit lane % 32
        const uint32_t* w = keep32 + (size_t)wk.pos(c, r) * (EC_K / 32) + 2 * wave + (lane >> 5);
#pragma unroll
        for (int k = 0; k < EC_KT; ++k) kw[r][k] = w[8 * k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < EC_KT; ++k) x[r][k] = 0.f;
    }
  }
}
// dropout on arrival: xd = keep ? x * scale : 0 (keep == NULL: x as it is)
MMF_DEV void ec_apply(const EcArgs& A, int tid, const float (&x)[EC_RC][EC_KT], const uint32_t (&kw)[EC_RC][EC_KT],
                      float (&xd)[EC_RC][EC_KT]) {
  const int bit = tid & 31;
#pragma unroll
  for (int r = 0; r < EC_RC; ++r)
#pragma unroll
    for (int k = 0; k < EC_KT; ++k)
      xd[r][k] = !A.keep ? x[r][k] : (((kw[r][k] >> bit) & 1) ? x[r][k] * A.scale : 0.f);
}

__global__ __launch_bounds__(256) void effcls_train_epoch_kernel(EcArgs A) {
  __shared__ float s_red[4][EC_RC][2];  // per wave, the wave's sum of the partial logits of (row, class)
  __shared__ float s_dl[EC_RC][2], s_loss[EC_RC], s_cor[EC_RC], s_b[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float pv[EC_SLOTS], mv[EC_SLOTS], vv[EC_SLOTS], g[EC_SLOTS];
#pragma unroll
  for (int q = 0; q < EC_SLOTS; ++q) {
    const bool live = ec_live(q, tid);
    const int p = live ? ec_index(q, tid) : 0;
    pv[q] = live ? A.params[p] : 0.f;
    mv[q] = live ? A.exp_avg[p] : 0.f;
    vv[q] = live ? A.exp_avg_sq[p] : 0.f;
    g[q] = 0.f;
  }
  if (tid < 2) s_b[tid] = pv[2 * EC_KT];

  const int nsteps = (A.N + A.batch - 1) / A.batch;
  const EcWalk wk{A.N, A.batch, nsteps};
  // xn, kn: the next chunk's rows and mask words, raw; pe: the raw permutation entries of the chunk after it; thread
  // r < 16 also holds row r's raw label (labn) and its own entry of the chunk after (mype)
  float xn[EC_RC][EC_KT];
  uint32_t kn[EC_RC][EC_KT];
  int pe[EC_RC], src[EC_RC], labn = 0, mype = 0;
#pragma unroll
  for (int r = 0; r < EC_RC; ++r)
#pragma unroll
    for (int k = 0; k < EC_KT; ++k) kn[r][k] = 0u;
  {
    const Chunk first{0, 0}, second = wk.next(first);
#pragma unroll
    for (int r = 0; r < EC_RC; ++r) {
      const int pos = wk.pos(first, r);
      src[r] = ec_src(A, pos, ec_entry(A, pos));
    }
    ec_fetch(A, wk, first, src, tid, xn, kn);
    if (tid < EC_RC) {
      const int pos = wk.pos(first, tid), s0 = ec_src(A, pos, ec_entry(A, pos));
      if (s0 >= 0) labn = A.labels[s0];
      mype = ec_entry(A, wk.pos(second, tid));
    }
#pragma unroll
    for (int r = 0; r < EC_RC; ++r) pe[r] = ec_entry(A, wk.pos(second, r));
  }
  for (int st = 0; st < nsteps; ++st) {
    const int rows = min(A.batch, A.N - st * A.batch);
    const float inv_rows = 1.0f / (float)rows;
    float loss_sum = 0.f, cor_sum = 0.f;  // thread 0
    // the step's optimizer scalars: a function of the hyperparameters and the global step number alone
    const AdamScalars ad = adam_scalars(A.lr, A.beta1, A.beta2, A.eps, A.wd, A.step0 + st + 1);
    const float wdf = (float)A.wd;
    const bool decay = A.wd != 0.0;
#pragma unroll
    for (int q = 0; q < EC_SLOTS; ++q) g[q] = 0.f;

    for (int c0 = 0; c0 < rows; c0 += EC_RC) {
      const int nr = min(EC_RC, rows - c0);
      float xc[EC_RC][EC_KT];
      ec_apply(A, tid, xn, kn, xc);
      const int labc = labn & 1;
      // the next chunk's rows (its entries arrived a chunk ago), then the entries of the chunk after it: all raw
      const Chunk nxt = wk.next(Chunk{st, c0}), nn = wk.next(nxt);
#pragma unroll
      for (int r = 0; r < EC_RC; ++r) src[r] = ec_src(A, wk.pos(nxt, r), pe[r]);
      ec_fetch(A, wk, nxt, src, tid, xn, kn);
      if (tid < EC_RC) {
        const int s1 = ec_src(A, wk.pos(nxt, tid), mype);
        if (s1 >= 0) labn = A.labels[s1];
        mype = ec_entry(A, wk.pos(nn, tid));
      }
#pragma unroll
      for (int r = 0; r < EC_RC; ++r) pe[r] = ec_entry(A, wk.pos(nn, r));

      // partial logits: the thread's chain, then the wave's tree -- all 16 rows level by level (a missing row is
      // zeros), so the 32 butterflies overlap instead of queueing behind each other's cross-lane latency
      float pl[EC_RC][2];
#pragma unroll
      for (int r = 0; r < EC_RC; ++r) {
        float p0 = 0.f, p1 = 0.f;
#pragma unroll
        for (int k = 0; k < EC_KT; ++k) {
          p0 = fmaf(pv[k], xc[r][k], p0);
          p1 = fmaf(pv[EC_KT + k], xc[r][k], p1);
        }
        pl[r][0] = p0;
        pl[r][1] = p1;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {  // wave_sum's butterfly
#pragma unroll
        for (int r = 0; r < EC_RC; ++r) {
          pl[r][0] += __shfl_xor(pl[r][0], o, 64);
          pl[r][1] += __shfl_xor(pl[r][1], o, 64);
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < EC_RC; ++r)
          if (r < nr) { s_red[wave][r][0] = pl[r][0]; s_red[wave][r][1] = pl[r][1]; }
      }
      __syncthreads();  // the previous chunk's / step's readers of s_dl are done; the new biases are visible
      if (tid < nr) {
        const int r = tid;
        const float l0 = (((s_red[0][r][0] + s_red[1][r][0]) + s_red[2][r][0]) + s_red[3][r][0]) + s_b[0];
        const float l1 = (((s_red[0][r][1] + s_red[1][r][1]) + s_red[2][r][1]) + s_red[3][r][1]) + s_b[1];
        const CeRow o = ce_row(l0, l1, labc);
        s_loss[r] = o.loss;
        s_cor[r] = o.hit ? 1.f : 0.f;
        s_dl[r][0] = o.d0 * inv_rows;
        s_dl[r][1] = o.d1 * inv_rows;
      }
      __syncthreads();
      // the owners' gradient sums over the chunk's rows, ascending
#pragma unroll
      for (int r = 0; r < EC_RC; ++r) {
        if (r < nr) {
          const float d0 = s_dl[r][0], d1 = s_dl[r][1];
#pragma unroll
          for (int k = 0; k < EC_KT; ++k) {
            g[k] = fmaf(d0, xc[r][k], g[k]);
            g[EC_KT + k] = fmaf(d1, xc[r][k], g[EC_KT + k]);
          }
          g[2 * EC_KT] += (tid & 1) ? d1 : d0;
          if (tid == 0) { loss_sum += s_loss[r]; cor_sum += s_cor[r]; }
        }
      }
    }

    // torch.optim.Adam (single-tensor form): L2 decay into the gradient, bias correction by the global step
#pragma unroll
    for (int q = 0; q < EC_SLOTS; ++q) {
      adam_update(ad, decay ? fmaf(wdf, pv[q], g[q]) : g[q], pv[q], mv[q], vv[q]);
    }
    // (the readers of s_b of this step passed the chunk's second barrier; the next readers wait for the next first one)
    if (tid < 2) s_b[tid] = pv[2 * EC_KT];
    if (tid == 0) {
      A.step_loss[st] = loss_sum * inv_rows;
      A.step_correct[st] = (int32_t)cor_sum;
    }
  }
#pragma unroll
  for (int q = 0; q < EC_SLOTS; ++q) {
    if (ec_live(q, tid)) {
      const int p = ec_index(q, tid);
      A.params[p] = pv[q];
      A.exp_avg[p] = mv[q];
      A.exp_avg_sq[p] = vv[q];
      if (A.grad_out) A.grad_out[p] = g[q];  // the loss gradient (what p.grad holds), without the L2 term
    }
  }
}

// validate's forward: batch blockIdx.x = bank rows blockIdx.x * batch .., no dropout; the training kernel's chains and tree
__global__ __launch_bounds__(256) void effcls_eval_kernel(const float* __restrict__ feat, const int32_t* __restrict__ labels,
                                                          int R, int batch, const float* __restrict__ params,
                                                          float* __restrict__ batch_loss, float* __restrict__ row_logits) {
  __shared__ float s_red[4][EC_EB][2];
  __shared__ float s_loss[EC_EB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * batch, rows = min(batch, R - r0);
  float w[2 * EC_KT];
#pragma unroll
  for (int q = 0; q < 2 * EC_KT; ++q) w[q] = params[ec_index(q, tid)];
  for (int c0 = 0; c0 < rows; c0 += 8) {
    float x[8][EC_KT];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int k = 0; k < EC_KT; ++k)
        x[r][k] = c0 + r < rows ? feat[(size_t)(r0 + c0 + r) * EC_K + tid + 256 * k] : 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (c0 + r < rows) {
        float p0 = 0.f, p1 = 0.f;
#pragma unroll
        for (int k = 0; k < EC_KT; ++k) {
          p0 = fmaf(w[k], x[r][k], p0);
          p1 = fmaf(w[EC_KT + k], x[r][k], p1);
        }
        p0 = wave_sum(p0);
        p1 = wave_sum(p1);
        if (lane == 0) { s_red[wave][c0 + r][0] = p0; s_red[wave][c0 + r][1] = p1; }
      }
    }
  }
  __syncthreads();
  if (tid < rows) {
    const int r = tid;
    const float l0 = (((s_red[0][r][0] + s_red[1][r][0]) + s_red[2][r][0]) + s_red[3][r][0]) + params[2 * EC_K];
    const float l1 = (((s_red[0][r][1] + s_red[1][r][1]) + s_red[2][r][1]) + s_red[3][r][1]) + params[2 * EC_K + 1];
    row_logits[(size_t)(r0 + r) * 2] = l0;
    row_logits[(size_t)(r0 + r) * 2 + 1] = l1;
    s_loss[r] = ce_row(l0, l1, labels[r0 + r] & 1).loss;
  }
  __syncthreads();
  if (tid == 0) {
    float sum = 0.f;
    for (int r = 0; r < rows; ++r) sum += s_loss[r];
    batch_loss[blockIdx.x] = sum * (1.0f / (float)rows);
  }
}

// one thread per pixel: its C bytes from the mirrored column
__global__ __launch_bounds__(256) void hflip_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       size_t pixels, int W, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const size_t line = i / (size_t)W;
  const int x = (int)(i - line * (size_t)W);
  const uint8_t* s = src + (line * (size_t)W + (size_t)(W - 1 - x)) * (size_t)C;
  uint8_t* d = dst + i * (size_t)C;
  for (int c = 0; c < C; ++c) d[c] = s[c];
}

}  // namespace

hipError_t launch_effcls_train_epoch(const float* feat, const int32_t* labels, int R, const int32_t* perm, int N,
                                     const uint64_t* keep, float p_drop, int batch, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, int step0, float* params,
                                     float* exp_avg, float* exp_avg_sq, float* step_loss, int32_t* step_correct,
                                     float* grad_out, hipStream_t s) {
  if (R < 1 || N < 1 || batch < 1 || batch > EC_EB || !(p_drop >= 0.f && p_drop < 1.f)) return hipErrorInvalidValue;
  EcArgs a{feat, labels, R, perm, N, keep, keep ? (float)(1.0 / (1.0 - (double)p_drop)) : 1.0f, batch, lr, beta1, beta2,
           eps, weight_decay, step0, params, exp_avg, exp_avg_sq, step_loss, step_correct, grad_out};
  hipLaunchKernelGGL(effcls_train_epoch_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_effcls_eval(const float* feat, const int32_t* labels, int R, int batch, const float* params,
                              float* batch_loss, float* row_logits, hipStream_t s) {
  if (R < 1 || batch < 1 || batch > EC_EB) return hipErrorInvalidValue;
  hipLaunchKernelGGL(effcls_eval_kernel, dim3((unsigned)((R + batch - 1) / batch)), dim3(256), 0, s, feat, labels, R,
                     batch, params, batch_loss, row_logits);
  return hipGetLastError();
}

hipError_t launch_hflip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, hipStream_t s) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return hipErrorInvalidValue;
  const size_t pixels = (size_t)B * H * W, blocks = (pixels + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hflip_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, pixels, W, C);
  return hipGetLastError();
}
