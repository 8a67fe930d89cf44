// What the four device trainers (fusion_train.hip, clip_train.hip, head_train.hip, effnet_train.hip) share: the
// rules their bit-reproducibility rests on, stated once.  Included by those four files only.
#pragma once
#include <cmath>

#include "common.h"

#define MMF_HOST_DEV __host__ __device__ __forceinline__

// b^n by squaring, a function of (b, n) alone
MMF_HOST_DEV double ipow(double b, int n) {
  double r = 1.0;
  while (n > 0) {
    if (n & 1) r *= b;
    b *= b;
    n >>= 1;
  }
  return r;
}

// The fp32 scalars of one Adam / AdamW step (torch.optim's single-tensor form, bias correction by the global step):
// each computed in double from the hyperparameters and the step number alone and rounded ONCE, so a step's bits do
// not depend on which launch ran it, nor on whether the host or the device formed them.
struct AdamScalars {
  float decay, w1, b2, w2, eps, step_size, bc2s;
};
MMF_HOST_DEV AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, double wd, int step) {
  const double bc1 = 1.0 - ipow(beta1, step), bc2 = 1.0 - ipow(beta2, step);
  return {(float)(1.0 - lr * wd), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
          (float)(lr / bc1), (float)sqrt(bc2)};
}

// both moments and the step of one element; weight decay is the caller's: torch.optim.Adam's goes into g beforehand
// (effnet_train.hip: fmaf(wd, p, g) where wd != 0), AdamW's is adamw_update below
MMF_DEV void adam_update(const AdamScalars& A, float g, float& p, float& m, float& v) {
  m = m + A.w1 * (g - m);
  v = v * A.b2 + A.w2 * (g * g);
  p = p - A.step_size * (m / (sqrtf(v) / A.bc2s + A.eps));
}
// torch.optim.AdamW: the decoupled decay first
MMF_DEV void adamw_update(const AdamScalars& A, float g, float& p, float& m, float& v) {
  p = p * A.decay;
  adam_update(A, g, p, m, v);
}

// sum of 256 values, one per thread, by a fixed tree (s = 128, 64, ..., 1); the result on every thread
MMF_DEV float block_tree_sum(float v, float* red, int tid) {
  __syncthreads();  // earlier readers of red are done
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// one row of a two-class cross-entropy from its logits: the loss (m + logf(e0 + e1)) - logit[label], m the larger
// logit; whether the argmax is the label; softmax - onehot (the caller scales it by its 1 / rows)
struct CeRow {
  float loss;
  bool hit;
  float d0, d1;
};
MMF_DEV CeRow ce_row(float l0, float l1, int lab) {
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m), den = e0 + e1;
  CeRow o;
  o.loss = (m + logf(den)) - (lab ? l1 : l0);
  o.hit = (l1 > l0) == (lab != 0);  // a tie is class 0 (torch.max)
  o.d0 = e0 / den - (lab ? 0.f : 1.f);
  o.d1 = e1 / den - (lab ? 1.f : 0.f);
  return o;
}

// An epoch of N positions in minibatches of `batch` (the last one short), each walked RC rows at a time.
// A chunk: rows c0 .. c0 + RC - 1 of minibatch st.
struct Chunk {
  int st, c0;
};
template <int RC>
struct EpochWalk {
  int N, batch, nsteps;
  MMF_DEV int rows(int st) const { return min(batch, N - st * batch); }
  MMF_DEV Chunk next(Chunk c) const { return (c.c0 + RC < rows(c.st)) ? Chunk{c.st, c.c0 + RC} : Chunk{c.st + 1, 0}; }
  // position in the epoch order of row r of chunk c, -1 where there is none
  MMF_DEV int pos(Chunk c, int r) const {
    return (c.st < nsteps && c.c0 + r < rows(c.st)) ? c.st * batch + c.c0 + r : -1;
  }
};
