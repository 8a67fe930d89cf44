// Small fp32 kernels at the ends of the path: the RoBERTa dual heads (and a copy of the CLS rows they
// read), the FusionJudge MLP with verdict / explanation rule, cosine rows, mmf_analyze_mixed's finish
// and a strided fill (the Truth-Vault search is vault.hip).
// These are latency/L2-bound: they run in exact fp32 like the reference.
#include "common.h"
#include "kernels.h"

namespace {

// misinfo_forensics.py:57-69, 97-98, 342-347: two Linear(768,256)-ReLU-Linear(256,2) heads on the
// CLS row, softmax[:, 1].  Block = 4 rows x ONE head (blockIdx.y: 0 = ai, 1 = misinfo), so a block
// streams 0.75 MB of W1 instead of 1.5 MB (the per-block L2 stream is what bounds this kernel at
// the end of the RoBERTa tower); W1 stored transposed [768][256] so a k-step of the 256 hidden
// units reads one coalesced 1-KB row.  Per head the arithmetic order is unchanged.
__global__ __launch_bounds__(1024) void text_heads_kernel(const float* x, int row_stride, const float* w1a,
                                                         const float* b1a, const float* w2a, const float* b2a,
                                                         const float* w1m, const float* b1m, const float* w2m,
                                                         const float* b2m, float* ai_logits, float* mi_logits,
                                                         float* scores, int score_stride, int B, const int* ovf) {
  // 1024 threads: hidden unit h = tid % 256 of K-slice ks = tid / 256 (192 inputs each), so each
  // thread's dependent load/FMA chain is a quarter of the 768; slices combined in fixed order.
  constexpr int KS = 4, KL = 768 / KS;
  __shared__ float xs[4][768];
  __shared__ float hp[KS][4][256];  // [slice][row][hidden] partial sums
  __shared__ float red[4][4][2];    // [wave][row][o]
  const int tid = threadIdx.x, r0 = blockIdx.x * 4, h = tid & 255, ks = tid >> 8, head = blockIdx.y;
  const float* w1h = head ? w1m : w1a;
  const float* b1 = head ? b1m : b1a;
  const float* w2 = head ? w2m : w2a;
  const float* b2 = head ? b2m : b2a;
  float* logits = head ? mi_logits : ai_logits;
  for (int i = tid; i < 4 * 768; i += 1024) {
    const int r = i / 768, c = i % 768;
    xs[r][c] = (r0 + r < B) ? x[(size_t)(r0 + r) * row_stride + c] : 0.f;
  }
  __syncthreads();
  {
    const float* w1 = w1h + (size_t)ks * KL * 256 + h;
    float hsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int k = 0; k < KL; ++k) {
      const float w = w1[(size_t)k * 256];
#pragma unroll
      for (int r = 0; r < 4; ++r) hsum[r] = fmaf(w, xs[r][ks * KL + k], hsum[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) hp[ks][r][h] = hsum[r];
  }
  __syncthreads();
  if (tid < 256) {  // waves 0-3: hidden units -> ReLU -> the 2 output logits per row
    float part[4][2];
    const float w20 = w2[h], w21 = w2[256 + h], bb = b1[h];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float hs = hp[0][r][h];
#pragma unroll
      for (int q = 1; q < KS; ++q) hs += hp[q][r][h];
      const float hv = fmaxf(hs + bb, 0.f);
      part[r][0] = hv * w20;
      part[r][1] = hv * w21;
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const float v = wave_sum(part[r][o]);
        if (lane == 0) red[wave][r][o] = v;
      }
  }
  __syncthreads();
  if (tid < 4 && r0 + tid < B) {
    const int r = tid, row = r0 + r;
    float l[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) l[o] = red[0][r][o] + red[1][r][o] + red[2][r][o] + red[3][r][o];
    l[0] += b2[0]; l[1] += b2[1];
    if (ovf && ovf[row]) l[0] = l[1] = __builtin_nanf("");  // the sequence's fp16 stream overflowed (norm.hip)
    if (logits) { logits[row * 2] = l[0]; logits[row * 2 + 1] = l[1]; }
    if (scores) {  // softmax(l)[1] = exp(l1 - m) / (exp(l0 - m) + exp(l1 - m))
      const float m = fmaxf(l[0], l[1]);
      const float e0 = expf(l[0] - m), e1 = expf(l[1] - m);
      scores[(size_t)row * score_stride + head] = e1 / (e0 + e1);
    }
  }
}

// The rows text_heads_kernel reads, as they are (mmf_text_pooled): 192 threads per row, a float4 each.
__global__ __launch_bounds__(192) void text_cls_rows_kernel(const float* x, int row_stride, const int* ovf, float* out) {
  const int b = blockIdx.x, t = threadIdx.x;
  float4 v = *reinterpret_cast<const float4*>(x + (size_t)b * row_stride + t * 4);
  if (ovf && ovf[b]) v.x = v.y = v.z = v.w = __builtin_nanf("");  // the sequence's fp16 stream overflowed (norm.hip)
  *reinterpret_cast<float4*>(out + (size_t)b * 768 + t * 4) = v;
}

// misinfo_forensics.py:575-615 (fusion_verdict) + 742-765 (fallback explanation rule cascade).
// One wave per row (it sits at the very end of the step, after the towers join, so its latency is
// fully exposed: a thread per row walked ~2.4k dependent FMAs, ~17 us).  Lane o computes hidden
// unit o of Linear(5,64), lanes < 32 the units of Linear(64,32) from the wave's LDS row, lane 0
// the two logits; every dot product keeps the ascending-index fmaf order of the scalar form.
// The pieces below are shared by fusion_kernel and mixed_finish_kernel (mmf_analyze_mixed), and
// common.h's wave_rowdot by rowdot_kernel, mixed_finish_kernel and the vault kernels (vault.hip), so a
// row's bits do not depend on which of them computed it.
//
// The block's LDS image of the fusion layer (4 waves = 4 rows per block)
struct FusionLds {
  float sw0[64 * 5], sb0[64], sw3[32 * 65], sb3[32], sw5[64], sb5[2];
  float hs[4][64], h2[4][32];
};

// stage the weights (all 256 threads; the caller's __syncthreads() follows)
MMF_DEV void fusion_stage(FusionLds& L, const float* w0, const float* b0, const float* w3, const float* b3,
                          const float* w5, const float* b5, int tid) {
  for (int i = tid; i < 320; i += 256) L.sw0[i] = w0[i];
  for (int i = tid; i < 2048; i += 256) L.sw3[(i >> 6) * 65 + (i & 63)] = w3[i];  // padded rows: no bank conflicts
  if (tid < 64) { L.sb0[tid] = b0[tid]; L.sw5[tid] = w5[tid]; }
  if (tid < 32) L.sb3[tid] = b3[tid];
  if (tid < 2) L.sb5[tid] = b5[tid];
}

// the MLP of the wave's row x[5] from the staged weights -> softmax (p0, p1), valid on every lane.
// Called by all 256 threads of the block after the barrier that follows fusion_stage.
MMF_DEV void fusion_mlp(FusionLds& L, const float* x, int wave, int lane, float* p0, float* p1) {
  {
    float a = L.sb0[lane];
#pragma unroll
    for (int i = 0; i < 5; ++i) a = fmaf(L.sw0[lane * 5 + i], x[i], a);
    L.hs[wave][lane] = fmaxf(a, 0.f);
  }
  __syncthreads();
  if (lane < 32) {
    float a = L.sb3[lane];
#pragma unroll 16
    for (int i = 0; i < 64; ++i) a = fmaf(L.sw3[lane * 65 + i], L.hs[wave][i], a);
    L.h2[wave][lane] = fmaxf(a, 0.f);
  }
  __syncthreads();
  float l0 = L.sb5[0], l1 = L.sb5[1];
  for (int o = 0; o < 32; ++o) {
    l0 = fmaf(L.sw5[o], L.h2[wave][o], l0);
    l1 = fmaf(L.sw5[32 + o], L.h2[wave][o], l1);
  }
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  *p0 = e0 / (e0 + e1);
  *p1 = e1 / (e0 + e1);
}

// _generate_fallback_explanation's cascade (misinfo_forensics.py:742-765) over (ai, misinfo, deepfake,
// clip_similarity, vault_discrepancy)
MMF_DEV int explanation_rule(const float* x) {
  int rr = 5;
  if (x[4] > 0.7f) rr = 0;
  else if (x[2] > 0.7f) rr = 1;
  else if (x[0] > 0.7f) rr = 2;
  else if (x[1] > 0.7f) rr = 3;
  else if (x[3] < 0.3f) rr = 4;
  return rr;
}

// one row's (probs, verdict, confidence, rule) from the probabilities (p0 real, p1 fake) -- lane 0 only
MMF_DEV void write_verdict(int row, float p0, float p1, const float* x, float* probs, int32_t* verdict, float* conf,
                           int32_t* rule) {
  probs[(size_t)row * 2] = p0;
  probs[(size_t)row * 2 + 1] = p1;
  const int v = p1 > 0.5f ? 1 : 0;
  if (verdict) verdict[row] = v;
  if (conf) conf[row] = v ? p1 : p0;
  if (rule) rule[row] = explanation_rule(x);
}

__global__ __launch_bounds__(256) void fusion_kernel(const float* x5, const float* w0, const float* b0,
                                                     const float* w3, const float* b3, const float* w5,
                                                     const float* b5, float* probs, int32_t* verdict, float* conf,
                                                     int32_t* rule, int B) {
  __shared__ FusionLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < B;
  float x[5];  // (issued before the weight staging: one load latency for both)
#pragma unroll
  for (int i = 0; i < 5; ++i) x[i] = live ? x5[(size_t)row * 5 + i] : 0.f;
  fusion_stage(L, w0, b0, w3, b3, w5, b5, tid);
  __syncthreads();
  float p0, p1;
  fusion_mlp(L, x, wave, lane, &p0, &p1);
  if (!live || lane != 0) return;
  write_verdict(row, p0, p1, x, probs, verdict, conf, rule);
}

__global__ __launch_bounds__(256) void rowdot_kernel(const float* a, const float* c, float* out, int ostride, int B,
                                                     int C) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  const float s = wave_rowdot(a + (size_t)row * C, c + (size_t)row * C, C, lane);
  if (lane == 0) out[(size_t)row * ostride] = s;
}

// mmf_analyze_mixed's finish (kernels.h MixedFinishArgs): one wave per batch row, as fusion_kernel --
// it sits after the join, so its latency is exposed.  A row's list positions come from row_map; a
// position outside its list counts as absent, and a "both" position only counts with the text and
// image positions beside it, so every read below is inside its buffer whatever the map holds.
__global__ __launch_bounds__(256) void mixed_finish_kernel(MixedFinishArgs a) {
  __shared__ FusionLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < a.B;
  int ti = -1, ii = -1, ci = -1;
  if (live) {
    ti = a.row_map[(size_t)row * 3];
    ii = a.row_map[(size_t)row * 3 + 1];
    ci = a.row_map[(size_t)row * 3 + 2];
  }
  const bool has_t = ti >= 0 && ti < a.nT, has_i = ii >= 0 && ii < a.nI;
  const bool has_c = has_t && has_i && ci >= 0 && ci < a.nC;
  const bool vault = has_i && a.c_sims != nullptr;
  float x[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (has_t) { x[0] = a.text2[(size_t)ti * 2]; x[1] = a.text2[(size_t)ti * 2 + 1]; }
  if (has_i) x[2] = a.deepfake[ii];
  float top1 = 0.f;
  int top1_idx = -1;
  if (vault) {
    x[4] = a.c_disc[ii];
    top1 = a.c_sims[(size_t)ii * 5];
    top1_idx = a.c_idx[(size_t)ii * 5];
  }
  if (a.nC > 0) fusion_stage(L, a.w0, a.b0, a.w3, a.b3, a.w5, a.b5, tid);  // (kernel-uniform)
  // wave-uniform branches: the whole wave works on one row
  if (has_c) x[3] = wave_rowdot(a.v_emb + (size_t)ii * 512, a.t_emb + (size_t)ci * 512, 512, lane);
  float tsim = 0.f;
  // vault.hip's hit (vault_top1): top-1 above the threshold (a NaN or an empty slot is not)
  if (has_c && vault && a.title && top1 > a.thresh && top1_idx >= 0)
    tsim = wave_rowdot(a.t_emb + (size_t)ci * 512, a.title + (size_t)top1_idx * 512, 512, lane);
  if (live && lane < 5) {
    if (a.top_sims) a.top_sims[(size_t)row * 5 + lane] = vault ? a.c_sims[(size_t)ii * 5 + lane] : 0.f;
    if (a.top_idx) a.top_idx[(size_t)row * 5 + lane] = vault ? a.c_idx[(size_t)ii * 5 + lane] : -1;
  }
  float p0 = 0.f, p1 = 0.f;
  if (a.nC > 0) {
    __syncthreads();
    fusion_mlp(L, x, wave, lane, &p0, &p1);
  }
  if (!live || lane != 0) return;
#pragma unroll
  for (int i = 0; i < 5; ++i) a.scores5[(size_t)row * 5 + i] = x[i];
  if (a.text_sim) a.text_sim[row] = tsim;
  if (!has_c) {  // misinfo_forensics.py:883-899: text -> misinfo, else max(deepfake, vault_discrepancy)
    const float fake = fminf(fmaxf(has_t ? x[1] : fmaxf(x[2], x[4]), 0.f), 1.f);
    p0 = 1.f - fake;
    p1 = fake;
  }
  write_verdict(row, p0, p1, x, a.probs, a.verdict, a.conf, a.rule);
}

}  // namespace

hipError_t launch_text_heads(const float* x, int row_stride, const float* w1a, const float* b1a, const float* w2a,
                             const float* b2a, const float* w1m, const float* b1m, const float* w2m,
                             const float* b2m, float* ai_logits, float* mi_logits, float* scores, int score_stride,
                             int B, hipStream_t s, const int* ovf) {
  hipLaunchKernelGGL(text_heads_kernel, dim3((B + 3) / 4, 2), dim3(1024), 0, s, x, row_stride, w1a, b1a, w2a, b2a, w1m,
                     b1m, w2m, b2m, ai_logits, mi_logits, scores, score_stride, B, ovf);
  return hipGetLastError();
}

hipError_t launch_text_cls_rows(const float* x, int row_stride, const int* ovf, float* out, int B, hipStream_t s) {
  if (B < 1 || row_stride % 4 || (((uintptr_t)x | (uintptr_t)out) & 15)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_cls_rows_kernel, dim3(B), dim3(192), 0, s, x, row_stride, ovf, out);
  return hipGetLastError();
}

hipError_t launch_fusion(const float* x5, const float* w0, const float* b0, const float* w3, const float* b3,
                         const float* w5, const float* b5, float* probs, int32_t* verdict, float* conf,
                         int32_t* rule, int B, hipStream_t s) {
  hipLaunchKernelGGL(fusion_kernel, dim3((B + 3) / 4), dim3(256), 0, s, x5, w0, b0, w3, b3, w5, b5, probs,
                     verdict, conf, rule, B);
  return hipGetLastError();
}

hipError_t launch_rowdot(const float* a, const float* c, float* out, int ostride, int B, int C, hipStream_t s) {
  hipLaunchKernelGGL(rowdot_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a, c, out, ostride, B, C);
  return hipGetLastError();
}

hipError_t launch_mixed_finish(const MixedFinishArgs& a, hipStream_t s) {
  if (a.B <= 0 || !a.row_map || !a.scores5 || !a.probs) return hipErrorInvalidValue;
  // a list the batch uses needs its buffers (the kernel reads them for every position inside the list)
  if ((a.nT > 0 && !a.text2) || (a.nI > 0 && (!a.deepfake || !a.v_emb)) ||
      (a.nC > 0 && (!a.t_emb || !a.w0 || !a.b0 || !a.w3 || !a.b3 || !a.w5 || !a.b5)) ||
      (a.c_sims && (!a.c_idx || !a.c_disc)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(mixed_finish_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

namespace {
__global__ void fill_strided_kernel(float* p, int stride, int B, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) p[(size_t)i * stride] = v;
}
}  // namespace

hipError_t launch_fill_strided(float* p, int stride, int B, float v, hipStream_t s) {
  hipLaunchKernelGGL(fill_strided_kernel, dim3((B + 255) / 256), dim3(256), 0, s, p, stride, B, v);
  return hipGetLastError();
}
