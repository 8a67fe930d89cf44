// torchvision's ColorJitter on staged uint8 windows, byte-exact with its PIL backend (mmf_color_jitter_u8; the
// arithmetic is jitter_math.h).  Two ordinary launches on one stream, grid (chunks, B), no atomics:
//   1. jitter_luma_sum_kernel, for images whose chain holds a contrast: the operations in front of the contrast
//      applied in registers, L formed, the chunk's integer sum of L to ws[b][chunk].
//   2. jitter_apply_kernel: the block adds up its image's partials (integers: any order gives the same sum), forms
//      the mean as ImageStat does, and applies the whole chain.
// A chunk is a range of pixels, a multiple of four long, so any H x W works.  A thread takes four pixels = twelve
// bytes as three dwords where the image's first byte is dword-aligned in src and in dst; otherwise, and for the
// last one to three pixels of an image, single bytes.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "jitter_math.h"  // last: it switches FMA contraction off for the rest of the file

namespace {
using jitter::Chain;
using jitter::Rgb;

constexpr int kThreads = 256;
constexpr int kGroup = 4;  // pixels per thread and step
struct __attribute__((aligned(4))) Dwords3 {
  uint32_t x, y, z;
};

// Four pixels (or the last n < 4 of the image) at pixel g of an image.
__device__ __forceinline__ void load_group(const uint8_t* img, size_t g, int n, bool dwords, Rgb (&px)[kGroup]) {
  uint8_t raw[3 * kGroup] = {};
  if (dwords && n == kGroup) {
    const Dwords3 v = *reinterpret_cast<const Dwords3*>(img + 3 * g);
    const uint32_t w[3] = {v.x, v.y, v.z};
#pragma unroll
    for (int j = 0; j < 3 * kGroup; ++j) raw[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
    for (int j = 0; j < 3 * n; ++j) raw[j] = img[3 * g + j];
  }
#pragma unroll
  for (int j = 0; j < kGroup; ++j) px[j] = Rgb{raw[3 * j], raw[3 * j + 1], raw[3 * j + 2]};
}

__device__ __forceinline__ void store_group(uint8_t* img, size_t g, int n, bool dwords, const Rgb (&px)[kGroup]) {
  uint8_t raw[3 * kGroup];
#pragma unroll
  for (int j = 0; j < kGroup; ++j) {
    raw[3 * j] = (uint8_t)px[j].r;
    raw[3 * j + 1] = (uint8_t)px[j].g;
    raw[3 * j + 2] = (uint8_t)px[j].b;
  }
  if (dwords && n == kGroup) {
    uint32_t w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      w[j] = (uint32_t)raw[4 * j] | ((uint32_t)raw[4 * j + 1] << 8) | ((uint32_t)raw[4 * j + 2] << 16) |
             ((uint32_t)raw[4 * j + 3] << 24);
    *reinterpret_cast<Dwords3*>(img + 3 * g) = Dwords3{w[0], w[1], w[2]};
  } else {
    for (int j = 0; j < 3 * n; ++j) img[3 * g + j] = raw[j];
  }
}

// Sum over the block, in every thread.
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (tid < half) s_red[tid] += s_red[tid + half];
    __syncthreads();
  }
  return s_red[0];
}

__device__ __forceinline__ Chain block_chain(const int32_t* ops, const float* factors, const int32_t* hue_shift) {
  const size_t b = blockIdx.y;
  return jitter::make_chain(ops + 4 * b, factors + 3 * b, hue_shift[b]);
}

// pixels P per image; chunk c owns pixels [c * per, min(P, (c + 1) * per)), per a multiple of kGroup.
__global__ __launch_bounds__(kThreads) void jitter_luma_sum_kernel(const uint8_t* __restrict__ src, size_t P, size_t per,
                                                                  const int32_t* __restrict__ ops,
                                                                  const float* __restrict__ factors,
                                                                  const int32_t* __restrict__ hue_shift,
                                                                  unsigned long long* __restrict__ ws) {
  __shared__ unsigned long long s_red[kThreads];
  const Chain c = block_chain(ops, factors, hue_shift);
  if (c.contrast_at == 4) return;  // the same in every thread: nobody reads this image's partials
  const uint8_t* img = src + (size_t)blockIdx.y * 3 * P;
  const bool dwords = ((uintptr_t)img & 3) == 0;
  const size_t p0 = (size_t)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
  unsigned long long sum = 0;
  for (size_t g = p0 + (size_t)threadIdx.x * kGroup; g < p1; g += (size_t)kThreads * kGroup) {
    const int n = p1 - g < (size_t)kGroup ? (int)(p1 - g) : kGroup;
    Rgb px[kGroup];
    load_group(img, g, n, dwords, px);
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
      if (j < n) sum += (unsigned)jitter::luma(jitter::apply(px[j], c, 0, c.contrast_at, 0));
  }
  sum = block_sum(sum, s_red);
  if (threadIdx.x == 0) ws[(size_t)blockIdx.y * kJitterChunks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void jitter_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               size_t P, size_t per, const int32_t* __restrict__ ops,
                                                               const float* __restrict__ factors,
                                                               const int32_t* __restrict__ hue_shift,
                                                               const unsigned long long* __restrict__ ws) {
  __shared__ unsigned long long s_red[kThreads];
  const Chain c = block_chain(ops, factors, hue_shift);
  int mean = 0;
  if (c.contrast_at != 4) {  // gridDim.x <= kJitterChunks = kThreads partials, one per thread
    const unsigned long long part =
        threadIdx.x < gridDim.x ? ws[(size_t)blockIdx.y * kJitterChunks + threadIdx.x] : 0ull;
    mean = jitter::contrast_mean(block_sum(part, s_red), P);
  }
  const uint8_t* img = src + (size_t)blockIdx.y * 3 * P;
  uint8_t* out = dst + (size_t)blockIdx.y * 3 * P;
  const bool dwords = (((uintptr_t)img | (uintptr_t)out) & 3) == 0;
  const size_t p0 = (size_t)blockIdx.x * per, p1 = p0 + per < P ? p0 + per : P;
  for (size_t g = p0 + (size_t)threadIdx.x * kGroup; g < p1; g += (size_t)kThreads * kGroup) {
    const int n = p1 - g < (size_t)kGroup ? (int)(p1 - g) : kGroup;
    Rgb px[kGroup];
    load_group(img, g, n, dwords, px);
#pragma unroll
    for (int j = 0; j < kGroup; ++j) px[j] = jitter::apply(px[j], c, 0, 4, mean);
    store_group(out, g, n, dwords, px);
  }
}

static_assert(kJitterChunks == kThreads, "jitter_apply_kernel reads one partial per thread");
}  // namespace

hipError_t launch_color_jitter_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ops,
                                  const float* factors, const int32_t* hue_shift, uint64_t* ws, hipStream_t s) {
  if (B < 1 || B > kJitterMaxBatch || H < 1 || W < 1) return hipErrorInvalidValue;
  const size_t P = (size_t)H * (size_t)W;
  if (P > kJitterMaxPixels) return hipErrorInvalidValue;
  const size_t step = (size_t)kThreads * kGroup;
  size_t chunks = (P + step - 1) / step;
  if (chunks > (size_t)kJitterChunks) chunks = kJitterChunks;  const size_t per = ((P + chunks - 1) / chunks + kGroup - 1) / kGroup * kGroup;
  const dim3 grid((unsigned)chunks, (unsigned)B);
  auto* partials = reinterpret_cast<unsigned long long*>(ws);
  hipLaunchKernelGGL(jitter_luma_sum_kernel, grid, dim3(kThreads), 0, s, src, P, per, ops, factors, hue_shift, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jitter_apply_kernel, grid, dim3(kThreads), 0, s, src, dst, P, per, ops, factors, hue_shift,
                     partials);
  return hipGetLastError();
}
