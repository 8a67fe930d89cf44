// torchvision's GaussianBlur on staged uint8 windows (mmf_gaussian_blur_u8): a KY x KX stencil on interleaved RGB
// with reflected borders, weights float32 [B][KY][KX] formed on the host.  One ordinary launch, grid (tiles, B), no
// atomics, no workspace.
//
// A row of an image is read as 3 * W bytes: tap j of output byte k is byte k + 3 * (j - KX / 2) of the row, so
// the channel needs no arithmetic.  A workgroup owns a tile of kTileRows rows x kTileBytes bytes and stages it,
// with KY / 2 rows above and below and 3 * (KX / 2) bytes left and right (rounded up to whole dwords), in LDS as
// bytes; rows and pixels outside the image are reflected while staging, so the sums carry no bounds logic.  A
// thread produces four neighbouring bytes of kRun rows: it walks the kRun + KY - 1 staged rows once, turns the
// bytes of each into floats once, and adds each row into every output row it is a tap of.
//
// The order of the additions is the specification (tests/blur_refs.np_blur): per output acc = 0, then for i (rows)
// outer and j (columns) inner acc = acc + w[i][j] * byte, the product rounded before the add; rintf, clamp, byte.
// Walking the staged rows downwards visits each output's i in increasing order and j runs inside it, so tiling and
// unrolling leave that order alone.  (5, 9) is compiled with constant tap counts and the weights in registers;
// every other size runs the same text with run-time bounds and the largest halo.
//
// Global loads and stores go in dwords where the address is dword-aligned (every row of an image whose first byte
// is aligned and whose W is a multiple of four) and in single bytes otherwise, and at a row's two ends.
#include <hip/hip_runtime.h>

#include "kernels.h"

#pragma clang fp contract(off)  // to the end of the file: every product rounded before its add

namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 64;                            // threads across a tile: one wavefront per row of four-byte runs
constexpr int kRun = 8;                               // output rows per thread
constexpr int kTileBytes = 4 * kLanes;                // 256
constexpr int kTileRows = kRun * (kThreads / kLanes); // 32
static_assert(kTileBytes == kBlurTileBytes && kTileRows == kBlurTileRows, "kernels.h states the tile");
typedef float float2v __attribute__((ext_vector_type(2)));

// Index p mirrored into 0 .. n - 1 without repeating the edge sample (torch's "reflect").  One reflection is all a
// needed sample takes (n > the halo); the clamp keeps every other index, which feeds no output, inside the row.
__device__ __forceinline__ int reflect(long long p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2ll * n - 2 - p;
  return p < 0 ? 0 : (p >= n ? n - 1 : (int)p);
}

// KX = KY = 0: run-time tap counts kx, ky (odd, <= kBlurMaxTaps) in the largest halo.
template <int KX, int KY>
__global__ __launch_bounds__(kThreads) void gaussian_blur_kernel(const uint8_t* __restrict__ src,
                                                                 uint8_t* __restrict__ dst, int H, int W, int kx_rt,
                                                                 int ky_rt, int col_tiles,
                                                                 const float* __restrict__ weights,
                                                                 const int32_t* __restrict__ apply) {
  constexpr bool kFixed = KX != 0;
  constexpr int HJ = kFixed ? KX / 2 : kBlurMaxTaps / 2;  // halo in pixels
  constexpr int HY = kFixed ? KY / 2 : kBlurMaxTaps / 2;  // halo in rows
  constexpr int HB = (3 * HJ + 3) & ~3;                   // halo in bytes, whole dwords
  constexpr int LW = (kTileBytes + 2 * HB) / 4;           // dwords per staged row
  constexpr int ROWS = kTileRows + 2 * HY;
  constexpr int ND = (HB + 3 + 3 * HJ) / 4 + 1;           // dwords of a staged row one thread reads
  static_assert(HB >= 3 * HJ && ND <= LW - (kLanes - 1), "a thread's reads stay inside its staged row");
  __shared__ uint32_t s_tile[ROWS * LW];

  const int kx = kFixed ? KX : kx_rt, ky = kFixed ? KY : ky_rt;
  const int hj = kx / 2, hy = ky / 2;
  const size_t b = blockIdx.y;
  const long long row_bytes = 3ll * W;
  const uint8_t* img = src + b * (size_t)H * (size_t)row_bytes;
  uint8_t* out = dst + b * (size_t)H * (size_t)row_bytes;
  const int y0 = (int)(blockIdx.x / (unsigned)col_tiles) * kTileRows;
  const long long bx0 = (long long)(blockIdx.x % (unsigned)col_tiles) * kTileBytes;
  const int tx = threadIdx.x & (kLanes - 1), ty = threadIdx.x / kLanes;
  const long long bx = bx0 + 4 * tx;  // the thread's first output byte in its rows
  const bool blurred = apply[b] != 0;  // the same in every thread of the block

  uint32_t packed[kRun];
  if (!blurred) {  // RandomApply did not fire: the thread's bytes as they are
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
      const int y = y0 + ty * kRun + o;
      packed[o] = 0;
      if (y >= H || bx >= row_bytes) continue;
      const uint8_t* p = img + (size_t)y * (size_t)row_bytes + bx;
      if (bx + 3 < row_bytes && ((uintptr_t)p & 3) == 0) {
        packed[o] = *reinterpret_cast<const uint32_t*>(p);
      } else {
        for (int e = 0; e < 4 && bx + e < row_bytes; ++e) packed[o] |= (uint32_t)p[e] << (8 * e);
      }
    }
  } else {
    // ---- stage the tile and its halo; staged row lr is image row y0 + lr - HY, staged byte lc is row byte
    // bx0 + lc - HB.  Rows and bytes past what an output of the image reads are left alone.
    for (int idx = threadIdx.x; idx < ROWS * LW; idx += kThreads) {
      const int lr = idx / LW, lw = idx - lr * LW;
      const long long gy = (long long)y0 + lr - HY, q0 = bx0 + 4 * lw - HB;
      if (gy >= (long long)H + hy || q0 >= row_bytes + 3 * hj) continue;
      const uint8_t* row = img + (size_t)reflect(gy, H) * (size_t)row_bytes;
      uint32_t v = 0;
      if (q0 >= 0 && q0 + 3 < row_bytes && ((uintptr_t)(row + q0) & 3) == 0) {
        v = *reinterpret_cast<const uint32_t*>(row + q0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned q = (unsigned)(q0 + e + 3 * (HB / 3 + 1));  // q0 >= -HB: non-negative, the pixel shifted
          const int pix = (int)(q / 3u) - (HB / 3 + 1), ch = (int)(q % 3u);
          v |= (uint32_t)row[3 * (size_t)reflect(pix, W) + ch] << (8 * e);
        }
      }
      s_tile[idx] = v;
    }
    __syncthreads();

    // ---- the sums
    const float* wts = weights + b * (size_t)(kx * ky);
    float wreg[kFixed ? KX * KY : 1];
    if constexpr (kFixed) {
#pragma unroll
      for (int t = 0; t < KX * KY; ++t) wreg[t] = wts[t];
    }
    float2v acc[kRun][2];  // the thread's four bytes as two pairs: packed multiplies and adds, each lane rounded alone
#pragma unroll
    for (int o = 0; o < kRun; ++o)
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[o][h] = float2v{0.0f, 0.0f};
    const uint32_t* mine = s_tile + (ty * kRun + (HY - hy)) * LW + tx;  // the first row the thread's first output reads
    const int rows = kRun + ky - 1;
    constexpr int kUnrollRows = kFixed ? kRun + KY - 1 : 1;  // constant taps: each (row, output row) pair its own code
#pragma clang loop unroll_count(kUnrollRows)
    for (int r = 0; r < rows; ++r) {
      float px[4 * ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const uint32_t v = mine[r * LW + d];
#pragma unroll
        for (int e = 0; e < 4; ++e) px[4 * d + e] = (float)((v >> (8 * e)) & 255u);
      }
#pragma unroll
      for (int o = 0; o < kRun; ++o) {
        const int i = r - o;  // this staged row is tap row i of output row o
        if (i < 0 || i >= ky) continue;
#pragma unroll
        for (int jj = -HJ; jj <= HJ; ++jj) {
          if (jj < -hj || jj > hj) continue;
          float w;
          if constexpr (kFixed) w = wreg[i * KX + jj + HJ];
          else w = wts[i * kx + jj + hj];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float2v prod = float2v{w, w} * float2v{px[HB + 2 * h + 3 * jj], px[HB + 2 * h + 3 * jj + 1]};
            acc[o][h] = acc[o][h] + prod;
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
      packed[o] = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = rintf(acc[o][c >> 1][c & 1]);  // half to even
        packed[o] |= (uint32_t)(v >= 0.0f ? (v <= 255.0f ? (int)v : 255) : 0) << (8 * c);  // a NaN becomes 0
      }
    }
  }

#pragma unroll
  for (int o = 0; o < kRun; ++o) {
    const int y = y0 + ty * kRun + o;
    if (y >= H || bx >= row_bytes) continue;
    uint8_t* p = out + (size_t)y * (size_t)row_bytes + bx;
    if (bx + 3 < row_bytes && ((uintptr_t)p & 3) == 0) {
      *reinterpret_cast<uint32_t*>(p) = packed[o];
    } else {
      for (int e = 0; e < 4 && bx + e < row_bytes; ++e) p[e] = (uint8_t)(packed[o] >> (8 * e));
    }
  }
}

}  // namespace

hipError_t launch_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int KX, int KY,
                                   const float* weights, const int32_t* apply, hipStream_t s) {
  if (B < 1 || B > kBlurMaxBatch || H < 1 || W < 1 || (size_t)H * (size_t)W > kBlurMaxPixels) return hipErrorInvalidValue;
  if (KX < 1 || KY < 1 || KX > kBlurMaxTaps || KY > kBlurMaxTaps || !(KX & 1) || !(KY & 1)) return hipErrorInvalidValue;
  if (W <= KX / 2 || H <= KY / 2) return hipErrorInvalidValue;
  const long long col_tiles = (3ll * W + kTileBytes - 1) / kTileBytes, row_tiles = ((long long)H + kTileRows - 1) / kTileRows;
  const dim3 grid((unsigned)(col_tiles * row_tiles), (unsigned)B);  // < 2^31 tiles for H * W <= kBlurMaxPixels
  if (KX == 5 && KY == 9)
    hipLaunchKernelGGL((gaussian_blur_kernel<5, 9>), grid, dim3(kThreads), 0, s, src, dst, H, W, KX, KY, (int)col_tiles,
                       weights, apply);
  else
    hipLaunchKernelGGL((gaussian_blur_kernel<0, 0>), grid, dim3(kThreads), 0, s, src, dst, H, W, KX, KY, (int)col_tiles,
                       weights, apply);
  return hipGetLastError();
}
