// A JPEG save-and-reload round trip on staged uint8 windows (mmf_jpeg_roundtrip_u8), byte-exact with Pillow's
// Image.save(format="JPEG", quality=q) followed by a load (the reference's RandomJPEGCompression,
// misinformation_dataset.py:18-57).  Huffman coding is lossless, so no bit stream is formed: the forward half of
// libjpeg (jccolor.c RGB -> YCbCr, 4:2:0 with jcsample.c's h2v2_downsample, the edges replicated as jcprepct.c and
// jcsample.c replicate them -- columns in the input, rows below the image in each downsampled component --,
// jfdctint.c's islow forward DCT,
// jcdctmgr.c's quantisation by jpeg_set_quality's tables) runs straight into the inverse half the decoder has
// (jpeg_math.h).  Restated in tests/jpeg_encode_refs.py.  Two ordinary launches on one stream, no atomics:
//   jpeg_enc_blocks_kernel: one 8x8 block of one component per thread (a Y block reads 8x8 pixels, a chroma block
//                           16x16): convert, downsample, forward DCT, quantise, dequantise, IDCT, all in registers
//                           (the quantised coefficients never reach memory), 8 rows of 8 range-limited samples out.
//                           Adjacent threads = adjacent blocks of a block row: row reads and stores coalesce.  A
//                           block that leaves the decoder's exact range sets flags[image] = 1 (a plain store).
//   jpeg_enc_color_kernel : one output pixel per thread: fancy h2v2 upsampling, YCbCr -> RGB, three bytes out;
//                           an image of quality 0 is copied.
// Sample planes per image in ws: Y [bh0 * 8][bw0 * 8], then Cb and Cr [bhc * 8][bwc * 8].
#include "common.h"
#include "kernels.h"
#include "jpeg_math.h"

namespace {
using namespace jpegm;

constexpr int kThreads = 256;
// ITU T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
constexpr uint8_t kStdLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jpeg_set_quality(q, TRUE) for every q: s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((std * s + 50) / 100, 1, 255)
struct QTables {
  uint8_t t[101][2][64];  // [quality][luma, chroma][natural index]; row 0 is not a quality
};
constexpr QTables make_qtables() {
  QTables r{};
  for (int q = 0; q <= 100; ++q) {
    const int s = q == 0 ? 100 : q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; ++k) {
      const int y = (kStdLuma[k] * s + 50) / 100, c = (kStdChroma[k] * s + 50) / 100;
      r.t[q][0][k] = (uint8_t)(y < 1 ? 1 : y > 255 ? 255 : y);
      r.t[q][1][k] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
  }
  return r;
}
__constant__ constexpr QTables kQ = make_qtables();

// jccolor.c: FIX(x) = (int)(x * 65536 + 0.5)
constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }
constexpr int kYR = fix16(0.29900), kYG = fix16(0.58700), kYB = fix16(0.11400);
constexpr int kCbR = -fix16(0.16874), kCbG = -fix16(0.33126), kCbB = fix16(0.50000);
constexpr int kCrR = fix16(0.50000), kCrG = -fix16(0.41869), kCrB = -fix16(0.08131);
constexpr int kChromaOff = (128 << 16) + 32767;  // CBCR_OFFSET + ONE_HALF - 1

// One pass of jfdctint.c over d[0..7].  Products and sums are formed modulo 2^32: for level-shifted samples up to
// +-1024 (launch_jpeg_block_roundtrip's bound; pixels give +-128) every output fits an int, an intermediate sum of
// pass 2 need not.
template <bool kFirst>
MMF_DEV void fdct_1d(const int* d, int* o) {
  using U = uint32_t;
  constexpr int n = kFirst ? 11 : 15;
  auto descale = [](U v, int s) { return (int)(v + (1u << (s - 1))) >> s; };
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kFirst) {
    o[0] = (t10 + t11) * 4;  // << PASS1_BITS
    o[4] = (t10 - t11) * 4;
  } else {
    o[0] = (t10 + t11 + 2) >> 2;
    o[4] = (t10 - t11 + 2) >> 2;
  }
  U z1 = (U)(t12 + t13) * (U)kF0541;
  o[2] = descale(z1 + (U)t13 * (U)kF0765, n);
  o[6] = descale(z1 - (U)t12 * (U)kF1847, n);
  z1 = (U)(t4 + t7);
  U z2 = (U)(t5 + t6), z3 = (U)(t4 + t6), z4 = (U)(t5 + t7);
  const U z5 = (z3 + z4) * (U)kF1175;
  const U m4 = (U)t4 * (U)kF0298, m5 = (U)t5 * (U)kF2053, m6 = (U)t6 * (U)kF3072, m7 = (U)t7 * (U)kF1501;
  z1 *= (U)-kF0899;
  z2 *= (U)-kF2562;
  z3 = z3 * (U)-kF1961 + z5;
  z4 = z4 * (U)-kF0390 + z5;
  o[7] = descale(m4 + z1 + z3, n);
  o[5] = descale(m5 + z2 + z4, n);
  o[3] = descale(m6 + z2 + z3, n);
  o[1] = descale(m7 + z1 + z4, n);
}

// d: a block's level-shifted samples in, its IDCT pass-2 outputs (before the range limit) out.  qt: the 64 table
// bytes as 16 dwords.  kCoef: also the quantised coefficients to coef[64].  Returns whether the block stayed in
// the decoder's exact range (oracle.jpeg_decode.in_exact_range's three conditions); where it did not, what
// follows the failed condition runs on zeros, so that no product can overflow, and d means nothing.
template <bool kCoef>
MMF_DEV bool block_roundtrip(int (&d)[64], const uint32_t (&qt)[16], int16_t* coef) {
  // forward pass 1: rows
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    fdct_1d<true>(d + r * 8, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) d[r * 8 + k] = o[k];
  }
  // forward pass 2: columns
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int in[8], o[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) in[v] = d[v * 8 + u];
    fdct_1d<false>(in, o);
#pragma unroll
    for (int v = 0; v < 8; ++v) d[v * 8 + u] = o[v];
  }
  // jcdctmgr.c quantisation (divisor 8 t: the forward DCT's outputs are 8 times the DCT), then dequantisation
  bool ok1 = true;
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int t = (int)((qt[k >> 2] >> (8 * (k & 3))) & 255u);
    const uint32_t qv = (uint32_t)t << 3;
    const int c = d[k];
    const int n = (int)(((uint32_t)(c < 0 ? -c : c) + (qv >> 1)) / qv);
    const int qc = c < 0 ? -n : n;
    if (kCoef) coef[k] = (int16_t)qc;
    const int dq = qc * t;
    ok1 = ok1 && dq >= -32767 && dq <= 32767;  // condition 1: the dequantised value fits a 16-bit lane
    d[k] = dq;
  }
  // inverse pass 1: columns (d[v * 8 + u], inputs down a column) -> workspace
  int ws[64];
  bool ok2 = true;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int in[8], o[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) in[v] = ok1 ? d[v * 8 + u] : 0;
    idct_1d(in, o, 11);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      ok2 = ok2 && o[v] >= -32767 && o[v] <= 32767;  // condition 2: so does the workspace
      ws[v * 8 + u] = o[v];
    }
  }
  // inverse pass 2: rows
  bool ok3 = true;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int in[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ok2 ? ws[r * 8 + k] : 0;
    idct_1d(in, o, 18);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ok3 = ok3 && o[k] >= -512 && o[k] <= 511;  // condition 3: the range limit is a clamp
      d[r * 8 + k] = o[k];
    }
  }
  return ok1 && ok2 && ok3;
}

// N pixels of row y from column x0 on, as the 3 N / 4 dwords they fill in memory; columns past the image replicate
// the last.  Whole dword loads where the run lies inside the row and starts dword-aligned, single bytes otherwise.
// y < H, x0 < W.
template <int N>
MMF_DEV void load_row(const uint8_t* __restrict__ img, int W, int y, int x0, uint32_t (&w)[3 * N / 4]) {
  static_assert((3 * N) % 4 == 0, "whole dwords");
  const uint8_t* row = img + (size_t)y * W * 3;
  const uint8_t* p = row + (size_t)x0 * 3;
  if (x0 + N <= W && ((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 3 * N / 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < 3 * N / 4; ++k) w[k] = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const uint8_t* q = row + (size_t)min(x0 + j, W - 1) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) w[(3 * j + ch) >> 2] |= (uint32_t)q[ch] << (8 * ((3 * j + ch) & 3));
    }
  }
}

// byte i of a run of dwords
template <int K>
MMF_DEV int byte_at(const uint32_t (&w)[K], int i) {
  return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
}

struct EncGeom {
  int H, W;
  int bw0, bh0, bwc, bhc;  // block grids: luma, chroma
  int cw, ch;              // chroma samples that reach a pixel: ceil(W / 2), ceil(H / 2)
  int n0, nc;              // blocks per component
  int s1, s2, total;       // the thread index where Cb's and Cr's blocks start; all threads per image
  size_t image_bytes;      // ws per image: 64 (n0 + 2 nc)
};

MMF_DEV bool quality_ok(int q) { return q >= 1 && q <= 100; }

// grid (ceil(g.total / 256), B); block 256
__global__ __launch_bounds__(kThreads) void jpeg_enc_blocks_kernel(const uint8_t* __restrict__ src, const EncGeom g,
                                                                  const int32_t* __restrict__ quality,
                                                                  uint8_t* __restrict__ ws,
                                                                  int32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int q = quality[b];
  if (!quality_ok(q)) return;  // a copy: the colour kernel reads no samples of this image
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int c = t >= g.s2 ? 2 : t >= g.s1 ? 1 : 0;
  const int rem = t - (c == 2 ? g.s2 : c == 1 ? g.s1 : 0);
  if (rem >= (c ? g.nc : g.n0)) return;
  const int bw = c ? g.bwc : g.bw0;
  const int by = rem / bw, bx = rem - by * bw;
  const uint8_t* img = src + (size_t)b * g.H * g.W * 3;
  int d[64];
  if (c == 0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint32_t px[6];
      load_row<8>(img, g.W, min(by * 8 + r, g.H - 1), bx * 8, px);  // bx * 8 < W: bw0 = ceil(W / 8)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        d[r * 8 + j] =
            ((kYR * byte_at(px, 3 * j) + kYG * byte_at(px, 3 * j + 1) + kYB * byte_at(px, 3 * j + 2) + 32768) >> 16) -
            128;
    }
  } else {
    const int kr = c == 1 ? kCbR : kCrR, kg = c == 1 ? kCbG : kCrG, kb = c == 1 ? kCbB : kCrB;
    // bx * 16 < W and by * 16 < H: the block holds chroma sample (bx * 8, by * 8), which reaches a pixel
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      // jcprepct.c: the input gets the one row that makes its height even; below the image's last chroma row the
      // grid repeats that DOWNSAMPLED row (not what downsampling a repeated last input row would give for an even H)
      const int cy = min(by * 8 + r, g.ch - 1);
      int sum[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        uint32_t px[12];
        load_row<16>(img, g.W, min(2 * cy + half, g.H - 1), bx * 16, px);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int a =
              (kr * byte_at(px, 6 * j) + kg * byte_at(px, 6 * j + 1) + kb * byte_at(px, 6 * j + 2) + kChromaOff) >> 16;
          const int e =
              (kr * byte_at(px, 6 * j + 3) + kg * byte_at(px, 6 * j + 4) + kb * byte_at(px, 6 * j + 5) + kChromaOff) >>
              16;
          sum[j] = half ? sum[j] + a + e : a + e;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) d[r * 8 + j] = ((sum[j] + 1 + (j & 1)) >> 2) - 128;  // bias 1, 2, 1, 2, ...
    }
  }
  uint32_t qt[16];
  const uint4* qrow = reinterpret_cast<const uint4*>(kQ.t[q][c ? 1 : 0]);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint4 v = qrow[i];
    qt[4 * i] = v.x;
    qt[4 * i + 1] = v.y;
    qt[4 * i + 2] = v.z;
    qt[4 * i + 3] = v.w;
  }
  const bool ok = block_roundtrip<false>(d, qt, nullptr);
  uint8_t* plane = ws + (size_t)b * g.image_bytes + (size_t)(c == 0 ? 0 : g.n0 + (c - 1) * g.nc) * 64;
  const int pitch = bw * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r)
    *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + r) * pitch + bx * 8) = range_limit_row(d + r * 8);
  if (!ok) flags[b] = 1;  // every thread that stores here stores the same value
}

// grid (ceil(H W / 256), B); block 256
__global__ __launch_bounds__(kThreads) void jpeg_enc_color_kernel(const uint8_t* __restrict__ src,
                                                                 uint8_t* __restrict__ dst, const EncGeom g,
                                                                 const int32_t* __restrict__ quality,
                                                                 const uint8_t* __restrict__ ws) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= g.H * g.W) return;
  const size_t at = ((size_t)b * g.H * g.W + p) * 3;
  if (!quality_ok(quality[b])) {
    dst[at] = src[at];
    dst[at + 1] = src[at + 1];
    dst[at + 2] = src[at + 2];
    return;
  }
  const int y = p / g.W, x = p - y * g.W;
  const uint8_t* s0 = ws + (size_t)b * g.image_bytes;
  const uint8_t* s1 = s0 + (size_t)g.n0 * 64;
  const uint8_t* s2 = s1 + (size_t)g.nc * 64;
  const int Y = s0[(size_t)y * (g.bw0 * 8) + x];
  const int cb = upsample_h2v2(s1, g.bwc * 8, x, y, g.cw, g.ch);
  const int cr = upsample_h2v2(s2, g.bwc * 8, x, y, g.cw, g.ch);
  const uint32_t rgb = ycc_to_rgb(Y, cb, cr);
  dst[at] = (uint8_t)rgb;
  dst[at + 1] = (uint8_t)(rgb >> 8);
  dst[at + 2] = (uint8_t)(rgb >> 16);
}

// n blocks, one per thread: the device functions above on raw sample blocks (launch_jpeg_block_roundtrip)
__global__ __launch_bounds__(kThreads) void jpeg_block_roundtrip_kernel(const int16_t* __restrict__ blocks,
                                                                       const uint8_t* __restrict__ table, int n,
                                                                       int16_t* __restrict__ coefs,
                                                                       uint8_t* __restrict__ samples,
                                                                       int32_t* __restrict__ outside) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int d[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) d[k] = blocks[(size_t)i * 64 + k];
  uint32_t qt[16];
#pragma unroll
  for (int k = 0; k < 16; ++k)
    qt[k] = (uint32_t)table[4 * k] | (uint32_t)table[4 * k + 1] << 8 | (uint32_t)table[4 * k + 2] << 16 |
            (uint32_t)table[4 * k + 3] << 24;
  int16_t cf[64];
  const bool ok = block_roundtrip<true>(d, qt, cf);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    coefs[(size_t)i * 64 + k] = cf[k];
    samples[(size_t)i * 64 + k] = (uint8_t)range_limit_idct(d[k]);
  }
  outside[i] = ok ? 0 : 1;
}

bool make_geom(int H, int W, EncGeom* g) {
  if (H < 1 || W < 1 || (double)H * W > (double)kJpegEncMaxPixels) return false;
  g->H = H;
  g->W = W;
  g->cw = (W + 1) / 2;
  g->ch = (H + 1) / 2;
  g->bw0 = (W + 7) / 8;
  g->bh0 = (H + 7) / 8;
  g->bwc = (g->cw + 7) / 8;
  g->bhc = (g->ch + 7) / 8;
  g->n0 = g->bw0 * g->bh0;  // <= (H + 7) (W + 7) / 64: an int with room to spare (H W <= 2^30)
  g->nc = g->bwc * g->bhc;
  g->s1 = g->n0;  // the components' blocks packed in the thread index (measured against wavefront-aligned starts)
  g->s2 = g->n0 + g->nc;
  g->total = g->n0 + 2 * g->nc;
  g->image_bytes = (size_t)64 * ((size_t)g->n0 + 2 * (size_t)g->nc);
  return true;
}

}  // namespace

size_t jpeg_roundtrip_ws_bytes(int H, int W) {
  EncGeom g;
  return make_geom(H, W, &g) ? g.image_bytes : 0;
}

hipError_t launch_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* quality,
                                    uint8_t* ws, int32_t* flags, hipStream_t s) {
  EncGeom g;
  if (B < 1 || B > kJpegEncMaxBatch || !make_geom(H, W, &g)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)B * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jpeg_enc_blocks_kernel, dim3((g.total + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, src, g,
                     quality, ws, flags);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jpeg_enc_color_kernel, dim3((H * W + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, src, dst,
                     g, quality, ws);
  return hipGetLastError();
}

hipError_t launch_jpeg_block_roundtrip(const int16_t* blocks, const uint8_t* table, int n, int16_t* coefs,
                                       uint8_t* samples, int32_t* outside, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_block_roundtrip_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, blocks,
                     table, n, coefs, samples, outside);
  return hipGetLastError();
}
