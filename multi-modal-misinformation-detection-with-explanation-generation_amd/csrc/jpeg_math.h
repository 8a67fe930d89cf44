// The integer arithmetic of libjpeg's inverse half that the decoder (jpeg.hip) and the save-and-reload round trip
// (jpeg_encode.hip) share, bit-exact with Pillow's libjpeg-turbo (restated in oracle/jpeg_decode.py): jidctint.c's
// 1-D islow pass, jdmaster.c's post-IDCT range limit, jdsample.c's fancy (triangle) upsampling and jdcolor.c's
// YCbCr -> RGB.  Include after common.h.
#pragma once

namespace jpegm {

// jidctint.c / jfdctint.c constants (FIX(x) at CONST_BITS = 13)
constexpr int kF0298 = 2446, kF0390 = 3196, kF0541 = 4433, kF0765 = 6270, kF0899 = 7373, kF1175 = 9633,
              kF1501 = 12299, kF1847 = 15137, kF1961 = 16069, kF2053 = 16819, kF2562 = 20995, kF3072 = 25172;

MMF_DEV void idct_1d(const int* d, int* o, int shift) {
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * kF0541;
  const int tmp2 = z1 + z3 * (-kF1847);
  const int tmp3 = z1 + z2 * kF0765;
  const int tmp0 = (d[0] + d[4]) * 8192;  // << CONST_BITS (as a multiply: defined for negatives)
  const int tmp1 = (d[0] - d[4]) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * kF1175;
  t0 *= kF0298;
  t1 *= kF2053;
  t2 *= kF3072;
  t3 *= kF1501;
  z1 *= -kF0899;
  z2 *= -kF2562;
  z3 = z3 * (-kF1961) + z5;
  z4 = z4 * (-kF0390) + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const int r = 1 << (shift - 1);
  o[0] = (tmp10 + t3 + r) >> shift;
  o[7] = (tmp10 - t3 + r) >> shift;
  o[1] = (tmp11 + t2 + r) >> shift;
  o[6] = (tmp11 - t2 + r) >> shift;
  o[2] = (tmp12 + t1 + r) >> shift;
  o[5] = (tmp12 - t1 + r) >> shift;
  o[3] = (tmp13 + t0 + r) >> shift;
  o[4] = (tmp13 - t0 + r) >> shift;
}

// jdmaster.c post-IDCT range limit: idct_range_limit[v & 1023] (CENTERJSAMPLE folded in).  A clamp for
// -512 <= v <= 511 only (512 wraps to 0, where libjpeg-turbo's SIMD IDCT saturates): the decoder's host half
// declines files with a block outside that range (jpeg_host.cpp block_in_range), so none reaches its kernel; the
// round trip flags the image (jpeg_encode.hip).
MMF_DEV uint32_t range_limit_idct(int v) {
  const int m = v & 1023;
  return (uint32_t)(m < 128 ? m + 128 : m < 512 ? 255 : m < 896 ? 0 : m - 896);
}

// Eight pass-2 outputs -> eight samples, as the two dwords of a row store
MMF_DEV uint2 range_limit_row(const int* o) {
  const uint32_t lo = range_limit_idct(o[0]) | range_limit_idct(o[1]) << 8 | range_limit_idct(o[2]) << 16 |
                      range_limit_idct(o[3]) << 24;
  const uint32_t hi = range_limit_idct(o[4]) | range_limit_idct(o[5]) << 8 | range_limit_idct(o[6]) << 16 |
                      range_limit_idct(o[7]) << 24;
  return make_uint2(lo, hi);
}

MMF_DEV int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jdsample.c h2v1 fancy upsampling of row r (dw real samples) at output column x:
// (3 in[j] + in[j -/+ 1] + 1 / 2) >> 2, edges replicated
MMF_DEV int upsample_h2v1(const uint8_t* r, int x, int dw) {
  const int j = x >> 1, jn = (x & 1) ? min(j + 1, dw - 1) : max(j - 1, 0), bias = (x & 1) ? 2 : 1;
  return (3 * r[j] + r[jn] + bias) >> 2;
}

// jdsample.c h2v2 fancy upsampling of a plane (pitch pc, dw x dh real samples) at output pixel (x, y): column sums
// 3 in[i] + in[i -/+ 1], then (3 cs[j] + cs[j -/+ 1] + 8 / 7) >> 4; the context rows and columns replicated
MMF_DEV int upsample_h2v2(const uint8_t* s, int pc, int x, int y, int dw, int dh) {
  const int i = y >> 1, iv = (y & 1) ? min(i + 1, dh - 1) : max(i - 1, 0);
  const int j = x >> 1, jn = (x & 1) ? min(j + 1, dw - 1) : max(j - 1, 0), bias = (x & 1) ? 7 : 8;
  const uint8_t *a = s + (size_t)i * pc, *b = s + (size_t)iv * pc;
  return (3 * (3 * a[j] + b[j]) + (3 * a[jn] + b[jn]) + bias) >> 4;
}

// jdcolor.c build_ycc_rgb_table / ycc_rgb_convert (FIX(x) = x * 65536 + 0.5): R | G << 8 | B << 16
MMF_DEV uint32_t ycc_to_rgb(int Y, int cb, int cr) {
  const int cbx = cb - 128, crx = cr - 128;
  const int R = clamp255(Y + ((91881 * crx + 32768) >> 16));
  const int G = clamp255(Y + ((-22554 * cbx + 32768 - 46802 * crx) >> 16));
  const int B = clamp255(Y + ((116130 * cbx + 32768) >> 16));
  return (uint32_t)R | (uint32_t)G << 8 | (uint32_t)B << 16;
}

}  // namespace jpegm
