// Pillow's uint8 colour arithmetic, per pixel (mmf_color_jitter_u8): ImageEnhance.Brightness / Contrast / Color
// (Image.blend against a degenerate image) and the HSV round trip of torchvision's adjust_hue.  Host and device:
// plain C++, so the same text can be held to Pillow on the CPU.  tests/jitter_refs.py restates it in numpy.
//
// Every result is exact only with each float / double operation rounded on its own: no a + b * c contracted into
// an FMA, divisions correctly rounded (the compiler's default).  Hence the pragma; it holds to the end of the
// translation unit, so include this file last.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMF_JIT_HD __host__ __device__ __forceinline__
#else
#define MMF_JIT_HD inline
#endif

#pragma clang fp contract(off)

namespace jitter {

enum : int { kBrightness = 0, kContrast = 1, kSaturation = 2, kHue = 3, kSkip = -1 };

struct Rgb {
  int r, g, b;
};

// One image's chain, already made safe: op[k] in -1..3, at most one contrast (at position contrast_at, else 4).
struct Chain {
  int op[4];
  float brightness, contrast, saturation;
  int shift;  // 0..255
  int contrast_at;
};

MMF_JIT_HD Chain make_chain(const int32_t* ops4, const float* factors3, int32_t hue_shift) {
  Chain c;
  c.contrast_at = 4;
  for (int k = 0; k < 4; ++k) {
    int op = ops4[k];
    if (op < kSkip || op > kHue) op = kSkip;
    if (op == kContrast) {
      if (c.contrast_at != 4) op = kSkip;  // a second contrast: skipped
      else c.contrast_at = k;
    }
    c.op[k] = op;
  }
  c.brightness = factors3[0];
  c.contrast = factors3[1];
  c.saturation = factors3[2];
  c.shift = hue_shift & 255;
  return c;
}

// convert("L")
MMF_JIT_HD int luma(const Rgb& p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }

// Image.blend(deg, img, a) for one byte: float32, the product rounded before the add.  0 <= a <= 1 keeps
// the sum inside 0..255 and truncates; any other factor (a NaN included) clips.
MMF_JIT_HD int blend(int deg, int v, float a) {
  const float prod = a * (float)(v - deg);
  const float t = (float)deg + prod;
  if (a >= 0.f && a <= 1.f) return (int)t & 255;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : ((int)t & 255));  // & 255: a NaN's conversion stays a byte
}

MMF_JIT_HD Rgb blend3(int deg, const Rgb& p, float a) { return Rgb{blend(deg, p.r, a), blend(deg, p.g, a), blend(deg, p.b, a)}; }

MMF_JIT_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV"), H += shift (uint8 wrap-around), convert("RGB").  Not the identity at shift 0.
MMF_JIT_HD Rgb hue(const Rgb& p, int shift) {
  const int mx = p.r > p.g ? (p.r > p.b ? p.r : p.b) : (p.g > p.b ? p.g : p.b);
  const int mn = p.r < p.g ? (p.r < p.b ? p.r : p.b) : (p.g < p.b ? p.g : p.b);
  if (mx == mn) return Rgb{mx, mx, mx};  // S = 0: (V, V, V) whatever H becomes
  // RGB -> HSV: float32 differences and quotients; the hue sum in float32 when R is the maximum and in double
  // otherwise, rounded to float32; h / 6 + 1, its fraction and the scale by 255 in double.
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const int S = clip8((int)((double)s * 255.0));
  const float rc = (float)(mx - p.r) / cr, gc = (float)(mx - p.g) / cr, bc = (float)(mx - p.b) / cr;
  float h;
  if (p.r == mx) h = bc - gc;
  else if (p.g == mx) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  const double y = (double)h / 6.0 + 1.0;  // in (0.8, 1.9): fmod(y, 1.0) is y - floor(y), exactly
  const float hf = (float)(y - floor(y));
  const int H = (clip8((int)((double)hf * 255.0)) + shift) & 255;
  if (S == 0) return Rgb{mx, mx, mx};
  // HSV -> RGB: double throughout, round-half-even.
  const double h6 = (double)H * 6.0 / 255.0;
  const double i = floor(h6);
  const double f = h6 - i;
  const double fs = (double)S / 255.0;
  const double v = (double)mx;
  const int pp = clip8((int)rint(v * (1.0 - fs)));
  const int q = clip8((int)rint(v * (1.0 - fs * f)));
  const int t = clip8((int)rint(v * (1.0 - fs * (1.0 - f))));
  switch ((int)i % 6) {
    case 0: return Rgb{mx, t, pp};
    case 1: return Rgb{q, mx, pp};
    case 2: return Rgb{pp, mx, t};
    case 3: return Rgb{pp, q, mx};
    case 4: return Rgb{t, pp, mx};
    default: return Rgb{mx, pp, q};
  }
}

// Operations k0 .. k1 - 1 of the chain on one pixel, each result a byte before the next; `mean` is the contrast's.
MMF_JIT_HD Rgb apply(Rgb p, const Chain& c, int k0, int k1, int mean) {
  for (int k = k0; k < k1; ++k) {
    switch (c.op[k]) {
      case kBrightness: p = blend3(0, p, c.brightness); break;
      case kContrast: p = blend3(mean, p, c.contrast); break;
      case kSaturation: {
        const int L = luma(p);
        p = blend3(L, p, c.saturation);
        break;
      }
      case kHue: p = hue(p, c.shift); break;
      default: break;
    }
  }
  return p;
}

// int(ImageStat.Stat(L).mean[0] + 0.5): sum < 2^53, so the double quotient is Python's int / int.
MMF_JIT_HD int contrast_mean(uint64_t sum, uint64_t pixels) { return (int)((double)sum / (double)pixels + 0.5); }

}  // namespace jitter
