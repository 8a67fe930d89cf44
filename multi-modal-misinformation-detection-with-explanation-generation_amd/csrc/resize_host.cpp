// mmf_resize_pil's host side: the per-image resize jobs of Pillow's two-pass resampling, planned here
// and run by resize.hip.
#include <cmath>

#include "handle.h"

namespace {
// Pillow's support / taps / bounds on the host (the same double arithmetic as Resample.c) for the
// window bookkeeping; the coefficients themselves are computed on the device (resize.hip)
struct AxisPlan { double scale, support; int ks; };
AxisPlan axis_plan(int in_size, int out_size, int filt) {
  AxisPlan a;
  a.scale = (double)(float)in_size / out_size;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filt ? 2.0 : 1.0) * fs;
  a.ks = (int)std::ceil(a.support) * 2 + 1;
  return a;
}
void tap_range(const AxisPlan& a, int in_size, int xx, int* lo, int* hi) {
  const double center = (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *lo = xmin;
  *hi = xmax;
}
// one job = one image in one geometry: geom 0 = EfficientNet squash (bilinear), 1 = CLIP
// shortest-edge + centre crop (bicubic); returns false when a pass needs more than kResizeKMax taps
bool plan_job(int w, int h, int geom, ResizeJob* J) {
  *J = ResizeJob{};
  J->w = w;
  J->h = h;
  J->filt = geom;
  if (w == 224 && h == 224) {
    J->ow = J->oh = 224;
  } else if (geom == 0) {
    J->ow = J->oh = 224;
  } else {
    const int shrt = w <= h ? w : h, lng = w <= h ? h : w;
    const int new_long = (int)(224.0 * lng / shrt);
    J->ow = w <= h ? 224 : new_long;
    J->oh = w <= h ? new_long : 224;
    J->cx = (J->ow - 224) / 2;
    J->cy = (J->oh - 224) / 2;
  }
  J->need_h = J->ow != w;
  J->need_v = J->oh != h;
  J->ksh = J->need_h ? axis_plan(w, J->ow, J->filt).ks : 1;
  J->ksv = J->need_v ? axis_plan(h, J->oh, J->filt).ks : 1;
  if (J->ksh > kResizeKMax || J->ksv > kResizeKMax) return false;
  if (J->need_v) {
    const AxisPlan a = axis_plan(h, J->oh, J->filt);
    int lo, hi;
    tap_range(a, h, J->cy, &lo, &hi);
    J->y0 = lo;
    tap_range(a, h, J->cy + 223, &lo, &hi);
    J->y1 = hi;
  } else {
    J->y0 = J->cy;
    J->y1 = J->cy + 224;
  }
  // Image.resize (Pillow's Image.py) resamples a source more than 100 times as tall as wide whose height shrinks
  // vertically first, to (w, oh), and horizontally after; with one pass alone the order is moot
  if (J->need_h && J->need_v && (long long)h > (long long)w * 100 && J->oh < h) {
    const AxisPlan a = axis_plan(w, J->ow, J->filt);
    int lo, hi;
    tap_range(a, w, J->cx, &lo, &hi);
    J->x0 = lo;
    tap_range(a, w, J->cx + 223, &lo, &hi);
    J->x1 = hi;
  }
  return true;
}
// lines of the first pass: source rows, or source columns where the vertical pass runs first
int first_pass_lines(const ResizeJob& J) { return J.x1 > 0 ? J.x1 - J.x0 : J.y1 - J.y0; }
}  // namespace

extern "C" {

int mmf_resize_pil(mmf_handle* h, const uint8_t* src, const int64_t* offsets, const int32_t* wh, int B,
                   int pixel_bytes, uint8_t* out_effnet, uint8_t* out_clip, void* stream) {
  if (!h || !src || !offsets || !wh || B < 0) return fail(MMF_EINVAL, "null argument");
  if (pixel_bytes != 3 && pixel_bytes != 4) return fail(MMF_EINVAL, "pixel_bytes must be 3 (RGB) or 4 (RGBX)");
  if (!out_effnet && !out_clip) return 0;
  HIPCHK(hipSetDevice(h->device));
  std::vector<ResizeJob> jobs;
  std::vector<uint8_t*> outs;
  long long tmp = 0;
  int coef = 0, max_rows = 0;
  for (int i = 0; i < B; ++i) {
    const int w = wh[2 * i], ht = wh[2 * i + 1];
    if (w <= 0 || ht <= 0) return fail(MMF_EINVAL, "image %d has size %dx%d", i, w, ht);
    for (int geom = 0; geom < 2; ++geom) {
      uint8_t* o = geom ? out_clip : out_effnet;
      if (!o) continue;
      ResizeJob J;
      if (!plan_job(w, ht, geom, &J))
        return fail(MMF_ERANGE, "image %d (%dx%d): downscale beyond %d taps per output pixel", i, w, ht, kResizeKMax);
      J.src_off = offsets[i];
      J.ps = pixel_bytes;
      J.tmp_off = tmp;
      J.coef_off = coef;
      tmp += (long long)first_pass_lines(J) * 224 * 3;
      coef += 224 * (J.ksh + J.ksv);
      max_rows = std::max(max_rows, first_pass_lines(J));
      jobs.push_back(J);
      outs.push_back(o + (size_t)i * 224 * 224 * 3);
    }
  }
  auto& R = h->rs;
  const size_t nj = jobs.size();
  if (nj > R.cap_jobs || (size_t)coef > R.cap_coef || (size_t)tmp > R.cap_tmp) {
    CHK(free_group(h, AG_RESIZE));
    R.cap_jobs = std::max(nj, R.cap_jobs);
    R.cap_coef = std::max((size_t)coef, R.cap_coef);
    R.cap_tmp = std::max((size_t)tmp, R.cap_tmp);
    CHK(dev_alloc(h, &R.jobs, R.cap_jobs, AG_RESIZE));
    CHK(dev_alloc(h, &R.outs, R.cap_jobs, AG_RESIZE));
    CHK(dev_alloc(h, &R.bounds, R.cap_jobs * 2 * 224 * 2, AG_RESIZE));
    CHK(dev_alloc(h, &R.coef, R.cap_coef, AG_RESIZE));
    CHK(dev_alloc(h, &R.tmp, R.cap_tmp, AG_RESIZE));
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(R.jobs, jobs.data(), nj * sizeof(ResizeJob), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(R.outs, outs.data(), nj * sizeof(uint8_t*), hipMemcpyHostToDevice, s));
  HIPCHK(launch_resize_pil(src, R.jobs, (int)nj, max_rows, R.coef, R.bounds, R.tmp, R.outs, s));
  HIPCHK(hipStreamSynchronize(s));  // the host job tables above are released on return
  return 0;
}

int mmf_resize_supported(int width, int height) {
  int32_t p[12];
  return mmf_resize_plan(width, height, 0, p) == 0 && mmf_resize_plan(width, height, 1, p) == 0 ? 1 : 0;
}

// Test-only: plan_job's geometry for one image (tests/test_resize_refs_cpu.py)
int mmf_resize_plan(int width, int height, int geom, int32_t* out12) {
  if (!out12) return fail(MMF_EINVAL, "null argument");
  if (width <= 0 || height <= 0) return fail(MMF_EINVAL, "resize_plan: size %dx%d", width, height);
  if (geom != 0 && geom != 1) return fail(MMF_EINVAL, "resize_plan: geom %d (0 EfficientNet, 1 CLIP)", geom);
  ResizeJob J;
  if (!plan_job(width, height, geom, &J))
    return fail(MMF_ERANGE, "resize_plan: %dx%d: downscale beyond %d taps per output pixel", width, height, kResizeKMax);
  const int32_t v[12] = {J.ow, J.oh, J.cx, J.cy, J.need_h, J.need_v, J.y0, J.y1, J.ksh, J.ksv, J.x0, J.x1};
  std::copy(v, v + 12, out12);
  return 0;
}

// Test-only: the coefficient kernel of mmf_resize_pil on the one job of a width x height image
// (tests/test_gpu_resize.py).  Synchronous: the job table is a temporary of this call
int mmf_resize_coef_raw(int width, int height, int geom, int32_t* coef, int32_t* bounds, void* stream) {
  if (!coef || !bounds) return fail(MMF_EINVAL, "null argument");
  if (width <= 0 || height <= 0) return fail(MMF_EINVAL, "resize_coef: size %dx%d", width, height);
  if (geom != 0 && geom != 1) return fail(MMF_EINVAL, "resize_coef: geom %d (0 EfficientNet, 1 CLIP)", geom);
  ResizeJob J;
  if (!plan_job(width, height, geom, &J))
    return fail(MMF_ERANGE, "resize_coef: %dx%d: downscale beyond %d taps per output pixel", width, height, kResizeKMax);
  hipStream_t s = (hipStream_t)stream;
  ResizeJob* dj = nullptr;
  HIPCHK(hipMalloc((void**)&dj, sizeof(ResizeJob)));
  hipError_t e = hipMemcpyAsync(dj, &J, sizeof(ResizeJob), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_resize_coef(dj, 1, coef, bounds, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  (void)hipFree(dj);
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(MMF_EIO, "resize_coef: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return 0;
}

}  // extern "C"
