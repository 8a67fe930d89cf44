// The EfficientNet-B0 tower's launch sequences (fp16 activations, and the fp32 tower of option
// effnet_fp32), its block geometry and the workspace sizes that follow from it.
#include "handle.h"

EffBlock eff_block(int si, int j) {
  const int* st = kStages[si];
  EffBlock B{};
  B.expand = st[0];
  B.k = st[1];
  B.stride = j == 0 ? st[2] : 1;
  B.cin = j == 0 ? st[3] : st[4];
  B.cout = st[4];
  B.cexp = B.cin * B.expand;
  B.csq = B.cin / 4 > 1 ? B.cin / 4 : 1;
  B.residual = (B.stride == 1 && B.cin == B.cout);
  return B;
}

EffSizes eff_sizes() {
  EffSizes z{(size_t)112 * 112 * 32, 0, 0, 0};
  int H = 112;
  for (int si = 0; si < 7; ++si)
    for (int j = 0; j < kStages[si][5]; ++j) {
      const EffBlock b = eff_block(si, j);
      const int Ho = (H - 1) / b.stride + 1;
      z.exp = std::max(z.exp, (size_t)H * H * b.cexp);
      z.dw = std::max(z.dw, (size_t)Ho * Ho * b.cexp);
      z.io = std::max(z.io, (size_t)Ho * Ho * b.cout);
      z.pool = std::max(z.pool, (size_t)dwconv_nchunks(H, H, b.cexp, b.stride) * b.cexp);
      H = Ho;
    }
  z.exp = std::max(z.exp, (size_t)7 * 7 * 1280);
  return z;
}

namespace {

// The EfficientNet activation workspaces hold max_batch images at the largest per-image size of each
// buffer; a batch chunk that starts at image b0 works in the disjoint slice b0 * (per-image max) on,
// so chunks of one batch can run concurrently on different streams (mmf_effnet_forward).
template <typename T>
struct EffWs {
  T *e_a, *e_b, *e_exp, *e_dw;  // T = f16_t: the fp16 tower; float: the fp32 tower's (Workspace e32_*)
  float *e_pool, *e_scale;
};
template <typename T>
EffWs<T> eff_ws(const Workspace& w, T* a, T* b, T* exp, T* dw, int b0) {
  const EffSizes es = eff_sizes();
  const size_t i = (size_t)b0;
  return EffWs<T>{a + i * es.io, b + i * es.io, exp + i * es.exp, dw + i * es.dw, w.e_pool + i * es.pool,
                  w.e_scale + i * 1280};
}

// The fp32 tower (option effnet_fp32): same network, same folded weights (fp32 copies of the 1x1
// convs), activations fp32 throughout -- no fusion, one launch per layer.
int run_effnet32(mmf_handle* h, const uint8_t* img, const float* xf32, int B, float* logits, float* score,
                 int score_stride, hipStream_t s, int img0, float* pooled, float* trunk) {
  if (h->ws.e32_cap_b < img0 + B) return fail(MMF_EINVAL, "effnet_fp32: fp32 tower workspaces not reserved");
  const EffWs<float> w = eff_ws(h->ws, h->ws.e32_a, h->ws.e32_b, h->ws.e32_exp, h->ws.e32_dw, img0);
  float* cur = w.e_a;
  float* nxt = w.e_b;
  {
    ProfScope ps(h, s, PK_STEM, 2.0 * B * 112 * 112 * 32 * 27, (double)B * (224 * 224 * 3 + 112 * 112 * 32 * 4));
    HIPCHK(launch_effnet_stem32(img, xf32, h->e_stem_w, h->e_stem_b, cur, B, s));
  }
  int H = 112, W = 112;
  for (const EffBlock& b : h->e_blocks) {
    const int Ho = (H - 1) / b.stride + 1, Wo = (W - 1) / b.stride + 1;
    const float* src = cur;
    if (b.expand != 1) {
      ProfScope ps(h, s, PK_PW32, 2.0 * B * H * W * b.cin * b.cexp, 4.0 * B * H * W * (b.cin + b.cexp));
      HIPCHK(launch_pw32(cur, b.e.w32, b.e.b, nullptr, 1, nullptr, w.e_exp, B * H * W, b.cexp, b.cin, 3 /* SiLU */, s,
                             h->opt.pw32_mfma));
      src = w.e_exp;
    }
    {
      ProfScope ps(h, s, PK_DW, 2.0 * B * Ho * Wo * b.cexp * b.k * b.k, 4.0 * B * b.cexp * ((double)H * W + Ho * Wo));
      HIPCHK(launch_dw32(src, b.wd_t, b.bd, w.e_dw, B, H, W, b.cexp, b.k, b.stride, s));
    }
    {
      ProfScope ps(h, s, PK_SE, 4.0 * B * b.cexp * b.csq, 4.0 * B * b.cexp * ((double)Ho * Wo + 2));
      // as many pool chunks as the fp16 tower uses for this layer (fits e_pool by construction)
      const int nch = std::min(dwconv_nchunks(H, W, b.cexp, b.stride), Ho * Wo);
      HIPCHK(launch_sum32(w.e_dw, B, Ho * Wo, b.cexp, nch, w.e_pool, s));
      HIPCHK(launch_se(w.e_pool, nch, 1.0f / (float)(Ho * Wo), b.w1, b.b1, b.w2, b.b2, w.e_scale, B, b.cexp, b.csq, s,
                       true));
    }
    {
      ProfScope ps(h, s, PK_PW32, 2.0 * B * Ho * Wo * b.cexp * b.cout,
                   4.0 * B * Ho * Wo * (b.cexp + b.cout * (b.residual ? 2 : 1)));
      HIPCHK(launch_pw32(w.e_dw, b.p.w32, b.p.b, w.e_scale, Ho * Wo, b.residual ? cur : nullptr, nxt, B * Ho * Wo,
                         b.cout, b.cexp, 0, s, h->opt.pw32_mfma));
    }
    std::swap(cur, nxt);
    H = Ho;
    W = Wo;
  }
  if (trunk) {  // mmf_effnet_trunk: the last block's output, copied; no head GEMM, pool or classifier
    HIPCHK(hipMemcpyAsync(trunk, cur, sizeof(float) * (size_t)B * H * W * 320, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  {
    ProfScope ps(h, s, PK_PW32, 2.0 * B * H * W * 320 * 1280, 4.0 * B * H * W * (320 + 1280));
    HIPCHK(launch_pw32(cur, h->e_head.w32, h->e_head.b, nullptr, 1, nullptr, w.e_exp, B * H * W, 1280, 320, 3, s,
                       h->opt.pw32_mfma));
  }
  ProfScope ps(h, s, PK_GAP, (double)B * H * W * 1280 + 4.0 * B * 1280, (double)B * H * W * 1280 * 4);
  if (pooled) HIPCHK(launch_gap32_pooled(w.e_exp, H * W, 1280, pooled, B, s));
  else HIPCHK(launch_gap32(w.e_exp, H * W, 1280, h->e_cls_w, h->e_cls_b, logits, score, score_stride, B, s));
  return 0;
}

}  // namespace

int run_effnet(mmf_handle* h, const uint8_t* img, const float* xf32, int B, float* logits, float* score, int score_stride,
               hipStream_t s, int img0, float* pooled, float* trunk) {
  if (h->opt.effnet_fp32) return run_effnet32(h, img, xf32, B, logits, score, score_stride, s, img0, pooled, trunk);
  const EffWs<f16_t> w = eff_ws(h->ws, h->ws.e_a, h->ws.e_b, h->ws.e_exp, h->ws.e_dw, img0);
  f16_t* cur = w.e_a;
  f16_t* nxt = w.e_b;
  // option fuse_stem = 0: separate stem launch + stage-1 depthwise (A/B and parity tests)
  const EffBlock& b0 = h->e_blocks.front();
  const bool fuse_stem = h->opt.fuse_stem && b0.expand == 1 && b0.cexp == 32 && b0.k == 3 && b0.stride == 1;
  if (!fuse_stem) {
    ProfScope ps(h, s, PK_STEM, 2.0 * B * 112 * 112 * 32 * 27, (double)B * (224 * 224 * 3 + 112 * 112 * 32 * 2));
    if (xf32) HIPCHK(launch_effnet_stem_f32(xf32, h->e_stem_w, h->e_stem_b, cur, B, s));
    else HIPCHK(launch_effnet_stem(img, h->e_stem_w, h->e_stem_b, cur, B, s));
  }
  int H = 112, W = 112;
  for (const EffBlock& b : h->e_blocks) {
    const f16_t* src = cur;
    int nch = 0;
    const int Ho = (H - 1) / b.stride + 1, Wo = (W - 1) / b.stride + 1;
    // option fuse_expand = 0: separate expand launch (A/B)
    const bool fuse = b.expand != 1 && h->opt.fuse_expand && expand_dw_applicable(b.cin, b.cexp, b.k);
    if (&b == &b0 && fuse_stem) {
      // stem output recomputed per 18x18 halo tile: 1.27x the stem MACs, image patch read once
      ProfScope ps(h, s, PK_DW, 2.0 * B * 112 * 112 * 32 * (9 + 27 * 1.27),
                   (double)B * (224 * 224 * 3 * 1.34 + 112 * 112 * 32 * 2));
      HIPCHK(launch_effnet_stem_dw(img, xf32, h->e_stem_w, h->e_stem_b, b.wd, b.bd, w.e_dw, w.e_pool, B, &nch, s));
    } else if (fuse) {
      ProfScope ps(h, s, PK_DW, 2.0 * B * Ho * Wo * b.cexp * b.k * b.k + 2.0 * B * H * W * b.cin * b.cexp,
                   (double)B * 2 * ((double)H * W * b.cin * (b.cexp / 48) + (double)Ho * Wo * b.cexp));
      HIPCHK(launch_expand_dw(cur, b.cin, b.e.w, b.e.b, b.wd, b.bd, w.e_dw, w.e_pool, B, H, W, b.cexp, b.k, b.stride,
                              &nch, s));
    } else if (b.expand != 1) {
      GemmArgs g = gemm_args(cur, b.cin, b.e, B * H * W);
      g.act = 3;  // SiLU
      g.c16 = w.e_exp;
      CHK(gemm(h, g, s));
      src = w.e_exp;
    }
    if (!fuse && !(&b == &b0 && fuse_stem)) {
      ProfScope ps(h, s, PK_DW, 2.0 * B * Ho * Wo * b.cexp * b.k * b.k,
                   (double)B * b.cexp * 2 * ((double)H * W + (double)Ho * Wo));
      HIPCHK(launch_dwconv(src, b.wd, b.bd, w.e_dw, w.e_pool, B, H, W, b.cexp, b.k, b.stride, &nch, s,
                            1 | (h->opt.dw_cw32 ? 8 : 0)));
    }
    ProfScope ps(h, s, PK_SE, 4.0 * B * b.cexp * b.csq, (double)B * b.cexp * 4 * (nch + 1));
    HIPCHK(launch_se(w.e_pool, nch, 1.0f / (float)(Ho * Wo), b.w1, b.b1, b.w2, b.b2, w.e_scale, B, b.cexp, b.csq, s));
    GemmArgs g = gemm_args(w.e_dw, b.cexp, b.p, B * Ho * Wo);
    g.ascale = w.e_scale;
    g.rows_per_batch = Ho * Wo;
    if (b.residual) g.res16 = cur;
    g.c16 = nxt;
    CHK(gemm(h, g, s));
    std::swap(cur, nxt);
    H = Ho;
    W = Wo;
  }
  if (trunk) {  // mmf_effnet_trunk: the last block's output, every fp16 value converted exactly
    HIPCHK(launch_f16_rows_to_f32(cur, trunk, (size_t)B * H * W * 320, s));
    return 0;
  }
  GemmArgs g = gemm_args(cur, 320, h->e_head, B * H * W);
  g.act = 3;
  g.c16 = w.e_exp;
  CHK(gemm(h, g, s));
  ProfScope ps(h, s, PK_GAP, (double)B * H * W * 1280 + 4.0 * B * 1280, (double)B * H * W * 1280 * 2);
  if (pooled) HIPCHK(launch_gap_pooled(w.e_exp, H * W, 1280, pooled, B, s));
  else HIPCHK(launch_gap_classifier(w.e_exp, H * W, 1280, h->e_cls_w, h->e_cls_b, logits, score, score_stride, B, s));
  return 0;
}

// ---- test-only entry points: the fp16 tower's kernels on raw device operands (include/mmf_hip.h;
// tests/test_gpu_effnet_kernels.py).  Every shape check runs on the host before anything is launched.
namespace {

// a launcher's hipErrorInvalidValue is its "unsupported shape" answer; anything else is a HIP failure
int test_launch_rc(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  if (e == hipErrorInvalidValue) return fail(MMF_EINVAL, "%s: unsupported shape", what);
  return fail(MMF_EIO, "%s: %s", what, hipGetErrorString(e));
}

// what the depthwise launchers' geometry arithmetic and 32-bit byte offsets assume
bool dw_shape_ok(int B, int H, int W, int C, int k, int stride) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0) return false;
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2)) return false;
  return (double)H * W * C * 2.0 < 2147483648.0;
}

}  // namespace

extern "C" {

int mmf_dwconv_nchunks(int H, int W, int C, int stride) {
  if (H <= 0 || W <= 0 || C <= 0 || (stride != 1 && stride != 2)) return fail(MMF_EINVAL, "dwconv_nchunks: bad shape");
  return dwconv_nchunks(H, W, C, stride);
}

int mmf_dwconv_f16(const void* in, const float* w, const float* bias, void* out, float* pool_part, int B, int H, int W,
                   int C, int k, int stride, int flags, void* stream) {
  if (!in || !w || !bias || !out || !pool_part) return fail(MMF_EINVAL, "null argument");
  if (!dw_shape_ok(B, H, W, C, k, stride))
    return fail(MMF_EINVAL, "dwconv: unsupported shape (B=%d H=%d W=%d C=%d k=%d stride=%d)", B, H, W, C, k, stride);
  int nch = 0;
  return test_launch_rc(launch_dwconv((const f16_t*)in, w, bias, (f16_t*)out, pool_part, B, H, W, C, k, stride, &nch,
                                      (hipStream_t)stream, flags),
                        "dwconv");
}

int mmf_expand_dw_f16(const void* x, int cin, const void* we, const float* be, const float* w, const float* bias,
                      void* out, float* pool_part, int B, int H, int W, int C, int k, int stride, int ct, void* stream) {
  if (!x || !we || !be || !w || !bias || !out || !pool_part) return fail(MMF_EINVAL, "null argument");
  if (!dw_shape_ok(B, H, W, C, k, stride) || cin <= 0 || !expand_dw_applicable(cin, C, k))
    return fail(MMF_EINVAL, "expand_dw: not applicable (cin=%d C=%d k=%d stride=%d B=%d H=%d W=%d)", cin, C, k, stride,
                B, H, W);
  int nch = 0;
  return test_launch_rc(launch_expand_dw((const f16_t*)x, cin, (const f16_t*)we, be, w, bias, (f16_t*)out, pool_part,
                                         B, H, W, C, k, stride, &nch, (hipStream_t)stream, ct),
                        "expand_dw");
}

int mmf_se_f32(const float* pool_part, int nchunks, float inv_hw, const float* w1, const float* b1, const float* w2t,
               const float* b2, float* scale, int B, int C, int Csq, int precise, void* stream) {
  if (!pool_part || !w1 || !b1 || !w2t || !b2 || !scale) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || nchunks <= 0 || C <= 0 || Csq <= 0)
    return fail(MMF_EINVAL, "se: bad shape (B=%d nchunks=%d C=%d Csq=%d)", B, nchunks, C, Csq);
  return test_launch_rc(
      launch_se(pool_part, nchunks, inv_hw, w1, b1, w2t, b2, scale, B, C, Csq, (hipStream_t)stream, precise != 0), "se");
}

int mmf_effnet_stem_f16(const uint8_t* img_u8, const float* x_f32_nchw, const float* w, const float* bias, void* out,
                        int B, void* stream) {
  if (!w || !bias || !out) return fail(MMF_EINVAL, "null argument");
  if (!img_u8 == !x_f32_nchw) return fail(MMF_EINVAL, "stem: exactly one of img_u8 / x_f32_nchw");
  if (B <= 0) return fail(MMF_EINVAL, "stem: bad batch %d", B);
  const hipError_t e = x_f32_nchw ? launch_effnet_stem_f32(x_f32_nchw, w, bias, (f16_t*)out, B, (hipStream_t)stream)
                                  : launch_effnet_stem(img_u8, w, bias, (f16_t*)out, B, (hipStream_t)stream);
  return test_launch_rc(e, "stem");
}

int mmf_effnet_stem_dw_f16(const uint8_t* img_u8, const float* x_f32_nchw, const float* ws, const float* bs,
                           const float* wd, const float* bd, void* out, float* pool_part, int B, void* stream) {
  if (!ws || !bs || !wd || !bd || !out || !pool_part) return fail(MMF_EINVAL, "null argument");
  if (!img_u8 == !x_f32_nchw) return fail(MMF_EINVAL, "stem_dw: exactly one of img_u8 / x_f32_nchw");
  if (B <= 0 || B > 65535) return fail(MMF_EINVAL, "stem_dw: bad batch %d", B);
  int nch = 0;
  return test_launch_rc(
      launch_effnet_stem_dw(img_u8, x_f32_nchw, ws, bs, wd, bd, (f16_t*)out, pool_part, B, &nch, (hipStream_t)stream),
      "stem_dw");
}

int mmf_gap_classifier_f16(const void* x, int HW, int C, const float* w, const float* b, float* logits, float* score,
                           int score_stride, int B, void* stream) {
  if (!x || !w || !b || (!logits && !score)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || HW <= 0 || C <= 0) return fail(MMF_EINVAL, "gap_classifier: bad shape (B=%d HW=%d C=%d)", B, HW, C);
  return test_launch_rc(
      launch_gap_classifier((const f16_t*)x, HW, C, w, b, logits, score, score_stride, B, (hipStream_t)stream),
      "gap_classifier");
}

}  // extern "C"

// ---- test-only entry points: the fp32 tower's kernels (effnet_f32.hip, stem_kernel<*, float>) on raw
// device operands (include/mmf_hip.h; tests/test_gpu_effnet32_kernels.py).  The launchers check little
// themselves: what their float4 accesses, 32-bit geometry and grid sizes assume is checked here.
namespace {

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int mmf_pw32_variant(int M, int N, int K, int mfma, int32_t* d_nf_nc) {
  const Pw32Variant v = pw32_variant(M, N, K, mfma);
  if (mfma < 0 || mfma > 5 || v.kind == PW32_NONE)
    return fail(MMF_EINVAL, "pw32_variant: unsupported (M=%d N=%d K=%d mfma=%d)", M, N, K, mfma);
  if (d_nf_nc) {
    d_nf_nc[0] = v.D;
    d_nf_nc[1] = v.NF;
    d_nf_nc[2] = v.NC;
  }
  return v.kind;
}

int mmf_pw32_f32(const float* A, const float* W, const float* bias, const float* ascale, int rows_per_image,
                 const float* res, float* C, int M, int N, int K, int act, int mfma, void* stream) {
  if (!A || !W || !bias || !C) return fail(MMF_EINVAL, "null argument");
  if (mfma < 0 || mfma > 5) return fail(MMF_EINVAL, "pw32: mfma mode %d outside 0..5", mfma);
  if (M <= 0 || N <= 0 || K <= 0 || (N % 4) || (K % 4) || (ascale && rows_per_image <= 0) ||
      (act != 0 && act != 3 /* SiLU */))
    return fail(MMF_EINVAL, "pw32: unsupported (M=%d N=%d K=%d act=%d rows_per_image=%d)", M, N, K, act,
                rows_per_image);
  if (!al16(A) || !al16(W) || !al16(bias) || !al16(ascale) || !al16(res) || !al16(C))
    return fail(MMF_EINVAL, "pw32: operands must be 16-byte aligned");
  return test_launch_rc(
      launch_pw32(A, W, bias, ascale, rows_per_image, res, C, M, N, K, act, (hipStream_t)stream, mfma), "pw32");
}

int mmf_dw32_f32(const float* in, const float* w_tapmajor, const float* bias, float* out, int B, int H, int W, int C,
                 int k, int stride, void* stream) {
  if (!in || !w_tapmajor || !bias || !out) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 4) || (k != 3 && k != 5) || (stride != 1 && stride != 2))
    return fail(MMF_EINVAL, "dw32: unsupported shape (B=%d H=%d W=%d C=%d k=%d stride=%d)", B, H, W, C, k, stride);
  // the kernel's size_t offsets hold any buffer that exists; its grid is one thread per (image, output
  // row, group of outputs, 4 channels), at most as many as input elements / 4, and must fit 2^32 threads
  if ((double)B * H * W * C >= 4294967296.0) return fail(MMF_EINVAL, "dw32: B * H * W * C >= 2^32");
  if (!al16(in) || !al16(w_tapmajor) || !al16(out)) return fail(MMF_EINVAL, "dw32: operands must be 16-byte aligned");
  return test_launch_rc(launch_dw32(in, w_tapmajor, bias, out, B, H, W, C, k, stride, (hipStream_t)stream), "dw32");
}

int mmf_sum32_f32(const float* x, int B, int HW, int C, int nchunks, float* part, void* stream) {
  if (!x || !part) return fail(MMF_EINVAL, "null argument");
  // grid (C / 4 / L, ceil(nchunks L / 16), B) with L <= 16; pixel indices run to HW + 15 in an int
  if (B <= 0 || B > 65535 || HW <= 0 || HW > (1 << 20) || C <= 0 || (C % 16) || nchunks < 1 || nchunks > HW ||
      nchunks > 65535)
    return fail(MMF_EINVAL, "sum32: unsupported shape (B=%d HW=%d C=%d nchunks=%d)", B, HW, C, nchunks);
  if (!al16(x) || !al16(part)) return fail(MMF_EINVAL, "sum32: operands must be 16-byte aligned");
  return test_launch_rc(launch_sum32(x, B, HW, C, nchunks, part, (hipStream_t)stream), "sum32");
}

int mmf_gap32_f32(const float* x, int HW, int C, const float* w, const float* b, float* logits, float* score,
                  int score_stride, int B, void* stream) {
  if (!x || !w || !b || (!logits && !score)) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || B > (1 << 30) || HW <= 0 || C <= 0 || score_stride < 1)
    return fail(MMF_EINVAL, "gap32: bad shape (B=%d HW=%d C=%d score_stride=%d)", B, HW, C, score_stride);
  return test_launch_rc(launch_gap32(x, HW, C, w, b, logits, score, score_stride, B, (hipStream_t)stream), "gap32");
}

int mmf_effnet_stem32_f32(const uint8_t* img_u8, const float* x_f32_nchw, const float* w, const float* bias,
                          float* out_f32, int B, void* stream) {
  if (!w || !bias || !out_f32) return fail(MMF_EINVAL, "null argument");
  if (!img_u8 == !x_f32_nchw) return fail(MMF_EINVAL, "stem32: exactly one of img_u8 / x_f32_nchw");
  if (B <= 0 || B > 65535) return fail(MMF_EINVAL, "stem32: bad batch %d", B);
  if (!al16(out_f32)) return fail(MMF_EINVAL, "stem32: out must be 16-byte aligned");
  return test_launch_rc(launch_effnet_stem32(img_u8, x_f32_nchw, w, bias, out_f32, B, (hipStream_t)stream), "stem32");
}

}  // extern "C"
