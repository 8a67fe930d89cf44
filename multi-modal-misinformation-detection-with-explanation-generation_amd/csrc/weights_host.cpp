// Weight packing of libmmf_hip.so: the staged fp32 tensors of each component (mmf_load_tensor) become
// the device copies the launch sequences read -- fp16 / split fp16 weights, folded LayerNorms and
// BatchNorms, the per-head QKV interleave.
#include <cmath>

#include "handle.h"

namespace {

// float -> IEEE fp16 bits, round-to-nearest-even (the compiler's _Float16 conversion)
uint16_t f2h_host(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}

float h2f_host(uint16_t b) {
  _Float16 h;
  std::memcpy(&h, &b, 2);
  return (float)h;
}

template <typename T>
int upload(mmf_handle* h, T** dst, const std::vector<T>& v) {
  CHK(dev_alloc(h, dst, v.size(), h->cur_group));
  HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int up_f32(mmf_handle* h, float** dst, const std::vector<float>& v) { return upload(h, dst, v); }

namespace {

int up_f16(mmf_handle* h, f16_t** dst, const std::vector<float>& v) {
  std::vector<uint16_t> b(v.size());
  for (size_t i = 0; i < v.size(); ++i) b[i] = f2h_host(v[i]);
  return upload(h, dst, b);
}

// W [out][in] fp32 -> [W_hi | W_hi | W_lo] fp16 [out][3 in] (precise.hip: the K-concatenated weight)
int up_split3(mmf_handle* h, Lin16* dst, const std::vector<float>& w, const float* bias, int out, int in,
              int group = -1) {
  std::vector<uint16_t> b((size_t)out * 3 * in);
  for (int n = 0; n < out; ++n)
    for (int k = 0; k < in; ++k) {
      const float x = w[(size_t)n * in + k];
      const uint16_t hi = f2h_host(x);
      uint16_t* r = b.data() + (size_t)n * 3 * in;
      r[k] = hi;
      r[in + k] = hi;
      r[2 * in + k] = f2h_host(x - h2f_host(hi));
    }
  const int saved = h->cur_group;
  if (group >= 0) h->cur_group = group;
  const int r = upload(h, &dst->w, b);
  h->cur_group = saved;
  CHK(r);
  dst->b = const_cast<float*>(bias);
  dst->out = out;
  dst->in = 3 * in;
  return 0;
}

const HostT* get(mmf_handle* h, const std::string& name, size_t numel) {
  auto it = h->staged.find(name);
  if (it == h->staged.end()) {
    fail(MMF_EINVAL, "missing weight '%s'", name.c_str());
    return nullptr;
  }
  if (numel && it->second.numel() != numel) {
    fail(MMF_EINVAL, "weight '%s' has %zu elements, expected %zu", name.c_str(), it->second.numel(), numel);
    return nullptr;
  }
  return &it->second;
}

#define GET(var, name, n)                       \
  const HostT* var = get(h, (name), (n));       \
  if (!var) return MMF_EINVAL;

int load_f32(mmf_handle* h, float** dst, const std::string& name, size_t n) {
  GET(t, name, n);
  return up_f32(h, dst, t->f);
}
// per-column vectors the lazy-LN epilogues DMA in 256-column blocks: zero-padded by 256
constexpr int kColPad = 256;
int up_f32_padded(mmf_handle* h, float** dst, std::vector<float> v) {
  v.resize(v.size() + kColPad, 0.f);
  return up_f32(h, dst, v);
}
int load_f32_padded(mmf_handle* h, float** dst, const std::string& name, size_t n) {
  GET(t, name, n);
  return up_f32_padded(h, dst, t->f);
}
int load_ln(mmf_handle* h, LNp* ln, const std::string& p, int n) {
  CHK(load_f32_padded(h, &ln->g, p + ".weight", n));
  return load_f32_padded(h, &ln->b, p + ".bias", n);
}
int load_lin(mmf_handle* h, Lin16* l, const std::string& p, int out, int in, bool bias, Lin16* split3 = nullptr,
             int split3_group = -1) {
  GET(w, p + ".weight", (size_t)out * in);
  CHK(up_f16(h, &l->w, w->f));
  if (bias) CHK(load_f32_padded(h, &l->b, p + ".bias", out));
  l->out = out;
  l->in = in;
  if (split3) CHK(up_split3(h, split3, w->f, l->b, out, in, split3_group));
  return 0;
}
// LN(x) W^T + b with LN = (gamma, beta) folded (gemm.hip lazy LN): w' = fp16(w diag(gamma)),
// u = sum_k w'[n][k] over the fp16 values (so acc - mean u is exactly sum_k w'(s_k - mean)),
// c = b + w beta, both in double
// dst_h / u_h (nullable; a fused QKV, out = 3 in): the same (w', u, c) with rows interleaved per head as qkv_h
int fold_ln_lin(mmf_handle* h, Lin16* dst, float** u, const std::vector<float>& w, const std::vector<float>& b,
                int out, int in, const std::vector<float>& g, const std::vector<float>& beta, Lin16* dst_h = nullptr,
                float** u_h = nullptr) {
  std::vector<float> wf((size_t)out * in), uv(out), c(out);
  for (int n = 0; n < out; ++n) {
    double su = 0.0, sc = b[n];
    for (int k = 0; k < in; ++k) {
      const float x = w[(size_t)n * in + k] * g[k];
      wf[(size_t)n * in + k] = x;
      su += (double)h2f_host(f2h_host(x));
      sc += (double)w[(size_t)n * in + k] * beta[k];
    }
    uv[n] = (float)su;
    c[n] = (float)sc;
  }
  CHK(up_f16(h, &dst->w, wf));
  CHK(up_f32_padded(h, &dst->b, c));
  CHK(up_f32_padded(h, u, uv));
  dst->out = out;
  dst->in = in;
  if (dst_h) {
    const int H = in;
    std::vector<float> wh(wf.size()), uh(out), ch(out);
    for (int hd = 0; hd < H / 64; ++hd)
      for (int part = 0; part < 3; ++part)
        for (int d = 0; d < 64; ++d) {
          const size_t src = (size_t)part * H + hd * 64 + d, dr = (size_t)hd * 192 + part * 64 + d;
          std::memcpy(wh.data() + dr * in, wf.data() + src * in, sizeof(float) * in);
          uh[dr] = uv[src];
          ch[dr] = c[src];
        }
    CHK(up_f16(h, &dst_h->w, wh));
    CHK(up_f32_padded(h, &dst_h->b, ch));
    CHK(up_f32_padded(h, u_h, uh));
    dst_h->out = out;
    dst_h->in = in;
  }
  return 0;
}
int fold_ln_named(mmf_handle* h, Lin16* dst, float** u, const std::string& lin, int out, int in,
                  const std::string& ln) {
  GET(w, lin + ".weight", (size_t)out * in);
  GET(b, lin + ".bias", out);
  GET(g, ln + ".weight", in);
  GET(be, ln + ".bias", in);
  return fold_ln_lin(h, dst, u, w->f, b->f, out, in, g->f, be->f);
}
// fused QKV: rows [q; k; v] of [3*H][H] + bias; with ln (non-empty) also the LN-folded copy; with
// heads also the per-head interleaved copy qkv_h (row 192 h + 64 part + d = row H part + 64 h + d)
int load_qkv(mmf_handle* h, EncLayer* L, const std::string& q, const std::string& k, const std::string& v, int H,
             const std::string& ln, bool heads = false, bool split3 = false) {
  Lin16* l = &L->qkv;
  std::vector<float> w((size_t)3 * H * H), b((size_t)3 * H);
  const std::string names[3] = {q, k, v};
  for (int i = 0; i < 3; ++i) {
    GET(tw, names[i] + ".weight", (size_t)H * H);
    GET(tb, names[i] + ".bias", (size_t)H);
    std::memcpy(w.data() + (size_t)i * H * H, tw->f.data(), sizeof(float) * H * H);
    std::memcpy(b.data() + (size_t)i * H, tb->f.data(), sizeof(float) * H);
  }
  CHK(up_f16(h, &l->w, w));
  CHK(up_f32_padded(h, &l->b, b));
  l->out = 3 * H;
  l->in = H;
  if (split3) CHK(up_split3(h, &L->qkv3, w, l->b, 3 * H, H, AG_TP0));
  if (heads) {
    std::vector<float> wh(w.size()), bh(b.size());
    for (int hd = 0; hd < H / 64; ++hd)
      for (int part = 0; part < 3; ++part)
        for (int d = 0; d < 64; ++d) {
          const size_t src = (size_t)part * H + hd * 64 + d, dst = (size_t)hd * 192 + part * 64 + d;
          std::memcpy(wh.data() + dst * H, w.data() + src * H, sizeof(float) * H);
          bh[dst] = b[src];
        }
    CHK(up_f16(h, &L->qkv_h.w, wh));
    CHK(up_f32_padded(h, &L->qkv_h.b, bh));
    L->qkv_h.out = 3 * H;
    L->qkv_h.in = H;
  }
  if (ln.empty()) return 0;
  GET(g, ln + ".weight", H);
  GET(be, ln + ".bias", H);
  return fold_ln_lin(h, &L->qkv_f, &L->qkv_u, w, b, 3 * H, H, g->f, be->f, &L->qkv_fh, &L->qkv_uh);
}

// BatchNorm (eval) folded into the preceding conv: w' = w * g/sqrt(v+eps), b' = beta - m*g/sqrt(v+eps)
int fold_bn(mmf_handle* h, const std::string& conv, const std::string& bn, int cout, size_t per_out,
            std::vector<float>* w, std::vector<float>* b) {
  GET(cw, conv + ".weight", (size_t)cout * per_out);
  GET(g, bn + ".weight", cout);
  GET(be, bn + ".bias", cout);
  GET(m, bn + ".running_mean", cout);
  GET(v, bn + ".running_var", cout);
  w->resize((size_t)cout * per_out);
  b->resize(cout);
  for (int o = 0; o < cout; ++o) {
    const double s = (double)g->f[o] / std::sqrt((double)v->f[o] + 1e-5);
    for (size_t i = 0; i < per_out; ++i) (*w)[(size_t)o * per_out + i] = (float)(cw->f[(size_t)o * per_out + i] * s);
    (*b)[o] = (float)((double)be->f[o] - (double)m->f[o] * s);
  }
  return 0;
}

// an EfficientNet 1x1 conv (BN folded): the fp16 weight, its fp32 copy (effnet_fp32 tower) and the bias
int up_conv1x1(mmf_handle* h, Lin16* l, const std::vector<float>& w, const std::vector<float>& b, int out, int in) {
  CHK(up_f16(h, &l->w, w));
  CHK(up_f32(h, &l->w32, w));
  CHK(up_f32(h, &l->b, b));
  l->out = out;
  l->in = in;
  return 0;
}

std::vector<float> transpose(const std::vector<float>& a, int rows, int cols) {
  std::vector<float> t((size_t)rows * cols);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = a[(size_t)r * cols + c];
  return t;
}

}  // namespace

int finalize_text(mmf_handle* h) {
  const std::string p = "roberta.";
  CHK(load_f32(h, &h->r_word, p + "embeddings.word_embeddings.weight", (size_t)50265 * 768));
  CHK(load_f32(h, &h->r_pos, p + "embeddings.position_embeddings.weight", (size_t)514 * 768));
  {
    GET(t, p + "embeddings.token_type_embeddings.weight", 0);
    std::vector<float> t0(t->f.begin(), t->f.begin() + 768);
    CHK(up_f32(h, &h->r_type0, t0));
  }
  CHK(load_ln(h, &h->r_embln, p + "embeddings.LayerNorm", 768));
  {
    // RoBERTa's residual stream IS a LayerNorm output (post-LN): x_c = beta_c + gamma_c xhat_c, and
    // over C channels |xhat_c| <= sqrt(C - 1) (reached when one channel carries all of the row's
    // variance -- exactly the outlier-channel case), so |x_c| <= |beta_c| + sqrt(767) |gamma_c| is a
    // sound bound for every input.  Trained models put O(1e2-1e3) "outlier" values in a few
    // channels; stored in fp16 alone (2^-11 relative) their rounding shifts every next LayerNorm's
    // mean coherently across all channels (tests/test_gpu_outliers.py: 1.6e-3 at a 900-level
    // outlier vs 2.2e-4 on the plain draw), so above kHiloMag the split hi + lo stream (~22 bits)
    // is used.  (Round 3 bounded |xhat| by 4, which a dominating channel exceeds: VERDICT r3.)
    constexpr float kHiloMag = 64.f;
    const float kXhatMax = std::sqrt(767.f);
    float mag = 0.f;
    auto scan = [&](const std::string& ln) -> int {
      GET(g, ln + ".weight", 768);
      GET(b, ln + ".bias", 768);
      for (int c = 0; c < 768; ++c) mag = std::max(mag, std::fabs(b->f[c]) + kXhatMax * std::fabs(g->f[c]));
      return 0;
    };
    CHK(scan(p + "embeddings.LayerNorm"));
    for (int i = 0; i < 12; ++i) {
      const std::string l = p + "encoder.layer." + std::to_string(i) + ".";
      CHK(scan(l + "attention.output.LayerNorm"));
      CHK(scan(l + "output.LayerNorm"));
    }
    h->r_stream_mag = mag;
    h->r_hilo_auto = mag > kHiloMag ? 1 : 0;
  }
  // the precise mode's K-concatenated weights (+510 MB) are packed unless the layout is pinned to an
  // fp16 stream (text_hilo 0 / 1): the load-time calibration (engine.py) may select the mode
  // (each kind's K-concatenated weights in its own allocation group AG_TP0 + k, so that the engine's
  // calibration can release the kinds the selected mode does not read: option text_precise_packed)
  const bool sp = h->opt.text_hilo < 0 || h->opt.text_hilo >= 2;
  h->r_precise = 0;
  for (int k = 0; k < 4; ++k) CHK(free_group(h, AG_TP0 + k));
  for (int i = 0; i < 12; ++i) {
    const std::string l = p + "encoder.layer." + std::to_string(i) + ".";
    EncLayer& L = h->r_layers[i];
    L.qkv3 = L.o3 = L.fc13 = L.fc23 = Lin16{};
    CHK(load_qkv(h, &L, l + "attention.self.query", l + "attention.self.key", l + "attention.self.value", 768, "",
                 true, sp));
    CHK(load_lin(h, &L.o, l + "attention.output.dense", 768, 768, true, sp ? &L.o3 : nullptr, AG_TP0 + 1));
    CHK(load_ln(h, &L.ln1, l + "attention.output.LayerNorm", 768));
    CHK(load_lin(h, &L.fc1, l + "intermediate.dense", 3072, 768, true, sp ? &L.fc13 : nullptr, AG_TP0 + 2));
    CHK(load_lin(h, &L.fc2, l + "output.dense", 768, 3072, true, sp ? &L.fc23 : nullptr, AG_TP0 + 3));
    CHK(load_ln(h, &L.ln2, l + "output.LayerNorm", 768));
  }
  h->r_precise = sp ? 15 : 0;
  for (int hd = 0; hd < 2; ++hd) {
    const std::string n = hd ? "misinfo_head" : "ai_head";
    GET(w1, n + ".0.weight", (size_t)256 * 768);
    float** w1d = hd ? &h->h_w1m : &h->h_w1a;
    CHK(up_f32(h, w1d, transpose(w1->f, 256, 768)));
    CHK(load_f32(h, hd ? &h->h_b1m : &h->h_b1a, n + ".0.bias", 256));
    CHK(load_f32(h, hd ? &h->h_w2m : &h->h_w2a, n + ".3.weight", 512));
    CHK(load_f32(h, hd ? &h->h_b2m : &h->h_b2a, n + ".3.bias", 2));
  }
  return 0;
}

int finalize_effnet(mmf_handle* h) {
  const std::string p = "efficientnet.features.";
  std::vector<float> w, b;
  CHK(fold_bn(h, p + "0.0", p + "0.1", 32, 27, &w, &b));
  CHK(up_f32(h, &h->e_stem_w, w));
  CHK(up_f32(h, &h->e_stem_b, b));
  h->e_blocks.clear();
  for (int si = 0; si < 7; ++si) {
    for (int j = 0; j < kStages[si][5]; ++j) {
      EffBlock B = eff_block(si, j);
      const std::string bp = p + std::to_string(si + 1) + "." + std::to_string(j) + ".block.";
      int i = 0;
      if (B.expand != 1) {
        CHK(fold_bn(h, bp + "0.0", bp + "0.1", B.cexp, B.cin, &w, &b));
        CHK(up_conv1x1(h, &B.e, w, b, B.cexp, B.cin));
        i = 1;
      }
      CHK(fold_bn(h, bp + std::to_string(i) + ".0", bp + std::to_string(i) + ".1", B.cexp, (size_t)B.k * B.k, &w, &b));
      CHK(up_f32(h, &B.wd, w));
      CHK(up_f32(h, &B.wd_t, transpose(w, B.cexp, B.k * B.k)));
      CHK(up_f32(h, &B.bd, b));
      const std::string se = bp + std::to_string(i + 1) + ".";
      CHK(load_f32(h, &B.w1, se + "fc1.weight", (size_t)B.csq * B.cexp));
      CHK(load_f32(h, &B.b1, se + "fc1.bias", B.csq));
      {
        GET(w2, se + "fc2.weight", (size_t)B.cexp * B.csq);
        CHK(up_f32(h, &B.w2, transpose(w2->f, B.cexp, B.csq)));  // [csq][cexp] for coalesced fc2
      }
      CHK(load_f32(h, &B.b2, se + "fc2.bias", B.cexp));
      CHK(fold_bn(h, bp + std::to_string(i + 2) + ".0", bp + std::to_string(i + 2) + ".1", B.cout, B.cexp, &w, &b));
      CHK(up_conv1x1(h, &B.p, w, b, B.cout, B.cexp));
      h->e_blocks.push_back(B);
    }
  }
  CHK(fold_bn(h, p + "8.0", p + "8.1", 1280, 320, &w, &b));
  CHK(up_conv1x1(h, &h->e_head, w, b, 1280, 320));
  CHK(load_f32(h, &h->e_cls_w, "efficientnet.classifier.1.weight", 2 * 1280));
  CHK(load_f32(h, &h->e_cls_b, "efficientnet.classifier.1.bias", 2));
  return 0;
}

static int finalize_clip_layers(mmf_handle* h, EncLayer* layers, const std::string& base, int H, int I) {
  for (int i = 0; i < 12; ++i) {
    const std::string l = base + std::to_string(i) + ".";
    EncLayer& L = layers[i];
    CHK(load_qkv(h, &L, l + "self_attn.q_proj", l + "self_attn.k_proj", l + "self_attn.v_proj", H, l + "layer_norm1"));
    CHK(load_lin(h, &L.o, l + "self_attn.out_proj", H, H, true));
    CHK(load_ln(h, &L.ln1, l + "layer_norm1", H));
    CHK(load_lin(h, &L.fc1, l + "mlp.fc1", I, H, true));
    CHK(fold_ln_named(h, &L.fc1_f, &L.fc1_u, l + "mlp.fc1", I, H, l + "layer_norm2"));
    CHK(load_lin(h, &L.fc2, l + "mlp.fc2", H, I, true));
    CHK(load_ln(h, &L.ln2, l + "layer_norm2", H));
  }
  return 0;
}

int finalize_clip_vision(mmf_handle* h) {
  const std::string p = "clip.vision_model.";
  {
    GET(w, p + "embeddings.patch_embedding.weight", (size_t)768 * 3072);
    CHK(up_f16(h, &h->v_patch_w, w->f));  // [768][3*32*32] = (c, ky, kx) columns
  }
  CHK(load_f32(h, &h->v_cls, p + "embeddings.class_embedding", 768));
  CHK(load_f32(h, &h->v_pos, p + "embeddings.position_embedding.weight", 50 * 768));
  CHK(load_ln(h, &h->v_pre, p + "pre_layrnorm", 768));
  CHK(finalize_clip_layers(h, h->v_layers, p + "encoder.layers.", 768, 3072));
  CHK(load_ln(h, &h->v_post, p + "post_layernorm", 768));
  GET(pw, "clip.visual_projection.weight", (size_t)512 * 768);
  return up_f16(h, &h->v_proj, pw->f);
}

int finalize_clip_text(mmf_handle* h) {
  const std::string p = "clip.text_model.";
  CHK(load_f32(h, &h->t_tok, p + "embeddings.token_embedding.weight", (size_t)49408 * 512));
  CHK(load_f32(h, &h->t_pos, p + "embeddings.position_embedding.weight", 77 * 512));
  CHK(finalize_clip_layers(h, h->t_layers, p + "encoder.layers.", 512, 2048));
  CHK(load_ln(h, &h->t_final, p + "final_layer_norm", 512));
  GET(pw, "clip.text_projection.weight", (size_t)512 * 512);
  return up_f16(h, &h->t_proj, pw->f);
}

int finalize_fusion(mmf_handle* h) {
  CHK(load_f32(h, &h->f_w0, "fusion_layer.0.weight", 64 * 5));
  CHK(load_f32(h, &h->f_b0, "fusion_layer.0.bias", 64));
  CHK(load_f32(h, &h->f_w3, "fusion_layer.3.weight", 32 * 64));
  CHK(load_f32(h, &h->f_b3, "fusion_layer.3.bias", 32));
  CHK(load_f32(h, &h->f_w5, "fusion_layer.5.weight", 2 * 32));
  return load_f32(h, &h->f_b5, "fusion_layer.5.bias", 2);
}
