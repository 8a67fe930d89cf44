// C-ABI of libmmf_hip.so (include/mmf_hip.h): the extern "C" surface over the handle (handle.h) --
// options, workspaces, the fork/join of the towers and the profiling exports.  Host C++ over the HIP
// runtime; no torch types cross this ABI.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>

#include "handle.h"

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int free_group(mmf_handle* h, int group) {
  if (h->groups[group].empty()) return 0;
  HIPCHK(hipDeviceSynchronize());
  for (void* p : h->groups[group]) HIPCHK(hipFree(p));
  h->groups[group].clear();
  h->group_bytes[group] = 0;
  return 0;
}

int check_cap(mmf_handle* h, int B, int Lr, int Lc) {
  if (B <= 0) return fail(MMF_EINVAL, "batch must be > 0 (got %d)", B);
  if (B > h->cap_b || Lr > h->cap_lr || Lc > h->cap_lc)
    return fail(MMF_EINVAL, "shape B=%d Lr=%d Lc=%d exceeds reserved B=%d Lr=%d Lc=%d (call mmf_reserve)", B, Lr, Lc,
                h->cap_b, h->cap_lr, h->cap_lc);
  return 0;
}

namespace {

struct OptName { const char* name; int Options::*field; const char* env; };
const OptName kOptNames[] = {
    {"concurrent", &Options::concurrent, "MMF_CONCURRENT"},   {"fuse_stem", &Options::fuse_stem, "MMF_FUSE_STEM"},
    {"fuse_expand", &Options::fuse_expand, "MMF_FUSE_EXPAND"},
    {"gemm_splitk", &Options::gemm_splitk, "MMF_GEMM_SPLITK"}, {"gemm_config", &Options::gemm_config, "MMF_GEMM_CONFIG"},
    {"gemm_group_m", &Options::gemm_group_m, "MMF_GEMM_GROUPM"},
    {"text_hilo", &Options::text_hilo, "MMF_TEXT_HILO"}, {"text_prec_mask", &Options::text_prec_mask, "MMF_TEXT_PREC_MASK"},
    {"effnet_fp32", &Options::effnet_fp32, "MMF_EFFNET_FP32"},
    {"clip_res16", &Options::clip_res16, "MMF_CLIP_RES16"}, {"lazy_ln", &Options::lazy_ln, "MMF_LAZY_LN"},
    {"pw32_mfma", &Options::pw32_mfma, "MMF_PW32_MFMA"},
    {"effnet_chunks", &Options::effnet_chunks, "MMF_EFFNET_CHUNKS"}, {"dw_cw32", &Options::dw_cw32, "MMF_DW_CW32"},
    {"diag_skip", &Options::diag_skip, "MMF_DIAG_SKIP"}, {"qkv_attn", &Options::qkv_attn, "MMF_QKV_ATTN"},
    {"clip_qkv_attn", &Options::clip_qkv_attn, "MMF_CLIP_QKV_ATTN"},
    {"vault_ref", &Options::vault_ref, "MMF_VAULT_REF"}, {"vault_fused", &Options::vault_fused, "MMF_VAULT_FUSED"},
    {"mt_enqueue", &Options::mt_enqueue, "MMF_MT_ENQUEUE"}, {"last_q1", &Options::last_q1, "MMF_LAST_Q1"},
    {"after_text", &Options::after_text, "MMF_AFTER_TEXT"},
};
}  // namespace

Options& process_options() {
  static Options o = [] {
    Options d;
    for (const OptName& n : kOptNames) {
      const char* e = getenv(n.env);
      if (e && *e) d.*(n.field) = atoi(e);
    }
    return d;
  }();
  return o;
}

namespace {

const char* prof_kind_name(int k) {
  static const char* names[PK_COUNT - PK_ATTN] = {"attention", "layernorm", "embed+ln", "clip_im2col", "effnet_stem",
                                                  "dwconv", "se", "gap_classifier", "text_heads", "vault", "fusion",
                                                  "pw32"};
  static char gemm_names[PK_GEMM_LAST + 1][64];
  if (k >= 0 && k <= PK_GEMM_LAST) {
    if (!gemm_names[k][0]) {
      const int epi = (k / kGemmActs) % kGemmEpis;
      snprintf(gemm_names[k], sizeof(gemm_names[k]), epi ? "%s act=%d epi=%d" : "%s act=%d",
               gemm_config_name(k / (kGemmActs * kGemmEpis)), k % kGemmActs, epi);
    }
    return gemm_names[k];
  }
  return (k >= PK_ATTN && k < PK_COUNT) ? names[k - PK_ATTN] : "?";
}

// fork/join streams of the multi-tower entry points, created on first use
int ensure_towers(mmf_handle* h) {
  if (h->tower[0]) return 0;
  for (int i = 0; i < 3; ++i) {
    HIPCHK(hipStreamCreateWithFlags(&h->tower[i], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->join_ev[i], hipEventDisableTiming));
  }
  HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->text_ev, hipEventDisableTiming));
  return 0;
}

// the host threads of option mt_enqueue, started on first use
EnqueuePool& ensure_pool(mmf_handle* h) {
  if (!h->pool) h->pool.reset(new EnqueuePool(h->device));
  return *h->pool;
}

// The vault served by the fused similarity + top-k kernels (option vault_fused; top_k <= 8)
constexpr int kVaultChunk = 16384;  // rows the LDS sort kernel ranks at once (top_k > 8)
bool vault_is_fused(const mmf_handle* h) {
  return h->opt.vault_fused == 1 || (h->opt.vault_fused == 2 && h->vault_n > kVaultChunk);
}

// Top-k of q[B][512] against the handle's vault, behind mmf_vault_topk and both analysis tails.  Every
// path ranks bit-identical similarities under one total order, so the outputs do not depend on the path:
// the fused kernels (no similarity matrix), the similarity + top-k kernel pair over S[B][N], or, for
// top_k > 8 on more than 16384 rows, the pair per 16384-row chunk and a final sort of the chunks' k each.
// The workspaces were sized by ensure_sims (mmf_reserve, the vault setters, mmf_set_option).
int vault_search(mmf_handle* h, const float* q, int B, int k, const VaultOut& out, hipStream_t s) {
  Workspace& w = h->ws;
  const int N = h->vault_n, ref = h->opt.vault_ref;
  const char* unreserved = "vault search workspace not reserved (call mmf_reserve)";
  if (k <= 8 && vault_is_fused(h)) {
    if (!w.vs_ws) return fail(MMF_EINVAL, "%s", unreserved);
    HIPCHK(launch_vault_search(q, h->vault, B, N, k, out, w.vs_ws, 0, s));
    return 0;
  }
  if (k <= 8 || N <= kVaultChunk) {  // (the sort kernel of top_k > 8 holds at most kVaultChunk rows)
    if (w.s_cap_n < N) return fail(MMF_EINVAL, "%s", unreserved);
    HIPCHK(launch_vault_sims(q, h->vault, w.s_sims, B, N, 512, s, ref));
    HIPCHK(launch_vault_topk(w.s_sims, B, N, k, out, s, ref));
    return 0;
  }
  const int chunks = (N + kVaultChunk - 1) / kVaultChunk;
  if (k > 64 || (long long)chunks * k > kVaultChunk)
    return fail(MMF_EINVAL, "top_k = %d on a vault of %d rows: more than 16384 rows take top_k <= 64 and "
                            "ceil(N / 16384) * top_k <= 16384", k, N);
  if (w.s_cap_n < kVaultChunk || w.c_chunks < chunks) return fail(MMF_EINVAL, "%s", unreserved);
  for (int c = 0; c < chunks; ++c) {
    const int n = std::min(kVaultChunk, N - c * kVaultChunk);
    HIPCHK(launch_vault_sims(q, h->vault + (size_t)c * kVaultChunk * 512, w.s_sims, B, n, 512, s, ref));
    VaultOut part{};  // results only: the discrepancy and the caption similarity follow the final ranking
    part.sims = w.c_sims + (size_t)c * B * k;
    part.idx = w.c_idx + (size_t)c * B * k;
    HIPCHK(launch_vault_topk(w.s_sims, B, n, k, part, s, ref));
  }
  HIPCHK(launch_vault_sort_cand(w.c_sims, w.c_idx, chunks, kVaultChunk, B, k, out, s));
  return 0;
}

// after the towers joined: CLIP cosine, vault top-5, fusion (mmf_analyze_batch's last part)
int analyze_tail(mmf_handle* h, int B, float* scores5, float* text_sim, float* probs2, int32_t* verdict, float* conf,
                 int32_t* rule, float* top_sims, int32_t* top_idx, hipStream_t s) {
  Workspace& w = h->ws;
  HIPCHK(launch_rowdot(w.v_emb, w.t_emb, scores5 + 3, 5, B, 512, s));
  if (h->ready & RDY_VAULT) {
    ProfScope ps(h, s, PK_VAULT, 2.0 * B * h->vault_n * 512, (double)h->vault_n * 512 * 4 + (double)B * h->vault_n * 8);
    const VaultOut out{0.85f, top_sims, top_idx, scores5 + 4, 5, w.t_emb, h->vault_title, 512, text_sim};
    CHK(vault_search(h, w.v_emb, B, 5, out, s));
  } else {
    HIPCHK(launch_fill_strided(scores5 + 4, 5, B, 0.f, s));
    if (text_sim) HIPCHK(hipMemsetAsync(text_sim, 0, (size_t)B * 4, s));
    if (top_sims) HIPCHK(hipMemsetAsync(top_sims, 0, (size_t)B * 5 * 4, s));
    if (top_idx) HIPCHK(hipMemsetAsync(top_idx, 0xff, (size_t)B * 5 * 4, s));
  }
  ProfScope ps(h, s, PK_FUSION, 2.0 * B * (5 * 64 + 64 * 32 + 32 * 2), (double)B * (5 + 2 + 3) * 4);
  HIPCHK(launch_fusion(scores5, h->f_w0, h->f_b0, h->f_w3, h->f_b3, h->f_w5, h->f_b5, probs2, verdict, conf, rule, B,
                       s));
  return 0;
}

// The towers of one step: mmf_analyze_batch runs every tower on all B rows, mmf_analyze_mixed each on
// the rows that have its modality (a tower with no rows is not launched).  The ViT writes w.v_emb and
// the CLIP text tower w.t_emb; the text and EfficientNet scores go where the caller says.
struct TowerJobs {
  const int32_t *rob_ids, *rob_mask;  // [nT][Lr]
  int nT, Lr;
  float* text_scores;  // (ai, misinfo) at text_scores[r * text_stride + {0, 1}]
  int text_stride;
  const int32_t *clip_ids, *clip_mask;  // [nC][Lc]
  int nC, Lc;
  const uint8_t *img_eff, *img_clip;  // [nI][224][224][3]
  int nI;
  float* eff_scores;  // deepfake at eff_scores[r * eff_stride]
  int eff_stride;
};

// fork from stream s, run the towers side by side, join back into s.  B = the step's batch rows (it
// picks the enqueue form: host threads for B <= mt_enqueue, the event chain above it)
int run_towers(mmf_handle* h, const TowerJobs& j, int B, hipStream_t s) {
  Workspace& w = h->ws;
  // the per-kernel profiling pass runs the towers sequentially so event intervals are clean
  const int concurrent = h->opt.concurrent && !h->prof;
  if (concurrent) CHK(ensure_towers(h));
  // fork: the four towers only share read-only inputs and write disjoint workspaces/outputs
  hipStream_t st_text = s, st_eff = s, st_ctxt = s;
  if (concurrent) {
    HIPCHK(hipEventRecord(h->fork_ev, s));
    for (int i = 0; i < 3; ++i) HIPCHK(hipStreamWaitEvent(h->tower[i], h->fork_ev, 0));
    st_text = h->tower[0];
    st_eff = h->tower[1];
    st_ctxt = h->tower[2];
  }
  // diag_skip (diagnostic only, never set by the API or bench.py): towers left out to measure each
  // tower's marginal cost in the concurrent step (bit 1 text, 2 EfficientNet, 4 CLIP text, 8 ViT)
  const int skip = h->opt.diag_skip;
  const bool on_text = !(skip & 1) && j.nT > 0, on_ctxt = !(skip & 4) && j.nC > 0;
  const bool on_eff = !(skip & 2) && j.nI > 0, on_vit = !(skip & 8) && j.nI > 0;
  const int32_t *rob_ids = j.rob_ids, *rob_mask = j.rob_mask, *clip_ids = j.clip_ids, *clip_mask = j.clip_mask;
  const uint8_t *img_eff = j.img_eff, *img_clip = j.img_clip;
  const int nT = j.nT, Lr = j.Lr, nC = j.nC, Lc = j.Lc, nI = j.nI, text_stride = j.text_stride, eff_stride = j.eff_stride;
  float *text_scores = j.text_scores, *eff_scores = j.eff_scores;
  if (concurrent && h->opt.mt_enqueue > 0 && B <= h->opt.mt_enqueue) {
    // small batches: three host threads enqueue the text, CLIP-text and EfficientNet towers while
    // this thread enqueues the ViT, so every chain starts at once (each stream keeps its own order)
    EnqueuePool& pool = ensure_pool(h);
    float* t_emb = w.t_emb;
    const bool on[3] = {on_text, on_ctxt, on_eff};
    if (on[0]) pool.submit(0, [=] { return run_text(h, rob_ids, rob_mask, nT, Lr, nullptr, nullptr, text_scores, text_stride, st_text); });
    if (on[1]) pool.submit(1, [=] { return run_clip_text(h, clip_ids, clip_mask, nC, Lc, t_emb, st_ctxt); });
    if (on[2]) pool.submit(2, [=] { return run_effnet(h, img_eff, nullptr, nI, nullptr, eff_scores, eff_stride, st_eff, 0); });
    const int rc = on_vit ? run_clip_image(h, img_clip, nI, w.v_emb, s) : 0;
    int wrc = 0;
    std::string werr;  // the first failing worker's message (wait() writes it only on failure)
    for (int i = 0; i < 3; ++i) {
      if (!on[i]) continue;
      const int r = pool.wait(i, wrc ? nullptr : &werr);
      if (r && !wrc) wrc = r;
    }
    CHK(rc);
    if (wrc) return fail(wrc, "%s", werr.c_str());
  } else {
    // option after_text: the chosen towers' streams wait for the RoBERTa tower (its persistent GEMMs
    // then own every CU instead of sharing them with the other towers' launches)
    // (releasing them before RoBERTa's last layer or two, and EfficientNet chained behind a CLIP tower or
    // split over two streams, measured slower: DESIGN.md §1 round 5)
    const int after = concurrent && on_text ? h->opt.after_text : 0;
    if (on_text) CHK(run_text(h, rob_ids, rob_mask, nT, Lr, nullptr, nullptr, text_scores, text_stride, st_text, after ? h->text_ev : nullptr));
    if (after) {
      if (after & 2) HIPCHK(hipStreamWaitEvent(st_eff, h->text_ev, 0));
      if (after & 4) HIPCHK(hipStreamWaitEvent(st_ctxt, h->text_ev, 0));
      if (after & 8) HIPCHK(hipStreamWaitEvent(s, h->text_ev, 0));
    }
    if (on_ctxt) CHK(run_clip_text(h, clip_ids, clip_mask, nC, Lc, w.t_emb, st_ctxt));
    if (on_eff) CHK(run_effnet(h, img_eff, nullptr, nI, nullptr, eff_scores, eff_stride, st_eff));
    if (on_vit) CHK(run_clip_image(h, img_clip, nI, w.v_emb, s));
  }
  if (concurrent) {
    for (int i = 0; i < 3; ++i) {
      HIPCHK(hipEventRecord(h->join_ev[i], h->tower[i]));
      HIPCHK(hipStreamWaitEvent(s, h->join_ev[i], 0));
    }
  }
  return 0;
}

// after the towers of mmf_analyze_mixed joined: vault top-5 of the nI image rows into the compact
// workspaces, then the finish kernel (gather, cosines, scatter, fusion or single-modality verdict)
int mixed_tail(mmf_handle* h, const int32_t* row_map, int B, int nT, int nI, int nC, float* scores5, float* text_sim,
               float* probs2, int32_t* verdict, float* conf, int32_t* rule, float* top_sims, int32_t* top_idx,
               hipStream_t s) {
  Workspace& w = h->ws;
  const bool vault = nI > 0 && (h->ready & RDY_VAULT);
  if (vault) {
    ProfScope ps(h, s, PK_VAULT, 2.0 * nI * h->vault_n * 512, (double)h->vault_n * 512 * 4 + (double)nI * h->vault_n * 8);
    VaultOut out{};  // (the caption similarity is the finish kernel's: it knows which rows have a caption)
    out.thresh = 0.85f;
    out.sims = w.m_sims; out.idx = w.m_idx;
    out.disc = w.m_disc; out.disc_stride = 1;
    CHK(vault_search(h, w.v_emb, nI, 5, out, s));
  }
  MixedFinishArgs a{};
  a.row_map = row_map;
  a.B = B; a.nT = nT; a.nI = nI; a.nC = nC;
  a.text2 = w.m_text;
  a.deepfake = w.m_eff;
  a.v_emb = w.v_emb;
  a.t_emb = w.t_emb;
  if (vault) { a.c_sims = w.m_sims; a.c_idx = w.m_idx; a.c_disc = w.m_disc; a.title = h->vault_title; }
  a.thresh = 0.85f;
  if (nC > 0) { a.w0 = h->f_w0; a.b0 = h->f_b0; a.w3 = h->f_w3; a.b3 = h->f_b3; a.w5 = h->f_w5; a.b5 = h->f_b5; }
  a.scores5 = scores5; a.text_sim = text_sim; a.probs = probs2;
  a.verdict = verdict; a.conf = conf; a.rule = rule;
  a.top_sims = top_sims; a.top_idx = top_idx;
  ProfScope ps(h, s, PK_FUSION, 2.0 * nC * (5 * 64 + 64 * 32 + 32 * 2 + 2 * 512), (double)B * (3 + 5 + 2 + 3 + 10) * 4);
  HIPCHK(launch_mixed_finish(a, s));
  return 0;
}


// Workspaces of the precision modes, allocated while the mode is selected and freed when it is left
// (mmf_reserve, mmf_set_option, mmf_finalize) -- never from inside a launch sequence, which worker
// threads may be enqueueing (option mt_enqueue): the fp32 EfficientNet tower (effnet_fp32, ~10 MB per
// image) and the RoBERTa precise mode (text_hilo = 2, 40 KB per token row).
int ensure_mode_ws(mmf_handle* h) {
  if (!h->cap_b) return 0;
  Workspace& w = h->ws;
  const size_t rows = (size_t)h->cap_b * h->cap_lr;
  if (text_mode(h) >= 2) {
    if (w.t32_rows < rows) {
      CHK(free_group(h, AG_TEXT32));
      CHK(dev_alloc(h, &w.p32, rows * 3072, AG_TEXT32));
      CHK(dev_alloc(h, &w.s3, rows * 2304, AG_TEXT32));
      CHK(dev_alloc(h, &w.h3, rows * 9216, AG_TEXT32));
      w.t32_rows = rows;
    }
  } else if (w.t32_rows) {
    CHK(free_group(h, AG_TEXT32));
    w.p32 = nullptr;
    w.s3 = w.h3 = nullptr;
    w.t32_rows = 0;
  }
  if (h->opt.effnet_fp32) {
    if (w.e32_cap_b < h->cap_b) {
      CHK(free_group(h, AG_EFF32));
      const EffSizes es = eff_sizes();
      const size_t nb = (size_t)h->cap_b;
      CHK(dev_alloc(h, &w.e32_a, nb * es.io, AG_EFF32));
      CHK(dev_alloc(h, &w.e32_b, nb * es.io, AG_EFF32));
      CHK(dev_alloc(h, &w.e32_exp, nb * es.exp, AG_EFF32));
      CHK(dev_alloc(h, &w.e32_dw, nb * es.dw, AG_EFF32));
      w.e32_cap_b = h->cap_b;
    }
  } else if (w.e32_cap_b) {
    CHK(free_group(h, AG_EFF32));
    w.e32_a = w.e32_b = w.e32_exp = w.e32_dw = nullptr;
    w.e32_cap_b = 0;
  }
  return 0;
}

// The vault search workspaces (group AG_SIMS) for the reserved batch, the vault and option vault_fused,
// set up outside any launch sequence (mmf_reserve, the vault setters, mmf_set_option).  A vault that is
// served fused needs no S[cap_b][N]: it gets the candidate workspace, and above 16384 rows one chunk
// of S plus the per-chunk results for top_k > 8 -- none of which grows with N (the chunk results: 512
// bytes per query and 16384 rows).
int ensure_sims(mmf_handle* h) {
  if (!h->vault_n || !h->cap_b) return 0;
  Workspace& w = h->ws;
  const int N = h->vault_n;
  const bool fused = vault_is_fused(h), large = N > kVaultChunk;
  const int need_n = fused && large ? kVaultChunk : N;
  const int need_chunks = large ? (N + kVaultChunk - 1) / kVaultChunk : 0;
  if (w.s_cap_n == need_n && (w.vs_ws != nullptr) == fused && w.c_chunks == need_chunks) return 0;
  CHK(free_group(h, AG_SIMS));
  w.s_sims = nullptr; w.vs_ws = nullptr; w.c_sims = nullptr; w.c_idx = nullptr;
  w.s_cap_n = w.c_chunks = 0;
  CHK(dev_alloc(h, &w.s_sims, (size_t)h->cap_b * need_n, AG_SIMS));
  w.s_cap_n = need_n;
  if (fused) {
    uint8_t* p;
    CHK(dev_alloc(h, &p, vault_search_ws_bytes(h->cap_b, 8, 0), AG_SIMS));
    w.vs_ws = p;
  }
  if (need_chunks) {
    CHK(dev_alloc(h, &w.c_sims, (size_t)need_chunks * h->cap_b * 64, AG_SIMS));
    CHK(dev_alloc(h, &w.c_idx, (size_t)need_chunks * h->cap_b * 64, AG_SIMS));
    w.c_chunks = need_chunks;
  }
  return 0;
}

int set_vault_rows(mmf_handle* h, std::vector<float>& u, int N) {
  h->ready &= ~RDY_VAULT;
  CHK(free_group(h, AG_TITLES));  // titles belong to the previous vault
  h->vault_title = nullptr;
  CHK(free_group(h, AG_VAULT));
  h->cur_group = AG_VAULT;
  CHK(up_f32(h, &h->vault, u));
  h->vault_n = N;
  h->ready |= RDY_VAULT;
  h->ws.s_cap_n = 0;
  return ensure_sims(h);
}

}  // namespace

// =============================================================================================
extern "C" {

const char* mmf_last_error(void) { return g_err.c_str(); }
const char* mmf_version(void) { return "mmf_hip 0.1.0 gfx950"; }

int mmf_create(int device, mmf_handle** out) {
  if (!out) return fail(MMF_EINVAL, "out is NULL");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(MMF_EINVAL, "device %d out of range (%d devices)", device, n);
  HIPCHK(hipSetDevice(device));
  mmf_handle* h = new (std::nothrow) mmf_handle();
  if (!h) return fail(MMF_ENOMEM, "out of host memory");
  h->device = device;
  h->opt = process_options();
  *out = h;
  g_err.clear();
  return 0;
}

void mmf_destroy(mmf_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

int mmf_load_tensor(mmf_handle* h, const char* name, int dtype, int ndim, const int64_t* shape, const void* data) {
  if (!h || !name || (!data && ndim > 0) || ndim < 0 || ndim > 8) return fail(MMF_EINVAL, "bad argument");
  HostT t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(MMF_EINVAL, "negative dim in '%s'", name);
    t.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  if (dtype == MMF_DTYPE_I64) return 0;  // integer buffers (num_batches_tracked) carry no arithmetic
  if (dtype != MMF_DTYPE_F32) return fail(MMF_EINVAL, "unsupported dtype %d for '%s'", dtype, name);
  t.f.resize(n);
  if (n) std::memcpy(t.f.data(), data, n * sizeof(float));
  h->staged[name] = std::move(t);
  return 0;
}

int mmf_finalize(mmf_handle* h, int clip_eos_token_id) {
  if (!h) return fail(MMF_EINVAL, "null handle");
  HIPCHK(hipSetDevice(h->device));
  h->eos_id = clip_eos_token_id;
  int ready = h->ready;  // incremental: components not re-staged keep their packed weights
  std::string missing;
  // a re-staged component replaces its packed weights: its previous buffers are freed first
  auto attempt = [&](int bit, int group, const char* key, int (*fn)(mmf_handle*)) -> int {
    if (!h->staged.count(key)) return 0;
    ready &= ~bit;
    h->ready = ready;
    CHK(free_group(h, group));
    h->cur_group = group;
    int r = fn(h);
    if (r) return r;
    ready |= bit;
    return 0;
  };
  CHK(attempt(RDY_TEXT, AG_TEXT, "roberta.embeddings.word_embeddings.weight", finalize_text));
  CHK(attempt(RDY_EFFNET, AG_EFF, "efficientnet.features.0.0.weight", finalize_effnet));
  CHK(attempt(RDY_VISION, AG_VIS, "clip.vision_model.embeddings.patch_embedding.weight", finalize_clip_vision));
  CHK(attempt(RDY_CTEXT, AG_CTEXT, "clip.text_model.embeddings.token_embedding.weight", finalize_clip_text));
  CHK(attempt(RDY_FUSION, AG_FUSION, "fusion_layer.0.weight", finalize_fusion));
  h->ready = ready;
  h->staged.clear();
  HIPCHK(hipDeviceSynchronize());
  return ensure_mode_ws(h);
}

int mmf_ready(mmf_handle* h) { return h ? h->ready : 0; }

int mmf_reserve(mmf_handle* h, int B, int Lr, int Lc) {
  if (!h || B <= 0 || Lr <= 0 || Lr > 512 || Lc <= 0 || Lc > 77)
    return fail(MMF_EINVAL, "mmf_reserve: bad shape B=%d Lr=%d Lc=%d", B, Lr, Lc);
  HIPCHK(hipSetDevice(h->device));
  CHK(free_group(h, AG_WS));
  CHK(free_group(h, AG_SIMS));
  CHK(free_group(h, AG_EFF32));
  CHK(free_group(h, AG_TEXT32));
  h->ws = Workspace();
  h->cap_b = h->cap_lr = h->cap_lc = 0;
  Workspace& w = h->ws;
  auto A = [&](auto** p, size_t count) { return dev_alloc(h, p, count, AG_WS); };
  const size_t nb = (size_t)B, Mr = nb * Lr, Mv = nb * 50, Mt = nb * Lc;
  for (float** p : {&w.r_x, &w.r_y}) CHK(A(p, Mr * 768));
  CHK(A(&w.r_xb, Mr * 768));
  CHK(A(&w.r_lo, Mr * 768));
  CHK(A(&w.r_ovf, nb));
  CHK(A(&w.r_qkv, Mr * 2304));
  CHK(A(&w.r_ctx, Mr * 768));
  CHK(A(&w.r_h, Mr * 3072));
  CHK(A(&w.v_col, nb * 49 * 3072));
  CHK(A(&w.v_patch, nb * 49 * 768));
  CHK(A(&w.v_x, Mv * 768));  // (fp32 elements: the fp16 stream of option clip_res16 uses half of it)
  CHK(A(&w.v_xb, Mv * 768));
  CHK(A(&w.v_qkv, Mv * 2304));
  CHK(A(&w.v_ctx, Mv * 768));
  CHK(A(&w.v_h, Mv * 3072));
  CHK(A(&w.v_cls, nb * 768));
  CHK(A(&w.v_emb, nb * 512));
  CHK(A(&w.t_x, Mt * 512));
  CHK(A(&w.t_xb, Mt * 512));
  CHK(A(&w.t_qkv, Mt * 1536));
  CHK(A(&w.t_ctx, Mt * 512));
  CHK(A(&w.t_h, Mt * 2048));
  CHK(A(&w.t_pool, nb * 512));
  CHK(A(&w.t_emb, nb * 512));
  CHK(A(&w.t_eos, nb));
  CHK(A(&w.v_xc, nb * 768));
  CHK(A(&w.v_ctxc, nb * 768));
  CHK(A(&w.t_xc, nb * 512));
  CHK(A(&w.t_ctxc, nb * 512));
  auto stats_rows = [](size_t rows) { return (rows + 255) / 256 * 256 * kLnP; };  // float2 partials
  for (int i = 0; i < 2; ++i) {
    CHK(A(&w.v_st[i], stats_rows(Mv)));
    CHK(A(&w.t_st[i], stats_rows(Mt)));
  }
  // max over the skinny-M GEMMs (compact last layers: B rows; whole encoders of small batches: up to
  // the 512 rows gemm_config sends to the split-K path) of (K / 256) * N = 9216 per row
  w.sk_elems = (size_t)std::max(B, 512) * 9216;
  for (float** sk : {&w.sk_text, &w.sk_vit, &w.sk_ctext}) CHK(A(sk, w.sk_elems));
  // EfficientNet activation sizes per image
  const EffSizes es = eff_sizes();
  for (f16_t** p : {&w.e_a, &w.e_b}) CHK(A(p, nb * es.io));
  CHK(A(&w.e_exp, nb * es.exp));
  CHK(A(&w.e_dw, nb * es.dw));
  CHK(A(&w.e_pool, nb * es.pool));
  CHK(A(&w.e_scale, nb * 1280));
  CHK(A(&w.m_text, nb * 2));
  CHK(A(&w.m_eff, nb));
  CHK(A(&w.m_sims, nb * 5));
  CHK(A(&w.m_idx, nb * 5));
  CHK(A(&w.m_disc, nb));
  h->cap_b = B;
  h->cap_lr = Lr;
  h->cap_lc = Lc;
  CHK(ensure_sims(h));
  return ensure_mode_ws(h);
}

int mmf_text_forward(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* ai, float* mi,
                     float* scores2, void* stream) {
  if (!h || !ids || !mask) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_TEXT)) return fail(MMF_EINVAL, "text model (RoBERTa + heads) not loaded");
  if (L > 512) return fail(MMF_EINVAL, "RoBERTa length %d > 512 (position table ends at 514)", L);
  CHK(check_cap(h, B, L, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_text(h, ids, mask, B, L, ai, mi, scores2, 2, (hipStream_t)stream);
}

int mmf_text_pooled(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* cls, void* stream) {
  if (!h || !ids || !mask || !cls) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_TEXT)) return fail(MMF_EINVAL, "text model (RoBERTa + heads) not loaded");
  if (L < 1 || L > 512) return fail(MMF_EINVAL, "RoBERTa length %d outside 1..512 (position table ends at 514)", L);
  if ((uintptr_t)cls & 15) return fail(MMF_EINVAL, "text_pooled: cls must be 16-byte aligned");
  CHK(check_cap(h, B, L, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_text(h, ids, mask, B, L, nullptr, nullptr, nullptr, 2, (hipStream_t)stream, nullptr, cls);
}

int mmf_effnet_forward(mmf_handle* h, const uint8_t* img, int B, float* logits, float* score, void* stream) {
  if (!h || !img) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_EFFNET)) return fail(MMF_EINVAL, "EfficientNet not loaded");
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  const hipStream_t s = (hipStream_t)stream;
  // option effnet_chunks: the batch split into that many image chunks on concurrent streams (each
  // chunk's kernels fill the other's launch tails; per-image results are unchanged: every layer is
  // per image, and the GEMM rows do not depend on M)
  const int nc = std::min(std::max(h->opt.effnet_chunks, 1), 4);
  if (nc == 1 || B < 32 * nc) return run_effnet(h, img, nullptr, B, logits, score, 1, s);
  CHK(ensure_towers(h));
  HIPCHK(hipEventRecord(h->fork_ev, s));
  int b0 = 0;
  for (int c = 0; c < nc; ++c) {
    const int bc = B / nc + (c < B % nc ? 1 : 0);
    const hipStream_t cs = c ? h->tower[c - 1] : s;
    if (c) HIPCHK(hipStreamWaitEvent(cs, h->fork_ev, 0));
    CHK(run_effnet(h, img + (size_t)b0 * 224 * 224 * 3, nullptr, bc, logits ? logits + (size_t)b0 * 2 : nullptr,
                   score ? score + b0 : nullptr, 1, cs, b0));
    b0 += bc;
  }
  for (int c = 1; c < nc; ++c) {
    HIPCHK(hipEventRecord(h->join_ev[c - 1], h->tower[c - 1]));
    HIPCHK(hipStreamWaitEvent(s, h->join_ev[c - 1], 0));
  }
  return 0;
}

int mmf_effnet_forward_f32(mmf_handle* h, const float* x, int B, float* logits, float* score, void* stream) {
  if (!h || !x) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_EFFNET)) return fail(MMF_EINVAL, "EfficientNet not loaded");
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_effnet(h, nullptr, x, B, logits, score, 1, (hipStream_t)stream);
}

int mmf_clip_image(mmf_handle* h, const uint8_t* img, int B, float* emb, void* stream) {
  if (!h || !img || !emb) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_VISION)) return fail(MMF_EINVAL, "CLIP vision tower not loaded");
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_clip_image(h, img, B, emb, (hipStream_t)stream);
}

int mmf_clip_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* emb, void* stream) {
  if (!h || !ids || !mask || !emb) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_CTEXT)) return fail(MMF_EINVAL, "CLIP text tower not loaded");
  if (L > 77) return fail(MMF_EINVAL, "CLIP text length %d > 77", L);
  CHK(check_cap(h, B, 1, L));
  HIPCHK(hipSetDevice(h->device));
  return run_clip_text(h, ids, mask, B, L, emb, (hipStream_t)stream);
}

int mmf_clip_consistency(mmf_handle* h, const uint8_t* img, const int32_t* ids, const int32_t* mask, int B, int L,
                         float* img_emb, float* txt_emb, float* sim, void* stream) {
  if (!h || !img || !ids || !mask || !sim) return fail(MMF_EINVAL, "null argument");
  if ((h->ready & RDY_CLIP) != RDY_CLIP) return fail(MMF_EINVAL, "CLIP towers not loaded");
  if (L > 77) return fail(MMF_EINVAL, "CLIP text length %d > 77", L);
  CHK(check_cap(h, B, 1, L));
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  float* ie = img_emb ? img_emb : h->ws.v_emb;
  float* te = txt_emb ? txt_emb : h->ws.t_emb;
  CHK(ensure_towers(h));
  const int concurrent = h->opt.concurrent && !h->prof;
  hipStream_t st = s;
  if (concurrent) {  // the text tower beside the vision tower (disjoint workspaces)
    HIPCHK(hipEventRecord(h->fork_ev, s));
    HIPCHK(hipStreamWaitEvent(h->tower[2], h->fork_ev, 0));
    st = h->tower[2];
  }
  if (concurrent && h->opt.mt_enqueue > 0 && B <= h->opt.mt_enqueue) {  // as in mmf_analyze_batch
    EnqueuePool& pool = ensure_pool(h);
    pool.submit(1, [=] { return run_clip_text(h, ids, mask, B, L, te, st); });
    const int rc = run_clip_image(h, img, B, ie, s);
    std::string e;
    const int wrc = pool.wait(1, &e);
    CHK(rc);
    if (wrc) return fail(wrc, "%s", e.c_str());
  } else {
    CHK(run_clip_text(h, ids, mask, B, L, te, st));
    CHK(run_clip_image(h, img, B, ie, s));
  }
  if (concurrent) {
    HIPCHK(hipEventRecord(h->join_ev[2], h->tower[2]));
    HIPCHK(hipStreamWaitEvent(s, h->join_ev[2], 0));
  }
  HIPCHK(launch_rowdot(ie, te, sim, 1, B, 512, s));
  return 0;
}

int mmf_clip_pooled(mmf_handle* h, const uint8_t* img, const int32_t* ids, const int32_t* mask, int B, int L,
                    float* img_pooled, float* txt_pooled, void* stream) {
  if (!h || (img_pooled && !img) || (txt_pooled && (!ids || !mask))) return fail(MMF_EINVAL, "null argument");
  const int need = (img_pooled ? RDY_VISION : 0) | (txt_pooled ? RDY_CTEXT : 0);
  if ((h->ready & need) != need) return fail(MMF_EINVAL, "CLIP towers not loaded");
  if (!txt_pooled) L = 1;
  if (L < 1 || L > 77) return fail(MMF_EINVAL, "CLIP text length %d outside 1..77", L);
  CHK(check_cap(h, B, 1, L));
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!img_pooled || !txt_pooled) {
    if (img_pooled) return run_clip_image_pooled(h, img, B, img_pooled, s);
    if (txt_pooled) return run_clip_text_pooled(h, ids, mask, B, L, txt_pooled, s);
    return 0;
  }
  CHK(ensure_towers(h));
  const int concurrent = h->opt.concurrent && !h->prof;
  hipStream_t st = s;
  if (concurrent) {  // the text tower beside the vision tower, as the consistency call
    HIPCHK(hipEventRecord(h->fork_ev, s));
    HIPCHK(hipStreamWaitEvent(h->tower[2], h->fork_ev, 0));
    st = h->tower[2];
  }
  CHK(run_clip_text_pooled(h, ids, mask, B, L, txt_pooled, st));
  CHK(run_clip_image_pooled(h, img, B, img_pooled, s));
  if (concurrent) {
    HIPCHK(hipEventRecord(h->join_ev[2], h->tower[2]));
    HIPCHK(hipStreamWaitEvent(s, h->join_ev[2], 0));
  }
  return 0;
}

int mmf_set_clip_projections(mmf_handle* h, const float* visual_f32, const float* text_f32, void* stream) {
  if (!h) return fail(MMF_EINVAL, "null argument");
  const int need = (visual_f32 ? RDY_VISION : 0) | (text_f32 ? RDY_CTEXT : 0);
  if ((h->ready & need) != need || (visual_f32 && !h->v_proj) || (text_f32 && !h->t_proj))
    return fail(MMF_EINVAL, "CLIP towers not loaded");
  if (((uintptr_t)visual_f32 | (uintptr_t)text_f32) & 15) return fail(MMF_EINVAL, "projections must be 16-byte aligned");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (visual_f32) HIPCHK(launch_f32_to_f16(visual_f32, h->v_proj, (size_t)512 * 768, s));
  if (text_f32) HIPCHK(launch_f32_to_f16(text_f32, h->t_proj, (size_t)512 * 512, s));
  return 0;
}

int64_t mmf_clip_train_ws_bytes(int batch) { return (int64_t)clip_train_ws_bytes(batch); }

namespace {
// the trainer entry points' shared checks: 0, or MMF_EINVAL with `what` in front
int check_ws(const char* what, int64_t ws_bytes, size_t need) {
  if (ws_bytes >= (int64_t)need) return 0;
  return fail(MMF_EINVAL, "%s: ws of %lld bytes, %lld needed", what, (long long)ws_bytes, (long long)need);
}
// every pointer of ps on an `align`-byte boundary, the dropout masks (has_keep) on an 8-byte one; null pointers pass
int check_aligned(const char* what, int align, std::initializer_list<const void*> ps, bool has_keep = false,
                  const void* keep = nullptr) {
  uintptr_t a = 0;
  for (const void* p : ps) a |= (uintptr_t)p;
  if (!(a & (uintptr_t)(align - 1)) && !((uintptr_t)keep & 7)) return 0;
  return fail(MMF_EINVAL, "%s: pointers must be %d-byte aligned%s", what, align, has_keep ? " (keep: 8)" : "");
}
}  // namespace

int mmf_clip_train_epoch(const float* img_feat, const float* txt_feat, int N, const int32_t* perm, int batch,
                         double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                         int step0, float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                         float* step_gnorm, float* grad_out, void* ws, int64_t ws_bytes, void* stream) {
  if (!img_feat || !txt_feat || !perm || !params || !exp_avg || !exp_avg_sq || !step_loss || !step_gnorm || !ws)
    return fail(MMF_EINVAL, "null argument");
  if (N < 1 || batch < 1 || batch > 64 || step0 < 0)
    return fail(MMF_EINVAL, "clip_train_epoch: N=%d (>= 1) batch=%d (1..64) step0=%d (>= 0)", N, batch, step0);
  CHK(check_ws("clip_train_epoch", ws_bytes, clip_train_ws_bytes(batch)));
  CHK(check_aligned("clip_train_epoch", 16, {img_feat, txt_feat, params, exp_avg, exp_avg_sq, grad_out, ws}));
  HIPCHK(launch_clip_train_epoch(img_feat, txt_feat, N, perm, batch, lr, beta1, beta2, eps, weight_decay, max_norm,
                                 step0, params, exp_avg, exp_avg_sq, step_loss, step_gnorm, grad_out, (float*)ws,
                                 (hipStream_t)stream));
  return 0;
}

int mmf_clip_contrastive_eval(const float* img_feat, const float* txt_feat, int N, int batch, const float* params,
                              float* batch_loss, float* row_cos, void* ws, int64_t ws_bytes, void* stream) {
  if (!img_feat || !txt_feat || !params || !batch_loss || !row_cos || !ws) return fail(MMF_EINVAL, "null argument");
  if (N < 1 || batch < 1 || batch > 64)
    return fail(MMF_EINVAL, "clip_contrastive_eval: N=%d (>= 1) batch=%d (1..64)", N, batch);
  CHK(check_ws("clip_contrastive_eval", ws_bytes, clip_train_ws_bytes(batch)));
  CHK(check_aligned("clip_contrastive_eval", 16, {img_feat, txt_feat, params, ws}));
  HIPCHK(launch_clip_contrastive_eval(img_feat, txt_feat, N, batch, params, batch_loss, row_cos, (float*)ws,
                                      (hipStream_t)stream));
  return 0;
}

int64_t mmf_clip_train_trials_ws_bytes(int trials, int batch_max) {
  return (int64_t)clip_train_trials_ws_bytes(trials, batch_max);
}

namespace {
static_assert(kClipTrialsMax == MMF_CLIP_TRIALS_MAX && kClipTrialStride == MMF_CLIP_TRIAL_STRIDE, "header and kernels");
// the trial calls' shared checks: the trial count, N, every active trial's batch (and step0 where given), and that
// `stride` rows of output hold every active trial's ceil(N / batch)
int check_trials(const char* what, int N, int trials, const int32_t* batch, const int32_t* step0, const int32_t* active,
                 int stride) {
  if (trials < 1 || trials > MMF_CLIP_TRIALS_MAX || N < 1)
    return fail(MMF_EINVAL, "%s: trials=%d (1..%d) N=%d (>= 1)", what, trials, MMF_CLIP_TRIALS_MAX, N);
  for (int t = 0; t < trials; ++t) {
    if (active && !active[t]) continue;
    if (batch[t] < 1 || batch[t] > 64 || (step0 && step0[t] < 0))
      return fail(MMF_EINVAL, "%s: trial %d: batch=%d (1..64) step0=%d (>= 0)", what, t, batch[t], step0 ? step0[t] : 0);
    if ((N + batch[t] - 1) / batch[t] > stride)
      return fail(MMF_EINVAL, "%s: trial %d has %d steps, the outputs' rows hold %d", what, t,
                  (N + batch[t] - 1) / batch[t], stride);
  }
  return 0;
}
}  // namespace

int mmf_clip_train_epoch_trials(const float* img_feat, const float* txt_feat, int N, int trials, const int32_t* perm,
                                const int32_t* batch, const double* lr, const double* weight_decay,
                                const double* max_norm, const int32_t* step0, const int32_t* active, double beta1,
                                double beta2, double eps, float* params, float* exp_avg, float* exp_avg_sq,
                                float* step_loss, float* step_gnorm, int max_nsteps, void* ws, int64_t ws_bytes,
                                void* stream) {
  if (!img_feat || !txt_feat || !perm || !batch || !lr || !weight_decay || !max_norm || !step0 || !params || !exp_avg ||
      !exp_avg_sq || !step_loss || !step_gnorm || !ws)
    return fail(MMF_EINVAL, "null argument");
  CHK(check_trials("clip_train_epoch_trials", N, trials, batch, step0, active, max_nsteps));
  CHK(check_ws("clip_train_epoch_trials", ws_bytes, clip_train_trials_ws_bytes(trials, 64)));
  CHK(check_aligned("clip_train_epoch_trials", 16, {img_feat, txt_feat, params, exp_avg, exp_avg_sq, ws}));
  HIPCHK(launch_clip_train_epoch_trials(img_feat, txt_feat, N, trials, perm, batch, lr, weight_decay, max_norm, step0,
                                        active, beta1, beta2, eps, params, exp_avg, exp_avg_sq, step_loss, step_gnorm,
                                        max_nsteps, nullptr, (float*)ws, (hipStream_t)stream));
  return 0;
}

int mmf_clip_contrastive_eval_trials(const float* img_feat, const float* txt_feat, int N, int trials,
                                     const int32_t* batch, const int32_t* active, const float* params,
                                     float* batch_loss, float* row_cos, int max_nb, void* ws, int64_t ws_bytes,
                                     void* stream) {
  if (!img_feat || !txt_feat || !batch || !params || !batch_loss || !row_cos || !ws)
    return fail(MMF_EINVAL, "null argument");
  CHK(check_trials("clip_contrastive_eval_trials", N, trials, batch, nullptr, active, max_nb));
  CHK(check_ws("clip_contrastive_eval_trials", ws_bytes, clip_train_trials_ws_bytes(trials, 64)));
  CHK(check_aligned("clip_contrastive_eval_trials", 16, {img_feat, txt_feat, params, ws}));
  HIPCHK(launch_clip_contrastive_eval_trials(img_feat, txt_feat, N, trials, batch, active, params, batch_loss, row_cos,
                                             max_nb, (float*)ws, (hipStream_t)stream));
  return 0;
}

int64_t mmf_head_train_ws_bytes(int batch) { return (int64_t)head_train_ws_bytes(batch); }

int mmf_head_train_epoch(const float* feat, const int32_t* labels, int N, const int32_t* perm, const uint64_t* keep,
                         float p_drop, int batch, const double* lr_steps, double beta1, double beta2, double eps,
                         double weight_decay, double max_norm, int step0, float* params, float* exp_avg,
                         float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* step_gnorm, float* grad_out,
                         void* ws, int64_t ws_bytes, void* stream) {
  if (!feat || !labels || !perm || !lr_steps || !params || !exp_avg || !exp_avg_sq || !step_loss || !step_correct ||
      !step_gnorm || !ws)
    return fail(MMF_EINVAL, "null argument");
  if (N < 1 || batch < 1 || batch > 64 || step0 < 0 || !(p_drop >= 0.f && p_drop < 1.f))
    return fail(MMF_EINVAL, "head_train_epoch: N=%d (>= 1) batch=%d (1..64) step0=%d (>= 0) p_drop=%g ([0, 1))", N,
                batch, step0, (double)p_drop);
  CHK(check_ws("head_train_epoch", ws_bytes, head_train_ws_bytes(batch)));
  CHK(check_aligned("head_train_epoch", 16, {feat, params, exp_avg, exp_avg_sq, grad_out, ws}, true, keep));
  HIPCHK(launch_head_train_epoch(feat, labels, N, perm, keep, p_drop, batch, lr_steps, beta1, beta2, eps, weight_decay,
                                 max_norm, step0, params, exp_avg, exp_avg_sq, step_loss, step_correct, step_gnorm,
                                 grad_out, (float*)ws, (hipStream_t)stream));
  return 0;
}

int mmf_head_eval(const float* feat, const int32_t* labels, int N, int batch, const float* params, float* batch_loss,
                  float* row_logits, void* ws, int64_t ws_bytes, void* stream) {
  if (!feat || !labels || !params || !batch_loss || !row_logits || !ws) return fail(MMF_EINVAL, "null argument");
  if (N < 1 || batch < 1 || batch > 64) return fail(MMF_EINVAL, "head_eval: N=%d (>= 1) batch=%d (1..64)", N, batch);
  CHK(check_ws("head_eval", ws_bytes, head_train_ws_bytes(batch)));
  CHK(check_aligned("head_eval", 16, {feat, params, ws}));
  HIPCHK(launch_head_eval(feat, labels, N, batch, params, batch_loss, row_logits, (float*)ws, (hipStream_t)stream));
  return 0;
}

int mmf_effnet_pooled(mmf_handle* h, const uint8_t* img, int B, float* pooled, void* stream) {
  if (!h || !img || !pooled) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_EFFNET)) return fail(MMF_EINVAL, "EfficientNet not loaded");
  if ((uintptr_t)pooled & 15) return fail(MMF_EINVAL, "effnet_pooled: pooled must be 16-byte aligned");
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_effnet(h, img, nullptr, B, nullptr, nullptr, 1, (hipStream_t)stream, 0, pooled);
}

int mmf_effnet_trunk(mmf_handle* h, const uint8_t* img, int B, float* trunk, void* stream) {
  if (!h || !img || !trunk) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_EFFNET)) return fail(MMF_EINVAL, "EfficientNet not loaded");
  if ((uintptr_t)trunk & 15) return fail(MMF_EINVAL, "effnet_trunk: trunk must be 16-byte aligned");
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  return run_effnet(h, img, nullptr, B, nullptr, nullptr, 1, (hipStream_t)stream, 0, nullptr, trunk);
}

int mmf_hflip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, void* stream) {
  if (!src || !dst) return fail(MMF_EINVAL, "null argument");
  if (B < 1 || H < 1 || W < 1 || C < 1 || (double)B * H * W >= 549755813888.0 /* 2^39 pixels: the grid */)
    return fail(MMF_EINVAL, "hflip_u8: bad shape (B=%d H=%d W=%d C=%d)", B, H, W, C);
  if (dst == src) return fail(MMF_EINVAL, "hflip_u8: dst must not be src");
  HIPCHK(launch_hflip_u8(src, dst, B, H, W, C, (hipStream_t)stream));
  return 0;
}

static_assert(kJitterChunks == MMF_JITTER_CHUNKS, "header and kernels");
int mmf_color_jitter_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ops, const float* factors,
                        const int32_t* hue_shift, uint64_t* ws, void* stream) {
  if (!src || !dst || !ops || !factors || !hue_shift || !ws) return fail(MMF_EINVAL, "null argument");
  if (B < 1 || B > kJitterMaxBatch || H < 1 || W < 1 || (double)H * W > (double)kJitterMaxPixels)
    return fail(MMF_EINVAL, "color_jitter_u8: bad shape (B=%d (1..%d) H=%d W=%d (H*W <= 2^40))", B, kJitterMaxBatch, H,
                W);
  if (dst == src) return fail(MMF_EINVAL, "color_jitter_u8: dst must not be src");
  if ((((uintptr_t)ops | (uintptr_t)factors | (uintptr_t)hue_shift) & 3) || ((uintptr_t)ws & 7))
    return fail(MMF_EINVAL, "color_jitter_u8: ops, factors and hue_shift must be 4-byte aligned, ws 8-byte");
  HIPCHK(launch_color_jitter_u8(src, dst, B, H, W, ops, factors, hue_shift, ws, (hipStream_t)stream));
  return 0;
}

int mmf_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int KX, int KY, const float* weights,
                         const int32_t* apply, void* stream) {
  if (!src || !dst || !weights || !apply) return fail(MMF_EINVAL, "null argument");
  if (B < 1 || B > kBlurMaxBatch || H < 1 || W < 1 || (double)H * W > (double)kBlurMaxPixels)
    return fail(MMF_EINVAL, "gaussian_blur_u8: bad shape (B=%d (1..%d) H=%d W=%d (H*W <= 2^30))", B, kBlurMaxBatch, H, W);
  if (KX < 1 || KY < 1 || KX > kBlurMaxTaps || KY > kBlurMaxTaps || !(KX & 1) || !(KY & 1))
    return fail(MMF_EINVAL, "gaussian_blur_u8: KX=%d KY=%d must be odd, 1..%d", KX, KY, kBlurMaxTaps);
  if (W <= KX / 2 || H <= KY / 2)
    return fail(MMF_EINVAL, "gaussian_blur_u8: the reflection needs W=%d > KX/2=%d and H=%d > KY/2=%d", W, KX / 2, H,
                KY / 2);
  {  // a tile's halo reads rows that other workgroups write: any overlap, not only dst == src, would corrupt
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, n = (uintptr_t)B * (uintptr_t)H * (uintptr_t)W * 3;
    if (s0 < d0 + n && d0 < s0 + n) return fail(MMF_EINVAL, "gaussian_blur_u8: dst must not overlap src");
  }
  if (((uintptr_t)weights | (uintptr_t)apply) & 3)
    return fail(MMF_EINVAL, "gaussian_blur_u8: weights and apply must be 4-byte aligned");
  HIPCHK(launch_gaussian_blur_u8(src, dst, B, H, W, KX, KY, weights, apply, (hipStream_t)stream));
  return 0;
}

int64_t mmf_jpeg_roundtrip_ws_bytes(int H, int W) { return (int64_t)jpeg_roundtrip_ws_bytes(H, W); }

int mmf_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* quality, uint8_t* ws,
                          int32_t* flags, void* stream) {
  if (!src || !dst || !quality || !ws || !flags) return fail(MMF_EINVAL, "null argument");
  if (B < 1 || B > kJpegEncMaxBatch || H < 1 || W < 1 || (double)H * W > (double)kJpegEncMaxPixels)
    return fail(MMF_EINVAL, "jpeg_roundtrip_u8: bad shape (B=%d (1..%d) H=%d W=%d (H*W <= 2^30))", B, kJpegEncMaxBatch,
                H, W);
  if (dst == src) return fail(MMF_EINVAL, "jpeg_roundtrip_u8: dst must not be src");
  if ((((uintptr_t)quality | (uintptr_t)flags) & 3) || ((uintptr_t)ws & 7))
    return fail(MMF_EINVAL, "jpeg_roundtrip_u8: quality and flags must be 4-byte aligned, ws 8-byte");
  HIPCHK(launch_jpeg_roundtrip_u8(src, dst, B, H, W, quality, ws, flags, (hipStream_t)stream));
  return 0;
}

int mmf_effcls_train_epoch(const float* feat, const int32_t* labels, int R, const int32_t* perm, int N,
                           const uint64_t* keep, float p_drop, int batch, double lr, double beta1, double beta2,
                           double eps, double weight_decay, int step0, float* params, float* exp_avg,
                           float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* grad_out, void* stream) {
  if (!feat || !labels || !perm || !params || !exp_avg || !exp_avg_sq || !step_loss || !step_correct)
    return fail(MMF_EINVAL, "null argument");
  if (R < 1 || N < 1 || batch < 1 || batch > 64 || step0 < 0 || !(p_drop >= 0.f && p_drop < 1.f))
    return fail(MMF_EINVAL, "effcls_train_epoch: R=%d N=%d (>= 1) batch=%d (1..64) step0=%d (>= 0) p_drop=%g ([0, 1))",
                R, N, batch, step0, (double)p_drop);
  CHK(check_aligned("effcls_train_epoch", 4,
                    {feat, params, exp_avg, exp_avg_sq, step_loss, grad_out, labels, perm, step_correct}, true, keep));
  HIPCHK(launch_effcls_train_epoch(feat, labels, R, perm, N, keep, p_drop, batch, lr, beta1, beta2, eps, weight_decay,
                                   step0, params, exp_avg, exp_avg_sq, step_loss, step_correct, grad_out,
                                   (hipStream_t)stream));
  return 0;
}

int mmf_effcls_eval(const float* feat, const int32_t* labels, int R, int batch, const float* params, float* batch_loss,
                    float* row_logits, void* stream) {
  if (!feat || !labels || !params || !batch_loss || !row_logits) return fail(MMF_EINVAL, "null argument");
  if (R < 1 || batch < 1 || batch > 64) return fail(MMF_EINVAL, "effcls_eval: R=%d (>= 1) batch=%d (1..64)", R, batch);
  CHK(check_aligned("effcls_eval", 4, {feat, labels, params, batch_loss, row_logits}));
  HIPCHK(launch_effcls_eval(feat, labels, R, batch, params, batch_loss, row_logits, (hipStream_t)stream));
  return 0;
}

static_assert(kEffHeadParams == MMF_EFFHEAD_PARAMS, "header and kernels");
int64_t mmf_effhead_ws_bytes(int batch) { return (int64_t)effhead_ws_bytes(batch); }
// the kernels use bn_eps as an fp32 value: that value, not the double, must be positive and finite
static bool effhead_eps_ok(double bn_eps) {
  const float e = (float)bn_eps;
  return e > 0.0f && std::isfinite(e);
}

int mmf_effhead_train_epoch(const float* trunk, const int32_t* labels, int R, const int32_t* perm, int N,
                            const uint64_t* keep, float p_drop, int batch, const float* bn_mean, const float* bn_var,
                            double bn_eps, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int step0, float* params, float* exp_avg, float* exp_avg_sq, float* step_loss,
                            int32_t* step_correct, float* grad_out, void* ws, int64_t ws_bytes, void* stream) {
  if (!trunk || !labels || !perm || !bn_mean || !bn_var || !params || !exp_avg || !exp_avg_sq || !step_loss ||
      !step_correct || !ws)
    return fail(MMF_EINVAL, "null argument");
  if (R < 1 || N < 1 || batch < 1 || batch > 64 || step0 < 0 || !(p_drop >= 0.f && p_drop < 1.f))
    return fail(MMF_EINVAL, "effhead_train_epoch: R=%d N=%d (>= 1) batch=%d (1..64) step0=%d (>= 0) p_drop=%g ([0, 1))",
                R, N, batch, step0, (double)p_drop);
  if (!effhead_eps_ok(bn_eps))
    return fail(MMF_EINVAL, "effhead_train_epoch: bn_eps=%g must be positive and finite as an fp32 value", bn_eps);
  CHK(check_ws("effhead_train_epoch", ws_bytes, effhead_ws_bytes(batch)));
  CHK(check_aligned("effhead_train_epoch", 4, {labels, perm, bn_mean, bn_var, step_loss, step_correct}));
  CHK(check_aligned("effhead_train_epoch", 16, {trunk, params, exp_avg, exp_avg_sq, grad_out, ws}, true, keep));
  HIPCHK(launch_effhead_train_epoch(trunk, labels, R, perm, N, keep, p_drop, batch, bn_mean, bn_var, bn_eps, lr, beta1,
                                    beta2, eps, weight_decay, step0, params, exp_avg, exp_avg_sq, step_loss,
                                    step_correct, grad_out, (float*)ws, (hipStream_t)stream));
  return 0;
}

int mmf_effhead_eval(const float* trunk, const int32_t* labels, int R, int batch, const float* params,
                     const float* bn_mean, const float* bn_var, double bn_eps, float* batch_loss, float* row_logits,
                     void* ws, int64_t ws_bytes, void* stream) {
  if (!trunk || !labels || !params || !bn_mean || !bn_var || !batch_loss || !row_logits || !ws)
    return fail(MMF_EINVAL, "null argument");
  if (R < 1 || batch < 1 || batch > 64) return fail(MMF_EINVAL, "effhead_eval: R=%d (>= 1) batch=%d (1..64)", R, batch);
  if (!effhead_eps_ok(bn_eps))
    return fail(MMF_EINVAL, "effhead_eval: bn_eps=%g must be positive and finite as an fp32 value", bn_eps);
  CHK(check_ws("effhead_eval", ws_bytes, effhead_ws_bytes(batch)));
  CHK(check_aligned("effhead_eval", 4, {labels, bn_mean, bn_var, batch_loss, row_logits}));
  CHK(check_aligned("effhead_eval", 16, {trunk, params, ws}));
  HIPCHK(launch_effhead_eval(trunk, labels, R, batch, params, bn_mean, bn_var, bn_eps, batch_loss, row_logits,
                             (float*)ws, (hipStream_t)stream));
  return 0;
}

int mmf_set_vault(mmf_handle* h, const float* V, int N, int D) {
  if (!h || !V || N <= 0 || D != 512) return fail(MMF_EINVAL, "mmf_set_vault: need N > 0 rows of D = 512");
  HIPCHK(hipSetDevice(h->device));
  std::vector<float> u((size_t)N * D);
  for (int i = 0; i < N; ++i) {
    double s = 0;
    for (int d = 0; d < D; ++d) s += (double)V[(size_t)i * D + d] * V[(size_t)i * D + d];
    const float nrm = (float)std::sqrt(s);  // a zero row gives 0/0 = NaN, as numpy does
    for (int d = 0; d < D; ++d) u[(size_t)i * D + d] = V[(size_t)i * D + d] / nrm;
  }
  return set_vault_rows(h, u, N);
}

int mmf_set_vault_normalized(mmf_handle* h, const float* Vhat, int N, int D) {
  if (!h || !Vhat || N <= 0 || D != 512) return fail(MMF_EINVAL, "mmf_set_vault_normalized: need N > 0 rows of D = 512");
  HIPCHK(hipSetDevice(h->device));
  std::vector<float> u(Vhat, Vhat + (size_t)N * D);
  return set_vault_rows(h, u, N);
}

int mmf_set_vault_titles(mmf_handle* h, const int32_t* ids, const int32_t* mask, int N, int L, void* stream) {
  if (!h || !ids || !mask) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_VAULT) || N != h->vault_n) return fail(MMF_EINVAL, "set the vault (N=%d) first", h->vault_n);
  if (!(h->ready & RDY_CTEXT)) return fail(MMF_EINVAL, "CLIP text tower not loaded");
  if (L > h->cap_lc || h->cap_b <= 0) return fail(MMF_EINVAL, "reserve CLIP length >= %d first", L);
  HIPCHK(hipSetDevice(h->device));
  CHK(free_group(h, AG_TITLES));
  h->vault_title = nullptr;
  float* t;
  CHK(dev_alloc(h, &t, (size_t)N * 512, AG_TITLES));
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < N; i += h->cap_b) {
    const int n = std::min(h->cap_b, N - i);
    CHK(run_clip_text(h, ids + (size_t)i * L, mask + (size_t)i * L, n, L, t + (size_t)i * 512, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  h->vault_title = t;
  return 0;
}

int mmf_vault_topk(mmf_handle* h, const float* q, int B, int k, float thresh, float* sims, int32_t* idx, float* disc,
                   const float* temb, float* tsim, void* stream) {
  if (!h || !q) return fail(MMF_EINVAL, "null argument");
  if (!(h->ready & RDY_VAULT)) return fail(MMF_EINVAL, "vault not loaded");
  if (k < 1 || k > h->vault_n) return fail(MMF_EINVAL, "top_k must be in [1, N=%d]", h->vault_n);
  CHK(check_cap(h, B, 1, 1));
  HIPCHK(hipSetDevice(h->device));
  const VaultOut out{thresh, sims, idx, disc, 1, temb, h->vault_title, 512, tsim};
  return vault_search(h, q, B, k, out, (hipStream_t)stream);
}

int mmf_fusion(mmf_handle* h, const float* x5, int B, float* probs, int32_t* verdict, float* conf, int32_t* rule,
               void* stream) {
  if (!h || !x5 || !probs || B <= 0) return fail(MMF_EINVAL, "bad argument");
  if (!(h->ready & RDY_FUSION)) return fail(MMF_EINVAL, "fusion layer not loaded");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(launch_fusion(x5, h->f_w0, h->f_b0, h->f_w3, h->f_b3, h->f_w5, h->f_b5, probs, verdict, conf, rule, B,
                       (hipStream_t)stream));
  return 0;
}

int mmf_fusion_train_epoch(const float* scores5, const int32_t* labels, int N, const int32_t* perm,
                           const uint64_t* keep, float p_drop, int batch, double lr, double beta1, double beta2,
                           double eps, double weight_decay, int step0, float* params, float* exp_avg,
                           float* exp_avg_sq, float* step_loss, int32_t* step_correct, float* grad_out, void* stream) {
  if (!scores5 || !labels || !perm || !params || !exp_avg || !exp_avg_sq || !step_loss || !step_correct)
    return fail(MMF_EINVAL, "null argument");
  if (N < 1 || batch < 1 || batch > 256 || !(p_drop >= 0.f && p_drop < 1.f))
    return fail(MMF_EINVAL, "fusion_train_epoch: N=%d (>= 1) batch=%d (1..256) p_drop=%g ([0, 1))", N, batch,
                (double)p_drop);
  HIPCHK(launch_fusion_train_epoch(scores5, labels, N, perm, keep, p_drop, batch, lr, beta1, beta2, eps, weight_decay,
                                   step0, params, exp_avg, exp_avg_sq, step_loss, step_correct, grad_out,
                                   (hipStream_t)stream));
  return 0;
}

int mmf_analyze_batch(mmf_handle* h, const int32_t* rob_ids, const int32_t* rob_mask, int Lr, const int32_t* clip_ids,
                      const int32_t* clip_mask, int Lc, const uint8_t* img_eff, const uint8_t* img_clip, int B,
                      float* scores5, float* text_sim, float* probs2, int32_t* verdict, float* conf, int32_t* rule,
                      float* top_sims, int32_t* top_idx, void* stream) {
  if (!h || !rob_ids || !rob_mask || !clip_ids || !clip_mask || !img_eff || !scores5 || !probs2)
    return fail(MMF_EINVAL, "null argument");
  if ((h->ready & RDY_MODELS) != RDY_MODELS) return fail(MMF_EINVAL, "not all models loaded (ready mask %d)", h->ready);
  if (Lr > 512 || Lc > 77) return fail(MMF_EINVAL, "lengths Lr=%d (<=512) Lc=%d (<=77)", Lr, Lc);
  CHK(check_cap(h, B, Lr, Lc));
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!img_clip) img_clip = img_eff;
  TowerJobs j{};
  j.rob_ids = rob_ids; j.rob_mask = rob_mask; j.nT = B; j.Lr = Lr; j.text_scores = scores5; j.text_stride = 5;
  j.clip_ids = clip_ids; j.clip_mask = clip_mask; j.nC = B; j.Lc = Lc;
  j.img_eff = img_eff; j.img_clip = img_clip; j.nI = B; j.eff_scores = scores5 + 2; j.eff_stride = 5;
  CHK(run_towers(h, j, B, s));
  return analyze_tail(h, B, scores5, text_sim, probs2, verdict, conf, rule, top_sims, top_idx, s);
}

int mmf_analyze_mixed(mmf_handle* h, const int32_t* row_map, int B, int nT, int nI, int nC, const int32_t* rob_ids,
                      const int32_t* rob_mask, int Lr, const int32_t* clip_ids, const int32_t* clip_mask, int Lc,
                      const uint8_t* img_eff, const uint8_t* img_clip, float* scores5, float* text_sim, float* probs2,
                      int32_t* verdict, float* conf, int32_t* rule, float* top_sims, int32_t* top_idx, void* stream) {
  if (!h || !row_map || !scores5 || !probs2) return fail(MMF_EINVAL, "null argument");
  if (B <= 0 || nT < 0 || nI < 0 || nC < 0 || nC > nT || nC > nI || nT + nI - nC != B)
    return fail(MMF_EINVAL, "counts nT=%d nI=%d nC=%d do not describe a batch of B=%d rows with a text, an image or both "
                            "(nT + nI - nC == B, nC <= nT, nC <= nI)", nT, nI, nC, B);
  if ((nT && (!rob_ids || !rob_mask)) || (nI && !img_eff) || (nC && (!clip_ids || !clip_mask)))
    return fail(MMF_EINVAL, "null input of a list with rows (nT=%d nI=%d nC=%d)", nT, nI, nC);
  // only the components this batch uses must be loaded
  const int need = (nT ? RDY_TEXT : 0) | (nI ? RDY_EFFNET | RDY_VISION : 0) | (nC ? RDY_CTEXT | RDY_FUSION : 0);
  if ((h->ready & need) != need)
    return fail(MMF_EINVAL, "models of this batch not loaded (needs mask %d, ready mask %d)", need, h->ready);
  if (!nT) Lr = 1;
  if (!nC) Lc = 1;
  if (Lr <= 0 || Lc <= 0 || Lr > 512 || Lc > 77) return fail(MMF_EINVAL, "lengths Lr=%d (1..512) Lc=%d (1..77)", Lr, Lc);
  CHK(check_cap(h, B, Lr, Lc));
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!img_clip) img_clip = img_eff;
  Workspace& w = h->ws;
  TowerJobs j{};
  j.rob_ids = rob_ids; j.rob_mask = rob_mask; j.nT = nT; j.Lr = Lr; j.text_scores = w.m_text; j.text_stride = 2;
  j.clip_ids = clip_ids; j.clip_mask = clip_mask; j.nC = nC; j.Lc = Lc;
  j.img_eff = img_eff; j.img_clip = img_clip; j.nI = nI; j.eff_scores = w.m_eff; j.eff_stride = 1;
  CHK(run_towers(h, j, B, s));
  return mixed_tail(h, row_map, B, nT, nI, nC, scores5, text_sim, probs2, verdict, conf, rule, top_sims, top_idx, s);
}

int mmf_profile_begin(mmf_handle* h) {
  if (!h) return fail(MMF_EINVAL, "null handle");
  h->prof = true;
  h->prof_recs.clear();
  h->ev_used = 0;
  return 0;
}

int mmf_profile_end(mmf_handle* h, int max_kinds, int* counts, double* ms, double* flops, double* bytes) {
  if (!h || max_kinds < PK_COUNT || !counts || !ms || !flops || !bytes)
    return fail(MMF_EINVAL, "mmf_profile_end needs arrays of >= %d kinds", (int)PK_COUNT);
  h->prof = false;
  for (int k = 0; k < max_kinds; ++k) {
    counts[k] = 0;
    ms[k] = flops[k] = bytes[k] = 0.0;
  }
  if (!h->prof_recs.empty()) HIPCHK(hipEventSynchronize(h->ev_pool[h->prof_recs.back().ev + 1]));
  for (const auto& r : h->prof_recs) {
    if (r.kind < 0 || r.kind >= PK_COUNT) continue;
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, h->ev_pool[r.ev], h->ev_pool[r.ev + 1]));
    counts[r.kind] += 1;
    ms[r.kind] += t;
    flops[r.kind] += r.flops;
    bytes[r.kind] += r.bytes;
  }
  h->prof_recs.clear();
  h->ev_used = 0;
  return PK_COUNT;
}

const char* mmf_profile_kind_name(int kind) { return prof_kind_name(kind); }

int mmf_set_option(mmf_handle* h, const char* name, int value) {
  if (!name) return fail(MMF_EINVAL, "null option name");
  if (h && !strcmp(name, "text_precise_packed")) {
    // release the precise-mode weights of the GEMM kinds not in `value` (the engine's calibration, once
    // it has selected a mode that does not read them); packing happens only at weight load
    if (value & ~h->r_precise & 15)
      return fail(MMF_EINVAL, "text_precise_packed %d: only a subset of the packed kinds (%d) can be kept; re-load the "
                              "text model to re-pack", value, h->r_precise);
    if (text_mode(h) >= 2 && (h->opt.text_prec_mask & 15 & ~value))
      return fail(MMF_EINVAL, "text_precise_packed %d: the selected precise mode (text_prec_mask %d) reads them", value,
                  h->opt.text_prec_mask);
    (void)hipSetDevice(h->device);
    for (int k = 0; k < 4; ++k) {
      if (!((h->r_precise >> k) & 1) || ((value >> k) & 1)) continue;
      CHK(free_group(h, AG_TP0 + k));
      for (EncLayer& L : h->r_layers) (k == 0 ? L.qkv3 : k == 1 ? L.o3 : k == 2 ? L.fc13 : L.fc23) = Lin16{};
    }
    h->r_precise = value & 15;
    return 0;
  }
  Options& o = h ? h->opt : process_options();
  for (const OptName& n : kOptNames)
    if (!strcmp(n.name, name)) {
      if (h && (h->ready & RDY_TEXT)) {
        const bool prec = !strcmp(name, "text_hilo") ? value >= 2 : o.text_hilo >= 2;
        const int pm = (!strcmp(name, "text_prec_mask") ? value : o.text_prec_mask) & 15;
        if ((!strcmp(name, "text_hilo") || !strcmp(name, "text_prec_mask")) && prec && (pm & ~h->r_precise))
          return fail(MMF_EINVAL, "text_hilo = 2 with text_prec_mask %d needs precise-mode weights that are not packed "
                                  "(packed: %d; re-load the text model with text_hilo -1 or 2)", pm, h->r_precise);
      }
      o.*(n.field) = value;
      if (h) {
        (void)hipSetDevice(h->device);
        if (!strcmp(name, "vault_fused")) CHK(ensure_sims(h));  // (and the vault's, this one)
        return ensure_mode_ws(h);  // (precision modes: their workspaces follow the selection)
      }
      return 0;
    }
  return fail(MMF_EINVAL, "unknown option '%s'", name);
}

const char* mmf_option_name(int i) {
  constexpr int n = (int)(sizeof(kOptNames) / sizeof(kOptNames[0]));
  return (i >= 0 && i < n) ? kOptNames[i].name : nullptr;
}

int mmf_get_option(mmf_handle* h, const char* name, int* value) {
  if (!name || !value) return fail(MMF_EINVAL, "null argument");
  if (h && !strcmp(name, "text_hilo_effective")) {  // read-only: the stream layout run_text uses
    *value = text_mode(h);
    return 0;
  }
  if (h && !strcmp(name, "text_precise_packed")) {  // kinds whose precise-mode weights are packed
    *value = h->r_precise;
    return 0;
  }
  const Options& o = h ? h->opt : process_options();
  for (const OptName& n : kOptNames)
    if (!strcmp(n.name, name)) {
      *value = o.*(n.field);
      return 0;
    }
  return fail(MMF_EINVAL, "unknown option '%s'", name);
}


int mmf_jpeg_reconstruct(mmf_handle* h, const uint8_t* packed, const uint32_t* block_off, const int64_t* pk_off,
                         const uint16_t* qt, const int64_t* coef_blocks, const int32_t* infos, const int64_t* out_offsets,
                         int B, int max_blocks, int max_pixels, uint8_t* samples, uint8_t* out_rgbx, void* stream) {
  if (!h || B < 0) return fail(MMF_EINVAL, "null argument");
  if (B == 0) return 0;
  if (!packed || !block_off || !pk_off || !qt || !coef_blocks || !infos || !out_offsets || !samples || !out_rgbx)
    return fail(MMF_EINVAL, "null argument");
  if (max_blocks <= 0 || max_pixels <= 0) return fail(MMF_EINVAL, "max_blocks / max_pixels must be positive");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(launch_jpeg_reconstruct(packed, block_off, pk_off, qt, coef_blocks, infos, out_offsets, B, max_blocks,
                                 max_pixels, samples, out_rgbx, (hipStream_t)stream));
  return 0;
}

int64_t mmf_device_bytes(mmf_handle* h) {
  if (!h) return 0;
  int64_t t = 0;
  for (size_t b : h->group_bytes) t += (int64_t)b;
  return t;
}

// the fields every test-only GEMM entry point below passes through
static GemmArgs test_gemm_args(const void* A, int lda, const void* W, int ldw, const float* bias, void* c16, int ldc,
                               int M, int N, int K, int act) {
  GemmArgs g{};
  g.A = (const f16_t*)A;
  g.lda = lda;
  g.W = (const f16_t*)W;
  g.ldw = ldw;
  g.bias = bias;
  g.c16 = (f16_t*)c16;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  g.act = act;
  return g;
}

int mmf_gemm_f16(const void* A, int lda, const void* W, int ldw, const float* bias, const float* residual, float* c32,
                  void* c16, int ldc, int M, int N, int K, int act, void* stream) {
  GemmArgs g = test_gemm_args(A, lda, W, ldw, bias, c16, ldc, M, N, K, act);
  g.res32 = residual;
  g.ldr = ldc;
  g.c32 = c32;
  apply_options(process_options(), &g);
  if (!A || !W || (!c32 && !c16)) return fail(MMF_EINVAL, "null argument");
  hipError_t e = launch_gemm(g, (hipStream_t)stream);
  if (e != hipSuccess) return fail(MMF_EIO, "gemm: %s", hipGetErrorString(e));
  return 0;
}

int mmf_gemm_f16_ex(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res16,
                     const float* ascale, int rows_per_batch, void* c16, int ldc, int M, int N, int K, int act,
                     void* stream) {
  GemmArgs g = test_gemm_args(A, lda, W, ldw, bias, c16, ldc, M, N, K, act);
  g.res16 = (const f16_t*)res16;
  g.ldr = ldc;
  g.ascale = ascale;
  g.rows_per_batch = rows_per_batch;
  apply_options(process_options(), &g);
  if (!A || !W || !c16) return fail(MMF_EINVAL, "null argument");
  if (ascale && rows_per_batch <= 0) return fail(MMF_EINVAL, "rows_per_batch must be > 0 with ascale");
  hipError_t e = launch_gemm(g, (hipStream_t)stream);
  if (e != hipSuccess) return fail(MMF_EIO, "gemm: %s", hipGetErrorString(e));
  return 0;
}

int mmf_gemm_f16_split(const void* A, int lda, const void* W, int ldw, const float* bias, void* c16, int ldc, int M,
                       int N, int K, int act, int split_lo, void* stream) {
  GemmArgs g = test_gemm_args(A, lda, W, ldw, bias, c16, ldc, M, N, K, act);
  g.epi = 4;
  g.split_lo = split_lo ? 1 : 0;
  apply_options(process_options(), &g);
  if (!A || !W || !c16 || !bias) return fail(MMF_EINVAL, "null argument");
  if (!gemm_epi_ok(g)) return fail(MMF_EINVAL, "split-operand epilogue not applicable (M=%d N=%d K=%d ldc=%d act=%d)", M, N, K, ldc, act);
  hipError_t e = launch_gemm(g, (hipStream_t)stream);
  if (e != hipSuccess) return fail(MMF_EIO, "gemm: %s", hipGetErrorString(e));
  return 0;
}

int mmf_attention_f16(const void* qkv, const int32_t* mask, void* out, int B, int L, int H, int causal,
                       void* stream) {
  if (!qkv || !out) return fail(MMF_EINVAL, "null argument");
  hipError_t e = launch_attention((const f16_t*)qkv, 3 * H * 64, mask, (f16_t*)out, H * 64, B, L, H, causal,
                                  (hipStream_t)stream);
  if (e != hipSuccess) return fail(MMF_EIO, "attention: %s", hipGetErrorString(e));
  return 0;
}

int64_t mmf_vault_search_ws_bytes(int B, int k, int nblocks) {
  if (B < 1 || k < 1 || k > 8 || nblocks < 0 || nblocks > 65535) return 0;
  return (int64_t)vault_search_ws_bytes(B, k, nblocks);
}

int mmf_vault_search_rows(const float* q_unit, const float* bank_unit, int B, int N, int D, int k, float thresh,
                          float* sims, int32_t* idx, float* disc, int disc_stride, const float* text_emb,
                          const float* title_bank, float* text_sim, void* ws, int64_t ws_bytes, int nblocks,
                          void* stream) {
  if (!q_unit || !bank_unit || !ws) return fail(MMF_EINVAL, "null argument");
  if (B < 1 || N < 1 || D != 512) return fail(MMF_EINVAL, "mmf_vault_search_rows: need B > 0, N > 0 rows of D = 512");
  if (k < 1 || k > 8) return fail(MMF_EINVAL, "mmf_vault_search_rows: top_k must be in [1, 8] (got %d)", k);
  if (nblocks < 0 || nblocks > 65535) return fail(MMF_EINVAL, "mmf_vault_search_rows: nblocks must be in [0, 65535]");
  if (disc && disc_stride < 1) return fail(MMF_EINVAL, "mmf_vault_search_rows: disc_stride must be >= 1");
  const int64_t need = mmf_vault_search_ws_bytes(B, k, nblocks);
  if (ws_bytes < need)
    return fail(MMF_EINVAL, "mmf_vault_search_rows: workspace of %lld bytes, needs %lld", (long long)ws_bytes,
                (long long)need);
  const VaultOut out{thresh, sims, idx, disc, disc_stride, text_emb, title_bank, 512, text_sim};
  hipError_t e = launch_vault_search(q_unit, bank_unit, B, N, k, out, ws, nblocks, (hipStream_t)stream);
  if (e != hipSuccess) return fail(MMF_EIO, "vault search: %s", hipGetErrorString(e));
  return 0;
}

}  // extern "C"
