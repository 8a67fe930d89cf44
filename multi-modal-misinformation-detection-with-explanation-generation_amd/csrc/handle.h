// Internal to libmmf_hip.so (not installed): the handle behind include/mmf_hip.h, its error, allocation
// and profiling plumbing, and the launch wrappers the towers share.  The host side is one file per
// seam: weights_host.cpp packs the weights, text_host.cpp / clip_host.cpp / effnet_host.cpp hold the
// towers' launch sequences, resize_host.cpp the Pillow resize planner, capi.cpp the extern "C" surface (mixed_plan.cpp: its one
// host-only function that needs neither the handle nor HIP; test_host.cpp: the transformer kernels' test-only
// entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mmf_hip.h"
#include "kernels.h"

#pragma GCC visibility push(hidden)  // linkage across the library's own files only: nothing here is exported

// the calling thread's message behind mmf_last_error (capi.cpp); fail() sets it and returns `code`
extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(MMF_EIO, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define CHK(expr)            \
  do {                       \
    int r_ = (expr);         \
    if (r_ != 0) return r_;  \
  } while (0)

struct HostT {
  std::vector<int64_t> shape;
  std::vector<float> f;
  size_t numel() const { return f.size(); }
};

struct Lin16 {
  f16_t* w = nullptr;
  float* b = nullptr;
  int out = 0, in = 0;
  float* w32 = nullptr;  // fp32 copy of w (EfficientNet 1x1 convs: the effnet_fp32 tower)
};
// output rows [r0, r0 + n) of a linear layer (the K / V or Q part of a fused QKV weight)
inline Lin16 rows_of(const Lin16& l, int r0, int n) {
  Lin16 r = l;
  r.w += (size_t)r0 * l.in;
  r.b += r0;
  r.out = n;
  return r;
}
struct LNp { float* g = nullptr; float* b = nullptr; };
// qkv_f / fc1_f (CLIP): the QKV and FFN-1 projections with their input LayerNorm folded in (lazy
// LN, gemm.hip): w' = fp16(w diag(gamma)), bias c = b + w beta, u = rows of w' summed (fp16 values)
struct EncLayer {
  Lin16 qkv, o, fc1, fc2;
  LNp ln1, ln2;
  Lin16 qkv_f, fc1_f;
  float *qkv_u = nullptr, *fc1_u = nullptr;
  Lin16 qkv_h;  // RoBERTa: the fused QKV with rows interleaved per head, [q_h; k_h; v_h] (gemm.hip epi 3)
  // CLIP: qkv_f / qkv_u with the same per-head row interleave (gemm.hip epi 5, option clip_qkv_attn)
  Lin16 qkv_fh;
  float* qkv_uh = nullptr;
  // RoBERTa precise mode (text_hilo = 2, precise.hip): [W_hi | W_hi | W_lo] along K (in = 3 K), the
  // bias shared with the fp16 copy
  Lin16 qkv3, o3, fc13, fc23;
};

struct EffBlock {
  int expand, k, stride, cin, cout, cexp, csq, residual;
  Lin16 e, p;            // expand / project 1x1 convs (BN folded)
  float* wd = nullptr;   // depthwise [cexp][k*k] (BN folded)
  float* wd_t = nullptr; // the same, tap-major [k*k][cexp] (fp32 tower)
  float* bd = nullptr;
  float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;  // SE
};

// EfficientNet-B0 stages: expand, kernel, stride, cin, cout, blocks
inline constexpr int kStages[7][6] = {{1, 3, 1, 32, 16, 1},  {6, 3, 2, 16, 24, 2},   {6, 5, 2, 24, 40, 2},  {6, 3, 2, 40, 80, 3},
                                      {6, 5, 1, 80, 112, 3}, {6, 5, 2, 112, 192, 4}, {6, 3, 1, 192, 320, 1}};

struct Workspace {
  // RoBERTa
  float *r_x = nullptr, *r_y = nullptr;
  uint16_t* r_lo = nullptr;  // fp16 low part of the split post-LN residual stream (hi = r_xb)
  int* r_ovf = nullptr;      // [cap_b] overflow sentinel of the fp16 / split stream (norm.hip; run_text)
  f16_t *r_xb = nullptr, *r_qkv = nullptr, *r_ctx = nullptr, *r_h = nullptr;
  // CLIP vision
  f16_t *v_col = nullptr, *v_xb = nullptr, *v_qkv = nullptr, *v_ctx = nullptr, *v_h = nullptr, *v_cls = nullptr;
  float *v_patch = nullptr, *v_x = nullptr, *v_emb = nullptr, *v_xc = nullptr;
  f16_t* v_ctxc = nullptr;
  // CLIP text
  f16_t *t_xb = nullptr, *t_qkv = nullptr, *t_ctx = nullptr, *t_h = nullptr, *t_pool = nullptr, *t_ctxc = nullptr;
  float *t_x = nullptr, *t_emb = nullptr, *t_xc = nullptr;
  int32_t* t_eos = nullptr;
  // lazy-LN row partials of the CLIP streams (gemm.hip), two per tower (a producer writes the one
  // its stream's previous partials are not in): [rows padded to 256][kLnP] float2
  float2 *v_st[2] = {nullptr, nullptr}, *t_st[2] = {nullptr, nullptr};
  // EfficientNet
  f16_t *e_a = nullptr, *e_b = nullptr, *e_exp = nullptr, *e_dw = nullptr;
  float *e_pool = nullptr, *e_scale = nullptr;
  // fp32 EfficientNet activations (option effnet_fp32), allocated on first use for cap_b images
  float *e32_a = nullptr, *e32_b = nullptr, *e32_exp = nullptr, *e32_dw = nullptr;
  int e32_cap_b = 0;
  // RoBERTa precise mode (text_hilo = 2, group AG_TEXT32, allocated while the mode is selected): the
  // fp32 qkv / FFN hidden [rows][3072], the K-concatenated operands of the stream / ctx [rows][2304]
  // and of the FFN hidden [rows][9216]
  float* p32 = nullptr;
  f16_t *s3 = nullptr, *h3 = nullptr;
  size_t t32_rows = 0;
  // split-K partials of the skinny-M GEMMs, one per tower (the towers run on concurrent streams)
  float *sk_text = nullptr, *sk_vit = nullptr, *sk_ctext = nullptr;
  size_t sk_elems = 0;
  // vault
  float* s_sims = nullptr;  // S[cap_b][s_cap_n]: the whole vault, or one 16384-row chunk of a large fused one
  int s_cap_n = 0;
  void* vs_ws = nullptr;    // fused search candidates (vault_search_ws_bytes(cap_b, 8, 0)), while the vault is served fused
  // top_k > 8 on a vault of more than 16384 rows: per-chunk results [c_chunks][cap_b][64]
  float* c_sims = nullptr;
  int32_t* c_idx = nullptr;
  int c_chunks = 0;
  // mmf_analyze_mixed: the towers' compact results (text scores [nT][2], deepfake [nI], vault top-5
  // and discrepancy of the nI image rows) that its finish kernel gathers into batch order
  float *m_text = nullptr, *m_eff = nullptr, *m_sims = nullptr, *m_disc = nullptr;
  int32_t* m_idx = nullptr;
};
constexpr int kLnP = 8;  // lazy-LN partials per row a GEMM accepts (gemm.hip kLnPMax)

// Run-time options.  Defaults come from the environment ONCE per process (MMF_* variables, for the
// A/B tools), are copied into every handle at mmf_create and changed with mmf_set_option; no kernel
// launch reads the environment.  (capi.cpp holds the table of their names.)
struct Options {
  int concurrent = 1;   // towers of mmf_analyze_batch on concurrent streams
  int fuse_stem = 1;    // stem fused into the stage-1 depthwise conv
  int fuse_expand = 1;  // 1x1 expand fused into the depthwise conv (stages 2 - 4.3: effnet.hip expand_dw_applicable)
  int gemm_splitk = 1;  // split-K on the skinny-M GEMM path
  int gemm_config = -1; // forced GEMM instantiation (-1 = automatic)
  int gemm_group_m = 0; // persistent GEMM tile order
  int text_hilo = -1;   // RoBERTa residual stream as fp16 hi + fp16 lo (1), fp16 alone (0), or chosen at
                        // weight-load time from the LayerNorm parameters (-1, default: DESIGN §4); 2 = precise mode
  int text_prec_mask = 255;  // precise mode: bits 0-3 = GEMM kinds on hi / lo activations (1 QKV, 2 out-proj,
                             // 4 FFN-1, 8 FFN-2), bits 4-7 = the same kinds also on W_lo (3 products)
  int effnet_fp32 = 0;  // EfficientNet tower with fp32 activations (effnet_f32.hip) instead of fp16
  int clip_res16 = 1;   // CLIP pre-LN residual streams in fp16 (1, default) or fp32 (0)
  int lazy_ln = 1;      // CLIP encoder LayerNorms folded into the GEMM epilogues (gemm.hip)
  int pw32_mfma = 5;    // fp32 tower's 1x1 convs on the fp32-input MFMA (2: loads 3 K-chunks ahead, 1: one ahead;
                        // 3 / 4: whole-row tiles for the N <= 256 launches with K <= 64 / any K; 5: 4 where the
                        // row grid has the blocks for it) or the fp32-FMA VALU kernel (0) -- every mode bit-identical
  int dw_cw32 = 1;      // 32-channel groups for the standalone depthwise convs (effnet.hip dw_geometry; B=512 3.648 -> 3.595 ms)
  int effnet_chunks = 2;  // mmf_effnet_forward: batch chunks on concurrent streams (B=512: 3.82 -> 3.57 ms in bench.py)
  int qkv_attn = 1;     // RoBERTa L = 128: attention in the QKV GEMM's epilogue (gemm.hip epi 3)
  int clip_qkv_attn = 1;  // CLIP towers, lazy LN: attention in the QKV consumer's epilogue (gemm.hip epi 5; bit 1 ViT,
                        // bit 2 text tower: 0 / 1 = neither / both, 2 = ViT only, 4 = text only)
  int mt_enqueue = 64;  // batches of <= this many pairs: the towers enqueued by host threads side by side
  int last_q1 = 1;      // compact last encoder layers: K / V of every row, Q + attention of the pooled rows only
                        // (bit 1: RoBERTa -- QKV 4.5 -> K/V 3 persistent rounds; bit 2: CLIP towers, whose K/V
                        // GEMMs round to as many rounds as QKV: measured slower, off)
  int diag_skip = 0;    // diagnostic: towers mmf_analyze_batch leaves out (bitmask; measurement only)
  int vault_ref = 0;    // diagnostic: vault similarities on the VALU kernel and top-k by full sort (the
                        // reference kernels the production ones are bit-identical to)
  int vault_fused = 2;  // vault search without the similarity matrix (vault.hip vault_search_partial_kernel): 0 = the
                        // two-kernel path, 1 = fused wherever top_k <= 8, 2 = fused iff the vault has > 16384 rows
  int after_text = 12;  // towers of the concurrent B > mt_enqueue step that start only once RoBERTa is done
                        // (bitmask as diag_skip: 2 EfficientNet, 4 CLIP text, 8 ViT)
};
// (Round 6 measured and removed gemm_kloop -- ping-pong and A-ring K loops; round 5 removed
// the options whose variants were measured slower and stayed off: gemm_ring, gemm_wide,
// gemm_w4, dw_v2, dw_persist, ln_prod256, cu_split, fuse_expand32, qkv_attn_gm, splitk_fix, gemm_tq,
// se_group, splitk_min_k, and pinned gemm_prio = 2 / dw_ct = 1; DESIGN.md §3 keeps each measurement.)

// the process defaults (capi.cpp): what a handle starts from and what the handle-less test entry points use
Options& process_options();

inline void apply_options(const Options& o, GemmArgs* g) {
  g->force_cfg = o.gemm_config >= 0 ? o.gemm_config + 1 : 0;
  g->no_splitk = o.gemm_splitk ? 0 : 1;
  g->group_m = o.gemm_group_m;
}

// Device allocations are owned per group so that re-loading one component (or the vault, or the
// workspaces) frees exactly what it replaces.
enum AllocGroup {
  AG_WS = 0, AG_TEXT, AG_EFF, AG_VIS, AG_CTEXT, AG_FUSION, AG_VAULT, AG_TITLES, AG_SIMS, AG_EFF32, AG_RESIZE, AG_TEXT32,
  // the RoBERTa precise mode's K-concatenated weights, one group per GEMM kind (bit k of option
  // text_prec_mask <-> group AG_TP0 + k: QKV, out-proj, FFN-1, FFN-2), releasable one kind at a time
  AG_TP0, AG_TP1, AG_TP2, AG_TP3,
  AG_COUNT
};

// Bits of mmf_handle::ready, one per loaded component (ABI: mmf_ready, engine.py)
enum Ready {
  RDY_TEXT = 1, RDY_EFFNET = 2, RDY_VISION = 4, RDY_CTEXT = 8, RDY_FUSION = 16, RDY_VAULT = 32,
  RDY_CLIP = RDY_VISION | RDY_CTEXT, RDY_MODELS = RDY_TEXT | RDY_EFFNET | RDY_CLIP | RDY_FUSION  // all five models
};

// Host threads that enqueue mmf_analyze_batch's towers side by side (option mt_enqueue).  A small
// batch is host-enqueue bound: each tower is a chain of ~140 launches at ~2.3 us of host time each,
// and enqueued one tower after another the last tower starts ~0.8 ms into the call.  Each worker
// owns one tower stream; HIP's current device is per thread, so every worker sets it once.
struct EnqueuePool {
  struct Slot {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool busy = false, quit = false;
    int rc = 0;
    std::string err;
  };
  Slot slots[3];
  int device;
  explicit EnqueuePool(int dev) : device(dev) {
    for (Slot& sl : slots) sl.th = std::thread([this, &sl] { loop(sl); });
  }
  void loop(Slot& sl) {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(sl.mu);
    for (;;) {
      sl.cv.wait(lk, [&] { return sl.busy || sl.quit; });
      if (sl.quit) return;
      lk.unlock();
      const int rc = sl.job();
      std::string e = rc ? g_err : std::string();  // (g_err is this worker's thread-local message)
      lk.lock();
      sl.rc = rc;
      sl.err = e;
      sl.busy = false;
      sl.cv.notify_all();
    }
  }
  void submit(int i, std::function<int()> f) {
    Slot& sl = slots[i];
    std::lock_guard<std::mutex> lk(sl.mu);
    sl.job = std::move(f);
    sl.busy = true;
    sl.cv.notify_all();
  }
  int wait(int i, std::string* err) {
    Slot& sl = slots[i];
    std::unique_lock<std::mutex> lk(sl.mu);
    sl.cv.wait(lk, [&] { return !sl.busy; });
    if (sl.rc && err) *err = sl.err;
    return sl.rc;
  }
  ~EnqueuePool() {
    for (Slot& sl : slots) {
      {
        std::lock_guard<std::mutex> lk(sl.mu);
        sl.quit = true;
      }
      sl.cv.notify_all();
    }
    for (Slot& sl : slots)
      if (sl.th.joinable()) sl.th.join();
  }
};

struct mmf_handle {
  int device = 0;
  int eos_id = 49407;
  std::map<std::string, HostT> staged;
  std::vector<void*> groups[AG_COUNT];
  size_t group_bytes[AG_COUNT] = {};
  int cur_group = AG_TEXT;  // group of the weight uploads of the component being finalized
  Options opt;
  int ready = 0;  // Ready bits
  // RoBERTa + heads
  float *r_word = nullptr, *r_pos = nullptr, *r_type0 = nullptr;
  LNp r_embln;
  EncLayer r_layers[12];
  // post-LN stream magnitude bound from the loaded LayerNorms, max_c |beta_c| + 4 |gamma_c|, and
  // the split stream it selects under text_hilo = -1 (finalize_text)
  float r_stream_mag = 0.f;
  int r_hilo_auto = 0;
  int r_precise = 0;  // bitmask of the GEMM kinds whose precise-mode weights (EncLayer qkv3 ...) are packed
  float *h_w1a = nullptr, *h_b1a = nullptr, *h_w2a = nullptr, *h_b2a = nullptr;
  float *h_w1m = nullptr, *h_b1m = nullptr, *h_w2m = nullptr, *h_b2m = nullptr;
  // EfficientNet
  float *e_stem_w = nullptr, *e_stem_b = nullptr;
  std::vector<EffBlock> e_blocks;
  Lin16 e_head;
  float *e_cls_w = nullptr, *e_cls_b = nullptr;
  // CLIP vision
  f16_t* v_patch_w = nullptr;
  float *v_cls = nullptr, *v_pos = nullptr;
  LNp v_pre, v_post;
  EncLayer v_layers[12];
  f16_t* v_proj = nullptr;
  // CLIP text
  float *t_tok = nullptr, *t_pos = nullptr;
  EncLayer t_layers[12];
  LNp t_final;
  f16_t* t_proj = nullptr;
  // fusion
  float *f_w0 = nullptr, *f_b0 = nullptr, *f_w3 = nullptr, *f_b3 = nullptr, *f_w5 = nullptr, *f_b5 = nullptr;
  // vault
  float* vault = nullptr;        // [N][512] unit rows
  float* vault_title = nullptr;  // [N][512] unit title text embeddings (or null)
  int vault_n = 0;
  // workspace capacity
  Workspace ws;
  int cap_b = 0, cap_lr = 0, cap_lc = 0;
  // per-kernel event timing (mmf_profile_begin/end)
  struct ProfRec { int ev; int kind; double flops, bytes; };
  bool prof = false;
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool;
  int ev_used = 0;
  // fork/join streams of mmf_analyze_batch (text, effnet, clip-text towers beside the caller's)
  hipStream_t tower[3] = {nullptr, nullptr, nullptr};
  hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t text_ev = nullptr;  // RoBERTa tower done (option after_text)
  // option mt_enqueue (created on first use: ensure_pool).  Invariant: while the workers enqueue, no tower writes to the
  // handle -- every per-launch choice is read from `opt` (set between calls, never during one) and
  // every workspace is reserved before the call (mmf_reserve); the towers' launch sequences only read
  // the handle and enqueue on their own streams.
  std::unique_ptr<EnqueuePool> pool;
  // mmf_resize_pil workspaces (grow-only, group AG_RESIZE)
  struct ResizeWs {
    ResizeJob* jobs = nullptr;
    uint8_t** outs = nullptr;
    int32_t *coef = nullptr, *bounds = nullptr;
    uint8_t* tmp = nullptr;
    size_t cap_jobs = 0, cap_coef = 0, cap_tmp = 0;
  } rs;

  ~mmf_handle() {
    pool.reset();  // workers joined before their streams go
    for (auto& g : groups)
      for (void* p : g) (void)hipFree(p);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 3; ++i) {
      if (tower[i]) (void)hipStreamDestroy(tower[i]);
      if (join_ev[i]) (void)hipEventDestroy(join_ev[i]);
    }
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (text_ev) (void)hipEventDestroy(text_ev);
  }
};

// `count` elements of T in allocation group `group` (an empty request still gets 16 bytes)
template <typename T>
int dev_alloc(mmf_handle* h, T** p, size_t count, int group) {
  size_t bytes = count * sizeof(T);
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e != hipSuccess) return fail(MMF_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  h->groups[group].push_back(*p);
  h->group_bytes[group] += bytes;
  return 0;
}
// Free one group's buffers after the device has drained (any queued launch may still read them).
int free_group(mmf_handle* h, int group);

// ---- per-kernel timing: two hipEvents around each launch while profiling is on ------------
// GEMM launches are profiled per (tile instantiation, epilogue, activation) -- one kernel symbol
// each, so the numbers line up with a rocprofv3 kernel trace of the same run.
constexpr int kGemmActs = 5, kGemmEpis = 6;
enum ProfKind {
  PK_GEMM0 = 0, PK_GEMM_LAST = kGemmConfigs * kGemmEpis * kGemmActs - 1, PK_ATTN, PK_LN, PK_EMBED, PK_IM2COL, PK_STEM, PK_DW, PK_SE,
  PK_GAP, PK_HEADS, PK_VAULT, PK_FUSION, PK_PW32, PK_COUNT
};

struct ProfScope {
  mmf_handle* h;
  hipStream_t s;
  int ev = -1;
  ProfScope(mmf_handle* h_, hipStream_t s_, int kind, double flops, double bytes) : h(h_), s(s_) {
    if (!h->prof) return;
    while ((int)h->ev_pool.size() < h->ev_used + 2) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      h->ev_pool.push_back(e);
    }
    ev = h->ev_used;
    h->ev_used += 2;
    (void)hipEventRecord(h->ev_pool[ev], s);
    h->prof_recs.push_back({ev, kind, flops, bytes});
  }
  ~ProfScope() {
    if (ev >= 0) (void)hipEventRecord(h->ev_pool[ev + 1], s);
  }
};

// ---- profiled launch wrappers shared by the towers (inline: each tower's file compiles its own) ----
inline GemmArgs gemm_args(const f16_t* A, int lda, const Lin16& l, int M) {
  GemmArgs g{};
  g.A = A;
  g.lda = lda;
  g.W = l.w;
  g.ldw = l.in;
  g.bias = l.b;
  g.M = M;
  g.N = l.out;
  g.K = l.in;
  g.ldc = l.out;
  g.ldr = l.out;
  return g;
}

// split-K workspace: `elems` floats of partial planes
inline GemmArgs with_ws(GemmArgs g, float* ws, size_t elems) {
  g.ws = ws;
  g.ws_elems = elems;
  return g;
}

inline int gemm(mmf_handle* h, GemmArgs g, hipStream_t s) {
  apply_options(h->opt, &g);
  const double M = g.M, N = g.N, K = g.K;
  const double out_b = (g.c32 ? 4.0 : 0.0) + (g.c16 ? 2.0 : 0.0) + (g.res32 ? 4.0 : 0.0) + (g.res16 ? 2.0 : 0.0);
  // epi 3 also runs the attention of its rows (4 L^2 64 flops per sequence and head, L = 128) and
  // writes ctx (N / 3 columns) instead of qkv
  // (epi 5: the same for sequences of att_L rows)
  const double att = g.epi == 3   ? 4.0 * (M / 128) * (N / 192) * 128.0 * 128.0 * 64.0
                     : g.epi == 5 ? 4.0 * (M / g.att_L) * (N / 192) * (double)g.att_L * g.att_L * 64.0
                                  : 0.0;
  ProfScope ps(h, s, (gemm_config(g) * kGemmEpis + g.epi) * kGemmActs + g.act, 2.0 * M * N * K + att,
               2.0 * (M * K + N * K) + M * (g.epi == 3 || g.epi == 5 ? N / 3 : N) * out_b * (g.epi == 4 && g.split_lo ? 3 : 1));
  HIPCHK(launch_gemm(g, s));
  return 0;
}

inline int attn(mmf_handle* h, const f16_t* qkv, int ld, const int32_t* mask, f16_t* out, int ldo, int B, int L, int H,
                int causal, hipStream_t s) {
  ProfScope ps(h, s, PK_ATTN, 4.0 * B * H * (double)L * L * 64, (double)B * L * H * 64 * 2 * 4);
  HIPCHK(launch_attention(qkv, ld, mask, out, ldo, B, L, H, causal, s));
  return 0;
}

inline int lnorm(mmf_handle* h, const float* x, int ldx, const LNp& p, float* y32, int ldy32, f16_t* y16, int ldy16,
                 int rows, int C, hipStream_t s) {
  ProfScope ps(h, s, PK_LN, 8.0 * rows * C, (double)rows * C * (4 + (y32 ? 4 : 0) + (y16 ? 2 : 0)));
  HIPCHK(launch_layernorm(x, ldx, nullptr, 0, p.g, p.b, 1e-5f, y32, ldy32, y16, ldy16, rows, C, s));
  return 0;
}

inline int add_ln(mmf_handle* h, float* x, int ldx, const f16_t* y, int ldy, const LNp& p, float* s32, float* o32,
                  f16_t* o16, int ldo, int rows, int C, hipStream_t s) {
  ProfScope ps(h, s, PK_LN, 9.0 * rows * C, (double)rows * C * (4 + 2 + (s32 ? 4 : 0) + (o32 ? 4 : 0) + 2));
  HIPCHK(launch_add_ln(x, ldx, y, ldy, p.g, p.b, 1e-5f, s32, o32, o16, ldo, rows, C, s));
  return 0;
}

inline int add_ln(mmf_handle* h, f16_t* x, int ldx, const f16_t* y, int ldy, const LNp& p, f16_t* o16, int ldo,
                  int rows, int C, hipStream_t s) {
  ProfScope ps(h, s, PK_LN, 9.0 * rows * C, (double)rows * C * (2 + 2 + 2 + 2));
  HIPCHK(launch_add_ln(x, ldx, y, ldy, p.g, p.b, 1e-5f, x, o16, ldo, rows, C, s));
  return 0;
}

inline int add_ln_hilo(mmf_handle* h, f16_t* hi, uint16_t* lo, int ld, const f16_t* y, int ldy, const LNp& p, int rows,
                       hipStream_t s, int* ovf = nullptr, int L = 0) {
  ProfScope ps(h, s, PK_LN, 9.0 * rows * 768, (double)rows * 768 * (2 + 2 + 2 + 2 + 2));
  HIPCHK(launch_add_ln_hilo(hi, lo, ld, y, ldy, p.g, p.b, 1e-5f, rows, 768, s, ovf, L));
  return 0;
}

// ---- per-tower entry points ----------------------------------------------------------------
// weights_host.cpp: pack the staged tensors of one component into the current allocation group
int finalize_text(mmf_handle* h);
int finalize_effnet(mmf_handle* h);
int finalize_clip_vision(mmf_handle* h);
int finalize_clip_text(mmf_handle* h);
int finalize_fusion(mmf_handle* h);
int up_f32(mmf_handle* h, float** dst, const std::vector<float>& v);

int check_cap(mmf_handle* h, int B, int Lr, int Lc);  // capi.cpp
inline int text_mode(const mmf_handle* h) { return h->opt.text_hilo < 0 ? h->r_hilo_auto : h->opt.text_hilo; }

// heads_ev: recorded once the encoder is done, before the heads (mmf_analyze_batch's after_text event:
// the waiting towers start while the two small head MLPs run)
int run_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* ai, float* mi,
             float* scores, int score_stride, hipStream_t s, hipEvent_t heads_ev = nullptr, float* cls = nullptr);
int run_clip_image(mmf_handle* h, const uint8_t* img, int B, float* emb, hipStream_t s);
int run_clip_text(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* emb, hipStream_t s);
// the same towers up to the pooled LayerNorm: fp32 post_layernorm(CLS) [B][768] / final_layer_norm(EOS) [B][512]
int run_clip_image_pooled(mmf_handle* h, const uint8_t* img, int B, float* pooled, hipStream_t s);
int run_clip_text_pooled(mmf_handle* h, const int32_t* ids, const int32_t* mask, int B, int L, float* pooled,
                         hipStream_t s);
// a chunk starting at image img0 works in its own slice of every workspace (mmf_effnet_forward); pooled
// (mmf_effnet_pooled): the classifier's input rows fp32 [B][1280] instead of the classifier; trunk
// (mmf_effnet_trunk): the last MBConv block's output fp32 [B][49][320], and nothing after it
int run_effnet(mmf_handle* h, const uint8_t* img, const float* xf32, int B, float* logits, float* score, int score_stride,
               hipStream_t s, int img0 = 0, float* pooled = nullptr, float* trunk = nullptr);

// EfficientNet-B0: the geometry of block j of stage si (no weights), and the activation elements per
// image it implies: block input/output, expanded, depthwise output, SE pool partials (nchunks x
// channels), maxima over the network
EffBlock eff_block(int si, int j);
struct EffSizes { size_t io, exp, dw, pool; };
EffSizes eff_sizes();

#pragma GCC visibility pop
