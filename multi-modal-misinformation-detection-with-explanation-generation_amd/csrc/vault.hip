// The Truth-Vault search in exact fp32 like the reference: similarities (VALU and fp32-MFMA kernels)
// and top-k (register kernel for k <= 8, LDS sort above; fused similarity + top-k without the
// similarity matrix; chunked sort for large vaults).  The selected (value, index) pairs, the
// discrepancy and the caption similarity are bit-identical whichever path served a query: every
// path ranks with the one `better`, insert, wave selection and sort network below and ends in the
// one top-1 epilogue.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

// S[B][N] = Q[B][D] . V[N][D]^T, fp32 (misinfo_forensics.py:446).  Tile 16 queries x 64 rows,
// 64-deep K chunks staged through LDS with 16-B loads; the next chunk's loads (clamped rows,
// no divergent region) are in flight while the current one is consumed.  Every output is one
// fp32 FMA chain over k = 0 .. D-1 in order.  D % 64 == 0 (host-checked).
__global__ __launch_bounds__(256) void vault_sims_kernel(const float* q, const float* v, float* S, int B, int N,
                                                         int D) {
  constexpr int KC = 64, LD = KC + 4;  // row stride 68 floats: 16-B aligned, rows 4 banks apart
  __shared__ __attribute__((aligned(16))) float qs[16 * LD];
  __shared__ __attribute__((aligned(16))) float vs[64 * LD];
  const int tid = threadIdx.x, tq = tid >> 4, tv = tid & 15;
  const int q0 = blockIdx.y * 16, v0 = blockIdx.x * 64;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // this thread's chunk pieces: one float4 of Q (row tid / 16, col 4 (tid % 16)), four of V
  const int qr = tid >> 4, qc = (tid & 15) * 4;
  const float* qp = q + (size_t)min(q0 + qr, B - 1) * D + qc;
  const float* vp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) vp[i] = v + (size_t)min(v0 + qr + 16 * i, N - 1) * D + qc;
  float4 rq, rv[4];
  auto load = [&](int k0) {
    rq = *reinterpret_cast<const float4*>(qp + k0);
#pragma unroll
    for (int i = 0; i < 4; ++i) rv[i] = *reinterpret_cast<const float4*>(vp[i] + k0);
  };
  load(0);
  for (int k0 = 0; k0 < D; k0 += KC) {
    *reinterpret_cast<float4*>(qs + qr * LD + qc) = rq;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(vs + (qr + 16 * i) * LD + qc) = rv[i];
    __syncthreads();
    if (k0 + KC < D) load(k0 + KC);
#pragma unroll 16
    for (int k = 0; k < KC; ++k) {
      const float a = qs[tq * LD + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(a, vs[(tv + 16 * j) * LD + k], acc[j]);
    }
    __syncthreads();
  }
  if (q0 + tq < B) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (v0 + tv + 16 * j < N) S[(size_t)(q0 + tq) * N + v0 + tv + 16 * j] = acc[j];
  }
}

// The same similarities on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fmaf
// chain, as effnet_f32.hip's pw32m): BIT-IDENTICAL to vault_sims_kernel (every output the chain over
// k = 0 .. D-1 in order from 0) at the MFMA rate -- the launch sits on the step's serial tail.  Block
// = 64 vault rows x 16 queries, wave w = vault rows 16 w .. 16 w + 15; K in 16-deep chunks staged
// through LDS k-transposed ([row][g][s] = X[row][4 s + g]: a lane of group g reads its four steps'
// operands k = g, 4 + g, 8 + g, 12 + g with one ds_read_b128; step s covers k = 4 s .. 4 s + 3 in
// lane-group order), the next chunk's loads in flight under the current one's MFMAs.  Vault rows are
// the MFMA's A operand, so each lane ends with 4 consecutive vault rows of one query: 16-B stores.
__device__ __forceinline__ int vq_off(int row, int g) { return row * 16 + ((g ^ (((row >> 3) & 1) << 1)) << 2); }

// CH 16-deep chunks per LDS stage (one barrier per 16 CH of K; D % (16 CH) == 0, host-checked): the
// same chunk images and MFMA order as CH = 1, so the same ascending-k chains
template <int CH>
__global__ __launch_bounds__(256) void vault_sims_mfma_kernel(const float* __restrict__ q, const float* __restrict__ v,
                                                              float* __restrict__ S, int B, int N, int D) {
  __shared__ __attribute__((aligned(16))) float qs[2][CH][16 * 16];
  __shared__ __attribute__((aligned(16))) float vs[2][CH][64 * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * 64, b0 = blockIdx.y * 16;
  // loaders: V chunk 64 x 16 = one float4 per thread (row lr, k quad lc); Q chunk 16 x 16 = threads 0-63
  const int lr = tid >> 2, lc = tid & 3;
  const float* vp = v + (size_t)min(n0 + lr, N - 1) * D + lc * 4;  // clamped rows: loaded, never stored
  const float* qp = q + (size_t)min(b0 + (lr & 15), B - 1) * D + lc * 4;
  float4 rv[CH], rq[CH];
  auto gload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      rv[h] = *reinterpret_cast<const float4*>(vp + k0 + 16 * h);
      rq[h] = *reinterpret_cast<const float4*>(qp + k0 + 16 * h);
    }
  };
  auto lstore = [&](int buf) {  // k = 4 lc + e -> [row][g = e][s = lc]
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const float av[4] = {rv[h].x, rv[h].y, rv[h].z, rv[h].w}, bv[4] = {rq[h].x, rq[h].y, rq[h].z, rq[h].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) vs[buf][h][vq_off(lr, e) + lc] = av[e];
      if (tid < 64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) qs[buf][h][vq_off(lr, e) + lc] = bv[e];
      }
    }
  };
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nst = D / (16 * CH);
  gload(0);
  lstore(0);
  __syncthreads();
  for (int c = 0; c < nst; ++c) {
    const int buf = c & 1;
    if (c + 1 < nst) gload((c + 1) * 16 * CH);
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const float4 wf = *reinterpret_cast<const float4*>(&vs[buf][h][vq_off(wave * 16 + fr, fg)]);
      const float4 xf = *reinterpret_cast<const float4*>(&qs[buf][h][vq_off(fr, fg)]);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.x, xf.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.y, xf.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.z, xf.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.w, xf.w, acc, 0, 0, 0);
    }
    if (c + 1 < nst) lstore(buf ^ 1);
    __syncthreads();
  }
  // lane: S[query b0 + fr][vault rows n .. n + 3], n = n0 + 16 wave + 4 fg
  const int b = b0 + fr, n = n0 + wave * 16 + fg * 4;
  if (b < B) {
    float* dst = S + (size_t)b * N + n;
    if (n + 3 < N && ((N & 3) == 0)) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) dst[r] = acc[r];
    }
  }
}

// Ranking of the reference's np.argsort(sims)[-k:][::-1] (misinfo_forensics.py:449): value
// descending; numpy sorts NaN (a zero-norm vault row: 0/0 in the renormalisation, :443-445) after
// every number, so the reversed tail puts NaN rows FIRST.  The scans rank by a key: the similarity,
// with NaN mapped to +inf (a cosine of unit rows is never +inf) and mapped back on output; empty
// slots hold -inf with index -1.  Exact ties: numpy's default sort is not stable (its tie order is
// data- and platform-dependent); ties are ordered here by descending index = what a
// stable argsort would give.
MMF_DEV float rank_key(float v) { return v != v ? INFINITY : v; }
MMF_DEV float unkey(float k) { return k == INFINITY ? NAN : k; }
MMF_DEV bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia > ib); }

// (v, vi) into a lane's sorted top-K list
template <int K>
MMF_DEV void topk_insert(float (&tv)[K], int (&ti)[K], float v, int vi) {
  if (better(v, vi, tv[K - 1], ti[K - 1])) {
    tv[K - 1] = v; ti[K - 1] = vi;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
      if (better(tv[i], ti[i], tv[i - 1], ti[i - 1])) {
        const float a = tv[i]; tv[i] = tv[i - 1]; tv[i - 1] = a;
        const int b = ti[i]; ti[i] = ti[i - 1]; ti[i - 1] = b;
      }
    }
  }
}

// the wave's top K of its lanes' sorted lists of length L (K rounds of a wave arg-max over the heads,
// the winning lane pops), valid on every lane
template <int K, int L>
MMF_DEV void wave_topk(float (&tv)[L], int (&ti)[L], float (&outv)[K], int (&outi)[K]) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    float bv = tv[0];
    int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    outv[t] = bv; outi[t] = bi;
    if (ti[0] == bi) {
#pragma unroll
      for (int i = 0; i < L - 1; ++i) { tv[i] = tv[i + 1]; ti[i] = ti[i + 1]; }
      tv[L - 1] = -INFINITY; ti[L - 1] = -1;
    }
  }
}

// key[P] / id[P] in LDS, filled and barriered by the caller, sorted descending under `better` by a
// 1024-thread block (bitonic network); ends with a barrier
template <int P>
MMF_DEV void block_sort_desc(float (&key)[P], int (&id)[P], int tid) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P / 2; i += 1024) {
        const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
        const bool desc = (lo & size) == 0;  // descending segments; the final pass is all-descending
        const float a = key[lo], b = key[hi];
        const int ia = id[lo], ib = id[hi];
        if (desc ? better(b, ib, a, ia) : better(a, ia, b, ib)) {
          key[lo] = b; key[hi] = a;
          id[lo] = ib; id[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
}

// What follows from a query's best candidate (key0, id0), by one full wave that holds it on every
// lane: the discrepancy and the caption-title cosine.  (The k results are stored by each kernel.)
MMF_DEV void vault_top1(const VaultOut& o, int row, float key0, int id0, int lane) {
  const bool hit = key0 > o.thresh && key0 != INFINITY;  // NaN > thresh is false (so a hit is finite)
  if (lane == 0 && o.disc) o.disc[(size_t)row * o.disc_stride] = hit ? key0 : 0.f;
  if (o.tsim) {
    float d = 0.f;
    if (hit && o.temb && o.title)
      d = wave_rowdot(o.temb + (size_t)row * o.D, o.title + (size_t)id0 * o.D, o.D, lane);
    if (lane == 0) o.tsim[row] = d;
  }
}

// One 256-thread block per query row: each wave keeps per-lane top-K lists over its share of the
// columns (columns w * 64 + lane + 256 i, 8 loads in flight per lane), reduces them to the wave's
// top-K, and wave 0 merges the four waves' 4K candidates.  `better` is a strict total order (value,
// then index), so the K selected (value, index) pairs do not depend on how the columns were split.
template <int K>
__global__ __launch_bounds__(256) void vault_topk_kernel(const float* S, int B, int N, VaultOut o) {
  static_assert(4 * K <= 64, "wave 0 holds the 4K candidates one per lane");
  __shared__ float cv[4 * K];
  __shared__ int ci[4 * K];
  const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (row >= B) return;  // (uniform per block)
  float tv[K], outv[K];
  int ti[K], outi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { tv[i] = -INFINITY; ti[i] = -1; }
  const float* s = S + (size_t)row * N;
  for (int j0 = wave * 64 + lane; j0 < N; j0 += 256 * 8) {
    float vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) vv[u] = (j0 + 256 * u < N) ? rank_key(s[j0 + 256 * u]) : -INFINITY;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + 256 * u < N) topk_insert<K>(tv, ti, vv[u], j0 + 256 * u);
  }
  wave_topk<K>(tv, ti, outv, outi);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < K; ++t) { cv[wave * K + t] = outv[t]; ci[wave * K + t] = outi[t]; }
  }
  __syncthreads();
  if (wave != 0) return;
  // merge: lane l < 4K holds candidate l, a list of one
  float mv[1] = {lane < 4 * K ? cv[lane] : -INFINITY};
  int mi[1] = {lane < 4 * K ? ci[lane] : -1};
  wave_topk<K>(mv, mi, outv, outi);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (o.sims) o.sims[(size_t)row * K + t] = unkey(outv[t]);
      if (o.idx) o.idx[(size_t)row * K + t] = outi[t];
    }
  }
  vault_top1(o, row, outv[0], outi[0], lane);
}

// top-k for k > 8 (search_vault's top_k is a free parameter): one 1024-thread block per query row
// sorts n candidates (padded to P, a power of two; n <= P <= 16384, 128 KB of LDS) with the network
// above, then writes the first k.  The candidates are the row's n = N similarities S[row][0 .. N)
// or, CAND, for a vault of more than 16384 rows walked in chunks of chunk_rows rows (each through the
// similarity kernel and this one), the chunks' top-k results src / cidx [chunk][B][k] (similarities
// with NaN restored, chunk-local indices, -1 padding), n = chunks * k.
template <int P, bool CAND>
__global__ __launch_bounds__(1024) void vault_sort_kernel(const float* src, const int32_t* cidx, int n, int chunk_rows,
                                                          int B, int k, VaultOut o) {
  __shared__ float key[P];
  __shared__ int id[P];
  const int row = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < P; i += 1024) {
    float kv = -INFINITY;
    int ki = -1;
    if constexpr (CAND) {
      if (i < n) {
        const int c = i / k;
        const size_t at = ((size_t)c * B + row) * k + i % k;
        const int li = cidx[at];
        if (li >= 0) { kv = rank_key(src[at]); ki = c * chunk_rows + li; }
      }
    } else if (i < n) {
      kv = rank_key(src[(size_t)row * n + i]);
      ki = i;
    }
    key[i] = kv;
    id[i] = ki;
  }
  __syncthreads();
  block_sort_desc<P>(key, id, tid);
  for (int t = tid; t < k; t += 1024) {
    if (o.sims) o.sims[(size_t)row * k + t] = unkey(key[t]);
    if (o.idx) o.idx[(size_t)row * k + t] = id[t];
  }
  if (tid < 64) vault_top1(o, row, key[0], id[0], tid);
}

// ---------------------------------------------------------------------------------------------
// Fused similarity + top-k (mmf_vault_search_rows, option vault_fused): the result of
// vault_sims_mfma_kernel + vault_topk_kernel without S[B][N].  Every similarity is the same chain
// (v_mfma_f32_16x16x4_f32 over k = 0 .. 511 in order from 0, vault rows = A operand) and the ranking
// the same `better` order, so the selected (value, index) pairs are bit-identical.
//
// Partial kernel: grid (nblocks, ceil(B / 64)).  A block keeps its 64 queries in LDS for the whole
// kernel (four 16-query groups x 32 chunk images in vault_sims_mfma_kernel's k-transposed layout,
// 128 KB; rows past B are zero) and walks a contiguous range of 64-row vault tiles; wave w owns rows
// 16 w .. 16 w + 15 of each tile.  A wave fetches its 16 x 512 slice once per tile with 16-B loads
// (the next tile's loads are in flight while this one is consumed -- they are the only global loads
// of the loop, so nothing queues behind them), turns it into the MFMA's A layout through a 4 KB
// wave-private LDS scratch and holds it in 128 registers; the query groups then stream past it two
// at a time, one accumulator each, so the 40-cycle dependent MFMA latency hides behind the other
// chain's 32-cycle issue.  The loop has no block barrier.  Each lane keeps a register top-K per query
// group (its query 16 j + lane % 16, the rows it saw); at the end the 16 lists of a query (4 waves x
// 4 lane groups) meet in LDS and one thread per query writes the block's K candidates.
constexpr int kVsQ = 64;        // queries per block
constexpr int kVsAuto = 256;    // blocks of the automatic grid (one per CU: the block owns the LDS)

template <int K>
__global__ __launch_bounds__(256) void vault_search_partial_kernel(const float* __restrict__ q,
                                                                   const float* __restrict__ v, int B, int N,
                                                                   float* __restrict__ cv, int* __restrict__ ci) {
  __shared__ __attribute__((aligned(16))) float qs[4][32][16 * 16];  // [group][chunk][vq_off image]
  __shared__ __attribute__((aligned(16))) float ts[4][4][16 * 16];   // per wave: four chunk images
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int tiles = (N + 63) / 64, nb = gridDim.x;
  const int t0 = (int)((long long)blockIdx.x * tiles / nb), t1 = (int)((long long)(blockIdx.x + 1) * tiles / nb);
  const int q0 = blockIdx.y * kVsQ;
  const int ng = min(4, (B - q0 + 15) / 16);  // query groups of this block (>= 1)
  // the block's queries -> LDS: thread = (row tid / 4, k quad tid % 4) of a 16 x 16 chunk, as the
  // similarity kernel's loader; wave j stages group j
  {
    const int lr = lane >> 2, lc = lane & 3, b = q0 + wave * 16 + lr;
    const float* qp = q + (size_t)min(b, B - 1) * 512 + lc * 4;
#pragma unroll 4
    for (int h = 0; h < 32; ++h) {
      float4 x = *reinterpret_cast<const float4*>(qp + 16 * h);
      if (b >= B) x = make_float4(0.f, 0.f, 0.f, 0.f);
      const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) qs[wave][h][vq_off(lr, e) + lc] = xv[e];
    }
  }
  __syncthreads();
  float tv[4][K];
  int ti[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < K; ++i) { tv[j][i] = -INFINITY; ti[j][i] = -1; }
  // the wave's slice of a tile: lane = (row lane / 4, k quad lane % 4), 32 chunks
  const int lr = lane >> 2, lc = lane & 3;
  float4 rv[32];
  auto gload = [&](int t) {
    const float* vp = v + (size_t)min(t * 64 + wave * 16 + lr, N - 1) * 512 + lc * 4;  // clamped: loaded, never ranked
#pragma unroll
    for (int h = 0; h < 32; ++h) rv[h] = *reinterpret_cast<const float4*>(vp + 16 * h);
  };
  if (t0 < t1) gload(t0);
  for (int t = t0; t < t1; ++t) {
    // A layout through the wave's scratch, four chunks a round (the LDS serves a wave's accesses in
    // order; the wave barriers keep the compiler from moving them across each other)
    float4 a[32];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 x = rv[4 * r + c];
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) ts[wave][c][vq_off(lr, e) + lc] = xv[e];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < 4; ++c) a[4 * r + c] = *reinterpret_cast<const float4*>(&ts[wave][c][vq_off(fr, fg)]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (t + 1 < t1) gload(t + 1);
    const int n = t * 64 + wave * 16 + fg * 4;  // lane: rows n .. n + 3 of query 16 j + fr
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (2 * p >= ng) break;  // (uniform per block)
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 32; ++h) {
        const float4 x0 = *reinterpret_cast<const float4*>(&qs[2 * p][h][vq_off(fr, fg)]);
        const float4 x1 = *reinterpret_cast<const float4*>(&qs[2 * p + 1][h][vq_off(fr, fg)]);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].x, x0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].x, x1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].y, x0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].y, x1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].z, x0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].z, x1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].w, x0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h].w, x1.w, acc1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) topk_insert<K>(tv[2 * p], ti[2 * p], rank_key(acc0[r]), n + r);
      if (2 * p + 1 < ng) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) topk_insert<K>(tv[2 * p + 1], ti[2 * p + 1], rank_key(acc1[r]), n + r);
      }
    }
  }
  // the 16 lists of a query -> LDS (over the query images, which every wave is done with), one
  // thread per query selects the block's K
  __syncthreads();
  float* lv = &qs[0][0][0];                                  // [source 16][K][query 64]
  int* li = reinterpret_cast<int*>(&qs[0][0][0]) + 16 * K * kVsQ;
  const int src = wave * 4 + fg;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < K; ++i) {
      lv[(src * K + i) * kVsQ + 16 * j + fr] = tv[j][i];
      li[(src * K + i) * kVsQ + 16 * j + fr] = ti[j][i];
    }
  __syncthreads();
  if (tid < kVsQ && q0 + tid < B) {
    float bv[K];
    int bi[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { bv[i] = -INFINITY; bi[i] = -1; }
    for (int c = 0; c < 16 * K; ++c) {
      const int vi = li[c * kVsQ + tid];
      if (vi >= 0) topk_insert<K>(bv, bi, lv[c * kVsQ + tid], vi);
    }
    const size_t o = ((size_t)blockIdx.x * B + q0 + tid) * K;
#pragma unroll
    for (int i = 0; i < K; ++i) { cv[o + i] = bv[i]; ci[o + i] = bi[i]; }
  }
}

// Merge kernel: one wave per query ranks the nblocks * K candidates (keys, as the partial kernel
// left them) and ends as vault_topk_kernel does.
template <int K>
__global__ __launch_bounds__(64) void vault_search_merge_kernel(const float* __restrict__ cv, const int* __restrict__ ci,
                                                                int nblocks, int B, VaultOut o) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float tv[K], outv[K];
  int ti[K], outi[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { tv[i] = -INFINITY; ti[i] = -1; }
  for (int c = lane; c < nblocks * K; c += 64) {
    const size_t at = ((size_t)(c / K) * B + row) * K + c % K;
    const int vi = ci[at];
    if (vi >= 0) topk_insert<K>(tv, ti, cv[at], vi);
  }
  wave_topk<K>(tv, ti, outv, outi);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (o.sims) o.sims[(size_t)row * K + t] = unkey(outv[t]);
      if (o.idx) o.idx[(size_t)row * K + t] = outi[t];
    }
  }
  vault_top1(o, row, outv[0], outi[0], lane);
}

// f(std::integral_constant<int, V>) for the first of the compile-time sizes Vs (ascending) that holds
// the run-time n; false, with nothing called, if none does.  Over 1 .. 8 it turns a top_k >= 1 into
// the register kernels' K, over the sort sizes a candidate count into P.
template <int... Vs, class F>
bool with_size(long long n, F&& f) {
  return ((n <= Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace

#ifndef MMF_VAULT_CH
#define MMF_VAULT_CH 4  // 16-deep K chunks per LDS stage / barrier
#endif
hipError_t launch_vault_sims(const float* q, const float* v, float* S, int B, int N, int D, hipStream_t s, int ref) {
  if (D & 63) return hipErrorInvalidValue;
  if (B <= 0 || N <= 0) return hipSuccess;
  // the fp32-MFMA kernel; ref (option vault_ref, diagnostic): the VALU kernel it is bit-identical to
  // (tests/test_gpu_vault_edge.py::test_vault_kernels_match_reference_kernels)
  if (ref)
    hipLaunchKernelGGL(vault_sims_kernel, dim3((N + 63) / 64, (B + 15) / 16), dim3(256), 0, s, q, v, S, B, N, D);
  else if ((D % (16 * MMF_VAULT_CH)) == 0)
    hipLaunchKernelGGL(vault_sims_mfma_kernel<MMF_VAULT_CH>, dim3((N + 63) / 64, (B + 15) / 16), dim3(256), 0, s, q, v, S, B, N, D);
  else
    hipLaunchKernelGGL(vault_sims_mfma_kernel<1>, dim3((N + 63) / 64, (B + 15) / 16), dim3(256), 0, s, q, v, S, B, N, D);
  return hipGetLastError();
}

hipError_t launch_vault_topk(const float* S, int B, int N, int k, const VaultOut& out, hipStream_t s, int ref) {
  // k > N is the reference's argsort(...)[-k:] on a short vault: it keeps all N rows.  The
  // register kernels pad slots N..k-1 with (-inf, -1) (the host drops idx < 0), so a fixed k = 5
  // (mmf_analyze_batch) serves a vault of any size; the sort kernel pads the same way up to P.
  if (k < 1 || N < 1) return hipErrorInvalidValue;
  // ref (option vault_ref, diagnostic): every k through the full-sort kernel -- an independent
  // selection algorithm the register kernels must agree with bit for bit
  const bool ok = k <= 8 && !(ref && N <= 16384)
      ? with_size<1, 2, 3, 4, 5, 6, 7, 8>(k, [&](auto K) {  // one block (four waves) per query row
          hipLaunchKernelGGL(vault_topk_kernel<decltype(K)::value>, dim3(B), dim3(256), 0, s, S, B, N, out);
        })
      : with_size<2048, 4096, 8192, 16384>(std::max(N, k), [&](auto P) {
          hipLaunchKernelGGL((vault_sort_kernel<decltype(P)::value, false>), dim3(B), dim3(1024), 0, s, S, nullptr, N,
                             0, B, k, out);
        });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

int vault_search_blocks(int B, int N, int nblocks) {
  if (nblocks > 0) return nblocks;
  const int tiles = (N + 63) / 64, gy = (B + kVsQ - 1) / kVsQ;
  return std::max(1, std::min(tiles, kVsAuto / gy));
}

size_t vault_search_ws_bytes(int B, int k, int nblocks) {
  return (size_t)(nblocks > 0 ? nblocks : kVsAuto) * B * k * (sizeof(float) + sizeof(int32_t));
}

hipError_t launch_vault_search(const float* q, const float* v, int B, int N, int k, const VaultOut& out, void* ws,
                               int nblocks, hipStream_t s) {
  if (B < 1 || N < 1 || k < 1 || k > 8 || nblocks < 0 || !ws) return hipErrorInvalidValue;
  const int nb = vault_search_blocks(B, N, nblocks);
  float* cv = (float*)ws;
  int* ci = (int*)(cv + (size_t)nb * B * k);
  const dim3 grid(nb, (B + kVsQ - 1) / kVsQ);
  with_size<1, 2, 3, 4, 5, 6, 7, 8>(k, [&](auto K) {
    hipLaunchKernelGGL(vault_search_partial_kernel<decltype(K)::value>, grid, dim3(256), 0, s, q, v, B, N, cv, ci);
    hipLaunchKernelGGL(vault_search_merge_kernel<decltype(K)::value>, dim3(B), dim3(64), 0, s, cv, ci, nb, B, out);
  });
  return hipGetLastError();
}

hipError_t launch_vault_sort_cand(const float* cs, const int32_t* cidx, int chunks, int chunk_rows, int B, int k,
                                  const VaultOut& out, hipStream_t s) {
  if (chunks < 1 || k < 1 || B < 1) return hipErrorInvalidValue;
  const bool ok = with_size<2048, 16384>((long long)chunks * k, [&](auto P) {
    hipLaunchKernelGGL((vault_sort_kernel<decltype(P)::value, true>), dim3(B), dim3(1024), 0, s, cs, cidx, chunks * k,
                       chunk_rows, B, k, out);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

