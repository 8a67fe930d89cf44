// The persistent LDS-DMA GEMM's body (gemm.hip), included by gemm_glds_kernel (first tile = wgid).
// (Round 5 also included it into a grouped two-problem kernel, option clip_group, measured slower and
// removed; as a plain __global__ body it keeps the production kernels' code generation.)  Expects the
// template parameters BM, BN, WGM, WGN, ACT, PIPE2, EPI, DBG, the arguments g, tilesN, tiles, tilesM,
// gm, and MMF_GLDS_FIRST_TILE (an expression of wgid and nwg).
  // Persistent: one 512-thread workgroup per CU walks tiles t = i*gridDim + wgid.  The first
  // K-slab of the NEXT tile is DMA'd into the free LDS stage during the current tile's last
  // K-step, so only the very first tile pays the load latency and each epilogue's stores drain
  // underneath the next tile's first MFMAs.
  constexpr int NW = WGM * WGN;
  constexpr int TM = BM / WGM, TN = BN / WGN, MI = TM / 16, NI = TN / 16;
  constexpr int STAGE = (BM + BN) * BK;
  static_assert(NW == 8 && BM == 256, "8 waves, 256-row tiles");
  // EPI 3 (attention epilogue, RoBERTa QKV): a 40 KB gap between the two stages, so that the stage
  // the last K-step freed plus the gap hold q (32 KB) and k | v (64 KB) of the tile's two sequences
  // EPI 5 / 6 (CLIP QKV, 6 = causal): the lazy-LN consumer with the attention of the tile's S = 256 / L
  // whole sequences in its epilogue (attention_epilogue_seq); row panel tm starts at row tm * S * L
  constexpr bool ATTG = EPI == 5 || EPI == 6;
  constexpr bool ATT = EPI == 3 || ATTG;
  constexpr bool LNC = EPI == 1 || ATTG;  // lazy-LN consumer: (mean, rstd) from partials, u and c through LDS
  static_assert(!ATT || (BM == 256 && BN == 192 && WGM == 4 && WGN == 2 && PIPE2), "attention epilogue: 256x192");
  constexpr int XGAP = ATT ? 20480 : 0;  // f16 elements
  constexpr int SOFF = STAGE + XGAP;     // stage 1's offset
  constexpr bool ROWST = LNC;  // reads row statistics
  static_assert(EPI == 0 || BM == 256, "lazy-LN epilogues assume 256-row tiles");
  // ONE __shared__ object, carved: the operand stages | row partials | column vectors | row stats.
  // With a second LDS object in the kernel, hipcc's wait-count pass gives every LDS access alias
  // scopes and then cannot tell a fragment read of stage `cur` from an LDS-DMA into stage `cur ^ 1`
  // of the same object: it puts vmcnt(0) before each read that follows a DMA instruction (measured:
  // the interleaved DMA issue below ran the EPI 1 / 3 GEMMs 24-65 % slower until this was one object).
  // column vectors of a consumer tile: u | bias (bias through LDS frees the 4*NI bias registers the
  // plain path holds across the K loop); ATT: the key mask bias
  constexpr int kBiasCol = 256;
  // ATTG byte budget (163,840 available): stages 2 x 57,344 + gap 40,960 = 155,648 | u, c 2,048 | row
  // stats 2,048 | key bias 2,048 | zero row 128 = 161,920.  The 16 KB of row partials alias the head of the
  // gap: they are consumed at the third K-step, the gap is written only by the epilogue.
  constexpr int kStageB = (2 * STAGE + XGAP) * 2, kRowsB = (ROWST && !ATTG) ? BM * kLnPMax * 8 : 0;
  constexpr int kColsB = (ROWST || ATT) ? 512 * 4 : 0, kStatB = ROWST ? BM * 8 : 0;
  constexpr int kAttB = ATTG ? 512 * 4 + 128 : 0;  // key bias [S][LK] (S * LK <= 512) | a 128-B row of zeros
  __shared__ __attribute__((aligned(16))) char smem[kStageB + kRowsB + kColsB + kStatB + kAttB];
  static_assert(sizeof(smem) <= 160 * 1024, "LDS");
  f16_t* const lds = reinterpret_cast<f16_t*>(smem);
  float2* const lds_rows = reinterpret_cast<float2*>(smem + (ATTG ? STAGE * 2 : kStageB));
  float* const lds_cols = reinterpret_cast<float*>(smem + kStageB + kRowsB);
  float2* const lds_stat = reinterpret_cast<float2*>(smem + kStageB + kRowsB + kColsB);  // (mean, rstd) per row
  float* const lds_kbias = reinterpret_cast<float*>(smem + kStageB + kRowsB + kColsB + kStatB);
  f16_t* const lds_zrow = reinterpret_cast<f16_t*>(smem + kStageB + kRowsB + kColsB + kStatB + 512 * 4);

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int M = g.M, N = g.N;
  const int nk = g.K / BK;
  const int fr = lane & 15, fg = lane >> 4;
  const bool has_res = g.res32 || g.res16;
  const bool full8 = (N & 7) == 0;
  // byte extents of the epilogue operands (run_glds keeps them, and every offset formed below
  // for a row < M + BM, under 2^31)
  const uint32_t out_elems = (uint32_t)(M - 1) * g.ldc + (EPI == 4 && g.split_lo ? 3 * N : N);  // (EPI 4: hi | lo | hi)
  const rsrc_t rbias = make_rsrc(g.bias, (uint32_t)N * 4u);
  const rsrc_t rres = make_rsrc(g.res32 ? (const void*)g.res32 : (const void*)g.res16,
                                ((uint32_t)(M - 1) * g.ldr + N) * (g.res32 ? 4u : 2u));
  const rsrc_t rc32 = make_rsrc(g.c32, out_elems * 4u);
  const rsrc_t rc16 = make_rsrc(g.c16, out_elems * 2u);

  int t = MMF_GLDS_FIRST_TILE;
  if (t >= tiles) return;
  // ATTG: rows per panel = the whole sequences a 256-row tile holds; the partials through a descriptor
  // over the buffer's whole 256-row blocks (a panel's 256 rows may end past them: those read as zeros)
  int att_S = 0, att_rows = BM;
  if constexpr (ATTG) {
    att_S = BM / g.att_L;
    att_rows = att_S * g.att_L;
    if (tid < 32) reinterpret_cast<uint32_t*>(lds_zrow)[tid] = 0u;  // (visible after the first barrier below)
  }
  const rsrc_t rstat = make_rsrc(ATTG ? g.ln_in : nullptr, (uint32_t)((M + BM - 1) / BM * BM) * (uint32_t)g.ln_in_P * 8u);
  // first row of row panel tm
  auto row0_of = [&](int tm_) { return ATTG ? tm_ * att_rows : tm_ * BM; };
  GST_INIT()
  int tnext = 0;
  // s_setprio 1 for waves 0-3 (+0.4 % on the step, round-1 A/B; the old option gemm_prio = 2)
  if (wave < NW / 2) __builtin_amdgcn_s_setprio(1);
  // descriptor fills (glds_tile_buf) for every full row / column panel whose operand's byte extent
  // fits 32 bits: the per-lane source offset is one loop-invariant
  // VGPR and the panel base rides in the scalar soffset, so a K-step's DMA issue costs no VALU
  // (glds_tile: a clamped row and a 64-bit address per piece, ~6 VALU each, every K-step)
  const bool bufA = MMF_GLDS_BUF && (size_t)M * g.lda * 2 < ((size_t)1 << 32);
  const bool bufW = MMF_GLDS_BUF && (size_t)N * g.ldw * 2 < ((size_t)1 << 32);
  const rsrc_t ra = make_rsrc(g.A, bufA ? (uint32_t)((size_t)M * g.lda * 2) : 0u);
  const rsrc_t rw = make_rsrc(g.W, bufW ? (uint32_t)((size_t)N * g.ldw * 2) : 0u);
  const uint32_t lchunk = (uint32_t)(((lane & 7) ^ (lane >> 3)) * 16);
  const uint32_t aoff = (uint32_t)(lane >> 3) * (uint32_t)g.lda * 2u + lchunk;
  const uint32_t woff = (uint32_t)(lane >> 3) * (uint32_t)g.ldw * 2u + lchunk;
  auto stage = [&](int buf, int tile, int kt) {
    if constexpr (DBG == 2) return;
    int tm_, tn_;
    tile_coords(tile, tilesM, tilesN, gm, tm_, tn_);
    f16_t* nb = lds + buf * SOFF;
    if (bufA && row0_of(tm_) + BM <= M)
      glds_tile_buf<BM, NW>(ra, (uint32_t)g.lda * 2u, row0_of(tm_), kt * BK, aoff, nb, wave);
    else glds_tile<BM, NW>(g.A, g.lda, row0_of(tm_), M, kt * BK, nb, wave, lane);
    if (bufW && tn_ * BN + BN <= N)
      glds_tile_buf<BN, NW>(rw, (uint32_t)g.ldw * 2u, tn_ * BN, kt * BK, woff, nb + BM * BK, wave);
    else glds_tile<BN, NW>(g.W, g.ldw, tn_ * BN, N, kt * BK, nb + BM * BK, wave, lane);
  };
  // MMF_DMA_ILV (PIPE2 K loop): the next slab's LDS-DMA pieces are issued BETWEEN the first half-step's
  // MFMAs instead of all before them.  Per-phase stamps (-DMMF_GEMM_STAMP=2) put ~800-1050 cycles of a
  // 2,800-3,500-cycle K-step in the issue of a wave's 7-8 DMA instructions alone: the CU's LDS-DMA
  // path takes ~16 cycles per 1-KB piece, 56-64 pieces per step, and every wave stalled in that queue
  // before its first MFMA.  Interleaved, the queue drains under the MFMAs.  Branch-free pieces (the
  // scheduler interleaves only within a basic block): every piece through the buffer descriptor with
  // its whole offset in the range-checked voffset (rows past M / N read as zeros -- their outputs
  // are never stored), and on the very last K-step of the last tile a harmless reload of the current
  // tile's first slab into the stage nobody reads again.
  constexpr int PA = BM / (8 * NW), PW = BN / (8 * NW);  // DMA pieces per wave: A rows, W rows
  auto dma_piece = [&](int j, int buf, uint32_t abase, uint32_t wbase) {
    f16_t* nb = lds + buf * SOFF;
    if (j < PA) {
      const int seg = wave * PA + j;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)((__attribute__((address_space(3))) f16_t*)nb + seg * 512),
                                               16, aoff + abase + (uint32_t)(seg * 8) * (uint32_t)g.lda * 2u, 0, 0, 0);
    } else {
      const int seg = wave * PW + (j - PA);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rw, (lds_void_t*)((__attribute__((address_space(3))) f16_t*)nb + BM * BK + seg * 512), 16,
          woff + wbase + (uint32_t)(seg * 8) * (uint32_t)g.ldw * 2u, 0, 0, 0);
    }
  };
  // lazy-LN epilogue operands of tile (m0_, n0_) -> LDS (issued in the second K-step: every wave
  // has left the previous tile's epilogue by then; the K-step barriers' vmcnt(0) covers them)
  auto epi_dma = [&](int m0_, int n0_) {
    typedef __attribute__((address_space(3))) char lds_char_t;
    if constexpr (ATTG) {
      const uint32_t bytes = (uint32_t)BM * g.ln_in_P * 8u, base = (uint32_t)m0_ * (uint32_t)g.ln_in_P * 8u;
      for (uint32_t off = (uint32_t)wave * 1024u; off < bytes; off += NW * 1024u)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rstat, (lds_void_t*)((lds_char_t*)lds_rows + off), 16,
                                                 base + off + (uint32_t)lane * 16u, 0, 0, 0);
    } else if constexpr (ROWST) {  // the 256 rows' partials: 256 * P * 8 B, contiguous, whole KBs
      const uint32_t bytes = (uint32_t)BM * g.ln_in_P * 8u;
      const char* src = reinterpret_cast<const char*>(g.ln_in) + (size_t)m0_ * g.ln_in_P * 8;
      for (uint32_t off = (uint32_t)wave * 1024u; off < bytes; off += NW * 1024u)
        __builtin_amdgcn_global_load_lds((const void*)(src + off + lane * 16),
                                         (lds_void_t*)((lds_char_t*)lds_rows + off), 16, 0, 0);
    }
    if constexpr (LNC) {  // u[n0 .. n0 + 256)
      if (wave == NW - 1)
        __builtin_amdgcn_global_load_lds((const void*)(g.ln_u + n0_ + lane * 4), (lds_void_t*)lds_cols, 16, 0, 0);
    }
    if constexpr (ROWST) {  // bias[n0 .. n0 + 256) (buffers padded by 256)
      if (wave == NW - 3)
        __builtin_amdgcn_global_load_lds((const void*)(g.bias + n0_ + lane * 4),
                                         (lds_void_t*)((lds_char_t*)lds_cols + kBiasCol * 4), 16, 0, 0);
    }
  };
  stage(0, t, 0);
  __syncthreads();
  int cur = 0;
  for (; t < tiles; t = tnext) {
    tnext = t + nwg;
    GST()  // tile start (= the previous tile's epilogue end)
    int tm, tn;
    tile_coords(t, tilesM, tilesN, gm, tm, tn);
    const int m0 = row0_of(tm), n0 = tn * BN;
    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 bias_r[ROWST ? 1 : NI];  // this lane's epilogue bias columns, fetched under the K loop
    if constexpr (!ROWST) {
#pragma unroll
      for (int i = 0; i < NI; ++i) bias_r[i] = buf_load_f4(rbias, (uint32_t)(n0 + wn * TN + i * 16 + fg * 4) * 4u);
    }
    // bias of fragment column group i (ROWST: from LDS)
    auto bias_of = [&](int i) -> float4 {
      if constexpr (ROWST) return *reinterpret_cast<const float4*>(lds_cols + kBiasCol + wn * TN + i * 16 + fg * 4);
      else return bias_r[i];
    };

    for (int kt = 0; kt < nk; ++kt) {
      GSTP(0)
      if constexpr (ROWST) {
        if (kt == 1) epi_dma(m0, n0);
        if (kt == 2) {
          // the DMA'd partials -> (mean, rstd) of the tile's 256 rows (threads 0-255, one row each,
          // two passes over the LDS partials with a rolled loop: few live registers here, where the
          // K loop's accumulators are live), before this K-step's fragment reads; the epilogue
          // reads them after the K loop's later barriers
          if (tid < BM && BN == 192) {
            // 256x192 tiles have register room: all kLnPMax partial slots read at once, one LDS
            // latency.  Slots p >= P belong to the next rows or lie past the DMA'd block (any bit
            // pattern, NaN included), so they are SELECTED out, never weighted by 0.
            const int P = g.ln_in_P, tnin = g.ln_in_tn, C = LNC ? g.K : N;
            const float2* pr = lds_rows + tid * P;
            float2 pv[kLnPMax];
            float nv[kLnPMax];
#pragma unroll
            for (int pi = 0; pi < kLnPMax; ++pi) {
              const float2 v = pr[pi];
              pv[pi] = pi < P ? v : make_float2(0.f, 0.f);
              nv[pi] = pi < P ? (float)min(C - pi * tnin, tnin) : 0.f;
            }
            // explicit fmaf, the same operation sequence as the rolled loop below: a zero slot adds
            // an exact 0, so both tile widths give bit-identical statistics (the consumer's tile
            // width depends on M, and rows must not change with the batch they run in)
            float s1 = 0.f;
#pragma unroll
            for (int pi = 0; pi < kLnPMax; ++pi) s1 = fmaf(nv[pi], pv[pi].x, s1);
            const float mean = s1 / (float)C;
            float s2 = 0.f;
#pragma unroll
            for (int pi = 0; pi < kLnPMax; ++pi) {
              const float d = pv[pi].x - mean;
              s2 += fmaf(nv[pi] * d, d, pv[pi].y);
            }
            lds_stat[tid] = make_float2(mean, rsqrtf(s2 / (float)C + g.ln_eps));
          } else if (tid < BM) {
            const int P = g.ln_in_P, tnin = g.ln_in_tn, C = LNC ? g.K : N;
            const float2* pr = lds_rows + tid * P;
            float s1 = 0.f;
#pragma unroll 1
            for (int pi = 0; pi < P; ++pi) s1 = fmaf((float)min(C - pi * tnin, tnin), pr[pi].x, s1);
            const float mean = s1 / (float)C;
            float s2 = 0.f;
#pragma unroll 1
            for (int pi = 0; pi < P; ++pi) {
              const float2 v = pr[pi];
              const float d = v.x - mean;
              s2 += fmaf((float)min(C - pi * tnin, tnin) * d, d, v.y);
            }
            lds_stat[tid] = make_float2(mean, rsqrtf(s2 / (float)C + g.ln_eps));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // (per tile shape, measured on the B=256 step: 256x256 tiles -3 to -6 % kernel time, the
      // attention-epilogue QKV -2 %; the 256x192 plain / producer tiles +2 to +4 %, so they keep the
      // up-front issue)
      constexpr bool ILV = MMF_DMA_ILV && PIPE2 && DBG == 0 && (BN == 256 || ATT || MMF_ILV_G192 > 0);
      // groups the pieces are spread over (256x192 plain / producer tiles: MMF_ILV_G192, A/B builds)
      constexpr int NG = (BN == 256 || ATT) ? NI : (MMF_ILV_G192 > 0 ? MMF_ILV_G192 : NI);
      uint32_t dma_a = 0, dma_w = 0;  // ILV: byte offsets of the next slab's row panels (wave-uniform)
      if constexpr (ILV) {
        int tm_d = tm, tn_d = tn, kt_d = kt + 1;
        if (kt + 1 >= nk) {
          kt_d = 0;
          if (tnext < tiles) tile_coords(tnext, tilesM, tilesN, gm, tm_d, tn_d);  // (else: reload slab 0 of t)
        }
        dma_a = (uint32_t)row0_of(tm_d) * (uint32_t)g.lda * 2u + (uint32_t)(kt_d * BK) * 2u;
        dma_w = (uint32_t)(tn_d * BN) * (uint32_t)g.ldw * 2u + (uint32_t)(kt_d * BK) * 2u;
      } else if (kt + 1 < nk) {
        stage(cur ^ 1, t, kt + 1);
      } else {
        if (tnext < tiles) stage(cur ^ 1, tnext, 0);
      }
      GSTP(1)
      const f16_t* Xs = lds + cur * SOFF;
      const f16_t* Ws = Xs + BM * BK;
      if constexpr (DBG == 1) {
      } else if constexpr (PIPE2) {
        // half-step pipeline: the second K-half's fragment reads are issued between the first
        // half's MFMAs (1 read per 2 MFMAs), so only the first half's reads are exposed after the
        // barrier
        f16x8 w0[NI], x0[MI], w1[NI], x1[MI];
#pragma unroll
        for (int i = 0; i < NI; ++i) w0[i] = as_f16x8(*reinterpret_cast<const uint4*>(Ws + swz(wn * TN + i * 16 + fr, fg)));
#pragma unroll
        for (int j = 0; j < MI; ++j) x0[j] = as_f16x8(*reinterpret_cast<const uint4*>(Xs + swz(wm * TM + j * 16 + fr, fg)));
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ILV) {
          // NI fenced groups, group i = the MI MFMAs of fragment row i (first half), preceded by its
          // share of the next slab's DMA pieces and of the second half's fragment reads
          constexpr int NP = PA + PW, NRD = NI + MI;
#pragma unroll
          for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int p = i * NP / NG; p < (i + 1) * NP / NG && i < NG; ++p) dma_piece(p, cur ^ 1, dma_a, dma_w);
#pragma unroll
            for (int r = i * NRD / NI; r < (i + 1) * NRD / NI; ++r) {
              if (r < NI) w1[r] = as_f16x8(*reinterpret_cast<const uint4*>(Ws + swz(wn * TN + r * 16 + fr, 4 + fg)));
              else x1[r - NI] = as_f16x8(*reinterpret_cast<const uint4*>(Xs + swz(wm * TM + (r - NI) * 16 + fr, 4 + fg)));
            }
#pragma unroll
            for (int j = 0; j < MI; ++j) acc[i][j] = mfma16x16x32(w0[i], x0[j], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
#pragma unroll
          for (int i = 0; i < NI; ++i)
            w1[i] = as_f16x8(*reinterpret_cast<const uint4*>(Ws + swz(wn * TN + i * 16 + fr, 4 + fg)));
#pragma unroll
          for (int j = 0; j < MI; ++j)
            x1[j] = as_f16x8(*reinterpret_cast<const uint4*>(Xs + swz(wm * TM + j * 16 + fr, 4 + fg)));
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j) acc[i][j] = mfma16x16x32(w0[i], x0[j], acc[i][j]);
#pragma unroll
          for (int q = 0; q < NI + MI; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NI * MI - 2 * (NI + MI), 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < MI; ++j) acc[i][j] = mfma16x16x32(w1[i], x1[j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
      } else if constexpr (BN == 192) {
        // 256x192 (wave tile 64x96): all 20 fragment reads of the K-step first, then its 48 MFMAs,
        // then the barrier -- pinned with sched_barriers (hipcc otherwise interleaves 2 reads +
        // lgkmcnt(0) per 8 MFMAs and sinks MFMAs below the barrier's vmcnt(0)).  Measured: these
        // GEMMs 3 % faster; the same schedule on the 256x256 tiles (24 reads, 64 MFMAs) 3-10 %
        // slower, so they keep the compiler's interleave below.
        f16x8 wf[2][NI], xf[2][MI];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
          for (int i = 0; i < NI; ++i)
            wf[ks][i] = as_f16x8(*reinterpret_cast<const uint4*>(Ws + swz(wn * TN + i * 16 + fr, ks * 4 + fg)));
#pragma unroll
          for (int j = 0; j < MI; ++j)
            xf[ks][j] = as_f16x8(*reinterpret_cast<const uint4*>(Xs + swz(wm * TM + j * 16 + fr, ks * 4 + fg)));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j) acc[i][j] = mfma16x16x32(wf[ks][i], xf[ks][j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          f16x8 wf[NI], xf[MI];
#pragma unroll
          for (int i = 0; i < NI; ++i)
            wf[i] = as_f16x8(*reinterpret_cast<const uint4*>(Ws + swz(wn * TN + i * 16 + fr, ks * 4 + fg)));
#pragma unroll
          for (int j = 0; j < MI; ++j)
            xf[j] = as_f16x8(*reinterpret_cast<const uint4*>(Xs + swz(wm * TM + j * 16 + fr, ks * 4 + fg)));
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j) acc[i][j] = mfma16x16x32(wf[i], xf[j], acc[i][j]);
        }
      }
      GSTP(2)
#ifdef MMF_GEMM_NOVMWAIT
      // measurement build only (outputs wrong): the step barrier without waiting for the next slab's
      // LDS-DMA (lgkmcnt(0) + raw s_barrier) -- how much of the barrier phase is the slab's landing
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_s_barrier();
#else
      __syncthreads();  // vmcnt(0): next stage landed; all reads of `cur` done before it is refilled
#endif
      GSTP(3)
      cur ^= 1;
#ifdef MMF_GEMM_STAMP
      if (kt == 0) GST()  // after the first K-step
#endif
    }
    GST()  // K loop done
    GST_TILE_DONE()

    // Epilogue.  The activation is a compile-time parameter (no per-element branch).  All traffic
    // is raw-buffer: out-of-range rows/columns read 0 / drop their stores, so there is no divergent
    // branch and no load that has to wait on the stores issued before it -- bias columns were
    // fetched at tile start and residual rows are loaded one fragment row AHEAD of the stores (one
    // vmcnt counter covers loads and stores in issue order).
    // lazy LN: (mean, rstd) of fragment row j -> lds_stat[wm * TM + j * 16 + fr] (computed at kt = 2)
    if constexpr (ATTG) {
      // q | k | v of head tn for the tile's 256 rows: r (acc - mean u) + c rounded to fp16 as the EPI 1 store
      // rounds it, into the 96 KB window (the stage the last K-step freed + the gap) as three [256][64]
      // images in attention.hip's swizzle; rows past the last whole sequence are written and never read
      f16_t* const win = lds + ((cur ^ 1) ? SOFF + STAGE - 49152 : 0);
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const int row = wm * TM + j * 16 + fr;
        const float2 st = lds_stat[row];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = wn * TN + i * 16 + fg * 4, part = c >> 6, d = c & 63;
          float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
          const float4 u = *reinterpret_cast<const float4*>(lds_cols + wn * TN + i * 16 + fg * 4);
          v[0] = st.y * (v[0] - st.x * u.x);
          v[1] = st.y * (v[1] - st.x * u.y);
          v[2] = st.y * (v[2] - st.x * u.z);
          v[3] = st.y * (v[3] - st.x * u.w);
          const float4 bi = bias_of(i);
          v[0] += bi.x;
          v[1] += bi.y;
          v[2] += bi.z;
          v[3] += bi.w;
          *reinterpret_cast<uint2*>(win + part * 16384 + swz(row, d >> 3) + (d & 7)) =
              make_uint2(pack2h(v[0], v[1]), pack2h(v[2], v[3]));
        }
      }
      switch ((g.att_L + 31) >> 5) {  // keys padded to 32, as launch_attention picks LK
        case 1: attention_epilogue_seq<32, EPI == 6>(g, win, lds_zrow, lds_kbias, m0, tn, M, att_S, wave, tid); break;
        case 2: attention_epilogue_seq<64, EPI == 6>(g, win, lds_zrow, lds_kbias, m0, tn, M, att_S, wave, tid); break;
        case 3: attention_epilogue_seq<96, EPI == 6>(g, win, lds_zrow, lds_kbias, m0, tn, M, att_S, wave, tid); break;
        default: attention_epilogue_seq<128, EPI == 6>(g, win, lds_zrow, lds_kbias, m0, tn, M, att_S, wave, tid);
      }
      continue;
    } else if constexpr (ATT) {
      attention_epilogue(g, acc, bias_r, lds + ((cur ^ 1) ? SOFF + STAGE - 49152 : 0), lds_cols, m0, tn, M, wm, wn,
                         wave, tid, fr, fg);
      continue;
    }
    if constexpr (EPI == 2) {
      // producer: out = acc + bias + residual, stored fp16 (in place over the residual is allowed:
      // each element is read before it is written, by one lane), then this wave's partial
      // (mean, M2) of the STORED values over its TN columns of each row
      const int Pout = (N + TN - 1) / TN, pidx = tn * WGN + wn;
      const int nval = min(max(N - (n0 + wn * TN), 0), TN);
      // every residual fragment of the tile requested up front: one HBM latency per tile instead
      // of one per fragment row
      uint2 rall[MI][NI];
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const uint32_t m = m0 + wm * TM + j * 16 + fr;
#pragma unroll
        for (int i = 0; i < NI; ++i)
          rall[j][i] = buf_load_u2(rres, (m * (uint32_t)g.ldr + (n0 + wn * TN + i * 16 + fg * 4)) * 2u);
      }
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const uint2* rcur = rall[j];
        const uint32_t m = m0 + wm * TM + j * 16 + fr;
        uint2 pk[NI];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int nl = wn * TN + i * 16 + fg * 4, n = n0 + nl;
          const float rv[4] = {lo_h(rcur[i].x), hi_h(rcur[i].x), lo_h(rcur[i].y), hi_h(rcur[i].y)};
          const float4 bi = bias_of(i);
          pk[i] = make_uint2(pack2h(acc[i][j][0] + bi.x + rv[0], acc[i][j][1] + bi.y + rv[1]),
                             pack2h(acc[i][j][2] + bi.z + rv[2], acc[i][j][3] + bi.w + rv[3]));
          const uint32_t e = n < N ? m * (uint32_t)g.ldc + n : (kOOB >> 2);
          buf_store_u2(rc16, e * 2u, pk[i]);
          if (n < N) sum += (lo_h(pk[i].x) + hi_h(pk[i].x)) + (lo_h(pk[i].y) + hi_h(pk[i].y));
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float mean = sum / (float)(nval > 0 ? nval : 1);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const float d0 = lo_h(pk[i].x) - mean, d1 = hi_h(pk[i].x) - mean;
          const float d2 = lo_h(pk[i].y) - mean, d3 = hi_h(pk[i].y) - mean;
          if (n0 + wn * TN + i * 16 + fg * 4 < N) q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        if (fg == 0 && (int)m < M && nval > 0) g.ln_out[(size_t)m * Pout + pidx] = make_float2(mean, q);
      }
      continue;
    }
    if (!has_res && !g.c32) {
      // fp16-only output: lanes l and l^16 own adjacent 4-column groups of one row; swap one
      // fragment of each pair so every lane stores 16 contiguous bytes (half the store issues)
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const uint32_t m = m0 + wm * TM + j * 16 + fr;
        float2 st = make_float2(0.f, 1.f);
        if constexpr (EPI == 1) st = lds_stat[wm * TM + j * 16 + fr];
#pragma unroll
        for (int i = 0; i < NI; i += 2) {
          uint2 pk[2], pl[2];  // (pl: EPI 4's lo words)
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            float v[4] = {acc[i + h2][j][0], acc[i + h2][j][1], acc[i + h2][j][2], acc[i + h2][j][3]};
            if constexpr (EPI == 1) {  // r (acc - mean u), then + c (the folded bias)
              const float4 u = *reinterpret_cast<const float4*>(lds_cols + wn * TN + (i + h2) * 16 + fg * 4);
              v[0] = st.y * (v[0] - st.x * u.x);
              v[1] = st.y * (v[1] - st.x * u.y);
              v[2] = st.y * (v[2] - st.x * u.z);
              v[3] = st.y * (v[3] - st.x * u.w);
            }
            const float4 bi = bias_of(i + h2);
            v[0] += bi.x;
            v[1] += bi.y;
            v[2] += bi.z;
            v[3] += bi.w;
            if (ACT != ACT_NONE) act4<ACT>(v);
            pk[h2] = make_uint2(pack2h(v[0], v[1]), pack2h(v[2], v[3]));
            if constexpr (EPI == 4)
              pl[h2] = make_uint2(pack2h(v[0] - lo_h(pk[h2].x), v[1] - hi_h(pk[h2].x)),
                                  pack2h(v[2] - lo_h(pk[h2].y), v[3] - hi_h(pk[h2].y)));
          }
          const bool odd = fg & 1;
          // even fg: cols (16i + 4fg) .. +7 of fragment i; odd fg: cols (16(i+1) + 4(fg-1)) .. +7
          // (v_permlane16_swap pairing: VALU, no ds_bpermute round trip)
          const int n8 = n0 + wn * TN + (odd ? (i + 1) * 16 + (fg - 1) * 4 : i * 16 + fg * 4);
          const uint4 o = pair_rows16(pk[0], pk[1]);
          uint32_t off = (m * (uint32_t)g.ldc + n8) * 2u;
#ifdef MMF_EPI_SKIP
          // measurement build only (outputs incomplete): the last MMF_EPI_SKIP of every MI row
          // fragments are not stored -- how the epilogue time scales with the bytes it writes
          if (j >= MI - MMF_EPI_SKIP * MI / 8) off = kOOB;
#endif
          if constexpr (EPI == 4) {  // the split operand row: hi | lo | hi (N % 8 == 0: epi_ok)
            buf_store_u4(rc16, n8 < N ? off : kOOB, o);
            if (g.split_lo) {
              buf_store_u4(rc16, n8 < N ? off + (uint32_t)N * 2u : kOOB, pair_rows16(pl[0], pl[1]));
              buf_store_u4(rc16, n8 < N ? off + (uint32_t)N * 4u : kOOB, o);
            }
          } else if (full8) {
            buf_store_u4(rc16, n8 < N ? off : kOOB, o);
          } else {  // N % 8 == 4: the last group of a row holds only 4 valid columns
            buf_store_u4(rc16, n8 + 8 <= N ? off : kOOB, o);
            buf_store_u2(rc16, (n8 + 8 > N && n8 < N) ? off : kOOB, make_uint2(o.x, o.y));
          }
        }
      }
      continue;
    }
    // general epilogue, instantiated per residual dtype so that no load sits under a branch
    auto epilogue = [&](auto res_is_f32) {
      constexpr bool R32 = decltype(res_is_f32)::value;
      float4 rcur[NI], rnext[NI];
      auto load_res = [&](float4* r, int j) {
        const uint32_t m = m0 + wm * TM + j * 16 + fr;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const uint32_t e = m * (uint32_t)g.ldr + (n0 + wn * TN + i * 16 + fg * 4);
          if constexpr (R32) {
            r[i] = buf_load_f4(rres, e * 4u);
          } else {
            const uint2 rr = buf_load_u2(rres, e * 2u);  // zeros when there is no residual
            r[i] = make_float4(lo_h(rr.x), hi_h(rr.x), lo_h(rr.y), hi_h(rr.y));
          }
        }
      };
      load_res(rcur, 0);
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        if (j + 1 < MI) load_res(rnext, j + 1);
        const uint32_t m = m0 + wm * TM + j * 16 + fr;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int n = n0 + wn * TN + i * 16 + fg * 4;
          const float4 bi = bias_of(i);
          float v[4] = {acc[i][j][0] + bi.x, acc[i][j][1] + bi.y, acc[i][j][2] + bi.z, acc[i][j][3] + bi.w};
          if (ACT != ACT_NONE) {
            act4<ACT>(v);
          }
          v[0] += rcur[i].x; v[1] += rcur[i].y; v[2] += rcur[i].z; v[3] += rcur[i].w;
          const uint32_t e = n < N ? m * (uint32_t)g.ldc + n : (kOOB >> 2);
          if (g.c32) buf_store_f4(rc32, e * 4u, make_float4(v[0], v[1], v[2], v[3]));
          if (g.c16) buf_store_u2(rc16, e * 2u, make_uint2(pack2h(v[0], v[1]), pack2h(v[2], v[3])));
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) rcur[i] = rnext[i];
      }
    };
    if (g.res32) epilogue(std::true_type{});
    else epilogue(std::false_type{});
  }
  GST_END()
