// Body of the attn_bwd_dkv_g4_kernel / attn_bwd_dkv_g4_win_kernel kernels (included inside them: each kernel compiles from this text
// with its own constexpr CAUSAL / WIN / W).
    constexpr int HD = 128, QT = 32, NKS = 8, NDB = 4;
    using Y = Lay<HD>;
    constexpr int TILE = QT * 256;                 // 8 KiB: 32 rows x 128 bf16
    constexpr int STREAM = 2 * TILE + 512;         // Q tile | dO tile | lse2[32] dsum[32] kstart[32] (+pad: keeps tile bases 256-B aligned)
    constexpr int STAGE = 2 * STREAM;              // the two head-pair streams
    __shared__ __attribute__((aligned(256))) char smem[4 * STAGE];

    const int lane = threadIdx.x & 63, hh = lane >> 5, lk = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kb = wave & 1, hp = wave >> 1;
#ifdef DKV_STAMPS
    unsigned long long st_entry, st_loop = 0, st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0, sum_a = 0, sum_b = 0, sum_c = 0, sum_d = 0, n_steps = 0;
    DKV_STAMP(st_entry);
#endif
    // GQA group of G query heads per KV head, walked as two head streams (hp = 0, 1) of NH = ceil(G / 2) heads each.  Odd G: the last
    // head slot of stream 1 is a dummy (it re-reads the group's last head with lse = +inf, i.e. p = 0 and dS = 0: it adds exact zeros,
    // and keeps the two streams' barrier counts equal).  G = 4: Llama-3 / Mistral; G = 7: Qwen2-7B.
    const int G = H / Hkv, NH = (G + 1) >> 1;
    int bx, hk, b;
    xcd_tile_map((L + 63) >> 6, Hkv, bx, hk, b, CAUSAL);
    const int kblk0 = bx * 64, k0 = kblk0 + kb * 32, key = k0 + lk;
    const int keyc = key < L ? key : L - 1;
    const float c = scale * LOG2E;
    const bool key_ok = key < L && (kmask == nullptr || kmask[(long)b * L + keyc] != 0);

    bf16x8 kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int ch = ks * 2 + hh;
        kf[ks] = as_bf16x8(*reinterpret_cast<const u32x4*>(K + ((long)b * L + keyc) * ldk + (long)hk * HD + ch * 8));
        vf[ks] = as_bf16x8(*reinterpret_cast<const u32x4*>(V + ((long)b * L + keyc) * ldv + (long)hk * HD + ch * 8));
    }
    f32x16 dkacc[NDB], dvacc[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dkacc[d][e] = 0.f; dvacc[d][e] = 0.f; }

    // query tiles that can see this key block: from the block's first key (causal) to the end of the sequence / of the keys' sample
    const int qstart = CAUSAL ? (kblk0 >> 5) : 0;
    int qlim = L;
    if constexpr (SEG) {
        const int kk = kblk0 + lane;
        int e = kk < L ? qend[(long)b * L + kk] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(e, o, 64); e = e > y ? e : y; }
        e = __builtin_amdgcn_readfirstlane(e);
        qlim = e < L ? e : L;
    }
    if constexpr (WIN) qlim = qlim < kblk0 + 63 + W ? qlim : kblk0 + 63 + W;      // beyond: no key of the block is in the window
    const int ntl = ((qlim + QT - 1) >> 5) - qstart;       // tiles per head (may be <= 0)
    // Tiles that need per-element masking are walked FIRST by a plain loop; the rest -- the bulk: interior tiles of fully valid key
    // blocks -- by the software-pipelined loop, whose body is one branch-free basic block.  Causal: the first two tiles of a head
    // touch the diagonal of this 64-key block.  Irregular blocks (padded keys; with segments: keys of more than one sample) mask
    // every tile.  The order only permutes a sum that is the same for every launch: deterministic.
    // (decided on all 64 keys of the block by every wave alike: the four waves must agree on the tile split)
    bool irregular;
    {
        const int kk = kblk0 + lane, kkc = kk < L ? kk : L - 1;
        irregular = !__all(kk < L && (kmask == nullptr || kmask[(long)b * L + kkc] != 0));
    }
    if constexpr (SEG) {
        const int kk = kblk0 + lane, kkc = kk < L ? kk : L - 1;
        const int e = qend[(long)b * L + kkc], e0 = __builtin_amdgcn_readfirstlane(e);
        irregular = irregular || !__all(e == e0 || kk >= L);
    }
    irregular = __builtin_amdgcn_readfirstlane((int)irregular) != 0;
    const int ntc = ntl > 0 ? ntl : 0;
    const int nm0 = irregular ? ntc : (CAUSAL ? (ntc < 2 ? ntc : 2) : 0);    // masked tiles per head (WIN: the diagonal ones)
    // WIN: the unmasked tiles are qstart + nm0 .. qcut - 1, the masked ones past them (the far edge) qcut .. qstart + ntc - 1
    const int qedge = (kblk0 + W) >> 5;                                     // (WIN) first query tile the far edge cuts
    const int qcut = WIN ? (qedge < qstart + nm0 ? qstart + nm0 : (qedge < qstart + ntc ? qedge : qstart + ntc)) : 0;
    const int nm = WIN ? nm0 + (qstart + ntc - qcut) : nm0;                 // masked tiles per head
    const int nu1 = ntc - nm;                                                // unmasked tiles per head
    const int qu0 = WIN ? qstart + nm0 : 0;                                  // (WIN) first unmasked tile; else qstart + nm

    // stage = (a) request the tile's lse / rowsum(dO*O) / kstart words into registers FIRST (oldest entries of the vmcnt queue:
    // their wait does not drain the DMA behind them), (b) issue the LDS-DMA of the Q and dO rows; (c) `stage_finish`, called at the
    // end of the iteration, puts the words into LDS.  Everything goes through buffer descriptors: the per-lane offsets are fixed for
    // the whole kernel, a tile adds one wave-uniform offset to them (no 64-bit address arithmetic in the loop), and rows beyond L are
    // out of range of the descriptor -> the DMA writes zeros (no clamping, no branches: the loop body stays one basic block).
    // A tile is (gi = which head of the pair, qt = query tile index).
    const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)(Q + (long)b * L * ldq), 0, (int)(unsigned)((long)L * ldq * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((void*)(dO + (long)b * L * ldo), 0, (int)(unsigned)((long)L * ldo * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void*)(LSE + (long)b * H * L), 0, (int)(unsigned)((long)H * L * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)(Dsum + (long)b * H * L), 0, (int)(unsigned)((long)H * L * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(SEG ? kstart + (long)b * L : nullptr), 0, SEG ? (int)(unsigned)((long)L * 4) : 0, 0x00020000);
    unsigned voQ[4], voD[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (kb * 4 + j) * 4 + (lane >> 4);
        const int cc = (lane & 15) ^ lds_swz(row);
        voQ[j] = (unsigned)(((long)row * ldq + cc * 8) * 2);
        voD[j] = (unsigned)(((long)row * ldo + cc * 8) * 2);
    }
    auto stage = [&](int gi, int qt, int slot, float& vl, float& vs, int& ksv) {
        const int q0 = qt * QT;
        const int hl = hp * NH + gi;                                  // head slot inside the group (hl >= G: the dummy slot)
        const int h = hk * G + (hl < G ? hl : G - 1);
        char* base = smem + slot * STAGE + hp * STREAM;
        // NB the hardware range check of a raw buffer covers the VECTOR offset only (the scalar offset is added after it), so the
        // tile offset is added into the vector offset: one v_add per access buys "rows beyond L read zeros" for the last tile
        const unsigned soL = (unsigned)(((long)h * L + q0) * 4);
        // a query row beyond L reads lse / dsum words of the next head (or zeros past the end): replaced in stage_finish
        vl = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsL, (unsigned)lk * 4u + soL, 0, 0));
        vs = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsS, (unsigned)lk * 4u + soL, 0, 0));
        if constexpr (SEG) ksv = (int)__builtin_amdgcn_raw_buffer_load_b32(rsK, (unsigned)lk * 4u + (unsigned)q0 * 4u, 0, 0);
        const unsigned soQ = (unsigned)(((long)q0 * ldq + (long)h * HD) * 2), soD = (unsigned)(((long)q0 * ldo + (long)h * HD) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int piece = kb * 4 + j;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (lds_void_t*)(base + piece * 1024), 16, voQ[j] + soQ, 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (lds_void_t*)(base + TILE + piece * 1024), 16, voD[j] + soD, 0, 0, 0);
        }
    };
    // the same in two parts for the merged step (ATTN_DKV_MERGED): the words at the top of the step, the DMA pieces one per MFMA slot
    auto stage_words = [&](int gi, int qt, float& vl, float& vs, int& ksv) {
        const int q0 = qt * QT;
        const int hl = hp * NH + gi;
        const int h = hk * G + (hl < G ? hl : G - 1);
        const unsigned soL = (unsigned)(((long)h * L + q0) * 4);
        vl = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsL, (unsigned)lk * 4u + soL, 0, 0));
        vs = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsS, (unsigned)lk * 4u + soL, 0, 0));
        if constexpr (SEG) ksv = (int)__builtin_amdgcn_raw_buffer_load_b32(rsK, (unsigned)lk * 4u + (unsigned)q0 * 4u, 0, 0);
    };
    auto stage_piece = [&](auto qc, int gi, int qt, int slot) {       // piece q = 2 j + (0: Q rows, 1: dO rows) of the tile
        constexpr int q = decltype(qc)::value, j = q >> 1;
        const int q0 = qt * QT;
        const int hl = hp * NH + gi;
        const int h = hk * G + (hl < G ? hl : G - 1);
        char* base = smem + slot * STAGE + hp * STREAM;
        const int piece = kb * 4 + j;
        if constexpr ((q & 1) == 0) {
            const unsigned soQ = (unsigned)(((long)q0 * ldq + (long)h * HD) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (lds_void_t*)(base + piece * 1024), 16, voQ[j] + soQ, 0, 0, 0);
        } else {
            const unsigned soD = (unsigned)(((long)q0 * ldo + (long)h * HD) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (lds_void_t*)(base + TILE + piece * 1024), 16, voD[j] + soD, 0, 0, 0);
        }
    };
    auto stage_finish = [&](int gi, int qt, int slot, float vl, float vs, int ksv) {
        const int qq = (hp * NH + gi < G) ? qt * QT + lk : 0x7fffffff;      // dummy head slot: every row is "beyond the last query"
        float* fp = reinterpret_cast<float*>(smem + slot * STAGE + hp * STREAM + 2 * TILE);
        const float val = hh == 0 ? vl * LOG2E : vs;
        // +inf beyond the last query that can see this key block -> p = 0: beyond L, and (packed samples) beyond the end of the
        // keys' sample -- for a regular block every key shares that end, so the tile straddling it needs no per-element mask
        fp[lane] = qq < qlim ? val : (hh == 0 ? INFINITY : 0.f);
        if constexpr (SEG) reinterpret_cast<int*>(fp)[2 * QT + lk] = ksv;
    };
    // S, dP of the tile in `slot` -> s, dp   (the first MFMA of each chain takes the constant 0 as its accumulator input)
    auto scores = [&](int slot, f32x16& s, f32x16& dp) {
        const char* sQ = smem + slot * STAGE + hp * STREAM;
        const char* sdO = sQ + TILE;
        f32x16 z;
#pragma unroll
        for (int e = 0; e < 16; ++e) z[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int off = Y::chunk_off(lk, ks * 2 + hh);
            const bf16x8 qa = *reinterpret_cast<const bf16x8*>(sQ + off);
            const bf16x8 da = *reinterpret_cast<const bf16x8*>(sdO + off);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], ks == 0 ? z : s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], ks == 0 ? z : dp, 0, 0, 0);
        }
    };
    // P and dS of a tile from its S, dP (in place: s <- P, dp <- dS)
    auto softmax_bwd = [&](auto masked, int q0, int slot, f32x16& s, f32x16& dp) {
        const float* sLse = reinterpret_cast<const float*>(smem + slot * STAGE + hp * STREAM + 2 * TILE);
        const float* sDs = sLse + QT;
        const int* sKs = reinterpret_cast<const int*>(sLse + 2 * QT);
        if constexpr (decltype(masked)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = (r & 3) + 8 * (r >> 2) + 4 * hh;
                float v = key_ok ? s[r] * c : -INFINITY;
                if (CAUSAL && key > q0 + ql) v = -INFINITY;
                if constexpr (SEG) { if (key < sKs[ql]) v = -INFINITY; }
                if constexpr (WIN) { if (key <= q0 + ql - W) v = -INFINITY; }
                const float p = __builtin_amdgcn_exp2f(v - sLse[ql]);
                s[r] = p;
                dp[r] = p * (dp[r] - sDs[ql]);       // the softmax scale is applied once, to the dK accumulators
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -sLse[ql]));
                s[r] = p;
                dp[r] = p * (dp[r] - sDs[ql]);
            }
        }
    };
    // dV^T += dO^T . P, dK^T += Q^T . dS  (transposing reads of the same row-major tiles)
    auto accumulate = [&](int slot, const f32x16& p, const f32x16& ds) {
        const char* sQ = smem + slot * STAGE + hp * STREAM;
        const char* sdO = sQ + TILE;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
            const bf16x8 pf = pack_frag(p, cp);
            const bf16x8 dsf = pack_frag(ds, cp);
#pragma unroll
            for (int d = 0; d < NDB; ++d) {
                const bf16x8 dot = read_tr_frag<HD>(sdO, 16 * cp, d * 32, lane);
                const bf16x8 qtf = read_tr_frag<HD>(sQ, 16 * cp, d * 32, lane);
                dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot, pf, dvacc[d], 0, 0, 0);
                dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dkacc[d], 0, 0, 0);
            }
        }
    };

    // ---- masked tiles: plain double-buffered walk (slots 0 / 1), tile j -> (gi = j / nm, qt = qstart + j % nm; WIN: the nm0 diagonal
    // tiles, then the far-edge tiles from qcut)
    {
        const int ntot = NH * nm;
        if (ntot > 0) {
            int gi = 0, qt = qstart;           // tile j = (head slot j / nm, query tile qstart + j % nm), carried instead of divided
            float vl, vs;
            int ksv = 0;
            stage(gi, qt, 0, vl, vs, ksv);
            stage_finish(gi, qt, 0, vl, vs, ksv);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int j = 0; j < ntot; ++j) {
                const int slot = j & 1;
                int gn = gi, qn = qt;
                if (j + 1 < ntot) {
                    if constexpr (WIN) {
                        const bool wrap = (qn + 1 == (nm > nm0 ? qcut + nm - nm0 : qstart + nm));
                        qn = wrap ? qstart : (qn + 1 == qstart + nm0 ? qcut : qn + 1);
                        gn += wrap ? 1 : 0;
                    } else {
                        const bool wrap = (qn + 1 == qstart + nm);
                        qn = wrap ? qstart : qn + 1;
                        gn += wrap ? 1 : 0;
                    }
                }
                stage(gn, qn, slot ^ 1, vl, vs, ksv);
                stage_finish(gn, qn, slot ^ 1, vl, vs, ksv);
                f32x16 s, dp;
                scores(slot, s, dp);
                softmax_bwd(std::true_type{}, qt * QT, slot, s, dp);
                accumulate(slot, s, dp);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                gi = gn;
                qt = qn;
            }
        }
    }
    // ---- unmasked tiles: 4-slot ring, three-stage software pipeline; tile j -> (gi = j / nu1, qt = qstart + nm + j % nu1; WIN: qu0 + j % nu1)
    // Step j runs, on ONE wave per SIMD:   MS(j+2): S, dP of tile j+2 (16 MFMAs, slots 0-15)
    //                                       SM(j+1): softmax backward of tile j+1 on the VALU, one element per two slots
    //                                       MA(j):   dV, dK accumulation of tile j (16 MFMAs, slots 16-31)
    // so every one of the 32 MFMA slots of a step shadows the same small bundle: its LDS fragment reads (requested PF slots ahead),
    // half a softmax element, a pack.  Register roles rotate with period 3, ring slots with period 4, the packed-fragment buffers
    // with period 2 -> the loop body is written out for 12 steps (all indices compile-time).  The score MFMAs are issued through
    // inline asm with VGPR destinations and the K / V fragments as AGPR operands: S and dP then need no v_accvgpr_read per
    // element (the accumulators proper -- dK, dV -- stay in AGPRs under the compiler's builtin).
    {
        const int n = NH * nu1;
        // tile j = (head slot j / nu1, query tile qstart + nm (WIN: qu0) + j % nu1); the staging cursor (pg, pq) walks the tiles one by one and
        // stays on the last tile once it is reached (re-staging it is harmless), so the loop carries no division
        int pg = 0, pq = WIN ? qu0 : qstart + nm, pj = 0;
        auto cursor_next = [&]() {
            if (pj + 1 < n) {
                const bool wrap = (pq + 1 == (WIN ? qu0 : qstart + nm) + nu1);
                pq = wrap ? (WIN ? qu0 : qstart + nm) : pq + 1;
                pg += wrap ? 1 : 0;
                ++pj;
            }
        };
        if (n > 0) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) { asm volatile("" : "+a"(kf[ks])); asm volatile("" : "+a"(vf[ks])); }
            {
                float v[3], w[3];
                int zz[3] = {0, 0, 0}, g[3], q[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) { g[t] = pg; q[t] = pq; stage(g[t], q[t], t, v[t], w[t], zz[t]); cursor_next(); }
#pragma unroll
                for (int t = 0; t < 3; ++t) stage_finish(g[t], q[t], t, v[t], w[t], zz[t]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            f32x16 sv[3], dv[3];          // S / dP -> P / dS of three tiles in flight (roles rotate)
            u32x4 pk[2][2][2];            // [parity][0: P, 1: dS][cp] packed bf16 fragments
            auto rowfrag = [&](const char* tq, int g) -> bf16x8 {          // g = 2 * ks + which (0: Q for S, 1: dO for dP)
                return *reinterpret_cast<const bf16x8*>(tq + (g & 1) * TILE + Y::chunk_off(lk, (g >> 1) * 2 + hh));
            };
            auto mfma_s = [&](auto first, f32x16& acc, const bf16x8& a, const bf16x8& bagpr) {
                if constexpr (decltype(first)::value)
                    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(bagpr));
                else
                    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(bagpr));
            };
            // softmax backward of ONE element r (in place) with the lse / dsum words of its tile
            auto sm_elem = [&](auto rc, f32x16& sx, f32x16& dx, const f32x4 (&lse4)[4], const f32x4 (&dsm4)[4]) {
                constexpr int r = decltype(rc)::value;
                if constexpr (kDkvAsmElems) {
                    // the element's four instructions as ONE statement: placed where the slot puts them (a volatile asm neither sinks to its
                    // user's block nor moves across the slot's MFMA), and without the two empty pinning statements of the C++ form, each of
                    // which the hazard recognizer pads with an s_nop (33 - 44 s_nop per 32-MFMA step, profiles/r05_attn_anatomy.md).  Same
                    // arithmetic: p = exp2(s * c - lse), dS = p * (dP - D); the v_sub between v_exp and its use covers the trans-use hazard
                    float p, ds;
                    asm volatile("v_fma_f32 %0, %2, %3, -%4\n\tv_exp_f32 %0, %0\n\tv_sub_f32 %1, %5, %6\n\tv_mul_f32 %1, %1, %0"
                                 : "=&v"(p), "=&v"(ds)
                                 : "v"(sx[r]), "v"(c), "v"(lse4[r >> 2][r & 3]), "v"(dx[r]), "v"(dsm4[r >> 2][r & 3]));
                    sx[r] = p;
                    dx[r] = ds;
                } else {
                    float l = lse4[r >> 2][r & 3];
                    asm volatile("" : "+v"(l));            // pins the element's arithmetic behind the slot's (volatile asm) MFMA
                    float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sx[r], c, -l));
                    float ds = p * (dx[r] - dsm4[r >> 2][r & 3]);
                    asm volatile("" : "+v"(p), "+v"(ds));  // ... and in front of the next one (IR sinking would move it to its user's block)
                    sx[r] = p;
                    dx[r] = ds;
                }
            };
            auto pack_pinned = [&](float a, float b2) -> unsigned {
                if constexpr (kDkvAsmElems) {
                    unsigned u;
                    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u) : "v"(a), "v"(b2));      // == pack_bf2 (round to nearest even), pinned
                    return u;
                } else {
                    asm volatile("" : "+v"(a));
                    unsigned u = pack_bf2(a, b2);
                    asm volatile("" : "+v"(u));
                    return u;
                }
            };
            auto load_words = [&](int slot, f32x4 (&lse4)[4], f32x4 (&dsm4)[4]) {
                const float* sLse = reinterpret_cast<const float*>(smem + slot * STAGE + hp * STREAM + 2 * TILE) + 4 * hh;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    lse4[g] = *reinterpret_cast<const f32x4*>(sLse + 8 * g);
                    dsm4[g] = *reinterpret_cast<const f32x4*>(sLse + QT + 8 * g);
                }
            };
            // ---- prologue: S, dP of tiles 0 and 1; softmax backward + packs of tile 0
            {
                const char* t0 = smem + 0 * STAGE + hp * STREAM;
                const char* t1 = smem + 1 * STAGE + hp * STREAM;
                static_for<0, 16>([&](auto gc) {
                    constexpr int g = decltype(gc)::value, ks = g >> 1;
                    if constexpr (g & 1) mfma_s(std::integral_constant<bool, ks == 0>{}, dv[0], rowfrag(t0, g), vf[ks]);
                    else mfma_s(std::integral_constant<bool, ks == 0>{}, sv[0], rowfrag(t0, g), kf[ks]);
                });
                static_for<0, 16>([&](auto gc) {
                    constexpr int g = decltype(gc)::value, ks = g >> 1;
                    if constexpr (g & 1) mfma_s(std::integral_constant<bool, ks == 0>{}, dv[1], rowfrag(t1, g), vf[ks]);
                    else mfma_s(std::integral_constant<bool, ks == 0>{}, sv[1], rowfrag(t1, g), kf[ks]);
                });
                asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // MFMA results -> VALU readers (the asm MFMAs are invisible to hipcc)
                f32x4 lse4[4], dsm4[4];
                load_words(0, lse4, dsm4);
                static_for<0, 16>([&](auto rc) { sm_elem(rc, sv[0], dv[0], lse4, dsm4); });
#pragma unroll
                for (int cp = 0; cp < 2; ++cp)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        pk[0][0][cp][e] = pack_bf2(sv[0][8 * cp + 2 * e], sv[0][8 * cp + 2 * e + 1]);
                        pk[0][1][cp][e] = pack_bf2(dv[0][8 * cp + 2 * e], dv[0][8 * cp + 2 * e + 1]);
                    }
            }
            // this lane's transposing-read addresses (tr_issue): [ring slot pair][d-block], first read / the read eight rows further down; ring
            // slot parity, the dO tile and the second 16-row half are immediate offsets
            unsigned trA[2][4], trB[2][4];
            if constexpr (kDkvTrAsm) {
                const int s16 = lane & 15, g16 = (lane >> 4) & 1;
                const int row = 4 * hh + (s16 >> 2);
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int col = d * 32 + 16 * g16 + (s16 & 3) * 4;
                    const int off = Y::chunk_off(row, col >> 3) + (col & 7) * 2;
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        trA[pr][d] = lds_addr_of(smem + pr * 2 * STAGE + hp * STREAM + off);
                        trB[pr][d] = lds_addr_of(smem + pr * 2 * STAGE + hp * STREAM + ((off + 8 * 256) ^ 32));
                    }
                }
            }
            auto step = [&](int j, auto kc) {
                constexpr int k = decltype(kc)::value;                 // position inside the 12-step trip
                constexpr int slot0 = k % 4, slot1 = (k + 1) % 4, slot2 = (k + 2) % 4, slot3 = (k + 3) % 4;
                constexpr int r0 = k % 3, r1 = (k + 1) % 3, r2 = (k + 2) % 3;     // roles of tiles j, j+1, j+2
                constexpr int par0 = k % 2, par1 = (k + 1) % 2;
                constexpr int PF = 4;
                const char* tq0 = smem + slot0 * STAGE + hp * STREAM;    // tile j: transposed fragments
                const char* tq2 = smem + slot2 * STAGE + hp * STREAM;    // tile j + 2: row fragments
                DKV_STAMP(st0);
                const int gi3 = pg, qt3 = pq;                 // tile j + 3 (or the last tile again)
                cursor_next();
                float vl, vs;
                int ksv = 0;
                // slot3 held tile j-1: released by the barrier that ended step j-1.  Merged step: only the lse / rowsum words are requested
                // here; the eight DMA pieces ride in the MFMA slots 1, 3, .. 15 (8 x ~60 cycles of issue with nothing else running cost the
                // grouped step 655 of its 3087 cycles, profiles/r05_attn_anatomy.md) -- early enough to land before the step's barrier
                if constexpr (kDkvMerged && kDkvDmaInSlots) stage_words(gi3, qt3, vl, vs, ksv);
                else stage(gi3, qt3, slot3, vl, vs, ksv);
                f32x4 lse4[4], dsm4[4];
                load_words(slot1, lse4, dsm4);
                bf16x8 fr[PF + 1];
#pragma unroll
                for (int g = 0; g < PF; ++g) fr[g] = rowfrag(tq2, g);
                DKV_STAMP(st1);
                FragU tf[4];
                // transposed fragment g = cp * 8 + d * 2 + which (0: dO^T for dV, 1: Q^T for dK) of tile j.  Hand-issued (kDkvTrAsm): the builtin
                // form put s_waitcnt vmcnt(0) in front of the step's first transposing read, i.e. the DMA of tile j + 3, issued at the top of
                // this very step, was waited for in the MIDDLE of the step instead of at its end.  The reads' completion is then counted by
                // hand: LDS operations retire in order, and behind the reads of fragment g only those of g + 1, g + 2 have been issued
                auto tr_issue = [&](auto gc2, FragU& dst) {
                    constexpr int g = decltype(gc2)::value, d = (g >> 1) & 3;
                    if constexpr (kDkvTrAsm) {
                        constexpr int imm = (slot0 & 1) * STAGE + ((g & 1) ? 0 : TILE) + (g >> 3) * 4096;
                        const unsigned a0 = trA[slot0 >> 1][d], a1 = trB[slot0 >> 1][d];      // (named: asm operands alone do not capture)
                        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst.h[0]) : "v"(a0), "i"(imm));
                        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst.h[1]) : "v"(a1), "i"(imm));
                    } else {
                        dst.f = read_tr_frag<HD>(tq0 + ((g & 1) ? 0 : TILE), 16 * (g >> 3), d * 32, lane);
                    }
                };
                auto tr_wait = [&](auto gc2, FragU& f) {
                    constexpr int g = decltype(gc2)::value;
                    if constexpr (kDkvTrAsm) {
                        if constexpr (g <= 13) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f.f));
                        else if constexpr (g == 14) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f.f));
                        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.f));
                    }
                };
                if constexpr (kDkvMerged) {
                    // MERGED order (round 5): the step's 32 MFMAs alternate between the two groups -- S(ks), dV, dP(ks), dK, S(ks + 1), ... -- so
                    // that two MFMAs on the SAME accumulator are four instructions apart.  In the grouped order below the score chains
                    // S(0) dP(0) S(1) dP(1) ... put every other MFMA behind its own predecessor's result (a 32x32x16 MFMA takes 16 passes;
                    // with VALU / LDS work issued in between, a dependent pair costs ~110 cycles instead of 64): the in-kernel stamps showed
                    // 1359 cycles for those 16 MFMAs against 775 for the 16 independent accumulation MFMAs (profiles/r05_attn_anatomy.md).
                    // Even slot m: item g = m / 2 of MS(j+2); odd slot: item g = (m - 1) / 2 of MA(j).  The transposed fragments of items 0-2 are
                    // requested at the top of the step (hand-issued: a builtin read would wait for the DMA issued just above), the cp = 0 packs
                    // of tile j + 1 move behind the softmax-backward elements they read (odd items 3, 7, 11, 15).
                    tr_issue(std::integral_constant<int, 0>{}, tf[0]);
                    tr_issue(std::integral_constant<int, 1>{}, tf[1]);
                    tr_issue(std::integral_constant<int, 2>{}, tf[2]);
                    static_for<0, 32>([&](auto mc) {
                        constexpr int m = decltype(mc)::value, g = m >> 1;
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr ((m & 1) == 0) {
                            constexpr int ks = g >> 1;
                            if constexpr (g & 1) mfma_s(std::integral_constant<bool, ks == 0>{}, dv[r2], fr[g % (PF + 1)], vf[ks]);
                            else mfma_s(std::integral_constant<bool, ks == 0>{}, sv[r2], fr[g % (PF + 1)], kf[ks]);
                            if constexpr (g + PF < 16) fr[(g + PF) % (PF + 1)] = rowfrag(tq2, g + PF);
                            if constexpr (g < 8) {
                                constexpr int e = g & 3;
                                if constexpr (g < 4) pk[par0][0][1][e] = pack_pinned(sv[r0][8 + 2 * e], sv[r0][8 + 2 * e + 1]);
                                else pk[par0][1][1][e] = pack_pinned(dv[r0][8 + 2 * e], dv[r0][8 + 2 * e + 1]);
                            }
                            if constexpr (g & 1) sm_elem(std::integral_constant<int, (g >> 1)>{}, sv[r1], dv[r1], lse4, dsm4);
                        } else {
                            constexpr int cp = g >> 3, d = (g >> 1) & 3;
                            asm volatile("" ::: "memory");
                            tr_wait(std::integral_constant<int, g>{}, tf[g & 3]);
                            if constexpr (g & 1) dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[g & 3].f, as_bf16x8(pk[par0][1][cp]), dkacc[d], 0, 0, 0);
                            else dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[g & 3].f, as_bf16x8(pk[par0][0][cp]), dvacc[d], 0, 0, 0);
                            if constexpr (g + 3 < 16) tr_issue(std::integral_constant<int, g + 3>{}, tf[(g + 3) & 3]);
                            if constexpr (kDkvDmaInSlots && g < 8) stage_piece(std::integral_constant<int, g>{}, gi3, qt3, slot3);
                            if constexpr (g & 1) sm_elem(std::integral_constant<int, 8 + (g >> 1)>{}, sv[r1], dv[r1], lse4, dsm4);
                            if constexpr ((g & 3) == 3) {       // elements 2 e, 2 e + 1 of tile j + 1 left the softmax backward in even item 4 e + 3
                                constexpr int e = g >> 2;
                                pk[par1][0][0][e] = pack_pinned(sv[r1][2 * e], sv[r1][2 * e + 1]);
                                pk[par1][1][0][e] = pack_pinned(dv[r1][2 * e], dv[r1][2 * e + 1]);
                            }
                        }
                    });
                    DKV_STAMP(st2);
                } else {
                    // slots 0-15: MS(j+2)  ||  SM(j+1) elements 0-7  ||  cp = 1 packs of tile j (its elements 8-15 finished last step)
                    static_for<0, 16>([&](auto gc) {
                        constexpr int g = decltype(gc)::value, ks = g >> 1;
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (g & 1) mfma_s(std::integral_constant<bool, ks == 0>{}, dv[r2], fr[g % (PF + 1)], vf[ks]);
                        else mfma_s(std::integral_constant<bool, ks == 0>{}, sv[r2], fr[g % (PF + 1)], kf[ks]);
                        if constexpr (g + PF < 16) fr[(g + PF) % (PF + 1)] = rowfrag(tq2, g + PF);
                        if constexpr (g < 8) {
                            constexpr int e = g & 3;
                            if constexpr (g < 4) pk[par0][0][1][e] = pack_pinned(sv[r0][8 + 2 * e], sv[r0][8 + 2 * e + 1]);
                            else pk[par0][1][1][e] = pack_pinned(dv[r0][8 + 2 * e], dv[r0][8 + 2 * e + 1]);
                        }
                        if constexpr (g & 1) sm_elem(std::integral_constant<int, (g >> 1)>{}, sv[r1], dv[r1], lse4, dsm4);
                        if constexpr (g >= 13) tr_issue(std::integral_constant<int, g - 13>{}, tf[g - 13]);
                    });
                    DKV_STAMP(st2);
                    // slots 16-31: MA(j)  ||  SM(j+1) elements 8-15  ||  cp = 0 packs of tile j+1
                    static_for<0, 16>([&](auto gc) {
                        constexpr int g = decltype(gc)::value, cp = g >> 3, d = (g >> 1) & 3;
                        __builtin_amdgcn_sched_barrier(0);
                        asm volatile("" ::: "memory");
                        tr_wait(gc, tf[g & 3]);
                        if constexpr (g & 1) dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[g & 3].f, as_bf16x8(pk[par0][1][cp]), dkacc[d], 0, 0, 0);
                        else dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf[g & 3].f, as_bf16x8(pk[par0][0][cp]), dvacc[d], 0, 0, 0);
                        if constexpr (g + 3 < 16) tr_issue(std::integral_constant<int, g + 3>{}, tf[(g + 3) & 3]);
                        if constexpr (g & 1) sm_elem(std::integral_constant<int, 8 + (g >> 1)>{}, sv[r1], dv[r1], lse4, dsm4);
                        if constexpr (g < 8) {
                            constexpr int e = g & 3;
                            if constexpr (g < 4) pk[par1][0][0][e] = pack_pinned(sv[r1][2 * e], sv[r1][2 * e + 1]);
                            else pk[par1][1][0][e] = pack_pinned(dv[r1][2 * e], dv[r1][2 * e + 1]);
                        }
                    });
                }
                __builtin_amdgcn_sched_barrier(0);
                DKV_STAMP(st3);
                stage_finish(gi3, qt3, slot3, vl, vs, ksv);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile j+3 landed (this wave's pieces)
                __syncthreads();
#ifdef DKV_STAMPS
                DKV_STAMP(st4);
                if (st_loop == 0) st_loop = st0;
                sum_a += st1 - st0; sum_b += st2 - st1; sum_c += st3 - st2; sum_d += st4 - st3; n_steps += 1;
#endif
            };
            int j = 0;
            while (true) {
#define DKV_STEP(K_) step(j, std::integral_constant<int, K_>{}); if (++j >= n) break;
                DKV_STEP(0) DKV_STEP(1) DKV_STEP(2) DKV_STEP(3) DKV_STEP(4) DKV_STEP(5)
                DKV_STEP(6) DKV_STEP(7) DKV_STEP(8) DKV_STEP(9) DKV_STEP(10) DKV_STEP(11)
#undef DKV_STEP
            }
            // (the asm MFMAs of the final steps wrote registers nothing reads; they retired long ago: 16 accumulation MFMAs and a
            // barrier follow them inside the step, so no keep-alive is needed -- and one would force the rotating roles to a common
            // register assignment at all twelve loop exits)
        }
    }
    // cross-stream reduction: [kb][which][d][r][lane] fp32; hp = 0 hands over its dV partial and finishes dK, hp = 1 the converse
    __syncthreads();
    {
        float* red = reinterpret_cast<float*>(smem);
        float* mine = red + ((kb * 2 + hp) * 64) * 64;          // region written by this wave
        const float* theirs = red + ((kb * 2 + (hp ^ 1)) * 64) * 64;
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) mine[(d * 16 + e) * 64 + lane] = hp == 0 ? dvacc[d][e] : dkacc[d][e];
        __syncthreads();
        if (key < L) {
            bf16_t* op = (hp == 0 ? dK + ((long)b * L + key) * lddk : dV + ((long)b * L + key) * lddv) + (long)hk * HD;
            const float sc = hp == 0 ? scale : 1.f;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float own = hp == 0 ? dkacc[d][4 * g4 + e] : dvacc[d][4 * g4 + e];
                        v[e] = (own + theirs[(d * 16 + 4 * g4 + e) * 64 + lane]) * sc;
                    }
                    u32x2 o;
                    o[0] = pack_bf2(v[0], v[1]);
                    o[1] = pack_bf2(v[2], v[3]);
                    *reinterpret_cast<u32x2*>(op + d * 32 + 8 * g4 + 4 * hh) = o;
                }
        }
    }
#ifdef DKV_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 4096) {
        unsigned long long st_exit;
        DKV_STAMP(st_exit);
        unsigned long long* o = g_dkv_stamps + (size_t)blockIdx.x * 8;
        o[0] = st_loop ? st_loop - st_entry : 0; o[1] = st_exit - st_entry; o[2] = n_steps; o[3] = sum_a; o[4] = sum_b; o[5] = sum_c; o[6] = sum_d;
        o[7] = (unsigned long long)bx;
    }
#endif
