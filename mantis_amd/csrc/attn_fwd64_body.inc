// Body of the attn_fwd64_kernel / attn_fwd64_win_kernel kernels (included inside them: each kernel compiles from this text
// with its own constexpr CAUSAL / WIN / W).
    __shared__ __attribute__((aligned(1024))) char smem[2 * NS * TILE + MAX_TILES * 8];

#ifdef FWD64_PROBE_TIMING
    const unsigned long long T0 = __builtin_amdgcn_s_memtime();
#endif
    const int lane = threadIdx.x & 63, hh = lane >> 5, lq = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gx = (L + 255) >> 8;
    int bx, h, b;
    xcd_tile_map(gx, H, bx, h, b, CAUSAL);
    const int hk = h / (H / Hkv);
    const int qbi = CAUSAL ? (gx - 1 - bx) : bx;   // causal: longest rows first
    const int qblk0 = qbi * 256, q0w = qblk0 + wave * 64;
    const float c = scale * LOG2E;

    // ---- prologue order: the key range, the first DMA pieces (K(f), V(f), K(f+1)), the Q rows and the key mask words all in flight
    // together, the rest of the ring behind them, register initialisation under the round trip
    asm volatile("" ::: AGPR_ALL);      // (declares the whole accumulator file as used)
    const int t_first = __builtin_amdgcn_readfirstlane(
        WIN ? (win_lo(qblk0, kstart ? kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] : 0, W) >> 6)
            : (kstart ? (kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] >> 6) : 0));
    const int kend = CAUSAL ? (qblk0 + 256 < Lk ? qblk0 + 256 : Lk) : Lk;
    const int ntiles = (kend + 63) >> 6;

    // ---- LDS fragment addresses (tile-relative; ring slot, key block and key chunk go into the instruction's immediate offset)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem;
    unsigned kaddr[8], vaddr[4], vaddr8[4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) kaddr[ks] = lds0 + OFF_K + Lay<HD>::chunk_off(lq, ks * 2 + hh);
    {
        const int s = lane & 15, g16 = (lane >> 4) & 1;
        const int row = 4 * hh + (s >> 2);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int col = d * 32 + 16 * g16 + (s & 3) * 4;
            const int off = Lay<HD>::chunk_off(row, col >> 3) + (col & 7) * 2;
            vaddr[d] = lds0 + OFF_V + off;
            vaddr8[d] = lds0 + OFF_V + ((off + 8 * 256) ^ 32);
        }
    }
    // ---- LDS-DMA geometry: a 64-row tile is 16 pieces of 4 rows x 256 B; this wave moves pieces 4w .. 4w+3 of K and of V
    const bf16_t* Kb = K + (long)b * Lk * ldk + (long)hk * HD;
    const bf16_t* Vb = V + (long)b * Lk * ldv + (long)hk * HD;
    unsigned voK[4], voV[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (wave * 4 + j) * 4 + (lane >> 4);
        const int ch = (lane & 15) ^ lds_swz(row);
        voK[j] = (unsigned)(((long)row * ldk + ch * 8) * 2);
        voV[j] = (unsigned)(((long)row * ldv + ch * 8) * 2);
    }
    // descriptor of tile t of K (or V): rows >= Lk (and whole tiles >= ntiles) read as zeros through the descriptor's range
    auto tile_desc = [&](const bf16_t* base, int ld, int t) __attribute__((always_inline)) {
        const int key0 = t * 64;
        int rows = Lk - key0;
        rows = rows > 64 ? 64 : rows;
        rows = t < ntiles ? rows : 0;
        rows = rows < 0 ? 0 : rows;
        int nrec = ((rows - 1) * ld + HD) * 2;
        nrec = rows > 0 ? nrec : 0;
        nrec = __builtin_amdgcn_readfirstlane(nrec);      // the clamp may be selected as v_med3: without this the descriptor lives in VGPRs and every DMA piece becomes a waterfall loop
        return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (long)key0 * ld), 0, nrec, 0x00020000);
    };
    // piece J of this wave's four -> ring slot `slot`
    auto dma_piece = [&](const __amdgpu_buffer_rsrc_t rs, const unsigned (&vo)[4], int ring_off, int slot, auto jsel)
                         __attribute__((always_inline)) {
        constexpr int J = decltype(jsel)::value;
#ifdef FWD64_PROBE_NO_DMA
        return;
#endif
        lds_void* d = (lds_void*)(smem + ring_off + slot * TILE + (wave * 4 + J) * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, d, 16, vo[J], 0, 0, 0);
    };
    // ---- K(f), V(f), K(f+1) first: what barrier(f) and the first K fragment reads wait for
    {
        const __amdgpu_buffer_rsrc_t rk0 = tile_desc(Kb, (int)ldk, t_first), rv0 = tile_desc(Vb, (int)ldv, t_first),
                                     rk1 = tile_desc(Kb, (int)ldk, t_first + 1);
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rk0, voK, OFF_K, 0, j); });
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rv0, voV, OFF_V, 0, j); });
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rk1, voK, OFF_K, 1, j); });
    }
    // ---- this wave's rows: Q loads (the fragments go to a[AQ ..] further down)
    int q[2], ks_q[2];
    u32x4 qreg[2][8];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        q[blk] = q0w + blk * 32 + lq;
        const int qc = q[blk] < L ? q[blk] : L - 1;
        ks_q[blk] = kstart ? kstart[(long)b * L + qc] : 0;
        if constexpr (WIN) ks_q[blk] = win_lo(q[blk], ks_q[blk], W);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            qreg[blk][ks] = *reinterpret_cast<const u32x4*>(Q + ((long)b * L + qc) * ldq + (long)h * HD + (ks * 2 + hh) * 8);
    }
    // key-liveness word of tile t (padding mask and the Lk tail): wave w ballots tiles f + w, f + w + 4, ... into LDS, eight loads in
    // flight at a time
    {
        unsigned long long* tb = reinterpret_cast<unsigned long long*>(smem + OFF_BITS);
        for (int t0 = t_first + wave; t0 < ntiles; t0 += 32) {
            int ok[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int key = (t0 + 4 * i) * 64 + lane;
                ok[i] = key < Lk;
                if (kmask != nullptr && ok[i]) ok[i] = kmask[(long)b * Lk + key] != 0;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned long long w = __ballot(ok[i]);
                if (lane == 0 && t0 + 4 * i < ntiles) tb[t0 + 4 * i - t_first] = w;
            }
        }
    }
    const unsigned bits_addr = lds0 + OFF_BITS;
    // asm: the compiler must see no LDS read in the loop.  The word of tile t+1 is requested right behind barrier(t) and collected at the
    // top of the next step, behind the lgkmcnt(0) that closes every step.
    u32x2 bits_w;
    auto request_bits = [&](int t) __attribute__((always_inline)) {
        asm volatile("ds_read_b64 %0, %1" : "=v"(bits_w) : "v"(bits_addr + (unsigned)(t - t_first) * 8u));
    };
    auto collect_bits = [&]() __attribute__((always_inline)) -> unsigned long long {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bits_w));
        return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)bits_w[1]) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)bits_w[0]);
    };

    // ---- accumulators and softmax state
    f32x16 sA[2], sB[2];       // S^T of the current tile: key block x (key row, query column)
    u32x4 pA[4], pB[4];        // P fragments (bf16 pairs): 16 keys each
    static_for<0, 128>([&](auto r) __attribute__((always_inline)) { agpr_write<AO + decltype(r)::value>(0u); });
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int e = 0; e < 16; ++e) { sA[sb][e] = -INFINITY; sB[sb][e] = -INFINITY; }      // the "previous tile" of the first one: P = 0
#pragma unroll
    for (int g = 0; g < 4; ++g) { pA[g] = u32x4{0u, 0u, 0u, 0u}; pB[g] = u32x4{0u, 0u, 0u, 0u}; }
    static_for<0, 16>([&](auto j) __attribute__((always_inline)) { vf_zero4<VF + 4 * decltype(j)::value>(); });      // V^T fragments
    Softmax smA, smB;
    smA.m = -INFINITY, smA.negm = 0.f, smA.th = -INFINITY, smA.l = 0.f, smA.l0 = 0.f, smA.tm = -INFINITY;
    smA.pw0 = smA.pw1 = smA.pw2 = 0.f, smA.tw0 = smA.tw1 = smA.tw2 = -INFINITY;
    smB.m = -INFINITY, smB.negm = 0.f, smB.th = -INFINITY, smB.l = 0.f, smB.l0 = 0.f, smB.tm = -INFINITY;
    smB.pw0 = smB.pw1 = smB.pw2 = 0.f, smB.tw0 = smB.tw1 = smB.tw2 = -INFINITY;

    // ---- softmax pieces
    // Score element E of a block: P = exp2(S c - m) against the row's CURRENT reference max -- no max pass in front of the exps.  The
    // tile's largest exponent is collected on the side (one v_max3 per two elements) and checked once, after element 31: only if some
    // row's exceeds th is the tile redone against a raised m (softmax_fixup; S is left intact for that -- P goes to a three-element
    // window and the bf16 fragment).  Rare: the first live tile of a row, then whenever a row's max grows by more than LAZY_TH.
    // The add into the running sum, the bf16 pair and the max trail the exp by one element: nothing right behind a v_exp depends on it.
    auto exp_elem = [&](auto ec, f32x16 (&s)[2], Softmax& sm, u32x4 (&p)[4]) __attribute__((always_inline)) {
        constexpr int E = decltype(ec)::value;
#ifdef FWD64_PROBE_NO_EXP
        return;
#endif
        if constexpr (E == 0) {
            sm.l0 = sm.l;
            sm.tm = -INFINITY;
        }
        if constexpr (E > 0) sm.l += WIN_P(sm, (E - 1));
        if constexpr (E >= 2 && (E & 1) == 0) {
            p[(E - 2) >> 3][((E - 2) & 7) >> 1] = pack_bf2(WIN_P(sm, (E - 2)), WIN_P(sm, (E - 1)));
            sm.tm = max3(sm.tm, WIN_T(sm, (E - 2)), WIN_T(sm, (E - 1)));
            asm volatile("" : "+v"(p[(E - 2) >> 3]), "+v"(sm.tm));       // pins: the code sinker would move all of this to the consumer
        }
        WIN_T(sm, E) = __builtin_fmaf(s[E >> 4][E & 15], c, sm.negm);
        WIN_P(sm, E) = __builtin_amdgcn_exp2f(WIN_T(sm, E));
        asm volatile("" : "+v"(WIN_P(sm, E)), "+v"(sm.l));
    };
    // the tile against a raised reference max (wave-uniform branch, rare): P, the fragments and the tile's sum again from S; l and O
    // (which does not hold this tile yet) rescaled
    auto softmax_fixup = [&](f32x16 (&s)[2], Softmax& sm, u32x4 (&p)[4], auto obc) __attribute__((always_inline)) {
        constexpr int OB = decltype(obc)::value;
        const float tmax = pair_max(sm.tm);
        const bool upd = tmax > sm.th;
        const float m_new = upd ? tmax - sm.negm : sm.m;
        const float alpha = upd ? __builtin_amdgcn_exp2f(sm.m - m_new) : 1.f;      // m = -inf: 0 (l0 and O are still 0)
        sm.m = m_new;
        sm.negm = m_new == -INFINITY ? 0.f : -m_new;
        sm.th = upd ? LAZY_TH : sm.th;
        float lsum = 0.f;
#pragma unroll
        for (int E = 0; E < 32; E += 2) {
            const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[E >> 4][E & 15], c, sm.negm));
            const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[E >> 4][(E & 15) + 1], c, sm.negm));
            lsum += p0 + p1;
            p[E >> 3][(E & 7) >> 1] = pack_bf2(p0, p1);
        }
        sm.l = sm.l0 * alpha + lsum;
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");       // this O's last MFMA is at least a phase back; belt and braces
        static_for<0, 16>([&](auto r) __attribute__((always_inline)) { agpr_scale4<OB + 4 * decltype(r)::value>(alpha); });
        asm volatile("s_nop 2" ::: "memory");                  // accvgpr_write -> MFMA src C
    };
    // element 31's trailing work, then the check
    auto exp_finish = [&](f32x16 (&s)[2], Softmax& sm, u32x4 (&p)[4], auto obc) __attribute__((always_inline)) {
#ifdef FWD64_PROBE_NO_EXP
        return;
#endif
        sm.l += WIN_P(sm, 31);
        p[3][3] = pack_bf2(WIN_P(sm, 30), WIN_P(sm, 31));
        sm.tm = max3(sm.tm, WIN_T(sm, 30), WIN_T(sm, 31));
        asm volatile("" : "+v"(p[3]), "+v"(sm.l));
        if (__builtin_expect(__any(sm.tm > sm.th), 0)) softmax_fixup(s, sm, p, obc);
    };
    // mask pre-pass: dead scores -> -inf (key padding bits, causal, sample start); keys of element (sb, r): sb*32 + (r&3) + 8*(r>>2) + 4*hh
    auto mask_scores = [&](f32x16 (&s)[2], int blk, int key0, unsigned long long bits) __attribute__((always_inline)) {
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");      // the scores' last MFMA may be only one gap back
        // everything lane- or tile-dependent is folded into three per-tile values so that the per-element tests compare against
        // immediates (nothing loop-invariant for the compiler to hoist into registers)
        const unsigned long long lb = bits >> (4 * hh);
        const unsigned w[2] = {(unsigned)lb, (unsigned)(lb >> 32)};
        const int dq = CAUSAL ? q[blk] - key0 - 4 * hh : 64;     // live iff kl <= dq
        const int dk = ks_q[blk] - key0 - 4 * hh;                // live iff kl >= dk
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kb = (r & 3) + 8 * (r >> 2), kl = sb * 32 + kb;
                const bool live = ((w[sb] >> kb) & 1u) && kl <= dq && kl >= dk;
                s[sb][r] = live ? s[sb][r] : -INFINITY;
            }
    };

    // ---- the rest of the ring: V(f+1) K(f+2) | V(f+2) K(f+3) -- what the steady-state count expects to find in flight
    static_for<2, NS>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        const __amdgpu_buffer_rsrc_t rv = tile_desc(Vb, (int)ldv, t_first + i - 1), rk = tile_desc(Kb, (int)ldk, t_first + i);
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rv, voV, OFF_V, i - 1, j); });
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rk, voK, OFF_K, i, j); });
    });
    asm volatile("" : "+v"(qreg[0][0]), "+v"(qreg[0][1]), "+v"(qreg[0][2]), "+v"(qreg[0][3]), "+v"(qreg[0][4]), "+v"(qreg[0][5]),
                 "+v"(qreg[0][6]), "+v"(qreg[0][7]), "+v"(qreg[1][0]), "+v"(qreg[1][1]), "+v"(qreg[1][2]), "+v"(qreg[1][3]),
                 "+v"(qreg[1][4]), "+v"(qreg[1][5]), "+v"(qreg[1][6]), "+v"(qreg[1][7]));
    static_for<0, 16>([&](auto ic) __attribute__((always_inline)) {
        constexpr int blk = decltype(ic)::value >> 3, ks = decltype(ic)::value & 7;
        agpr_write<AQ + 32 * blk + 4 * ks + 0>(qreg[blk][ks][0]);
        agpr_write<AQ + 32 * blk + 4 * ks + 1>(qreg[blk][ks][1]);
        agpr_write<AQ + 32 * blk + 4 * ks + 2>(qreg[blk][ks][2]);
        agpr_write<AQ + 32 * blk + 4 * ks + 3>(qreg[blk][ks][3]);
    });
    // wave-uniform sample-start bounds: no key below ks_min is live for any row, keys below ks_max[blk] need the pre-pass
    int ks_min = 0, ks_max[2] = {0, 0};
    if (kstart || WIN) {
        ks_min = -(int)wave_max((float)-(ks_q[0] < ks_q[1] ? ks_q[0] : ks_q[1]));     // exact below 2^24
        ks_max[0] = (int)wave_max((float)ks_q[0]);
        ks_max[1] = (int)wave_max((float)ks_q[1]);
        ks_min = __builtin_amdgcn_readfirstlane(ks_min);
        ks_max[0] = __builtin_amdgcn_readfirstlane(ks_max[0]);
        ks_max[1] = __builtin_amdgcn_readfirstlane(ks_max[1]);
    }
    asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" ::: "memory");      // K(f), V(f), K(f+1); the liveness words (ds_write)
    __builtin_amdgcn_s_barrier();      // raw: __syncthreads() is a fence and would drain the whole ring (vmcnt(0))
    request_bits(t_first);
    static_for<0, 16>([&](auto i) __attribute__((always_inline)) { lds_read_k<i.value, (i.value >> 3) * 32 * 256>(kaddr[i.value & 7]); });
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 2" ::: "memory");      // also: accvgpr_write (Q fragments, O = 0) -> MFMA operand

#ifdef FWD64_PROBE_TIMING
    const unsigned long long T1 = __builtin_amdgcn_s_memtime();
#endif
    // ---- one tile, ring slot SLOT = (t - t_first) & 1.  Gap n = MFMA n of the tile plus its fillers.
    auto tile = [&](auto slotc, int t, bool active, bool maskA, bool maskB, unsigned long long bits_t) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slotc)::value;
        constexpr int VS = SLOT * TILE;                                         // immediate offset of this tile's V slot
        constexpr int KN = ((SLOT + 1) % NS) * TILE;                            // next tile's K slot
        constexpr int VD = (SLOT + NS - 1) % NS, KD = SLOT;                     // slots the DMA of V(t+NS-1) / K(t+NS) goes to
        const int key0 = t * 64;
        if (active) {
            // Ph1: S_A(t) | B elements 14 .. 31 of the previous tile, its check
            static_for<0, 16>([&](auto i) __attribute__((always_inline)) {
                constexpr int I = i.value, ks = I >> 1, sb = I & 1;
                if constexpr (ks == 0) mfma_s0<sb * 8 + ks, ks>(sA[sb]);
                else mfma_s<sb * 8 + ks, ks>(sA[sb]);
                constexpr int e0 = 14 + (I * 18) / 16, e1 = 14 + ((I + 1) * 18) / 16;
                static_for<e0, e1>([&](auto e) __attribute__((always_inline)) { exp_elem(e, sB, smB, pB); });
                if constexpr (I == 15) exp_finish(sB, smB, pB, std::integral_constant<int, AO + 64>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        // barrier(t): V(t) and K(t+1) have landed for every wave (the 16 younger pieces may still fly); everybody is done with V(t-1)'s
        // slot and -- the K fragments of tile t were read a tile ago -- with K(t)'s
#ifndef FWD64_PROBE_NO_VMWAIT
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
#endif
#ifndef FWD64_PROBE_NO_BARRIER
        __builtin_amdgcn_s_barrier();
#endif
        request_bits(t + 1);
        if (active) {
            // Ph2: O_B += V(t-1)^T.P_B(t-1) | V^T fragments of tile t (fragment j is free once MFMA j has issued) | A elements 0 .. 13
            static_for<0, 16>([&](auto j) __attribute__((always_inline)) {
                constexpr int J = j.value;
                mfma_o<AO + 64 + 16 * (J & 3), J>(pB[J >> 2]);
                lds_read_vt<J, VS + (J >> 2) * 16 * 256>(vaddr[J & 3], vaddr8[J & 3]);
                if constexpr (J == 1) {
                    asm volatile("" : "+v"(sA[0]), "+v"(sA[1]));        // S_A's last MFMA is two gaps back: readable from here on
                    if (__builtin_expect(maskA, 0)) mask_scores(sA, 0, key0, bits_t);
                }
                if constexpr (J >= 2) exp_elem(std::integral_constant<int, J - 2>{}, sA, smA, pA);
                __builtin_amdgcn_sched_barrier(0);
            });
            // Ph3: S_B(t) | the DMA of V(t+NS-1) | A elements 14 .. 31, A's check
            const __amdgpu_buffer_rsrc_t rv = tile_desc(Vb, (int)ldv, t + NS - 1), rk = tile_desc(Kb, (int)ldk, t + NS);
            static_for<0, 16>([&](auto i) __attribute__((always_inline)) {
                constexpr int I = i.value, ks = I >> 1, sb = I & 1;
                if constexpr (ks == 0) mfma_s0<sb * 8 + ks, 8 + ks>(sB[sb]);
                else mfma_s<sb * 8 + ks, 8 + ks>(sB[sb]);
                if constexpr ((I & 3) == 1) dma_piece(rv, voV, OFF_V, VD, std::integral_constant<int, I / 4>{});
                constexpr int e0 = 14 + (I * 18) / 16, e1 = 14 + ((I + 1) * 18) / 16;
                static_for<e0, e1>([&](auto e) __attribute__((always_inline)) { exp_elem(e, sA, smA, pA); });
                if constexpr (I == 15) exp_finish(sA, smA, pA, std::integral_constant<int, AO>{});
                __builtin_amdgcn_sched_barrier(0);
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // V^T fragments (issued a phase ago)
            // Ph4: O_A += V(t)^T.P_A(t) | K fragments of tile t+1, then the DMA of K(t+NS) | B elements 0 .. 13
            static_for<0, 16>([&](auto j) __attribute__((always_inline)) {
                constexpr int J = j.value;
                mfma_o<AO + 16 * (J & 3), J>(pA[J >> 2]);
                if constexpr (J < 8) {
                    lds_read_k<2 * J, KN + ((2 * J) >> 3) * 32 * 256>(kaddr[(2 * J) & 7]);
                    lds_read_k<2 * J + 1, KN + ((2 * J + 1) >> 3) * 32 * 256>(kaddr[(2 * J + 1) & 7]);
                }
                if constexpr (J >= 9 && (J & 1) == 1) dma_piece(rk, voK, OFF_K, KD, std::integral_constant<int, (J - 9) / 2>{});
                if constexpr (J == 1) {
                    asm volatile("" : "+v"(sB[0]), "+v"(sB[1]));
                    if (__builtin_expect(maskB, 0)) mask_scores(sB, 1, key0, bits_t);
                }
                if constexpr (J >= 2) exp_elem(std::integral_constant<int, J - 2>{}, sB, smB, pB);
                __builtin_amdgcn_sched_barrier(0);
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // K fragments of tile t+1
        } else {
            // this wave has no live key in tile t: keep the ring going
            const __amdgpu_buffer_rsrc_t rv = tile_desc(Vb, (int)ldv, t + NS - 1), rk = tile_desc(Kb, (int)ldk, t + NS);
            static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rv, voV, OFF_V, VD, j); });
            static_for<0, 4>([&](auto j) __attribute__((always_inline)) { dma_piece(rk, voK, OFF_K, KD, j); });
            static_for<0, 16>([&](auto i) __attribute__((always_inline)) { lds_read_k<i.value, KN + (i.value >> 3) * 32 * 256>(kaddr[i.value & 7]); });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    };
    auto step = [&](auto slotc, int t) __attribute__((always_inline)) {
        const int key0 = t * 64;
        const unsigned long long bits = collect_bits();
        const bool active = !(CAUSAL && key0 > q0w + 63) && bits != 0ull && key0 + 63 >= ks_min;
        const bool part = bits != ~0ull;
        const bool maskA = part || (CAUSAL && key0 + 63 > q0w) || key0 < ks_max[0];
        const bool maskB = part || (CAUSAL && key0 + 63 > q0w + 32) || key0 < ks_max[1];
        tile(slotc, t, active, maskA, maskB, bits);
    };
    for (int t = t_first; t < ntiles; t += NS) {
        step(std::integral_constant<int, 0>{}, t);
        if (t + 1 >= ntiles) break;
        step(std::integral_constant<int, 1>{}, t + 1);
        if (t + 2 >= ntiles) break;
        step(std::integral_constant<int, 2>{}, t + 2);
        if (t + 3 >= ntiles) break;
        step(std::integral_constant<int, 3>{}, t + 3);
    }
#ifdef FWD64_PROBE_TIMING
    const unsigned long long T2 = __builtin_amdgcn_s_memtime();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the ring's last (empty) DMA pieces must not outlive the workgroup's LDS
    // ---- drain: the last live tile's block B -- elements 14 .. 31 and the check, then O_B += V^T.P_B
    static_for<14, 32>([&](auto e) __attribute__((always_inline)) { exp_elem(e, sB, smB, pB); });
    exp_finish(sB, smB, pB, std::integral_constant<int, AO + 64>{});
    asm volatile("s_nop 1" : "+v"(pB[0]), "+v"(pB[1]), "+v"(pB[2]), "+v"(pB[3]));
    static_for<0, 16>([&](auto j) __attribute__((always_inline)) { mfma_o<AO + 64 + 16 * (j.value & 3), j.value>(pB[j.value >> 2]); });
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");      // MFMA result -> v_accvgpr_read

    // ---- epilogue: O = O^T / l, LSE = m ln2 + ln l
    auto store_block = [&](auto blkc, const Softmax& sm) __attribute__((always_inline)) {
        constexpr int blk = decltype(blkc)::value;
        const float l_tot = sm.l + __shfl_xor(sm.l, 32, 64);
        const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
        bf16_t* op = O + ((long)b * L + q[blk]) * ldo + (long)h * HD;
        static_for<0, 16>([&](auto gc) __attribute__((always_inline)) {
            constexpr int d = decltype(gc)::value >> 2, g4 = decltype(gc)::value & 3, R = AO + 64 * blk + 16 * d + 4 * g4;
            const int dd = d * 32 + 8 * g4 + 4 * hh;
            u32x2 w;
            w[0] = pack_bf2(agpr_read<R>() * inv, agpr_read<R + 1>() * inv);
            w[1] = pack_bf2(agpr_read<R + 2>() * inv, agpr_read<R + 3>() * inv);
            if (q[blk] < L) *reinterpret_cast<u32x2*>(op + dd) = w;
        });
        if (q[blk] < L && hh == 0 && LSE) LSE[((long)b * H + h) * L + q[blk]] = l_tot > 0.f ? sm.m * LN2 + logf(l_tot) : INFINITY;
    };
    store_block(std::integral_constant<int, 0>{}, smA);
    store_block(std::integral_constant<int, 1>{}, smB);
#ifdef FWD64_PROBE_TIMING      // per wave: prologue / loop / epilogue cycles and the tile count, over the LSE words of its first rows
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long T3 = __builtin_amdgcn_s_memtime();
    if (lane == 0 && LSE && q0w + 3 < L) {
        float* w = LSE + ((long)b * H + h) * L + q0w;
        w[0] = (float)(T1 - T0);
        w[1] = (float)(T2 - T1);
        w[2] = (float)(T3 - T2);
        w[3] = (float)(ntiles - t_first);
    }
#endif
