// Body of the attn_fwd_kernel / attn_fwd_win_kernel kernels (included inside them: each kernel compiles from this text
// with its own constexpr CAUSAL / WIN / W).
    using C = AttnCfg<HD>;
    using Y = Lay<HD>;
    constexpr int TILE = 64 * Y::PITCH;
    constexpr int BUF = 2 * TILE + 64 * 4 + 16;
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, lq = lane & 31;
    const int gx = (L + 127) >> 7;
    int bx, h, b;
    xcd_tile_map(gx, H, bx, h, b, CAUSAL);
    const int hk = h / (H / Hkv);
    const int qb = CAUSAL ? (gx - 1 - bx) : bx;   // causal: longest rows first
    const int qblk0 = qb * 128, q0 = qblk0 + wave * 32, q = q0 + lq;
    const int qc = q < L ? q : L - 1;
    const float c = scale * LOG2E;
    // packed samples: query q attends keys >= kstart[q] only (its own sample; non-decreasing in q).  ks_q = this lane's bound,
    // ks_hi = the largest bound in the wave's 32 rows (tiles below it need per-element masking), t_first = first tile any row of
    // the workgroup's 128-query block can see
    const int ks_q = WIN ? win_lo(q, kstart ? kstart[(long)b * L + qc] : 0, W) : (kstart ? kstart[(long)b * L + qc] : 0);
    const int ks_hi = WIN ? __builtin_amdgcn_readfirstlane(
                                win_lo(q0 + 31, kstart ? kstart[(long)b * L + (q0 + 31 < L ? q0 + 31 : L - 1)] : 0, W))
                          : (kstart ? kstart[(long)b * L + (q0 + 31 < L ? q0 + 31 : L - 1)] : 0);
    const int t_first = WIN ? (win_lo(qblk0, kstart ? kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] : 0, W) >> 6)
                            : (kstart ? (kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] >> 6) : 0);
    // (WIN) the wave's first row; the wave-uniform bounds live in scalar registers
    const int ks_lo = WIN ? __builtin_amdgcn_readfirstlane(win_lo(q0, kstart ? kstart[(long)b * L + (q0 < L ? q0 : L - 1)] : 0, W)) : 0;

    bf16x8 qf[C::NKS];
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) {
        const int ch = ks * 2 + hh;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (ch * 8 < HD) v = *reinterpret_cast<const u32x4*>(Q + ((long)b * L + qc) * ldq + (long)h * HD + ch * 8);
        qf[ks] = as_bf16x8(v);
    }
    f32x16 oacc[C::NDB];
#pragma unroll
    for (int d = 0; d < C::NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int kend = CAUSAL ? (qblk0 + 128 < L ? qblk0 + 128 : L) : Lk;      // Lk: number of keys (== L except for cross attention)
    const int ntiles = (kend + 63) / 64;
    const bf16_t* Kb = K + (long)b * Lk * ldk + (long)hk * HD;
    const bf16_t* Vb = V + (long)b * Lk * ldv + (long)hk * HD;

    // tile t -> LDS buffer (t & 1): global -> registers -> LDS in one go (registers are only live across the copy, so the kernel
    // fits 2 waves per SIMD; the copy of tile t+1 overlaps the MFMA work of the co-resident workgroup / partner waves)
    // the key-mask word of a tile is fetched one stage() call ahead of its use (stage calls walk consecutive tiles): a load issued
    // here, behind the tile's DMA, would be waited for with vmcnt(0) -- wave 0 would sit out the whole DMA round trip on every tile
    // (measured on the Llama-3 geometry, round 3: forward 169 us without a key mask, 207 us with one)
    auto key_live = [&](int t) -> bool {
        const int key = t * 64 + (int)threadIdx.x;
        return threadIdx.x < 64 && key < Lk && (kmask == nullptr || kmask[(long)b * Lk + key] != 0);
    };
    bool live_next = key_live(t_first);
    auto stage = [&](int t) {
        const int key0 = t * 64;
        char* base = smem + (t & 1) * BUF;
        const bool ok = live_next;
        live_next = key_live(t + 1);
        if constexpr (Y::DMA) {
            stage_tile_dma<64>(Kb + (long)key0 * ldk, ldk, Lk - key0, base);
            stage_tile_dma<64>(Vb + (long)key0 * ldv, ldv, Lk - key0, base + TILE);
        } else {
            {
                TileRegs<64, C::NCH> rk;
                rk.load(Kb + (long)key0 * ldk, ldk, Lk - key0, HD);
                rk.store(base, C::PITCH);
            }
            {
                TileRegs<64, C::NCH> rv;
                rv.load(Vb + (long)key0 * ldv, ldv, Lk - key0, HD);
                rv.store(base + TILE, C::PITCH);
            }
        }
        if (threadIdx.x < 64) {     // wave 0: additive key bias (0 / -inf) + one flag "this tile has a masked key"
            float* bp = reinterpret_cast<float*>(base + 2 * TILE);
            bp[threadIdx.x] = ok ? 0.f : -INFINITY;
            const unsigned long long okm = __ballot(ok);
            if (threadIdx.x == 0) bp[64] = (okm == ~0ull) ? 0.f : 1.f;
        }
    };
    // register-staged layouts (hd != 128): the next tile's global loads are issued BEFORE this tile's MFMA / softmax work and written to
    // LDS AFTER it, so the HBM / L2 latency rides behind the compute instead of stalling the wave in front of it (24 VGPRs at hd 72 /
    // 80 / 96); the key bias words of the next tile go to its (free) LDS buffer right away
    auto stage_bias = [&](int t) {
        const bool ok = live_next;
        live_next = key_live(t + 1);
        if (threadIdx.x < 64) {
            float* bp = reinterpret_cast<float*>(smem + (t & 1) * BUF + 2 * TILE);
            bp[threadIdx.x] = ok ? 0.f : -INFINITY;
            const unsigned long long okm = __ballot(ok);
            if (threadIdx.x == 0) bp[64] = (okm == ~0ull) ? 0.f : 1.f;
        }
    };
    stage(t_first);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int t = t_first; t < ntiles; ++t) {
        const int key0 = t * 64;
        const char* sK = smem + (t & 1) * BUF;
        const char* sV = sK + TILE;
        const float* sBias = reinterpret_cast<const float*>(sK + 2 * TILE);
        const bool more = t + 1 < ntiles;
        TileRegs<64, C::NCH> nk_regs, nv_regs;          // (unused on the one-go paths)
        // hd <= 64 keeps the one-go copy: it runs 3 waves per SIMD at 168 VGPRs, which the 24 staging registers would cost
        // (measured: CLIP hd 64 29.3 -> 36.8 us with the split; hd 72 / 80 / 96, at 2 waves either way: -9 ... -16 %)
        constexpr bool SPLIT_STAGE = !Y::DMA && HD > 64;
        if constexpr (!SPLIT_STAGE) {
            if (more) stage(t + 1);
        } else {
            if (more) {
                const int kn = (t + 1) * 64;
                nk_regs.load(Kb + (long)kn * ldk, ldk, Lk - kn, HD);
                nv_regs.load(Vb + (long)kn * ldv, ldv, Lk - kn, HD);
                stage_bias(t + 1);
            }
        }
        // wave-uniform: skip tiles entirely in this wave's future, or (WIN) wholly behind its window (tiles wholly before the wave's
        // samples are harmless: fully masked, p = 0, running max stays -inf)
        if (!(CAUSAL && key0 > q0 + 31) && !(WIN && key0 + 63 < ks_lo)) {
            f32x16 s[2];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int e = 0; e < 16; ++e) s[sb][e] = 0.f;
            constexpr int FD = ATTN_FRAG_DEPTH;
            FragU fb4[8];                       // fragment ring (FD in flight) shared by the S phase (K rows) and the P.V phase (V^T)
            unsigned vaddr[4], vaddr8[4];
            if constexpr (Y::DMA) {
                const unsigned ldsK = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)sK;
                unsigned kaddr[8];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) kaddr[ks] = ldsK + Y::chunk_off(lq, ks * 2 + hh);
                {
                    const int sl = lane & 15, g16 = (lane >> 4) & 1;
                    const int row = 4 * hh + (sl >> 2);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int col = d * 32 + 16 * g16 + (sl & 3) * 4;
                        const int off = Y::chunk_off(row, col >> 3) + (col & 7) * 2;
                        vaddr[d] = ldsK + TILE + off;
                        vaddr8[d] = ldsK + TILE + ((off + 8 * Y::PITCH) ^ 32);
                    }
                }
                // S = K.Q^T: 16 MFMAs, K fragment i + 3 requested in the shadow of MFMA i
                // slot i computes key block i & 1, k-chunk i >> 1: consecutive MFMAs alternate between the two score accumulators (round 3:
                // eight back-to-back MFMAs into ONE accumulator wait for each other's result -- PMC: 32 % of the wave cycles were
                // MFMA-dependency stalls -- ATTN_S_INTERLEAVE=0 restores the old order for A/B)
#ifndef ATTN_S_INTERLEAVE
#define ATTN_S_INTERLEAVE 1
#endif
                static_for<0, FD>([&](auto ic) {
                    constexpr int i = decltype(ic)::value, fr = ATTN_S_INTERLEAVE ? (i & 1) * 8 + (i >> 1) : i;
                    issue_kfrag<fr>(fb4[i & 7].f, kaddr);
                });
                static_for<0, 16>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    constexpr int sb = ATTN_S_INTERLEAVE ? (i & 1) : (i >> 3), ks = ATTN_S_INTERLEAVE ? (i >> 1) : (i & 7);
                    wait_lgkm<(15 - i) < FD - 1 ? (15 - i) : FD - 1>();      // requested so far: fragments <= i + FD - 1
                    __builtin_amdgcn_sched_barrier(0);
                    s[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb4[i & 7].f, qf[ks], s[sb], 0, 0, 0);
                    if constexpr (i + FD < 16) {
                        constexpr int n = i + FD, fr = ATTN_S_INTERLEAVE ? (n & 1) * 8 + (n >> 1) : n;
                        issue_kfrag<fr>(fb4[n & 7].f, kaddr);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
                // the first FD V^T fragments travel while the softmax runs
                static_for<0, FD>([&](auto jc) { issue_vfrag<decltype(jc)::value>(fb4[decltype(jc)::value & 7], vaddr, vaddr8); });
            } else {
#pragma unroll
                for (int ks = 0; ks < C::NKS; ++ks)
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb) {        // alternate the two accumulators (see the hd-128 branch)
                        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + Y::chunk_off(sb * 32 + lq, ks * 2 + hh));
                        s[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[sb], 0, 0, 0);
                    }
            }
            float mx = -INFINITY;
            // wave-uniform: only tiles that touch the diagonal or contain masked keys pay for per-element masking
            const bool need_mask = (CAUSAL && key0 + 63 > q0) || sBias[64] != 0.f || key0 < ks_hi;
            if (need_mask) {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        float v = s[sb][r] * c + sBias[kl];
                        if (CAUSAL && key0 + kl > q) v = -INFINITY;
                        if (key0 + kl < ks_q) v = -INFINITY;
                        s[sb][r] = v;
                        mx = fmaxf(mx, v);
                    }
            } else {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sb][r]);      // raw scores: the scale is folded into the exp below
                mx *= c;                                                        // c > 0: max commutes with the scaling
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float msafe = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
            float psum = 0.f;
            if (need_mask) {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = __builtin_amdgcn_exp2f(s[sb][r] - msafe);
                        s[sb][r] = p;
                        psum += p;
                    }
            } else {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[sb][r], c, -msafe));
                        s[sb][r] = p;
                        psum += p;
                    }
            }
            l_run = l_run * alpha + psum;
            m_run = m_new;
            if (__any(alpha != 1.f)) {     // wave-uniform: once the running maxima have settled nothing needs rescaling
#pragma unroll
                for (int d = 0; d < C::NDB; ++d)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
            }
            if constexpr (Y::DMA) {
                // O^T += V^T.P: 16 MFMAs, V^T fragment j + 3 (two transposing reads) requested in the shadow of MFMA j
                bf16x8 pfr[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pfr[g] = pack_frag(s[g >> 1], g & 1);
                static_for<0, 16>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    wait_lgkm<((15 - j) < FD - 1 ? (15 - j) : FD - 1) * 2>();      // requested so far: fragments <= j + FD - 1 (two reads each)
                    __builtin_amdgcn_sched_barrier(0);
                    oacc[j & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb4[j & 7].f, pfr[j >> 2], oacc[j & 3], 0, 0, 0);
                    if constexpr (j + FD < 16) issue_vfrag<j + FD>(fb4[(j + FD) & 7], vaddr, vaddr8);
                    __builtin_amdgcn_sched_barrier(0);
                });
            } else {
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int cp = 0; cp < 2; ++cp) {
                        const bf16x8 pf = pack_frag(s[sb], cp);
#pragma unroll
                        for (int d = 0; d < C::NDB; ++d) {
                            const bf16x8 vf = read_tr_frag<HD>(sV, sb * 32 + 16 * cp, d * 32, lane);
                            oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[d], 0, 0, 0);
                        }
                    }
            }
        }
        if constexpr (SPLIT_STAGE) {
            if (more) {
                char* nb = smem + ((t + 1) & 1) * BUF;      // released by the barrier that ended iteration t - 1
                nk_regs.store(nb, C::PITCH);
                nv_regs.store(nb + TILE, C::PITCH);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next tile's DMA landed (this wave's pieces)
        __syncthreads();
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    if (q < L) {
        bf16_t* op = O + ((long)b * L + q) * ldo + (long)h * HD;
#pragma unroll
        for (int d = 0; d < C::NDB; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dd = d * 32 + 8 * g4 + 4 * hh;
                if (dd < HD) {
                    u32x2 o;
                    o[0] = pack_bf2(oacc[d][4 * g4] * inv, oacc[d][4 * g4 + 1] * inv);
                    o[1] = pack_bf2(oacc[d][4 * g4 + 2] * inv, oacc[d][4 * g4 + 3] * inv);
                    *reinterpret_cast<u32x2*>(op + dd) = o;
                }
            }
        if (hh == 0 && LSE) LSE[((long)b * H + h) * L + q] = l_tot > 0.f ? m_run * LN2 + logf(l_tot) : INFINITY;
    }
