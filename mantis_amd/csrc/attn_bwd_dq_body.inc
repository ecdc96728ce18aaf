// Body of the attn_bwd_dq_kernel / attn_bwd_dq_win_kernel kernels (included inside them: each kernel compiles from this text
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
    const int qb = CAUSAL ? (gx - 1 - bx) : bx;
    const int qblk0 = qb * 128, q0 = qblk0 + wave * 32, q = q0 + lq;
    const int qc = q < L ? q : L - 1;
    const float c = scale * LOG2E;
    // segment bounds of packed samples, window: see attn_fwd_body
    const int ks_q = WIN ? win_lo(q, kstart ? kstart[(long)b * L + qc] : 0, W) : (kstart ? kstart[(long)b * L + qc] : 0);
    const int ks_hi = WIN ? __builtin_amdgcn_readfirstlane(
                                win_lo(q0 + 31, kstart ? kstart[(long)b * L + (q0 + 31 < L ? q0 + 31 : L - 1)] : 0, W))
                          : (kstart ? kstart[(long)b * L + (q0 + 31 < L ? q0 + 31 : L - 1)] : 0);
    const int t_first = WIN ? (win_lo(qblk0, kstart ? kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] : 0, W) >> 6)
                            : (kstart ? (kstart[(long)b * L + (qblk0 < L ? qblk0 : L - 1)] >> 6) : 0);
    // (WIN) the wave's first row; the wave-uniform bounds live in scalar registers
    const int ks_lo = WIN ? __builtin_amdgcn_readfirstlane(win_lo(q0, kstart ? kstart[(long)b * L + (q0 < L ? q0 : L - 1)] : 0, W)) : 0;

    bf16x8 qf[C::NKS], dof[C::NKS];
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) {
        const int ch = ks * 2 + hh;
        u32x4 v = {0u, 0u, 0u, 0u}, w = {0u, 0u, 0u, 0u};
        if (ch * 8 < HD) {
            v = *reinterpret_cast<const u32x4*>(Q + ((long)b * L + qc) * ldq + (long)h * HD + ch * 8);
            w = *reinterpret_cast<const u32x4*>(dO + ((long)b * L + qc) * ldo + (long)h * HD + ch * 8);
        }
        qf[ks] = as_bf16x8(v);
        dof[ks] = as_bf16x8(w);
    }
    const float lse2 = LSE[((long)b * H + h) * L + qc] * LOG2E;
    // D = rowsum(dO * O): given, or (Ofwd != nullptr) computed here from the dO fragments already in registers -- the lane pair
    // (l, l + 32) covers the row's head dimension -- and published for the dK/dV kernel that runs after this one
    float dsum;
    if (Ofwd != nullptr) {
        float part = 0.f;
#pragma unroll
        for (int ks = 0; ks < C::NKS; ++ks) {
            const int ch = ks * 2 + hh;
            if (ch * 8 < HD) {
                const u32x4 o = *reinterpret_cast<const u32x4*>(Ofwd + ((long)b * L + qc) * ldout + (long)h * HD + ch * 8);
                union { bf16x8 f; u32x4 u; } dv;
                dv.f = dof[ks];
#pragma unroll
                for (int e = 0; e < 4; ++e) part += bf2f_lo(o[e]) * bf2f_lo(dv.u[e]) + bf2f_hi(o[e]) * bf2f_hi(dv.u[e]);
            }
        }
        dsum = part + __shfl_xor(part, 32, 64);
        if (hh == 0 && q < L) Dsum[((long)b * H + h) * L + q] = dsum;
    } else {
        dsum = Dsum[((long)b * H + h) * L + qc];
    }
    f32x16 acc[C::NDB];
#pragma unroll
    for (int d = 0; d < C::NDB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[d][e] = 0.f;

    const int kend = CAUSAL ? (qblk0 + 128 < L ? qblk0 + 128 : L) : Lk;
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
    stage(t_first);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int t = t_first; t < ntiles; ++t) {
        const int key0 = t * 64;
        const char* sK = smem + (t & 1) * BUF;
        const char* sV = sK + TILE;
        const float* sBias = reinterpret_cast<const float*>(sK + 2 * TILE);
        const bool more = t + 1 < ntiles;
        if (more) stage(t + 1);
        if (!(CAUSAL && key0 > q0 + 31) && !(WIN && key0 + 63 < ks_lo)) {
            const bool need_mask = (CAUSAL && key0 + 63 > q0) || sBias[64] != 0.f || key0 < ks_hi;   // wave-uniform
            // one 32-key half at a time: S, dP -> dS -> dQ contribution, so only 32 score registers are live (2 waves per SIMD)
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                f32x16 s, dp;
#pragma unroll
                for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < C::NKS; ++ks) {
                    const int off = Y::chunk_off(sb * 32 + lq, ks * 2 + hh);
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + off);
                    const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sV + off);
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dp, 0, 0, 0);
                }
                if (need_mask) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        float v = s[r] * c + sBias[kl];
                        if (CAUSAL && key0 + kl > q) v = -INFINITY;
                        if (key0 + kl < ks_q) v = -INFINITY;
                        const float p = __builtin_amdgcn_exp2f(v - lse2);  // lse = +inf for fully masked rows -> p = 0
                        s[r] = p * (dp[r] - dsum);             // the softmax scale is applied once, to the dQ accumulators
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = __builtin_amdgcn_exp2f(s[r] * c - lse2);
                        s[r] = p * (dp[r] - dsum);             // the softmax scale is applied once, to the dQ accumulators
                    }
                }
#pragma unroll
                for (int cp = 0; cp < 2; ++cp) {
                    const bf16x8 dsf = pack_frag(s, cp);
                    if constexpr (kDqTrAsm && Y::DMA) {
                        // hd 128: hand-issued K^T reads (the builtin's s_waitcnt vmcnt(0) would wait for the NEXT tile's DMA right here)
                        bf16x8 kt[4];
                        read_tr_frag4_sync(sK, sb * 32 + 16 * cp, lane, kt);
#pragma unroll
                        for (int d = 0; d < 4; ++d) acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt[d], dsf, acc[d], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int d = 0; d < C::NDB; ++d) {
                            const bf16x8 ktf = read_tr_frag<HD>(sK, sb * 32 + 16 * cp, d * 32, lane);
                            acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dsf, acc[d], 0, 0, 0);
                        }
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (q < L) {
        bf16_t* op = dQ + ((long)b * L + q) * lddq + (long)h * HD;
#pragma unroll
        for (int d = 0; d < C::NDB; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dd = d * 32 + 8 * g4 + 4 * hh;
                if (dd < HD) {
                    u32x2 o;
                    o[0] = pack_bf2(acc[d][4 * g4] * scale, acc[d][4 * g4 + 1] * scale);
                    o[1] = pack_bf2(acc[d][4 * g4 + 2] * scale, acc[d][4 * g4 + 3] * scale);
                    *reinterpret_cast<u32x2*>(op + dd) = o;
                }
            }
    }
