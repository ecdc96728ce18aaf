// Body of the attn_bwd_dkv_kernel / attn_bwd_dkv_win_kernel kernels (included inside them: each kernel compiles from this text
// with its own constexpr CAUSAL / WIN / W).
    using C = AttnCfg<HD>;
    using D = DkvCfg<HD>;
    constexpr int QT = 64;                          // query rows staged per barrier (processed as two 32-row passes)
    using Y = Lay<HD>;
    constexpr int TILE = QT * Y::PITCH;
    constexpr int BUF = 2 * TILE + 3 * QT * 4;      // Q tile | dO tile | lse2[QT] dsum[QT] kstart[QT]
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, lk = lane & 31;
    const int kg = wave / D::DS, dh = wave % D::DS;
    int bx, h, b;
    xcd_tile_map((Lk + D::KEYS - 1) / D::KEYS, H, bx, h, b, CAUSAL);  // L queries, Lk keys (== L except for cross attention)
    const int hk = h / (H / Hkv);
    const int kblk0 = bx * D::KEYS, k0 = kblk0 + kg * 32, key = k0 + lk;   // causal: key block 0 is the heaviest, first
    const int keyc = key < Lk ? key : Lk - 1;
    const float c = scale * LOG2E;
    const bool key_ok = key < Lk && (kmask == nullptr || kmask[(long)b * Lk + keyc] != 0);

    bf16x8 kf[C::NKS], vf[C::NKS];
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) {
        const int ch = ks * 2 + hh;
        u32x4 a = {0u, 0u, 0u, 0u}, w = {0u, 0u, 0u, 0u};
        if (ch * 8 < HD) {
            a = *reinterpret_cast<const u32x4*>(K + ((long)b * Lk + keyc) * ldk + (long)hk * HD + ch * 8);
            w = *reinterpret_cast<const u32x4*>(V + ((long)b * Lk + keyc) * ldv + (long)hk * HD + ch * 8);
        }
        kf[ks] = as_bf16x8(a);
        vf[ks] = as_bf16x8(w);
    }
    f32x16 dkacc[D::NDW], dvacc[D::NDW];
#pragma unroll
    for (int d = 0; d < D::NDW; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dkacc[d][e] = 0.f; dvacc[d][e] = 0.f; }

    const int qstart = CAUSAL ? (kblk0 / QT) : 0;  // first query tile that can see this key block
    int qlim = L;                                   // packed samples: no query at or beyond the end of these keys' sample sees them
    if (qend != nullptr) {
        __shared__ int s_qlim;
        if (threadIdx.x == 0) s_qlim = 0;
        __syncthreads();
        if (threadIdx.x < D::KEYS && kblk0 + (int)threadIdx.x < Lk) atomicMax(&s_qlim, qend[(long)b * Lk + kblk0 + threadIdx.x]);
        __syncthreads();
        qlim = s_qlim < L ? s_qlim : L;
    }
    if constexpr (WIN) qlim = qlim < kblk0 + D::KEYS - 1 + W ? qlim : kblk0 + D::KEYS - 1 + W;
    const int nqt = (qlim + QT - 1) / QT;
    const bf16_t* Qb = Q + (long)b * L * ldq + (long)h * HD;
    const bf16_t* dOb = dO + (long)b * L * ldo + (long)h * HD;

    auto stage = [&](int qt) {
        const int q0 = qt * QT;
        char* base = smem + ((qt - qstart) & 1) * BUF;
        if constexpr (Y::DMA) {
            stage_tile_dma<QT>(Qb + (long)q0 * ldq, ldq, L - q0, base);
            stage_tile_dma<QT>(dOb + (long)q0 * ldo, ldo, L - q0, base + TILE);
        } else {
            {
                TileRegs<QT, C::NCH> rq;
                rq.load(Qb + (long)q0 * ldq, ldq, L - q0, HD);
                rq.store(base, C::PITCH);
            }
            {
                TileRegs<QT, C::NCH> rdo;
                rdo.load(dOb + (long)q0 * ldo, ldo, L - q0, HD);
                rdo.store(base + TILE, C::PITCH);
            }
        }
        if (threadIdx.x < QT) {
            const int qq = q0 + threadIdx.x;
            reinterpret_cast<float*>(base + 2 * TILE)[threadIdx.x] = qq < L ? LSE[((long)b * H + h) * L + qq] * LOG2E : INFINITY;
            reinterpret_cast<float*>(base + 2 * TILE)[QT + threadIdx.x] = qq < L ? Dsum[((long)b * H + h) * L + qq] : 0.f;
            // rows beyond L: "sees no key" (keeps the wave-uniform need_mask test below, which looks at the pass's LAST row, sound)
            if constexpr (WIN)
                reinterpret_cast<int*>(base + 2 * TILE)[2 * QT + threadIdx.x] =
                    qq < L ? win_lo(qq, kstart == nullptr ? 0 : kstart[(long)b * L + qq], W) : 0x7fffffff;
            else
                reinterpret_cast<int*>(base + 2 * TILE)[2 * QT + threadIdx.x] =
                    kstart == nullptr ? 0 : (qq < L ? kstart[(long)b * L + qq] : 0x7fffffff);
        }
    };
    if (qstart < nqt) stage(qstart);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int qt = qstart; qt < nqt; ++qt) {
        const char* tQ = smem + ((qt - qstart) & 1) * BUF;
        if (qt + 1 < nqt) stage(qt + 1);
#pragma unroll 1
        for (int pass = 0; pass < QT / 32; ++pass) {
        const int q0 = qt * QT + pass * 32;
        const char* sQ = tQ + pass * 32 * Y::PITCH;
        const char* sdO = sQ + TILE;
        const float* sLse = reinterpret_cast<const float*>(tQ + 2 * TILE) + pass * 32;
        const float* sDs = sLse + QT;
        const int* sKs = reinterpret_cast<const int*>(tQ + 2 * TILE) + 2 * QT + pass * 32;
        // wave-uniform: skip passes whose every query precedes this wave's keys, or (WIN) is beyond all their windows
        if (!(CAUSAL && q0 + 31 < k0) && !(WIN && q0 >= k0 + 31 + W)) {
            f32x16 s, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < C::NKS; ++ks) {
                const int off = Y::chunk_off(lk, ks * 2 + hh);
                const bf16x8 qa = *reinterpret_cast<const bf16x8*>(sQ + off);
                const bf16x8 da = *reinterpret_cast<const bf16x8*>(sdO + off);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, vf[ks], dp, 0, 0, 0);
            }
            f32x16 ds;
            const bool need_mask = (CAUSAL && k0 + 31 > q0) || !__all(key_ok) || sKs[31] > k0;   // wave-uniform
            if (need_mask) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ql = (r & 3) + 8 * (r >> 2) + 4 * hh;
                    float v = key_ok ? s[r] * c : -INFINITY;
                    if (CAUSAL && key > q0 + ql) v = -INFINITY;
                    if (key < sKs[ql]) v = -INFINITY;
                    const float p = __builtin_amdgcn_exp2f(v - sLse[ql]);
                    s[r] = p;
                    ds[r] = p * (dp[r] - sDs[ql]);       // the softmax scale is applied once, to the dK accumulators
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ql = (r & 3) + 8 * (r >> 2) + 4 * hh;
                    const float p = __builtin_amdgcn_exp2f(s[r] * c - sLse[ql]);
                    s[r] = p;
                    ds[r] = p * (dp[r] - sDs[ql]);       // the softmax scale is applied once, to the dK accumulators
                }
            }
#pragma unroll
            for (int cp = 0; cp < 2; ++cp) {
                const bf16x8 pf = pack_frag(s, cp);
                const bf16x8 dsf = pack_frag(ds, cp);
#pragma unroll
                for (int d = 0; d < D::NDW; ++d) {
                    const int dcol = (dh * D::NDW + d) * 32;
                    const bf16x8 dot = read_tr_frag<HD>(sdO, 16 * cp, dcol, lane);
                    const bf16x8 qtf = read_tr_frag<HD>(sQ, 16 * cp, dcol, lane);
                    dvacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot, pf, dvacc[d], 0, 0, 0);
                    dkacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dkacc[d], 0, 0, 0);
                }
            }
        }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (key < Lk) {
        bf16_t* kp = dKp + ((long)b * Lk + key) * ldpk + (long)(H == Hkv ? hk : h) * HD;
        bf16_t* vp = dVp + ((long)b * Lk + key) * ldpv + (long)(H == Hkv ? hk : h) * HD;
#pragma unroll
        for (int d = 0; d < D::NDW; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int dd = (dh * D::NDW + d) * 32 + 8 * g4 + 4 * hh;
                if (dd < HD) {
                    u32x2 o, w;
                    o[0] = pack_bf2(dkacc[d][4 * g4] * scale, dkacc[d][4 * g4 + 1] * scale);
                    o[1] = pack_bf2(dkacc[d][4 * g4 + 2] * scale, dkacc[d][4 * g4 + 3] * scale);
                    w[0] = pack_bf2(dvacc[d][4 * g4], dvacc[d][4 * g4 + 1]);
                    w[1] = pack_bf2(dvacc[d][4 * g4 + 2], dvacc[d][4 * g4 + 3]);
                    *reinterpret_cast<u32x2*>(kp + dd) = o;
                    *reinterpret_cast<u32x2*>(vp + dd) = w;
                }
            }
    }
