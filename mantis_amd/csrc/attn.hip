// Fused softmax attention for gfx950 (flash-style, MFMA, online softmax in fp32) -- forward (ViT windows + Llama causal
// GQA with key-padding mask) and backward (Llama).
//
// Replaces (reference path): the attention call inside SiglipAttention / CLIPAttention / LlamaAttention
//   transformers/models/siglip/modeling_siglip.py:227-247,267-305 (non-causal, one window per image)
//   transformers/models/llama/modeling_llama.py:191-214,262-276 (causal + padding mask, GQA repeat_kv)
// reached from /root/reference/mantis/models/mllava/modeling_llava.py:456 and :510, where the reference calls the
// flash-attn CUDA extension (train_mllava.py:79-82) or the eager softmax.  Never materialises the LxL score matrix.
//
// Layout choices (CDNA4):
//  * scores are computed TRANSPOSED, S^T = K.Q^T via v_mfma_f32_32x32x16_bf16 with K rows as the A operand, so a lane owns ONE
//    query column (lane & 31) and 16 keys per 32-key block: the row max / row sum are in-lane reductions plus a single
//    lane <-> lane+32 exchange, and the rescale factor is lane-uniform.
//  * the P (or dS) accumulator registers feed the next MFMA's B operand DIRECTLY: the contraction order over keys is
//    permuted to match the accumulator layout (keys {4h+e+8c}), and the A operand follows the same permutation.
//  * operands whose contraction index is not their contiguous axis (V for P.V, K for dS.K, Q and dO for dK/dV) are read from
//    the SAME row-major LDS tile with ds_read_b64_tr_b16 (hardware transposing read: a 16-lane group fetches a 4x16 block and
//    lane t receives column t) -- no transposed copies in HBM or LDS.
//  * K/V (or Q/dO) tiles are double buffered in LDS: the next tile's global loads are issued into registers before the MFMA
//    work of the current tile and written to the other buffer afterwards (one barrier per tile).
//  * causal work is dispatched heaviest-first; the dK/dV kernel runs one workgroup per (key block, QUERY head) and a small
//    reduction sums the GQA group, so the grid is H/Hkv times larger than a per-kv-head walk.
// Algorithmic FLOPs: forward 4*L*Lk*hd per head (half for causal); backward 2.5x forward (+1x recompute of S and dP here).

#include "attn_common.h"

// ------------------------------------------------------------------------------------------------ forward
// grid (ceil(L/128), H, B); 4 waves x 32 query rows; KV tiles of 64 keys, double buffered.
// (Three workgroups per CU for the small head dims -- their 53.8 KB of LDS would allow it -- was measured: the 170-VGPR budget spills
// ~19 registers and the kernel gets SLOWER: hd 80 864 -> 1367 us, hd 72 162 -> 243 us, hd 96 206 -> 324 us; hd 64, no spills: equal.)
// Sliding window (WIN, causal only): query q sees keys q - W < key <= q, i.e. the per-query lower bound becomes
// lo(q) = max(kstart[q], q - W + 1) -- computed here, no bound array needed.  lo is non-decreasing in q like kstart, so the band is
// walked exactly like packed samples: the first tile is lo(first row), tiles below lo(last row of the wave) are the ones the far edge
// cuts (masked per element), tiles wholly below lo(first row of the wave) are skipped, the rest run unmasked.

template <int HD, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                       const bf16_t* __restrict__ V, const int* __restrict__ kmask,
                                                       bf16_t* __restrict__ O, float* __restrict__ LSE, int L, int Lk, int H, int Hkv,
                                                       long ldq, long ldk, long ldv, long ldo, float scale,
                                                       const int* __restrict__ kstart) {
    constexpr bool WIN = false;
    constexpr int W = 0;
#include "attn_fwd_body.inc"
}
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_fwd_win_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                           const bf16_t* __restrict__ V, const int* __restrict__ kmask,
                                                           bf16_t* __restrict__ O, float* __restrict__ LSE, int L, int Lk, int H, int Hkv,
                                                           long ldq, long ldk, long ldv, long ldo, float scale,
                                                           const int* __restrict__ kstart, int W) {
    constexpr bool CAUSAL = true, WIN = true;
#include "attn_fwd_body.inc"
}

// ------------------------------------------------------------------------------------------------ backward: D = rowsum(dO * O)
__global__ void attn_dsum_kernel(const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O, float* __restrict__ Dsum, long rows,
                                 int H, int HD, int L, long ldo) {
    // one wave per (token row, head); Dsum layout [B, H, L]
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows * H) return;
    const long row = w / H;
    const int h = (int)(w - row * H);
    float s = 0.f;
    for (int c = lane; c < HD / 8; c += 64) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(dO + row * ldo + (long)h * HD + c * 8);
        const u32x4 o = *reinterpret_cast<const u32x4*>(O + row * ldo + (long)h * HD + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += bf2f_lo(a[e]) * bf2f_lo(o[e]) + bf2f_hi(a[e]) * bf2f_hi(o[e]);
    }
    s = wave_sum(s);
    if (lane == 0) {
        const long b = row / L, l = row - b * L;
        Dsum[(b * H + h) * L + l] = s;
    }
}

// ------------------------------------------------------------------------------------------------ backward: dQ
// Same walk as the forward.  dQ^T[d][q] += K^T[d][key] . dS^T[key][q]  (K^T fragments: transposing reads of the K tile).
template <int HD, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                          const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
                                                          const int* __restrict__ kmask, const float* __restrict__ LSE,
                                                          float* __restrict__ Dsum, bf16_t* __restrict__ dQ, int L, int Lk, int H,
                                                          int Hkv, long ldq, long ldk, long ldv, long ldo, long lddq, float scale,
                                                          const bf16_t* __restrict__ Ofwd, long ldout,
                                                          const int* __restrict__ kstart) {
    constexpr bool WIN = false;
    constexpr int W = 0;
#include "attn_bwd_dq_body.inc"
}
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_win_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                              const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
                                                              const int* __restrict__ kmask, const float* __restrict__ LSE,
                                                              float* __restrict__ Dsum, bf16_t* __restrict__ dQ, int L, int Lk, int H,
                                                              int Hkv, long ldq, long ldk, long ldv, long ldo, long lddq, float scale,
                                                              const bf16_t* __restrict__ Ofwd, long ldout,
                                                              const int* __restrict__ kstart, int W) {
    constexpr bool CAUSAL = true, WIN = true;
#include "attn_bwd_dq_body.inc"
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// One workgroup per (key block, QUERY head, batch); GQA groups are summed afterwards.  A wave owns 32 keys and -- to keep the
// accumulators at 64 registers so that two waves fit per SIMD -- HALF of the head dimension when hd >= 64: waves (kg, dh)
// with the same key group kg recompute S and dP (cheap next to the exposed latency of 1 wave/SIMD) and each accumulates its
// own d-half of dK and dV.  Walks 32-row query tiles, double buffered.
//   S[q][key]  = Q . K^T      (lane owns ONE key column, 16 query rows per block)
//   dV^T[d][key] += dO^T[d][q] . P[q][key]        dK^T[d][key] += Q^T[d][q] . dS[q][key]
// dKp/dVp: per-QUERY-head outputs [B*L, H*hd] (row stride ldp), or the final dK/dV when H == Hkv.
template <int HD>
struct DkvCfg {
    static constexpr int DS = (AttnCfg<HD>::NDB >= 2 && AttnCfg<HD>::NDB % 2 == 0) ? 2 : 1;   // waves sharing a key group (d-split)
    static constexpr int NDW = AttnCfg<HD>::NDB / DS;          // 32-wide d-blocks per wave
    static constexpr int KEYS = (4 / DS) * 32;                 // keys per workgroup
};

// WIN: a key block is seen by the queries below min(qend, last key + W) only, and the per-row lower bound staged with each query tile
// is lo(q) = max(kstart[q], q - W + 1) (attn_fwd_body), so the masked passes are the diagonal ones plus those the far edge cuts.
template <int HD, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                              const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
                                                              const int* __restrict__ kmask, const float* __restrict__ LSE,
                                                              const float* __restrict__ Dsum, bf16_t* __restrict__ dKp,
                                                              bf16_t* __restrict__ dVp, int L, int Lk, int H, int Hkv, long ldq, long ldk,
                                                              long ldv, long ldo, long ldpk, long ldpv, float scale,
                                                              const int* __restrict__ kstart, const int* __restrict__ qend) {
    constexpr bool WIN = false;
    constexpr int W = 0;
#include "attn_bwd_dkv_body.inc"
}
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_win_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                  const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
                                                                  const int* __restrict__ kmask, const float* __restrict__ LSE,
                                                                  const float* __restrict__ Dsum, bf16_t* __restrict__ dKp,
                                                                  bf16_t* __restrict__ dVp, int L, int Lk, int H, int Hkv, long ldq,
                                                                  long ldk, long ldv, long ldo, long ldpk, long ldpv, float scale,
                                                                  const int* __restrict__ kstart, const int* __restrict__ qend, int W) {
    constexpr bool CAUSAL = true, WIN = true;
#include "attn_bwd_dkv_body.inc"
}

// dK[m, hk*hd + d] = sum_g dKp[m, (hk*G + g)*hd + d]  (and dV): fp32 sum of the G per-query-head partials, 16 B per lane
__global__ void attn_group_reduce_kernel(const bf16_t* __restrict__ pk, const bf16_t* __restrict__ pv, bf16_t* __restrict__ dK,
                                         bf16_t* __restrict__ dV, long rows, int Hkv, int G, int HD, long ldp, long lddk, long lddv) {
    const int cph = HD >> 3;
    const long total = rows * Hkv * cph;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cph);
        const long t = i / cph;
        const int hk = (int)(t % Hkv);
        const long r = t / Hkv;
        float ak[8], av[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { ak[e] = 0.f; av[e] = 0.f; }
        for (int g = 0; g < G; ++g) {
            const long off = r * ldp + (long)(hk * G + g) * HD + cc * 8;
            const u32x4 a = *reinterpret_cast<const u32x4*>(pk + off);
            const u32x4 w = *reinterpret_cast<const u32x4*>(pv + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ak[2 * e] += bf2f_lo(a[e]); ak[2 * e + 1] += bf2f_hi(a[e]);
                av[2 * e] += bf2f_lo(w[e]); av[2 * e + 1] += bf2f_hi(w[e]);
            }
        }
        u32x4 ok, ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ok[e] = pack_bf2(ak[2 * e], ak[2 * e + 1]); ov[e] = pack_bf2(av[2 * e], av[2 * e + 1]); }
        *reinterpret_cast<u32x4*>(dK + r * lddk + (long)hk * HD + cc * 8) = ok;
        *reinterpret_cast<u32x4*>(dV + r * lddv + (long)hk * HD + cc * 8) = ov;
    }
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV for GQA 4:1, hd 128
// One workgroup per (64-key block, KV head, batch); NO per-query-head partials in HBM, no group-reduce pass, S and dP computed once.
// Wave (kb, hp): kb = which 32 keys of the block, hp = which PAIR of the group's 4 query heads.  A wave owns its 32 keys over the
// FULL head dimension (dK and dV accumulators: 128 registers, K and V fragments: 64 registers -> one wave per SIMD, 512-register
// budget) and walks the 32-row query tiles of its two heads back to back as one stream; the two waves of a stream share the
// Q / dO tiles (LDS-DMA into a 3-stage ring, requested two tiles ahead, one barrier per tile).  The loop is software pipelined by
// hand: while the VALU turns tile i's S, dP into P and dS, the matrix pipe already computes S, dP of tile i+1.
//   MFMAs per (32 keys x 32 queries x head): S 8 + dP 8 + dV 8 + dK 8 = 32   (the per-query-head kernel above: 48, + the reduce)
// At the end the two streams' partial sums meet in LDS: wave hp = 0 finishes dK, wave hp = 1 finishes dV (fixed order: deterministic).
// Work per workgroup is at most (L/32 tiles x 4 heads x 2 key groups) / 4 waves, far below the per-CU average, so the causal
// imbalance is absorbed by the dispatch order (heaviest key block first) -- the reason the key block is 64 and not 128.
// Optional segment bounds for packed samples: kstart[b, q] = first key position query q may attend (its sample's start),
// qend[b, key] = one past the last query position that may attend key (its sample's end).
#ifdef DKV_STAMPS
// timing probe (tools/build_probe_lib.sh attn dkvstamps -DDKV_STAMPS; tools/attn_dkv_anatomy.py; never in the product build): wave 0 of every
// workgroup sums, over the steps of its software-pipelined loop, the s_memtime intervals step top -> DMA of tile j + 3 issued, first fragments
// requested -> MFMA 15 (S, dP of tile j + 2) -> MFMA 31 (dV, dK of tile j) -> behind the step's barrier; plus entry -> loop, entry -> exit.
// (s_memtime returns through lgkmcnt: every stamp also drains the LDS reads in flight -- read the PROPORTIONS.)
__device__ unsigned long long g_dkv_stamps[4096 * 8];
#define DKV_STAMP(var) do { var = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DKV_STAMP(var) do { } while (0)
#endif
// WIN (sliding window W, causal): the key block is seen by the query tiles from its diagonal up to min(qend, last key + W); of those, the two
// diagonal tiles and the tiles from the first one the far edge cuts, (kblk0 + W) / 32, are masked (key <= q - W -> p = 0, computed per
// element, no bound array), and the tiles between them -- wholly inside every key's window -- run on the pipelined loop.
template <bool CAUSAL, bool SEG>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv_g4_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const int* __restrict__ kmask, const int* __restrict__ kstart, const int* __restrict__ qend, const float* __restrict__ LSE,
    const float* __restrict__ Dsum, bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, int L, int H, int Hkv, long ldq, long ldk,
    long ldv, long ldo, long lddk, long lddv, float scale) {
    constexpr bool WIN = false;
    constexpr int W = 0;
#include "attn_bwd_dkv_g4_body.inc"
}
template <bool SEG>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv_g4_win_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, const bf16_t* __restrict__ dO,
    const int* __restrict__ kmask, const int* __restrict__ kstart, const int* __restrict__ qend, const float* __restrict__ LSE,
    const float* __restrict__ Dsum, bf16_t* __restrict__ dK, bf16_t* __restrict__ dV, int L, int H, int Hkv, long ldq, long ldk,
    long ldv, long ldo, long lddk, long lddv, float scale, int W) {
    constexpr bool CAUSAL = true, WIN = true;
#include "attn_bwd_dkv_g4_body.inc"
}

#ifdef DKV_STAMPS
// probe builds only: copy the stamps of the last attn_bwd_dkv_g4_kernel launch (n workgroups x 8 u64) to host memory
extern "C" int mantis_probe_dkv_stamps(void* host_dst, int n_wg) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_dkv_stamps), (size_t)n_wg * 64, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif

static int attn_num_cus() {
    static int cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        cached[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cached[dev];
}

// group sizes served by attn_bwd_dkv_g4_kernel: every even G, odd G from 5 on (one dummy head slot in G + 1: at most 1/6 wasted)
static inline bool attn_dkv_group_kernel_ok(int G) { return G >= 2 && (G % 2 == 0 || G >= 5); }

// attn_fwd64.hip: the hd-128 forward with 64 query rows per wave
int mantis_attn_fwd64_launch(bool causal, int B, hipStream_t s, const bf16_t* Q, const bf16_t* K, const bf16_t* V, const int* kmask,
                             bf16_t* O, float* LSE, int L, int Lk, int H, int Hkv, long ldq, long ldk, long ldv, long ldo, float scale,
                             const int* kstart, int window);

// The hd-128 forward runs on attn_fwd64_kernel (64 query rows per wave) from 1024 query rows on; MANTIS_ATTN_FWD64 = 0 (read once) keeps
// attn_fwd_kernel<128> for every length, = 1 forces attn_fwd64 for every length.  Same-box A/B, round 3, Llama-3 step geometry (B 2,
// L 2812, 32/8 heads): 197 vs 210 us without a key mask, 188 vs 215 us with one; Qwen2-7B geometry (L 4096, 28/4): 139 vs 176 us.
static int attn_fwd64_mode() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("MANTIS_ATTN_FWD64");
        v = (e && e[0] == '0') ? 0 : (e && e[0] == '1') ? 1 : 2;
    }
    return v;
}

template <int HD>
static int launch_fwd(bool causal, dim3 grid, hipStream_t s, const bf16_t* Q, const bf16_t* K, const bf16_t* V, const int* kmask,
                      bf16_t* O, float* LSE, int L, int Lk, int H, int Hkv, long ldq, long ldk, long ldv, long ldo, float scale,
                      const int* kstart, int window) {      // window: 0 = none, else the sliding window (causal, < L)
    if constexpr (HD == 128) {
        const int mode = attn_fwd64_mode();
        if ((mode == 1 || (mode == 2 && L >= 1024)) && Lk <= 65536)      // the kernel's per-tile liveness table holds 1024 tiles
            return mantis_attn_fwd64_launch(causal, (int)(grid.x / (cdiv(L, 128) * H)), s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk,
                                            ldv, ldo, scale, kstart, window);
    }
    if (window > 0) {
        MANTIS_LAUNCH((attn_fwd_win_kernel<HD>), grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, scale,
                      kstart, window);
        return mantis_check_launch();
    }
    if (causal)
        MANTIS_LAUNCH((attn_fwd_kernel<HD, true>), grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv,
                           ldo, scale, kstart);
    else
        MANTIS_LAUNCH((attn_fwd_kernel<HD, false>), grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv,
                           ldo, scale, kstart);
    return mantis_check_launch();
}

// (round 6: the opt-in 64-query-rows-per-wave dQ kernel of rounds 4 - 5, csrc/attn_dq64.hip, is gone: correct, but 266 vs 233 us against this
// file's attn_bwd_dq_kernel in every measurement of two rounds -- a 512-register kernel runs one workgroup per CU and nothing overlaps its
// prologue, profiles/r05_attn_anatomy.md -- and a kernel off the default path earns nothing.)
template <int HD>
static void launch_dq(bool causal, hipStream_t s, const bf16_t* Q, const bf16_t* K, const bf16_t* V, const bf16_t* dO, const int* kmask,
                      const float* LSE, float* Dsum, bf16_t* dQ, int B, int L, int Lk, int H, int Hkv, long ldq, long ldk, long ldv,
                      long ldo, long lddq, float scale, const bf16_t* Ofwd, long ldout, const int* kstart, int window) {
    const dim3 gq(cdiv(L, 128) * H * B);
    if (window > 0)
        MANTIS_LAUNCH((attn_bwd_dq_win_kernel<HD>), gq, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, dQ, L, Lk, H, Hkv, ldq, ldk, ldv,
                      ldo, lddq, scale, Ofwd, ldout, kstart, window);
    else if (causal)
        MANTIS_LAUNCH((attn_bwd_dq_kernel<HD, true>), gq, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, dQ, L, Lk, H, Hkv, ldq, ldk, ldv,
                           ldo, lddq, scale, Ofwd, ldout, kstart);
    else
        MANTIS_LAUNCH((attn_bwd_dq_kernel<HD, false>), gq, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, dQ, L, Lk, H, Hkv, ldq, ldk, ldv,
                           ldo, lddq, scale, Ofwd, ldout, kstart);
}

template <int HD>
static int launch_bwd(bool causal, hipStream_t s, const bf16_t* Q, const bf16_t* K, const bf16_t* V, const bf16_t* dO,
                      const int* kmask, const float* LSE, float* Dsum, bf16_t* dQ, bf16_t* dK, bf16_t* dV, bf16_t* ws, int B,
                      int L, int Lk, int H, int Hkv, long ldq, long ldk, long ldv, long ldo, long lddq, long lddk, long lddv, float scale,
                      const bf16_t* Ofwd, long ldout, const int* kstart, const int* qend, int window) {
    const dim3 gk(cdiv(Lk, DkvCfg<HD>::KEYS) * H * B);       // Lk keys per batch entry
    const int G = H / Hkv;
    if constexpr (HD == 128) {
        // GQA-aware dK/dV (no HBM partials, no group reduce); dQ as before (it also publishes Dsum).  Its grid is one workgroup per
        // (64-key block, KV head) with causal work that varies 64x across key blocks: below about two workgroups per CU the heaviest
        // block sets the time (Qwen2-7B at B = 1, L = 4096: 256 workgroups, 553 us vs 490 us for the per-query-head path, measured), so
        // other group sizes than Llama's take it only when the grid is either tiny or at least two rounds deep
        const long nwg = (long)cdiv(L, 64) * Hkv * B;
        const int cus = attn_num_cus();
        if (Lk == L && attn_dkv_group_kernel_ok(G) && (G == 4 || nwg >= 2L * cus || nwg <= cus / 2 || ws == nullptr)) {
            launch_dq<HD>(causal, s, Q, K, V, dO, kmask, LSE, Dsum, dQ, B, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, lddq, scale, Ofwd, ldout, kstart,
                          window);
            const dim3 g4(cdiv(L, 64) * Hkv * B);
#define DKV_G4(C_, S_) MANTIS_LAUNCH((attn_bwd_dkv_g4_kernel<C_, S_>), g4, dim3(256), 0, s, Q, K, V, dO, kmask, kstart, qend, LSE, \
                                          Dsum, dK, dV, L, H, Hkv, ldq, ldk, ldv, ldo, lddk, lddv, scale)
#define DKV_G4W(S_) MANTIS_LAUNCH((attn_bwd_dkv_g4_win_kernel<S_>), g4, dim3(256), 0, s, Q, K, V, dO, kmask, kstart, qend, LSE, \
                                       Dsum, dK, dV, L, H, Hkv, ldq, ldk, ldv, ldo, lddk, lddv, scale, window)
            if (window > 0) { if (kstart) DKV_G4W(true); else DKV_G4W(false); }
            else if (causal) { if (kstart) DKV_G4(true, true); else DKV_G4(true, false); }
            else { if (kstart) DKV_G4(false, true); else DKV_G4(false, false); }
#undef DKV_G4W
#undef DKV_G4
            return mantis_check_launch();
        }
    }
    if (G > 1 && ws == nullptr) return MANTIS_EINVAL;
    const long rows = (long)B * Lk;
    bf16_t* pk = G == 1 ? dK : ws;
    bf16_t* pv = G == 1 ? dV : ws + rows * H * HD;
    const long ldpk = G == 1 ? lddk : (long)H * HD, ldpv = G == 1 ? lddv : (long)H * HD;
    launch_dq<HD>(causal, s, Q, K, V, dO, kmask, LSE, Dsum, dQ, B, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, lddq, scale, Ofwd, ldout, kstart,
                  window);
    if (window > 0) {
        MANTIS_LAUNCH((attn_bwd_dkv_win_kernel<HD>), gk, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, pk, pv, L, Lk, H, Hkv,
                      ldq, ldk, ldv, ldo, ldpk, ldpv, scale, kstart, qend, window);
    } else if (causal) {
        MANTIS_LAUNCH((attn_bwd_dkv_kernel<HD, true>), gk, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, pk, pv, L, Lk, H, Hkv,
                           ldq, ldk, ldv, ldo, ldpk, ldpv, scale, kstart, qend);
    } else {
        MANTIS_LAUNCH((attn_bwd_dkv_kernel<HD, false>), gk, dim3(256), 0, s, Q, K, V, dO, kmask, LSE, Dsum, pk, pv, L, Lk, H, Hkv,
                           ldq, ldk, ldv, ldo, ldpk, ldpv, scale, kstart, qend);
    }
    if (G > 1) {
        const long total = rows * Hkv * (HD / 8);
        long g = (total + 255) / 256;
        g = g > 2048 ? 2048 : g;
        MANTIS_LAUNCH(attn_group_reduce_kernel, dim3((int)g), dim3(256), 0, s, pk, pv, dK, dV, rows, Hkv, G, HD, (long)H * HD,
                           lddk, lddv);
    }
    return mantis_check_launch();
}

extern "C" {

// Q [B,L,H,hd] (row stride ldq), K,V [B,L,Hkv,hd] (ldk, ldv), kmask int32[B,L] or NULL, O [B,L,H,hd] (ldo),
// LSE fp32 [B,H,L] or NULL.  hd in {16, 64, 72, 96, 128} (96: the Idefics2 perceiver resampler).
static int attn_fwd_impl(const void* Q, const void* K, const void* V, const int32_t* kmask, const int32_t* kstart, void* O, float* LSE,
                         int B, int L, int Lk, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale,
                         int causal, int window, void* stream);

int mantis_attn_fwd(const void* Q, const void* K, const void* V, const int32_t* kmask, const int32_t* kstart, void* O, float* LSE,
                    int B, int L, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, int causal,
                    void* stream) {
    return attn_fwd_impl(Q, K, V, kmask, kstart, O, LSE, B, L, L, H, Hkv, hd, ldq, ldk, ldv, ldo, scale, causal, 0, stream);
}

// Sliding-window causal attention (Mistral): query q attends key k iff q - window < k <= q (and the key mask / kstart allow it).
// window >= L is plain causal attention and takes mantis_attn_fwd's kernels (same bits); kstart optional as there.
int mantis_attn_fwd_window(const void* Q, const void* K, const void* V, const int32_t* kmask, const int32_t* kstart, void* O, float* LSE,
                           int B, int L, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale,
                           int causal, int window, void* stream) {
    if (window <= 0) return MANTIS_EINVAL;
    if (!causal) return MANTIS_EUNSUPPORTED;
    return attn_fwd_impl(Q, K, V, kmask, kstart, O, LSE, B, L, L, H, Hkv, hd, ldq, ldk, ldv, ldo, scale, causal, window < L ? window : 0,
                         stream);
}

// Cross attention: Lq query rows per batch entry (Q, O: [B*Lq, ...], LSE [B, H, Lq]) over Lk keys (K, V: [B*Lk, ...], kmask int32 [B, Lk]
// or NULL), non-causal.  The Idefics2 perceiver resampler's attention of 64 latent queries over concat[context, latents]
// (/root/reference/mantis/models/idefics2/modeling_idefics2.py:812-912).
int mantis_attn_fwd_cross(const void* Q, const void* K, const void* V, const int32_t* kmask, void* O, float* LSE, int B, int Lq, int Lk,
                          int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, void* stream) {
    if (Lk <= 0) return MANTIS_EINVAL;
    return attn_fwd_impl(Q, K, V, kmask, nullptr, O, LSE, B, Lq, Lk, H, Hkv, hd, ldq, ldk, ldv, ldo, scale, 0, 0, stream);
}

static int attn_fwd_impl(const void* Q, const void* K, const void* V, const int32_t* kmask, const int32_t* kstart, void* O, float* LSE,
                         int B, int L, int Lk, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale,
                         int causal, int window, void* stream) {
    if (B <= 0 || L <= 0 || H <= 0 || Hkv <= 0 || H % Hkv) return MANTIS_EINVAL;
    if (causal && Lk != L) return MANTIS_EINVAL;
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4) return MANTIS_EUNSUPPORTED;
    if (kstart != nullptr && !causal) return MANTIS_EUNSUPPORTED;     // a lower key bound alone is a block-diagonal mask only under causality
    const dim3 grid(cdiv(L, 128) * H * B);
    hipStream_t s = (hipStream_t)stream;
#define FWD(HD) return launch_fwd<HD>(causal != 0, grid, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, kmask, \
                                      (bf16_t*)O, LSE, L, Lk, H, Hkv, (long)ldq, (long)ldk, (long)ldv, (long)ldo, scale, kstart, \
                                      window)
    switch (hd) {
        case 16: FWD(16);
        case 64: FWD(64);
        case 72: FWD(72);
        case 80: FWD(80);
        case 96: FWD(96);
        case 128: FWD(128);
        default: return MANTIS_EUNSUPPORTED;
    }
#undef FWD
}

// 1 if mantis_attn_bwd needs the 2 * B*L*H*hd bf16 workspace for this geometry (per-query-head dK/dV partials), 0 if not
// 0: never needed (MHA; GQA 4:1 at hd 128 always runs the group kernel).  1: pass a workspace (other group sizes choose between the
// group kernel and the per-query-head path by grid size; without a workspace they are held to the group kernel where it exists).
int mantis_attn_bwd_needs_workspace(int H, int Hkv, int hd) { return (H == Hkv || (hd == 128 && H == 4 * Hkv)) ? 0 : 1; }

// Dsum [B,H,L] = rowsum(dO * O)
int mantis_attn_dsum(const void* dO, const void* O, float* Dsum, int B, int L, int H, int hd, int64_t ldo, void* stream) {
    if (hd % 8 || ldo % 8) return MANTIS_EUNSUPPORTED;
    const long rows = (long)B * L;
    MANTIS_LAUNCH(attn_dsum_kernel, dim3(cdiv(rows * H, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dO,
                       (const bf16_t*)O, Dsum, rows, H, hd, L, (long)ldo);
    return mantis_check_launch();
}

// dQ/dK/dV written with row strides lddq/lddk/lddv (head h at column h*hd).  workspace: 2 * B*L*H*hd bf16 when H > Hkv
// (per-query-head dK/dV partials, summed over the GQA group afterwards); unused when H == Hkv and on the GQA-aware path
// (hd 128, H = 4 Hkv; see mantis_attn_bwd_workspace_bytes).  kstart / qend (both or neither): segment bounds of packed samples.
// O (optional): the forward output [B*L, H*hd] (row stride ld_out).  If given, D = rowsum(dO * O) is computed inside the dQ kernel and
// written to Dsum (then a [B,H,L] fp32 scratch/output); if NULL, Dsum must hold it already (mantis_attn_dsum).
static int attn_bwd_impl(const void* Q, const void* K, const void* V, const void* O, const void* dO, const int32_t* kmask,
                         const int32_t* kstart, const int32_t* qend, const float* LSE, float* Dsum, void* dQ, void* dK, void* dV,
                         void* workspace, int B, int L, int Lk, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv,
                         int64_t ld_out, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int causal, int window,
                         void* stream);

int mantis_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const int32_t* kmask,
                    const int32_t* kstart, const int32_t* qend, const float* LSE, float* Dsum, void* dQ, void* dK, void* dV,
                    void* workspace, int B, int L, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ld_out,
                    int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int causal, void* stream) {
    return attn_bwd_impl(Q, K, V, O, dO, kmask, kstart, qend, LSE, Dsum, dQ, dK, dV, workspace, B, L, L, H, Hkv, hd, ldq, ldk, ldv, ld_out,
                         ldo, lddq, lddk, lddv, scale, causal, 0, stream);
}

// Backward of mantis_attn_fwd_window (same window; window >= L: mantis_attn_bwd's kernels, same bits).  Workspace as mantis_attn_bwd.
int mantis_attn_bwd_window(const void* Q, const void* K, const void* V, const void* O, const void* dO, const int32_t* kmask,
                           const int32_t* kstart, const int32_t* qend, const float* LSE, float* Dsum, void* dQ, void* dK, void* dV,
                           void* workspace, int B, int L, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ld_out,
                           int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int causal, int window, void* stream) {
    if (window <= 0) return MANTIS_EINVAL;
    if (!causal) return MANTIS_EUNSUPPORTED;
    return attn_bwd_impl(Q, K, V, O, dO, kmask, kstart, qend, LSE, Dsum, dQ, dK, dV, workspace, B, L, L, H, Hkv, hd, ldq, ldk, ldv, ld_out,
                         ldo, lddq, lddk, lddv, scale, causal, window < L ? window : 0, stream);
}

// Backward of mantis_attn_fwd_cross: dQ [B*Lq, H*hd], dK / dV [B*Lk, Hkv*hd]; Dsum fp32 [B, H, Lq] scratch; workspace 2 * B*Lk*H*hd bf16
// when H > Hkv (per-query-head dK/dV partials, summed over the GQA group afterwards).
int mantis_attn_bwd_cross(const void* Q, const void* K, const void* V, const void* O, const void* dO, const int32_t* kmask,
                          const float* LSE, float* Dsum, void* dQ, void* dK, void* dV, void* workspace, int B, int Lq, int Lk, int H,
                          int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ld_out, int64_t ldo, int64_t lddq,
                          int64_t lddk, int64_t lddv, float scale, void* stream) {
    if (Lk <= 0 || !O) return MANTIS_EINVAL;
    return attn_bwd_impl(Q, K, V, O, dO, kmask, nullptr, nullptr, LSE, Dsum, dQ, dK, dV, workspace, B, Lq, Lk, H, Hkv, hd, ldq, ldk, ldv,
                         ld_out, ldo, lddq, lddk, lddv, scale, 0, 0, stream);
}

static int attn_bwd_impl(const void* Q, const void* K, const void* V, const void* O, const void* dO, const int32_t* kmask,
                         const int32_t* kstart, const int32_t* qend, const float* LSE, float* Dsum, void* dQ, void* dK, void* dV,
                         void* workspace, int B, int L, int Lk, int H, int Hkv, int hd, int64_t ldq, int64_t ldk, int64_t ldv,
                         int64_t ld_out, int64_t ldo, int64_t lddq, int64_t lddk, int64_t lddv, float scale, int causal, int window,
                         void* stream) {
    if (B <= 0 || L <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || !Dsum) return MANTIS_EINVAL;
    if (causal && Lk != L) return MANTIS_EINVAL;
    if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || lddq % 4 || lddk % 8 || lddv % 8 || (O && ld_out % 8)) return MANTIS_EUNSUPPORTED;
    if ((kstart == nullptr) != (qend == nullptr)) return MANTIS_EINVAL;
    if (kstart != nullptr && !causal) return MANTIS_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
#define BWD(HD) return launch_bwd<HD>(causal != 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, (const bf16_t*)dO, \
                                      kmask, LSE, Dsum, (bf16_t*)dQ, (bf16_t*)dK, (bf16_t*)dV, (bf16_t*)workspace, B, L, Lk, H, Hkv, \
                                      (long)ldq, (long)ldk, (long)ldv, (long)ldo, (long)lddq, (long)lddk, (long)lddv, scale, \
                                      (const bf16_t*)O, (long)ld_out, kstart, qend, window)
    switch (hd) {
        case 16: BWD(16);
        case 64: BWD(64);
        case 96: BWD(96);
        case 128: BWD(128);
        default: return MANTIS_EUNSUPPORTED;
    }
#undef BWD
}

}  // extern "C"
