// Attention forward for hd = 128 with 64 query rows per wave (gfx950) -- the software-pipelined sibling of attn_fwd_kernel<128>
// (attn.hip), same entry point (mantis_attn_fwd / mantis_attn_fwd_cross), same masks, same output and LSE definition.
//
// Replaces (reference path): the LlamaAttention / Qwen2 attention call of the decoder forward,
//   transformers/models/llama/modeling_llama.py:191-214,262-276, reached from /root/reference/mantis/models/mllava/modeling_llava.py:456,510.
//
// Why a second kernel.  The 32-rows-per-wave forward issues ~7 non-MFMA instructions per MFMA where ~5 fit an MFMA's 32-cycle shadow,
// and leaves the overlap of one wave's softmax with the other wave's MFMAs to the arbiter of two waves per SIMD (round-2 PMC: MFMA pipe
// 27 % busy).  Here a workgroup is 4 waves = ONE per SIMD with the whole 512-register file, each wave owns 64 query rows as two 32-row
// blocks A and B, and ONE instruction stream interleaves the blocks by hand:
//   * every K fragment (ds_read_b128) and every V^T fragment (two transposing reads) feeds TWO MFMAs;
//   * the accumulator file holds what only MFMAs touch -- O (128 registers), the Q fragments (64), the K fragments (64, read from LDS
//     straight into AGPRs) -- and the arch VGPRs hold the scores, V^T fragments, P fragments and the softmax;
//   * per KV tile of 64 keys the stream is four phases of 16 MFMAs
//         Ph1  S_A(t)   = K(t).Q_A^T            Ph2  O_B += V(t-1)^T.P_B(t-1)
//         Ph3  S_B(t)   = K(t).Q_B^T            Ph4  O_A += V(t)^T.P_A(t)
//     so that each block's softmax has two phases of the OTHER block's MFMAs to hide in (A: Ph2-Ph3, B: Ph4-Ph1 of the next tile); the
//     fillers are dealt out per MFMA gap: one score element (fma, exp2, add, half a cvt_pk, half a max3) + the LDS fragment reads + the
//     LDS-DMA issues.  Measured (tools/mfma_filler_probe.hip): a gap hides ~28 cycles of issue -- VALU 4, v_exp 8, LDS read 8, DMA
//     piece ~54 -- so at hd 128 this loop is ISSUE-bound (~2500 cycles of issue per 2048 cycles of MFMA), not MFMA-bound;
//   * no max pass: the exps run against the row's CURRENT reference max m; the tile's largest exponent is collected on the side and
//     checked once per block and tile; only when a row exceeds m by more than 8 (exp2 domain: P <= 256, exact in fp32 / bf16 relative
//     precision) is the tile redone against a raised m and O / l rescaled (the scores stay intact for that).  Rare -- the first live
//     tile of a row, then almost never -- which it has to be: rescaling an AGPR-resident O costs 3 instructions per element;
//   * masks (key padding, causal diagonal, packed-sample start) are a pre-pass over the scores on the tiles that need one, so the
//     common stream is branch-free arithmetic; tiles with no live key for the wave (beyond its diagonal, all padding, before its
//     sample) skip the compute and only keep the workgroup's barrier / DMA protocol.
// LDS: K ring 4 x 16 KiB + V ring 4 x 16 KiB, filled by buffer_load ... lds through a per-tile descriptor (rows past Lk read as zeros),
// one barrier per tile: barrier(t) sits before Ph2(t); V(t) and K(t+1) must have landed before it (a COUNTED vmcnt: the two younger
// tiles' 16 pieces stay in flight), V(t+3) and K(t+4) are issued after it -- one workgroup per CU has nobody to hide an HBM round trip
// behind, so the ring runs 2.3 tiles (~5000 cycles) ahead.  Plus 8 KiB of per-tile key-liveness words (ballots of the padding mask),
// built once in the prologue so that the tile loop has no global load of its own.
#include "attn_common.h"

namespace {

constexpr int HD = 128;
constexpr int TILE = 64 * 256;                 // 64 keys x 256 B
constexpr int NS = 4;                          // ring slots per operand: a tile's DMA is issued NS - 2 (+ a bit) tiles before its barrier
constexpr int OFF_K = 0, OFF_V = NS * TILE;    // K ring, V ring
constexpr int OFF_BITS = 2 * NS * TILE;        // per-tile key-liveness words (8 B each)
constexpr int MAX_TILES = 1024;                // of one workgroup's key range (65536 keys); longer ranges take attn_fwd_kernel
constexpr float LAZY_TH = 8.0f;                // exp2-domain slack of the running max

typedef __attribute__((address_space(3))) void lds_void;

// ---- the accumulator file is owned by the asm statements below, by NUMBER (the compiler allocates no AGPR in this kernel: audit the
// build for v_accvgpr_* / scratch_* outside ASMSTART..ASMEND -- tools/attn_fwd64_audit.py):
//     a[  0: 63]  O^T of block A, d-block d at 16 d          a[128:159]  Q fragments of block A, hd chunk ks at 4 ks
//     a[ 64:127]  O^T of block B                             a[160:191]  Q fragments of block B
//     a[192:255]  K fragments of the current tile, fragment i = (key block) * 8 + (hd chunk) at 4 i
constexpr int AO = 0, AQ = 128, AK = 192;
// ... and so are the arch VGPRs v[192:255]: the 16 V^T fragments (fragment j = (key chunk of 16) * 4 + (d-block) at 192 + 4 j).  Left to
// the register allocator, the two 64-bit halves of a fragment (two transposing reads) become separate values that are copied into a
// 128-bit tuple -- or spilled to the accumulator file the moment they are "defined", before the LDS data has arrived.  Every statement
// that touches them lists all 64 as clobbers, so the compiler keeps nothing of its own there inside the loop.
constexpr int VF = 192;
#define VF_ALL                                                                                                                    \
    "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207",   \
    "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223",   \
    "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",   \
    "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
#define AGPR_ALL                                                                                                                  \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19",  \
    "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37",       \
    "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55",       \
    "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73",       \
    "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91",       \
    "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108",    \
    "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124",    \
    "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140",    \
    "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156",    \
    "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172",    \
    "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188",    \
    "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204",    \
    "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220",    \
    "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236",    \
    "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252",    \
    "a253", "a254", "a255"

// Timing probes (wrong results; tools/build_probe_lib.sh): FWD64_PROBE_TIMING (s_memtime stamps into the LSE buffer), FWD64_PROBE_NO_VMWAIT (no wait for the ring), FWD64_PROBE_NO_EXP (no
// exp / sum / pack fillers), FWD64_PROBE_NO_DMA (no ring refill in the loop), FWD64_PROBE_NO_LDS (no fragment reads), FWD64_PROBE_NO_MAX, FWD64_PROBE_NO_BARRIER
// ---- instruction helpers (the compiler counts and schedules none of these; see the wait / hazard notes at the call sites)
template <int KF, int QF>     // scores, C = 0: S^T(key block) = K fragment KF . Q fragment QF
__device__ __forceinline__ void mfma_s0(f32x16& d) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, a[%1:%2], a[%3:%4], 0" : "=v"(d) : "n"(AK + 4 * KF), "n"(AK + 4 * KF + 3), "n"(AQ + 4 * QF), "n"(AQ + 4 * QF + 3));
}
template <int KF, int QF>
__device__ __forceinline__ void mfma_s(f32x16& d) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, a[%1:%2], a[%3:%4], %0" : "+v"(d) : "n"(AK + 4 * KF), "n"(AK + 4 * KF + 3), "n"(AQ + 4 * QF), "n"(AQ + 4 * QF + 3));
}
template <int OB, int J>      // O^T(d-block at a[OB : OB + 15]) += V^T fragment J . P fragment
__device__ __forceinline__ void mfma_o(const u32x4& p) {
    asm volatile("v_mfma_f32_32x32x16_bf16 a[%0:%1], v[%2:%3], %4, a[%0:%1]"
                 :
                 : "n"(OB), "n"(OB + 15), "n"(VF + 4 * J), "n"(VF + 4 * J + 3), "v"(p)
                 : VF_ALL);
}
template <int KF, int OFF>
__device__ __forceinline__ void lds_read_k(unsigned addr) {                                 // K fragment KF -> its AGPRs
#ifdef FWD64_PROBE_NO_LDS
    return;
#endif
    asm volatile("ds_read_b128 a[%0:%1], %2 offset:%3" : : "n"(AK + 4 * KF), "n"(AK + 4 * KF + 3), "v"(addr), "i"(OFF));
}
template <int J, int OFF>
__device__ __forceinline__ void lds_read_vt(unsigned addr, unsigned addr8) {                // V^T fragment J: two transposing reads
#ifdef FWD64_PROBE_NO_LDS
    return;
#endif
    asm volatile("ds_read_b64_tr_b16 v[%0:%1], %4 offset:%6\n\tds_read_b64_tr_b16 v[%2:%3], %5 offset:%6"
                 :
                 : "n"(VF + 4 * J), "n"(VF + 4 * J + 1), "n"(VF + 4 * J + 2), "n"(VF + 4 * J + 3), "v"(addr), "v"(addr8), "i"(OFF)
                 : VF_ALL);
}
template <int R>
__device__ __forceinline__ void vf_zero4() {
    asm volatile("v_mov_b32 v[%0], 0\n\tv_mov_b32 v[%1], 0\n\tv_mov_b32 v[%2], 0\n\tv_mov_b32 v[%3], 0"
                 :
                 : "n"(R), "n"(R + 1), "n"(R + 2), "n"(R + 3)
                 : VF_ALL);
}
template <int R>
__device__ __forceinline__ void agpr_write(unsigned v) {
    asm volatile("v_accvgpr_write_b32 a[%0], %1" : : "n"(R), "v"(v));
}
template <int R>
__device__ __forceinline__ float agpr_read() {
    float v;
    asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(v) : "n"(R));
    return v;
}
template <int R>              // a[R .. R+3] *= f
__device__ __forceinline__ void agpr_scale4(float f) {
    float t0, t1, t2, t3;
    asm volatile(
        "v_accvgpr_read_b32 %0, a[%5]\n\tv_accvgpr_read_b32 %1, a[%6]\n\tv_accvgpr_read_b32 %2, a[%7]\n\tv_accvgpr_read_b32 %3, a[%8]\n\t"
        "v_mul_f32 %0, %0, %4\n\tv_mul_f32 %1, %1, %4\n\tv_mul_f32 %2, %2, %4\n\tv_mul_f32 %3, %3, %4\n\t"
        "v_accvgpr_write_b32 a[%5], %0\n\tv_accvgpr_write_b32 a[%6], %1\n\tv_accvgpr_write_b32 a[%7], %2\n\tv_accvgpr_write_b32 a[%8], %3"
        : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
        : "v"(f), "n"(R), "n"(R + 1), "n"(R + 2), "n"(R + 3));
}
__device__ __forceinline__ float max3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ float max2(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// max over the lane pair (l, l ^ 32): the two lanes that share a query row
__device__ __forceinline__ float pair_max(float v) {
    float a = v, b = v;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));       // VALU write -> permlane read -> VALU read
    return max2(a, b);
}

#define WIN_P(sm, I) (((I) % 3) == 0 ? (sm).pw0 : ((I) % 3) == 1 ? (sm).pw1 : (sm).pw2)
#define WIN_T(sm, I) (((I) % 3) == 0 ? (sm).tw0 : ((I) % 3) == 1 ? (sm).tw1 : (sm).tw2)

struct Softmax {          // per 32-row block, per lane (one query row per lane pair)
    float m;              // reference max of the exponent (exp2 domain): P = exp2(S c - m); -inf until the row's first live key
    float negm;           // -m, 0 while m = -inf
    float th;             // a tile whose largest exponent S c - m exceeds th raises m: LAZY_TH, -inf while m = -inf (any live key sets m)
    float l;              // this lane's share of the running sum
    // P and exponent of the last three elements (the sum, the bf16 pair and the max trail the exp by one element).  Scalars, and no two
    // P words adjacent: an indexed member, or a pair that can be fetched as one <2 x float>, keeps the struct in memory (which the
    // backend then "promotes" to LDS)
    float pw0;
    float l0;             // l before the current tile (for the fix-up)
    float pw1;
    float tm;             // largest exponent of the current tile so far
    float pw2;
    float tw0, tw1, tw2;
};

}  // namespace

// one 64-row block of one (batch, head).  WIN (sliding window W, causal): each row's lower key bound is lo(q) = max(kstart[q], q - W + 1),
// computed here; the sample-start machinery below then walks the band -- first tile lo(first row of the block), tiles wholly below every
// row's bound inactive, tiles below some row's bound through the masking pre-pass, the rest on the plain stream.
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn_fwd64_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                            const bf16_t* __restrict__ V, const int* __restrict__ kmask,
                                                            bf16_t* __restrict__ O, float* __restrict__ LSE, int L, int Lk, int H,
                                                            int Hkv, long ldq, long ldk, long ldv, long ldo, float scale,
                                                            const int* __restrict__ kstart) {
    constexpr bool WIN = false;
    constexpr int W = 0;
#include "attn_fwd64_body.inc"
}
__global__ __launch_bounds__(256, 1) void attn_fwd64_win_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                const bf16_t* __restrict__ V, const int* __restrict__ kmask,
                                                                bf16_t* __restrict__ O, float* __restrict__ LSE, int L, int Lk, int H,
                                                                int Hkv, long ldq, long ldk, long ldv, long ldo, float scale,
                                                                const int* __restrict__ kstart, int W) {
    constexpr bool CAUSAL = true, WIN = true;
#include "attn_fwd64_body.inc"
}

int mantis_attn_fwd64_launch(bool causal, int B, hipStream_t s, const bf16_t* Q, const bf16_t* K, const bf16_t* V, const int* kmask,
                             bf16_t* O, float* LSE, int L, int Lk, int H, int Hkv, long ldq, long ldk, long ldv, long ldo, float scale,
                             const int* kstart, int window) {
    const dim3 grid(cdiv(L, 256) * H * B);
    if (window > 0)
        MANTIS_LAUNCH(attn_fwd64_win_kernel, grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, scale,
                      kstart, window);
    else if (causal)
        MANTIS_LAUNCH((attn_fwd64_kernel<true>), grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, scale,
                      kstart);
    else
        MANTIS_LAUNCH((attn_fwd64_kernel<false>), grid, dim3(256), 0, s, Q, K, V, kmask, O, LSE, L, Lk, H, Hkv, ldq, ldk, ldv, ldo, scale,
                      kstart);
    return mantis_check_launch();
}
