// Launch planning of the bf16 GEMMs (gemm.hip, gemm176.hip): every decision a launch takes before it reaches a kernel -- operand checks, tile
// variant, K split of the incomplete last round, balanced remainder round, 176-row tile, paired dW, workspace -- each stated ONCE.  Host
// arithmetic only: no HIP include, no HIP call; the device's CU count is an argument (gemm.hip asks the runtime).  Compiles with a plain C++17
// compiler (tools/gemm_plan_dump.cpp; tests/test_gemm_plan.py holds every decision to tests/golden/gemm_plan.json) and inside gemm.hip, whose
// kernels share SkPlan, sk_bound and the SK_* constants.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define PLAN_HD __host__ __device__ __forceinline__
#else
#define PLAN_HD static inline
#endif
#include "gemm_flags.h"                     // BK, the EPI_* flag bits of the C-ABI, PAIR_*, return codes

#define SK_SLAB_FLOATS (256 * 256)
#define SK_MAX_ROUNDS 1                      // sub-rounds the remainder tiles' K parts may run as (workspace = SK_MAX_ROUNDS * #CU slabs)
#define SK_MINSEG 4
#define SK_BALANCED_MIN_STEPS 16            // ranges shorter than this: the equal split (its parts are >= 8 steps)
#define SK_BALANCED_MIN_GAIN 24             // K-steps per CU the balanced round must save over the equal split to be chosen
#define SK_EMPTY 0xFFFFu
struct SkPlan {                             // the balanced remainder round, see gemm_nt_ring16_kernel
    int units;                              // 0: equal split (S parts per tile, slab rt * S + part)
    int nspan;                              // slots of the tail region (a multiple of 8)
    unsigned short span[256];               // slot i (XCD i % 8): the range whose second segment runs there, or SK_EMPTY
};
// first step of range c (0 .. units) in the remainder's step sequence; T = rem * nk
// (32-bit on purpose: c <= 256 and T < 2^23, see sk_make_plan -- a 64-bit division is ~300 scalar instructions in a workgroup's prologue)
PLAN_HD int sk_bound(int c, int units, int T, int nk) {
    unsigned a = (unsigned)c * (unsigned)T / (unsigned)units;
    const unsigned r = a % (unsigned)nk;
    if (r < SK_MINSEG) a -= r;
    else if ((unsigned)nk - r < SK_MINSEG) a += (unsigned)nk - r;
    return (int)a;
}

static inline int plan_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline long tiles256(int M, int N) { return (long)plan_cdiv(M, 256) * plan_cdiv(N, 256); }

// ---- the process' configuration constants: read from the environment on first use, never written afterwards; no launch reads the environment
struct GemmEnv {
    int cus;            // MANTIS_GEMM_CUS: default CU budget (0 = the whole device)
    int split_max;      // MANTIS_GEMM_SPLIT_MAX: cap on the K split S (default 8; measurements)
    bool sk_balanced;   // MANTIS_GEMM_SK_BALANCED: 0 = equal split only
    bool sk_finish;     // MANTIS_GEMM_SK_FINISH: 0 = the round-4 in-kernel reduction by the last arriver (A/B measurements)
    int r176;           // MANTIS_GEMM_176: 0 = never, 1 = where the planner predicts a gain (default), 2 = wherever the kernel applies
    int ring;           // MANTIS_GEMM_RING: 12 / 13 / 14 = the ring kernel the automatic choice takes (A/B measurements); 0 = ring_variant_for()
    int pair;           // MANTIS_GEMM_PAIR: paired dW, 0 never, 1 where the model predicts a gain (default), 2 always
};
static inline const GemmEnv& gemm_env() {
    static const GemmEnv env = [] {
        const auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
        const auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
        const auto mode = [](const char* name) { const char* e = getenv(name); return (e && e[0] >= '0' && e[0] <= '2' && e[1] == 0) ? e[0] - '0' : 1; };
        const char* r = getenv("MANTIS_GEMM_RING");
        const int cus = num("MANTIS_GEMM_CUS"), smax = num("MANTIS_GEMM_SPLIT_MAX");
        const int ring = (r && r[0] == '1' && r[1] >= '2' && r[1] <= '4' && r[2] == 0) ? 10 + (r[1] - '0') : 0;
        return GemmEnv{cus > 0 ? cus : 0, smax > 0 ? smax : 8, on("MANTIS_GEMM_SK_BALANCED"), on("MANTIS_GEMM_SK_FINISH"), mode("MANTIS_GEMM_176"), ring,
                       mode("MANTIS_GEMM_PAIR")};
    }();
    return env;
}

// CU budget of the tile scheduler.  Rounds, the K split of an incomplete last round and the kernel choice are planned for plan_cus(req, #CU)
// compute units: all of the device by default; fewer when something else holds CUs for the length of a GEMM -- every RCCL channel is a
// workgroup that cannot share a CU with a ring workgroup (160 KiB of LDS each), so with C channels busy a launch planned for 256 CUs
// runs its "one round" as two.  The budget is a PER-CALL argument (bits 16-27 of `flags`; round 5 -- until round 4 a process-wide
// variable, which let two models / reducers of one process interfere); 0 = the default, MANTIS_GEMM_CUS or the whole device.  The split-K
// workspace is always sized for the whole device, so any budget fits it.  Results are deterministic for a given budget; across budgets the
// K-split of the remainder tiles differs, i.e. the fp32 summation order of those tiles (bf16 results agree to rounding, not bit for bit).
static inline int plan_cus(int req, int dev) {
    if (req <= 0) req = gemm_env().cus;
    if (req == 0) return dev;
    return req < 8 ? 8 : (req > dev ? dev : req);
}
static inline int flags_cus(int flags) { return (flags & EPI_CUS_MASK) >> EPI_CUS_SHIFT; }

// ---- the cost model, fitted to measurements on one MI355X.  256 x 256 ring kernels, one workgroup per CU, and the generic 128 x 128 kernel,
// two per CU: profiles/r01_gemm_experiments.md.  176 x 256 kernel and the margin a change of plan must win by: profiles/r06_experiments.md 1.
static constexpr double R256_STEP_US = 1.45;        // microseconds per K-step of a 256 x 256 tile
static constexpr double R256_FIXED_STEPS = 5.0;     // K-step equivalents per round: prologue, epilogue, launch
// K-split reduction in K-step equivalents: slab write, publish, S slab reads (sc1 write-through slabs instead of the release/acquire pair
// were measured equal at S = 2 and 12 % slower at S = 8)
static inline double sk_reduce_steps(int S) { return 8.0 + 1.7 * S; }
static constexpr double GEN_STEP_US = 1.05;         // generic kernel: per K-step of a round of 2 x #CU tiles of 128 x 128
static constexpr double GEN_FIXED_STEPS = 5.2;
#ifndef R176_STEP_US
#define R176_STEP_US 1.02                           // per K-step of a 176 x 256 tile
#endif
#ifndef R176_FIXED_US
#define R176_FIXED_US 7.5                           // microseconds per round, whole tiles only
#endif
static constexpr double PLAN_MARGIN = 0.97;         // the 176-row tile / the paired launch must be predicted >= 3 % faster

// K parts for the tiles of the ring kernel's incomplete last round: minimise K-steps per part + the measured reduction cost.
// S * rem <= #CU: ONE sub-round of split units.  Round 3 tried letting S * rem exceed the CU count (SK_MAX_ROUNDS = 3: for dX of gate|up,
// 96 remainder tiles x 448 K-steps, S = 8 fills all 256 CUs for three short sub-rounds instead of 192 CUs for one long one; the model
// predicted -15 % on the remainder): measured SLOWER, 984 -> 1216 us on the 8-wave kernel, 1027 -> 1481 us on the 4-wave one -- 768 slabs of
// 256 KiB written and read back cost far more than the model extrapolates.  The code path stays (SK_MAX_ROUNDS), the limit is 1.
static inline int ring_split(long ntiles, int nk, int cus) {
    const int rem = (int)(ntiles % cus);
    if (!rem) return 1;
    int best = 1;
    double cost = nk + R256_FIXED_STEPS, cost1 = -1.0;    // cost1: best single-sub-round split
    int best1 = 1;
    for (int S = 2; S <= gemm_env().split_max; ++S) {
        if (nk / S < 8) break;
        const int rounds = (S * rem + cus - 1) / cus;
        if (rounds > SK_MAX_ROUNDS) break;
        const double c = rounds * ((double)nk / S + R256_FIXED_STEPS) + sk_reduce_steps(S);
        if (rounds == 1 && (cost1 < 0 || c < cost1)) { cost1 = c; best1 = S; }
        if (c < cost) { cost = c; best = S; }
    }
    if (best > 1 && (best * rem + cus - 1) / cus > 1) {          // a multi-sub-round split must beat the alternatives clearly
        const double alt = cost1 > 0 && cost1 < nk + R256_FIXED_STEPS ? cost1 : nk + R256_FIXED_STEPS;
        if (cost > 0.9 * alt) return cost1 > 0 && cost1 < nk + R256_FIXED_STEPS ? best1 : 1;
    }
    return best;
}
// predicted launch time (us) of C[M,N] over K on the 256 x 256 ring kernels planned for `cus` CUs: whole rounds, then the K-split remainder
// round and its reduction
static inline double ring256_us(int M, int N, int K, int cus) {
    const int nk = plan_cdiv(K, BK);
    const long t = tiles256(M, N);
    const int S = ring_split(t, nk, cus);
    const long rem = t % cus;
    const int sub = rem ? (int)((S * rem + cus - 1) / cus) : 0;
    return R256_STEP_US * ((double)(t / cus) * (nk + R256_FIXED_STEPS)
                           + (rem ? sub * ((double)nk / S + R256_FIXED_STEPS) + (S > 1 ? sk_reduce_steps(S) : 0.0) : 0.0));
}
// tile variant by the cost model: 12 = "a ring kernel", 1 = the generic 128 x 128 kernel
static inline int gemm_pick_variant(int M, int N, int K, int cus) {
    // below two tile rows / columns the cost model decides too (M = 504 label rows of the lm_head used to fall to the 128x128 kernel
    // -- and, on the dX side, to a transposed weight copy: 2.3 ms instead of 0.58 ms); only genuinely small operands skip it
    if (M < 384 || N < 384) return 1;
    const long t128 = (long)plan_cdiv(M, 128) * plan_cdiv(N, 128);
    const double gen = GEN_STEP_US * (double)((t128 + 2 * cus - 1) / (2 * cus)) * (plan_cdiv(K, BK) + GEN_FIXED_STEPS);
    return ring256_us(M, N, K, cus) <= gen ? 12 : 1;
}
// ring kernel per shape (measured, profiles/r03_gemm_ring_variants.md)
// (1x MI355X, the fifteen GEMMs of a Mantis-8B decoder layer + head, every layout): the 8-wave 16x16x32 kernel (14) is 2-7 % faster than
// the 32x32x16 one (12) on twelve of them and within 3 % on the rest; the 4-wave kernel (13) is faster still -- 4-5 % over 14 -- where the
// main loop is all there is: row-major operands (NT) and a long per-CU K walk (rounds x K-steps), and slower everywhere else (its
// prologue, epilogue and K-split reduction run on half the waves)
static inline int ring_variant_for(int M, int N, int K, bool akm, bool bkm, int cus) {
    if (akm || bkm) return 14;
    const long rounds = (tiles256(M, N) + cus - 1) / cus;
    return rounds * plan_cdiv(K, BK) >= 400 ? 13 : 14;
}
// the 176-row tile where it turns the grid into whole rounds: rounds x (K-steps x loop time + fixed cost per tile) against ring256_us
static inline bool ring176_wins(int M, int N, int K, int cus) {
    const int mode = gemm_env().r176;
    if (mode == 0 || M < 176 * 2 || N < 256) return false;
    if (mode == 2) return true;
    const long t176 = (long)plan_cdiv(M, 176) * plan_cdiv(N, 256);
    const double us176 = (double)((t176 + cus - 1) / cus) * (plan_cdiv(K, BK) * R176_STEP_US + R176_FIXED_US);
    return us176 < PLAN_MARGIN * ring256_us(M, N, K, cus);
}
// two dW GEMMs that share K as ONE grid of whole tiles (mantis_gemm_bf16_tn_pair) against two launches
static inline bool tn_pair_wins(int M1, int N1, int M2, int N2, int K, int cus) {
    const int mode = gemm_env().pair;
    if (mode == 0 || gemm_env().ring) return false;
    if (mode == 2) return true;
    const long t = tiles256(M1, N1) + tiles256(M2, N2);
    const double both = R256_STEP_US * (double)((t + cus - 1) / cus) * (plan_cdiv(K, BK) + R256_FIXED_STEPS);
    return both < PLAN_MARGIN * (ring256_us(M1, N1, K, cus) + ring256_us(M2, N2, K, cus));
}
// The variant an entry point launches when its caller names none.  The entry points differ in exactly these three ways:
//   may_decline: the cost model may hand the shape to the generic kernel (returns 1; _nt launches it, _nt_sumsq refuses; _nt_fused and the
//                SwiGLU backward have ring epilogues only and do not ask)
//   ring12:      MANTIS_GEMM_RING=12 applies (_nt; the ring16-only entry points ignore it -- and, unlike 13 / 14, it then leaves _nt_fused's
//                176-row choice in place)
//   r176:        the 176-row tile is eligible (A row-major in _nt, always in _nt_fused, never in _nt_sumsq)
static inline int gemm_auto_variant(int M, int N, int K, bool akm, bool bkm, int cus, bool may_decline, bool ring12, bool r176) {
    if (may_decline && gemm_pick_variant(M, N, K, cus) != 12) return 1;
    const int forced = gemm_env().ring;
    if (forced >= (ring12 ? 12 : 13)) return forced;
    return r176 && ring176_wins(M, N, K, cus) ? 15 : ring_variant_for(M, N, K, akm, bkm, cus);
}

// ---- operands.  The ring kernels address theirs through buffer descriptors: unsigned 32-bit num_records, unsigned 32-bit lane offset and
// unsigned 32-bit scalar K-step offset (the hardware adds them to the 48-bit base without wrapping).  An operand of 4 GiB or more would wrap
// silently.  (The first guard stood at 2 GiB; the lm_head logits of 8192 rows x 152064 columns, 2.5 GB, then fell to the generic kernel at
// 0.34 PFLOP/s.  `gemm_operand_over_2gib` checks the 2-4 GiB range against the generic kernel.)
static constexpr long GEMM_BUFFER_LIMIT = (1L << 32) - (1L << 16);
static inline bool gemm_over_buffer_limit(int M, int N, int K, long lda, long ldb, bool akm, bool bkm) {
    return (long)(akm ? K : M) * lda * 2 >= GEMM_BUFFER_LIMIT || (long)(bkm ? K : N) * ldb * 2 >= GEMM_BUFFER_LIMIT;
}
// A, B 16-B aligned, lda / ldb % 8 == 0 and long enough for the layout.  Row-major operands are fetched in whole 16-B chunks along K: with
// K % 8 != 0 the tail chunk must meet zeros on the other side, which only a K-major operand (rows k >= K come from the zero page) guarantees;
// the row-major pad must be finite.  tile_c: the ring16-only entry points also want N % 256 == 0, ldc % 8 == 0 and C 16-B aligned; ring_only:
// ... and have no generic kernel to hand a >= 4 GiB operand to.  Dimensions > 0 are the caller's check (MANTIS_EINVAL, in its own order).
static inline int gemm_check_operands(const void* A, long lda, const void* B, long ldb, const void* C, long ldc, int M, int N, int K, bool akm,
                                      bool bkm, bool tile_c, bool ring_only) {
    const int K8 = (K + 7) / 8 * 8;
    if (lda % 8 || ldb % 8 || ldc < N || (((uintptr_t)A | (uintptr_t)B) & 15)) return MANTIS_EUNSUPPORTED;
    if ((!akm && lda < K8) || (!bkm && ldb < K8) || (akm && lda < M) || (bkm && ldb < N) || (!akm && !bkm && (K % 8))) return MANTIS_EUNSUPPORTED;
    if (tile_c && (N % 256 || ldc % 8 || ((uintptr_t)C & 15))) return MANTIS_EUNSUPPORTED;
    if (ring_only && gemm_over_buffer_limit(M, N, K, lda, ldb, akm, bkm)) return MANTIS_EUNSUPPORTED;
    return MANTIS_OK;
}

// ---- what an entry point launches: rc != 0 = refused; else the variant and the flags the kernel gets
struct GemmChoice { int rc, variant, flags; };
// mantis_gemm_bf16_nt: variant 1 = 128x128 generic kernel, 2 = 256x256 generic kernel, 12 = the 8-wave ring kernel (32x32x16 MFMA), 13 / 14 =
// the ring16 kernel (16x16x32 MFMA) with 4 / 8 waves: same tile, same work split, same results up to the accumulation order inside a K-step;
// 15 = the 176-row kernel
static inline GemmChoice gemm_nt_choose(const void* A, long lda, const void* B, long ldb, const void* C, long ldc, int M, int N, int K,
                                        const void* bias, const void* residual, long ldr, int flags, int dev_cus) {
    if (M <= 0 || N <= 0 || K <= 0 || (flags & EPI_SUMSQ)) return {MANTIS_EINVAL, 0, flags};      // bit 7 belongs to mantis_gemm_bf16_nt_sumsq
    const bool akm = flags & EPI_A_KMAJOR, bkm = flags & EPI_B_KMAJOR;
    if (const int rc = gemm_check_operands(A, lda, B, ldb, C, ldc, M, N, K, akm, bkm, false, false)) return {rc, 0, flags};
    if (((flags & EPI_BIAS) && !bias) || ((flags & EPI_RESIDUAL) && !residual)) return {MANTIS_EINVAL, 0, flags};
    // SwiGLU backward: residual = [gate | up], C = [dgate | dup], both [M, 2N]; only the ring kernel's epilogue has it
    if ((flags & EPI_SWIGLU_BWD) && (!residual || (flags & (EPI_BIAS | EPI_ACT_MASK | EPI_RESIDUAL | EPI_ACCUM)) || ldc < 2 * (long)N || ldr < 2 * (long)N))
        return {MANTIS_EINVAL, 0, flags};
    int variant = (flags & EPI_VARIANT_MASK) >> EPI_VARIANT_SHIFT;
    if (variant == 0) variant = gemm_auto_variant(M, N, K, akm, bkm, plan_cus(flags_cus(flags), dev_cus), !(flags & EPI_SWIGLU_BWD), true, !akm);
    const bool ring = variant >= 12 && variant <= 15;
    if (variant == 15 && akm) return {MANTIS_EUNSUPPORTED, 0, flags};               // the M side is row-major in the 176-row kernel
    if ((flags & EPI_SWIGLU_BWD) && (!ring || akm || !bkm)) return {MANTIS_EUNSUPPORTED, 0, flags};
    // >= 4 GiB operands go to the generic kernel (64-bit addresses) when the choice is ours, and are refused when a ring kernel was asked for
    if (ring && gemm_over_buffer_limit(M, N, K, lda, ldb, akm, bkm)) {
        if ((flags & EPI_VARIANT_MASK) || (flags & EPI_SWIGLU_BWD)) return {MANTIS_EUNSUPPORTED, 0, flags};
        return {MANTIS_OK, 1, flags | (1 << EPI_VARIANT_SHIFT)};
    }
    if (!ring && variant != 1 && variant != 2) return {MANTIS_EINVAL, 0, flags};
    return {MANTIS_OK, variant, flags};
}
// mantis_gemm_bf16_nt_sumsq: ring16 kernels (13 / 14) only, no bias / activation / residual
static inline GemmChoice gemm_sumsq_choose(const void* A, long lda, const void* B, long ldb, const void* C, long ldc, int M, int N, int K, int flags,
                                           const void* tile_sumsq, int dev_cus) {
    if (M <= 0 || N <= 0 || K <= 0 || !tile_sumsq) return {MANTIS_EINVAL, 0, flags};
    if (flags & ~(EPI_ACCUM | EPI_A_KMAJOR | EPI_B_KMAJOR | EPI_VARIANT_MASK | EPI_SK_INKERNEL | EPI_CUS_MASK)) return {MANTIS_EUNSUPPORTED, 0, flags};
    const bool akm = flags & EPI_A_KMAJOR, bkm = flags & EPI_B_KMAJOR;
    if (const int rc = gemm_check_operands(A, lda, B, ldb, C, ldc, M, N, K, akm, bkm, true, true)) return {rc, 0, flags};
    int variant = (flags & EPI_VARIANT_MASK) >> EPI_VARIANT_SHIFT;
    if (variant == 0) variant = gemm_auto_variant(M, N, K, akm, bkm, plan_cus(flags_cus(flags), dev_cus), true, false, false);
    if (variant != 13 && variant != 14) return {MANTIS_EUNSUPPORTED, 0, flags};
    return {MANTIS_OK, variant, (flags & ~EPI_VARIANT_MASK) | EPI_SUMSQ};
}
// mantis_gemm_bf16_nt_fused: NT layout, variants 13 - 15; `variant` carries bit 6 (EPI_SK_INKERNEL), bit 7 (EPI_SHARED_GPU) and bits 16-27 (the CU
// budget, as in mantis_gemm_bf16_nt's flags) besides the variant in bits 0-3
static inline GemmChoice gemm_fused_choose(const void* A, long lda, const void* B, long ldb, const void* C, long ldc, int M, int N, int K,
                                           const void* bias, int mode, const void* aux0, const void* aux1, long aux_ld, int aux_n, int variant,
                                           int dev_cus) {
    if (M <= 0 || N <= 0 || K <= 0 || (mode != PAIR_SWIGLU && mode != PAIR_ROPE) || !aux0) return {MANTIS_EINVAL, 0, 0};
    if (const int rc = gemm_check_operands(A, lda, B, ldb, C, ldc, M, N, K, false, false, true, true)) return {rc, 0, 0};
    if (aux_ld % 8 || ((uintptr_t)aux0 & 15)) return {MANTIS_EUNSUPPORTED, 0, 0};
    if (mode == PAIR_SWIGLU && (aux_ld < N / 2 || bias)) return {MANTIS_EUNSUPPORTED, 0, 0};
    if (mode == PAIR_ROPE && (aux_n % 128 || aux_n > N || aux_n < 0 || !aux1 || aux_ld < 64 || ((uintptr_t)aux1 & 15))) return {MANTIS_EUNSUPPORTED, 0, 0};
    const int flags = (bias ? EPI_BIAS : 0) | ((variant & 64) ? EPI_SK_INKERNEL : 0) | ((variant & 128) ? EPI_SHARED_GPU : 0) | (variant & EPI_CUS_MASK);
    variant &= 15;
    if (variant == 0) variant = gemm_auto_variant(M, N, K, false, false, plan_cus(flags_cus(flags), dev_cus), false, false, true);
    if (variant < 13 || variant > 15) return {MANTIS_EUNSUPPORTED, 0, flags};
    return {MANTIS_OK, variant, flags};
}

// mantis_gemm_bf16_tn_pair: both problems K-major on both sides, ring16 tiles, checked in turn
static inline int gemm_pair_check(const void* A1, long lda1, const void* B1, long ldb1, const void* C1, long ldc1, int M1, int N1, const void* ts1,
                                  const void* A2, long lda2, const void* B2, long ldb2, const void* C2, long ldc2, int M2, int N2, const void* ts2,
                                  int K, int flags) {
    if (K <= 0 || (ts1 == nullptr) != (ts2 == nullptr)) return MANTIS_EINVAL;
    if (flags & ~(EPI_ACCUM | EPI_CUS_MASK)) return MANTIS_EUNSUPPORTED;
    if (M1 <= 0 || N1 <= 0) return MANTIS_EINVAL;
    if (const int rc = gemm_check_operands(A1, lda1, B1, ldb1, C1, ldc1, M1, N1, K, true, true, true, true)) return rc;
    if (M2 <= 0 || N2 <= 0) return MANTIS_EINVAL;
    return gemm_check_operands(A2, lda2, B2, ldb2, C2, ldc2, M2, N2, K, true, true, true, true);
}

// ---- the balanced remainder plan of a launch (SkPlan), or units = 0 when the equal split already fills the planned CUs / the ranges would be short
static inline void sk_make_plan(SkPlan& plan, int rem, int S, int nk, int cus) {
    plan.units = plan.nspan = 0;
    const long T = (long)rem * nk;
    if (!gemm_env().sk_balanced || S * rem == cus || rem >= cus || cus > 256 || T / cus < SK_BALANCED_MIN_STEPS || T >= (1L << 23)) return;
    // what it buys: nk / S - T / units K-steps per CU; what it costs: a second prologue + slab store on the CUs that take a tail, more
    // slabs for the finishing pass -- measured ~25 - 30 us, i.e. ~20 K-steps (profiles/r05_experiments.md: dX(gate|up), 448 K-steps, -43 us;
    // down_proj forward, 224, -8 us; the 64- and 96-step shapes +8 ... +16 us): only where the saving is clearly larger
    if (nk / S - (int)(T / cus) < SK_BALANCED_MIN_GAIN) return;
    const int U = cus;
    if (U % 8) return;                                          // the tail placement assumes workgroup j of the remainder section runs on XCD j % 8
    int f[8][32], idx[8][32], n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < U; ++c) {
        const int a0 = sk_bound(c, U, (int)T, nk), a1 = sk_bound(c + 1, U, (int)T, nk);
        const int e = (a0 / nk + 1) * nk;
        if (a1 <= a0) return;                                   // a degenerate range: keep the equal split
        if (a1 > e) {
            if (a1 - e > nk) return;                            // a range spanning three tiles cannot happen for rem < units; be safe
            const int x = c & 7;
            int j = n[x]++;                                     // insertion by first-segment length (then range index): <= 32 per XCD
            while (j > 0 && f[x][j - 1] > e - a0) { f[x][j] = f[x][j - 1]; idx[x][j] = idx[x][j - 1]; --j; }
            f[x][j] = e - a0;
            idx[x][j] = c;
        }
    }
    int R = 0;
    for (int x = 0; x < 8; ++x) R = n[x] > R ? n[x] : R;
    plan.units = U;
    plan.nspan = 8 * R;
    for (int r = 0; r < R; ++r)
        for (int x = 0; x < 8; ++x) plan.span[8 * r + x] = r < n[x] ? (unsigned short)idx[x][r] : (unsigned short)SK_EMPTY;
}

// ---- the launch of a 256 x 256 ring kernel: tiles in rounds of `cus`, the tiles of an incomplete last round split S ways along K
struct RingPlan {
    int tiles_m, tiles_n, nk, ntiles, cus;
    int rem, S;         // tiles of the incomplete last round (0 = whole rounds) and their K parts (1 = no split)
    int full, grid;     // whole tiles (one workgroup each) and workgroups of the equal split: full + S * rem
    bool needs_ws;      // the split units meet in the caller's workspace
    bool finish;        // gemm_ring16_finish_kernel reduces the slabs on all CUs (ring16 kernels, unless EPI_SK_INKERNEL / MANTIS_GEMM_SK_FINISH=0)
    SkPlan sk;          // the balanced round where it pays (finish only)
    int grid16, S16;    // what the ring16 kernels take: balanced -> full + units + tail slots, and the number of remainder tiles for S
};
static inline RingPlan ring_make_plan(int M, int N, int K, int cus, bool ring16, bool inkernel) {
    RingPlan p;
    p.tiles_m = plan_cdiv(M, 256); p.tiles_n = plan_cdiv(N, 256); p.nk = plan_cdiv(K, BK); p.cus = cus;
    const long ntiles = (long)p.tiles_m * p.tiles_n;
    p.ntiles = (int)ntiles;
    p.rem = (int)(ntiles % cus);
    p.S = ring_split(ntiles, p.nk, cus);
    p.needs_ws = p.S > 1;
    p.full = p.S > 1 ? (int)(ntiles - p.rem) : (int)ntiles;
    p.grid = p.S > 1 ? p.full + p.S * p.rem : (int)ntiles;
    p.finish = ring16 && p.S > 1 && !inkernel && gemm_env().sk_finish;
    p.sk.units = p.sk.nspan = 0;
    if (p.finish) sk_make_plan(p.sk, p.rem, p.S, p.nk, cus);
    p.grid16 = p.sk.units ? p.full + p.sk.units + p.sk.nspan : p.grid;
    p.S16 = p.sk.units ? p.rem : p.S;
    return p;
}
// split-K workspace (caller-owned): [ticket counters: (#CU + 1) u32, padded to 256 B][fp32 slabs of 256 x 256: #CU for the equal split; the
// balanced round needs one per range (<= #CU) + one per crossed tile boundary (< #CU)].  Zero-initialised by the caller ONCE; every launch
// leaves the counters at zero (the last arriver of a tile resets its ticket), so one workspace serves any number of stream-ordered launches.
// The layout is that of the whole device, whatever the planning budget.  No allocation, no global state here.
static inline size_t sk_cnt_bytes(int dev_cus) { return (((size_t)(dev_cus + 1) * sizeof(unsigned int)) + 255) / 256 * 256; }
static inline size_t sk_ws_bytes(int cus) { return sk_cnt_bytes(cus) + (size_t)(SK_MAX_ROUNDS > 2 ? SK_MAX_ROUNDS : 2) * cus * SK_SLAB_FLOATS * sizeof(float); }
static inline int gemm_workspace_bytes(int M, int N, int K, int dev_cus) {
    if (M <= 0 && N <= 0 && K <= 0) return (int)sk_ws_bytes(dev_cus);
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return ring_make_plan(M, N, K, plan_cus(0, dev_cus), false, false).needs_ws ? (int)sk_ws_bytes(dev_cus) : 0;
}

// Remainder workgroup j (grid index - full) of a ring16 launch -> its unit: remainder tile (-1: an empty tail slot), first and end K-step, slab.
// Equal split: XCD-contiguous over the S * rem units, the K parts of a tile adjacent, slab = tile * S + part.  Balanced round: see SkPlan.
// gemm_nt_ring16_kernel states the same rule in its own text (its prologue is placed by hand and must not move by an instruction); the two
// are held together by the invariants of tests/test_gemm_remainder_plan.py, which reads this function through mantis_gemm_remainder_plan.
struct SkUnit { int tile, t0, t1, slab; };
static inline SkUnit sk_unit(int j, const RingPlan& p) {
    const int nk = p.nk;
    if (p.sk.units == 0) {
        const int nu = p.grid16 - p.full, q = nu >> 3, r = nu & 7, xcd = j & 7;
        const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (j >> 3);
        const int part = lin / p.rem, tl = lin - part * p.rem;
        return {tl, (int)((unsigned)nk * (unsigned)part / (unsigned)p.S), (int)((unsigned)nk * (unsigned)(part + 1) / (unsigned)p.S), tl * p.S + part};
    }
    const int U = p.sk.units, T = p.rem * nk;
    const bool first = j < U;
    const int c = first ? j : (int)p.sk.span[j - U];
    if (c == (int)SK_EMPTY) return {-1, 0, 0, 0};
    const int a0 = sk_bound(c, U, T, nk), a1 = sk_bound(c + 1, U, T, nk);
    const int tl = a0 / nk, e = (tl + 1) * nk;
    if (first) return {tl, a0 - tl * nk, (a1 < e ? a1 : e) - tl * nk, c};
    return {tl + 1, 0, a1 - e, U + tl};
}
// mantis_gemm_remainder_plan (documented there)
static inline int gemm_remainder_plan(int M, int N, int K, int cus, int* out, int cap) {
    if (M <= 0 || N <= 0 || K <= 0 || !out || cap < 8) return MANTIS_EINVAL;
    const RingPlan p = ring_make_plan(M, N, K, cus, true, false);
    const int nwg = p.grid16 - p.full;
    const int head[8] = {p.ntiles, p.full, p.S > 1 ? p.rem : 0, p.S, p.sk.units, p.sk.nspan, nwg, p.nk};
    for (int i = 0; i < 8; ++i) out[i] = head[i];
    int n = 8;
    for (int j = 0; j < nwg; ++j, n += 4) {
        const SkUnit u = sk_unit(j, p);
        if (n + 4 <= cap) { out[n] = u.tile; out[n + 1] = u.t0; out[n + 2] = u.t1; out[n + 3] = u.slab; }
    }
    return n;
}
