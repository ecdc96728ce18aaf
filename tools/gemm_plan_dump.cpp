// Every decision of the bf16 GEMM planner (mantis_amd/csrc/gemm_plan.h) over a sweep of shapes, layouts, CU budgets and entry points, as JSON on
// stdout -- host code only, for a 256-CU device:   c++ -std=c++17 -O1 tools/gemm_plan_dump.cpp -o dump && ./dump [reduced]
// tests/test_gemm_plan.py holds the output to tests/golden/gemm_plan.json ("reduced": the short sweep it runs once per value of each
// MANTIS_GEMM_* switch, a process each -- the switches are read once).  profiles/gemm_plan_refactor.md: how the fixture was recorded.
//   rows["M,N"]["K"][i] = the row of budget budgets[i]; more["M,N,K,budget"] = further rows.  A row: "pick_variant S full rem units tail-slots
//            remainder-workgroups digest-of-the-remainder-records needs-workspace grid-of-variant-12 grid-of-variant-14 entries"
//   entries: plain x 4 layouts (NT, B K-major, A K-major, both), sumsq x 4, fused SwiGLU (NT), fused RoPE (NT), SwiGLU backward x 4, variant 0:
//            the variant that launches as a hex digit, U = MANTIS_EUNSUPPORTED, I = MANTIS_EINVAL
//   operands[case] = the five entry kinds' return codes (0 = launches) + the paired launch's;  pairs["K,budget"] = tn_pair_wins over PAIR_SHAPES^2
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

struct Launch { int rc, variant, grid; };
#ifdef GEMM_PLAN_DUMP_BACKEND           // the same sweep over another statement of the planner (how the fixture was recorded from the parent commit)
#include GEMM_PLAN_DUMP_BACKEND
#else
#include "../mantis_amd/csrc/gemm_plan.h"
static const int DEV_CUS = 256;
static int be_budget(int cus) { return plan_cus(cus > 0 ? cus : 0, DEV_CUS); }
static int be_pick(int M, int N, int K, int cus) { return gemm_pick_variant(M, N, K, be_budget(cus)); }
static int be_remainder_plan(int M, int N, int K, int cus, int* out, int cap) { return gemm_remainder_plan(M, N, K, be_budget(cus), out, cap); }
static int be_workspace_bytes(int M, int N, int K) { return gemm_workspace_bytes(M, N, K, DEV_CUS); }
static int be_pair_wins(int M1, int N1, int M2, int N2, int K, int cus) { return tn_pair_wins(M1, N1, M2, N2, K, be_budget(cus)); }
static Launch launched(const GemmChoice& c, int M, int N, int K) {
    if (c.rc) return {c.rc, 0, 0};
    int grid = -1;                                       // 15: the 176-row launcher's own
    if (c.variant < 12) grid = c.variant == 2 ? (int)tiles256(M, N) : plan_cdiv(M, 128) * plan_cdiv(N, 128);
    else if (c.variant < 15) {
        const RingPlan p = ring_make_plan(M, N, K, plan_cus(flags_cus(c.flags), DEV_CUS), c.variant != 12, c.flags & EPI_SK_INKERNEL);
        grid = c.variant == 12 ? p.grid : p.grid16;
    }
    return {0, c.variant, grid};
}
static Launch be_nt(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, const void* bias, const void* res,
                    long ldr, int flags) {
    return launched(gemm_nt_choose(A, lda, B, ldb, C, ldc, M, N, K, bias, res, ldr, flags, DEV_CUS), M, N, K);
}
static Launch be_sumsq(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, int flags, float* ts) {
    return launched(gemm_sumsq_choose(A, lda, B, ldb, C, ldc, M, N, K, flags, ts, DEV_CUS), M, N, K);
}
static Launch be_fused(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, const void* bias, int mode,
                       void* aux0, const void* aux1, long aux_ld, int aux_n, int variant) {
    return launched(gemm_fused_choose(A, lda, B, ldb, C, ldc, M, N, K, bias, mode, aux0, aux1, aux_ld, aux_n, variant, DEV_CUS), M, N, K);
}
static int be_pair(const void* A1, long lda1, const void* B1, long ldb1, void* C1, long ldc1, int M1, int N1, float* ts1, const void* A2, long lda2,
                   const void* B2, long ldb2, void* C2, long ldc2, int M2, int N2, float* ts2, int K, int flags) {
    return gemm_pair_check(A1, lda1, B1, ldb1, C1, ldc1, M1, N1, ts1, A2, lda2, B2, ldb2, C2, ldc2, M2, N2, ts2, K, flags);
}
#endif

// operands are never dereferenced: aligned addresses stand for buffers
static char* const PA = (char*)0x10000000, * const PB = (char*)0x20000000, * const PC = (char*)0x30000000, * const PX = (char*)0x40000000;
static const int F_AKM = 4096, F_BKM = 8192, F_SWIGLU_BWD = 64, F_BIAS = 1;
static long up8(long x) { return (x + 7) / 8 * 8; }
static char code(const Launch& l) { return l.rc == -2 ? 'U' : l.rc ? 'I' : "0123456789abcdef"[l.variant & 15]; }

// one launch of entry kind `kind` (0 plain, 1 sumsq, 2 fused SwiGLU, 3 fused RoPE, 4 SwiGLU backward) with well-formed operands, then the
// deviations of `bad` (see OPERAND_CASES)
struct Bad { long dlda = 0, dldb = 0, dldc = 0, offA = 0, offB = 0, offC = 0; bool no_bias = false; };
static Launch entry(int kind, int M, int N, int K, bool akm, bool bkm, int budget, int variant, const Bad& bad = Bad()) {
    const long lda = (akm ? up8(M) : up8(K)) + bad.dlda, ldb = (bkm ? up8(N) : up8(K)) + bad.dldb;
    const long ldc = (kind == 4 ? 2L * N : N) + bad.dldc;
    const int flags = (akm ? F_AKM : 0) | (bkm ? F_BKM : 0) | (budget << 16);
    char *A = PA + bad.offA, *B = PB + bad.offB, *C = PC + bad.offC;
    switch (kind) {
        case 0: return be_nt(A, lda, B, ldb, C, ldc, M, N, K, bad.no_bias ? nullptr : PX, nullptr, 0, flags | (variant << 8) | (bad.no_bias ? F_BIAS : 0));
        case 1: return be_sumsq(A, lda, B, ldb, C, ldc, M, N, K, flags | (variant << 8), (float*)PX);
        case 2: return be_fused(A, lda, B, ldb, C, ldc, M, N, K, nullptr, 1, PX, nullptr, up8(N / 2), 0, variant | (budget << 16));
        case 3: return be_fused(A, lda, B, ldb, C, ldc, M, N, K, nullptr, 2, PX, PX + 4096, 64, 128, variant | (budget << 16));
        default: return be_nt(A, lda, B, ldb, C, ldc, M, N, K, nullptr, PX, 2L * N, flags | F_SWIGLU_BWD | (variant << 8));
    }
}

// "pick S full rem units tails nwg digest ws g12 g14 entries" of one (shape, budget); digest: FNV-1a over the remainder records, - = none
static std::string row(int M, int N, int K, int budget) {
    static int buf[8 + 4 * 1024];
    const int n = be_remainder_plan(M, N, K, budget, buf, 8 + 4 * 1024);
    unsigned long long h = 1469598103934665603ull;
    for (int i = 8; i < n; ++i) { h ^= (unsigned)buf[i]; h *= 1099511628211ull; }
    char e[15], dig[9] = "-", out[160];
    int k = 0;
    for (int kind = 0; kind < 5; ++kind)
        for (int lay = 0; lay < ((kind == 2 || kind == 3) ? 1 : 4); ++lay) e[k++] = code(entry(kind, M, N, K, lay & 2, lay & 1, budget, 0));
    e[k] = 0;
    if (n > 8) snprintf(dig, sizeof dig, "%08x", (unsigned)(h ^ (h >> 32)));
    snprintf(out, sizeof out, "%d %d %d %d %d %d %d %s %d %d %d %s", be_pick(M, N, K, budget), buf[3], buf[1], buf[2], buf[4], buf[5], buf[6], dig,
             be_workspace_bytes(M, N, K) != 0, entry(0, M, N, K, false, false, budget, 12).grid, entry(0, M, N, K, false, false, budget, 14).grid, e);
    return out;
}

int main(int argc, char** argv) {
    const bool reduced = argc > 1 && !strcmp(argv[1], "reduced");
    const std::vector<int> rMs = {504, 5624, 8192}, rNs = {384, 4096, 6144, 14336}, rKs = {512, 4096, 14336, 28672};
    const std::vector<int> Ms = reduced ? rMs : std::vector<int>{256, 383, 384, 504, 512, 2000, 4608, 5000, 5624, 6144, 8192};
    const std::vector<int> Ns = reduced ? rNs : std::vector<int>{256, 384, 1152, 2100, 3584, 3840, 4096, 6144, 14336, 28672, 128264};
    const std::vector<int> Ks = reduced ? rKs : std::vector<int>{64, 504, 512, 1152, 2048, 4096, 4304, 5624, 14336, 25600, 28672, 100000};
    // the budget axis is thinned to {default, 200} over the grid; 97 and 240 run over the reduced grid and the ragged shapes below.  The switch
    // runs take the default budget only, and leave out the operand cases (no switch bears on them)
    const std::vector<int> budgets = reduced ? std::vector<int>{0} : std::vector<int>{0, 200};
    // tests/test_gemm_remainder_plan.py's SHAPES that the grids do not hold; two ragged shapes at the other budgets
    const int extra[][4] = {{5624, 4096, 6144, 0}, {4096, 14336, 5624, 0}, {8192, 4096, 16384, 0}, {2000, 2100, 2048, 97}, {5624, 3840, 4096, 240}};
    printf("{\"dev_cus\": %d, \"default_budget\": %d, \"ws_bytes\": %d, \"budgets\": [%s], \"rows\": {", be_budget(1 << 20), be_budget(0),
           be_workspace_bytes(0, 0, 0), reduced ? "0" : "0, 200");
    bool first = true;
    for (int M : Ms) for (int N : Ns) {          // one line per (M, N): K -> one row per budget
        printf("%s\n  \"%d,%d\": {", first ? "" : ",", M, N);
        first = false;
        for (size_t i = 0; i < Ks.size(); ++i) {
            printf("%s\"%d\": [", i ? ", " : "", Ks[i]);
            for (size_t j = 0; j < budgets.size(); ++j) printf("%s\"%s\"", j ? ", " : "", row(M, N, Ks[i], budgets[j]).c_str());
            printf("]");
        }
        printf("}");
    }
    printf("\n}, \"more\": {");                 // "M,N,K,budget" -> row
    first = true;
    if (!reduced) {
        for (int M : rMs) for (int N : rNs) for (int K : rKs) for (int b : {97, 240}) {
            printf("%s\n  \"%d,%d,%d,%d\": \"%s\"", first ? "" : ",", M, N, K, b, row(M, N, K, b).c_str());
            first = false;
        }
        for (const auto& x : extra) printf(",\n  \"%d,%d,%d,%d\": \"%s\"", x[0], x[1], x[2], x[3], row(x[0], x[1], x[2], x[3]).c_str());
    }

    // good and bad operands for every entry kind at one shape, row-major (NT) and K-major (TN): which code comes back, and which check fires first
    struct Case { const char* name; int M, N, K; bool km; int variant; Bad bad; };
    const int M = 5624, N = 4096, K = 4096;
    Bad lda4, ldb4, ldc_short, ldc4, lda_short, offA, offB, offC, lda4_nobias, nobias;
    lda4.dlda = 4; ldb4.dldb = 4; ldc_short.dldc = -8; ldc4.dldc = 4; lda_short.dlda = -8; offA.offA = 8; offB.offB = 8; offC.offC = 8;
    lda4_nobias.dlda = 4; lda4_nobias.no_bias = true; nobias.no_bias = true;
    const Case cases[] = {
        {"good", M, N, K, false, 0, Bad()}, {"good_km", M, N, K, true, 0, Bad()}, {"lda%8", M, N, K, false, 0, lda4}, {"ldb%8_km", M, N, K, true, 0, ldb4},
        {"ldc<N", M, N, K, false, 0, ldc_short}, {"ldc%8", M, N, K, false, 0, ldc4}, {"lda<K", M, N, K, false, 0, lda_short},
        {"lda<M_km", M, N, K, true, 0, lda_short}, {"A+8", M, N, K, false, 0, offA}, {"B+8_km", M, N, K, true, 0, offB}, {"C+8", M, N, K, false, 0, offC},
        {"K%8", M, N, 4100, false, 0, Bad()}, {"K%8_km", M, N, 4100, true, 0, Bad()}, {"M=0", 0, N, K, false, 0, Bad()}, {"M=0,lda%8", 0, N, K, false, 0, lda4},
        {"K=0_km", M, N, 0, true, 0, Bad()}, {"no_bias", M, N, K, false, 0, nobias}, {"no_bias,lda%8", M, N, K, false, 0, lda4_nobias},
        {"4GiB", 8192, 128264, 100000, false, 0, Bad()}, {"4GiB_v14", 8192, 128264, 100000, false, 14, Bad()}, {"4GiB_km", 8192, 28672, 100000, true, 0, Bad()},
        {"v2", M, N, K, false, 2, Bad()}, {"v3", M, N, K, false, 3, Bad()}, {"v12_km", M, N, K, true, 12, Bad()}, {"v15", M, N, K, false, 15, Bad()},
        {"v15_km", M, N, K, true, 15, Bad()}, {"N%256", M, 2100, K, false, 0, Bad()}};
    printf("\n}, \"operands\": {");
    first = true;
    for (const Case& c : cases) {
        if (reduced) break;
        printf("%s\n  \"%s\": [", first ? "" : ",", c.name);
        first = false;
        for (int kind = 0; kind < 5; ++kind) {
            const bool km = c.km && kind != 2 && kind != 3;          // the fused entry point is NT
            printf("%d, ", entry(kind, c.M, c.N, c.K, km && kind != 4, km || kind == 4, 0, c.variant, c.bad).rc);
        }
        // the paired launch: the case's operands as problem 1 next to a good problem 2, and the other way round
        const Bad& b = c.bad;
        const long lda = up8(c.M) + b.dlda, ldb = up8(c.N) + b.dldb, ldc = c.N + b.dldc;
        printf("%d, %d]", be_pair(PA + b.offA, lda, PB + b.offB, ldb, PC + b.offC, ldc, c.M, c.N, nullptr, PA, 4096, PB, 4096, PC, 4096, 4096, 4096, nullptr, c.K, 0),
               be_pair(PA, 4096, PB, 4096, PC, 4096, 4096, 4096, (float*)PX, PA + b.offA, lda, PB + b.offB, ldb, PC + b.offC, ldc, c.M, c.N, (float*)PX, c.K, 32));
    }
    // a bad first problem next to an empty second one: the first problem's code
    if (!reduced) {
        printf(",\n  \"pair:lda%%8+M2=0\": [%d]", be_pair(PA, 4100, PB, 4096, PC, 4096, 4096, 4096, nullptr, PA, 4096, PB, 4096, PC, 4096, 0, 4096, nullptr, K, 0));
        printf(",\n  \"pair:ts1_only\": [%d]", be_pair(PA, 4096, PB, 4096, PC, 4096, 4096, 4096, (float*)PX, PA, 4096, PB, 4096, PC, 4096, 4096, 4096, nullptr, K, 0));
        printf(",\n  \"pair:flags\": [%d]", be_pair(PA, 4096, PB, 4096, PC, 4096, 0, 4096, nullptr, PA, 4096, PB, 4096, PC, 4096, 4096, 4096, nullptr, K, 1));
    }

    const int PAIR_SHAPES[][2] = {{4096, 14336}, {6144, 4096}, {4096, 4096}, {14336, 4096}, {1152, 1152}, {4608, 1152}, {512, 256}, {8192, 28672}};
    printf("\n}, \"pair_shapes\": [");
    for (int i = 0; i < 8; ++i) printf("%s[%d, %d]", i ? ", " : "", PAIR_SHAPES[i][0], PAIR_SHAPES[i][1]);
    printf("], \"pairs\": {");
    first = true;
    for (int Kp : {512, 5624, 14336})
        for (int b : {0, 97, 200, 240}) {
            std::string s;
            for (const auto& p : PAIR_SHAPES) for (const auto& q : PAIR_SHAPES) s += be_pair_wins(p[0], p[1], q[0], q[1], Kp, b) ? '1' : '0';
            printf("%s\n  \"%d,%d\": \"%s\"", first ? "" : ",", Kp, b, s.c_str());
            first = false;
        }
    printf("\n}}\n");
    return 0;
}
