// Greedy decoding with a KV cache, gfx950: the four kernels of one decode step that the training kernels do not serve.
//
// Replaces (reference path): the cached branch of HF LlamaAttention.forward (transformers/models/llama/modeling_llama.py, attention with
// `past_key_values`: append the new key / value, one query row over all cached keys), the M = batch linears around it, and the
// `argmax` of greedy search, as driven by /root/reference/mantis/models/mllava/modeling_llava.py:478-508,551-602.
//
// A decode step is memory-bound: every weight byte and every cached key / value byte is read once per token.
//   linear_skinny : C[M, N] = epi(A[M, K] . W[N, K]^T), 1 <= M <= 16.  One workgroup per 16-row strip of W; its waves (eight under 1024 strips,
//                   four from there on) split K in interleaved 128-element blocks.  W goes global -> VGPR with non-temporal 16-byte loads
//                   (read once) straight into the B operand of v_mfma_f32_16x16x32_bf16, the <= 16 activation rows (L2-resident) into the A
//                   operand; per-wave partial tiles meet in LDS and are summed in wave order.  No atomics, no workspace.
//   kv_cache_write: rows of a fused q|k|v buffer -> the cache (K, V: [B, Hkv, S_max, hd], head-major so that one (sample, kv head) is one
//                   contiguous stream), optionally rotating q (in place) and k on the way with rope_apply's arithmetic.
//   attn_decode   : grid = splits x Hkv x B; the H / Hkv query heads of a kv head share the workgroup, so K / V are read once per kv head,
//                   16 bytes per lane straight to VGPRs; online softmax per lane, fp32 partial (m, l, o) per split to a caller-owned
//                   workspace, a combine kernel sums the splits in split order.
//   argmax_rows   : first V columns of bf16 logits -> int64 index, ties to the lowest index.
//   greedy_select : the same argmax + one step of greedy search's bookkeeping (pad fill, column write, EOS test) with the finished flags
//                   kept on the device.
// All four are deterministic (fixed summation orders).
#include "common.h"

// ------------------------------------------------------------------------------------------------------------------ skinny linear
template <int NW>
__global__ __launch_bounds__(NW * 64) void linear_skinny_kernel(const bf16_t* __restrict__ A, long lda, const bf16_t* __restrict__ W, long ldw,
                                                                bf16_t* __restrict__ C, long ldc, int M, int N, int K,
                                                                const bf16_t* __restrict__ bias, const bf16_t* __restrict__ res, long ldr) {
    __shared__ float red[NW][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long n0 = (long)blockIdx.x * 16;
    const bool wlive = n0 + r < N, alive = r < M;
    const bf16_t* wp = W + (wlive ? (n0 + r) * ldw : 0);
    const bf16_t* ap = A + (alive ? (long)r * lda : 0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // k-block = 128 elements; lane group g covers k = kb * 128 + g * 32 + j * 8 .. + 8 for j = 0 .. 3 (64 contiguous bytes per lane, 256 per
    // row).  The contraction index is permuted the same way for both operands, which a dot product does not notice.
    const int nkb = (K + 127) >> 7;
#pragma unroll 2
    for (int kb = w; kb < nkb; kb += NW) {
        const int k0 = (kb << 7) + (g << 5);
        u32x4 wv[4], av[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j * 8;
            const bool in = k < K;
            wv[j] = (wlive && in) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + k)) : u32x4{0u, 0u, 0u, 0u};
            av[j] = (alive && in) ? *reinterpret_cast<const u32x4*>(ap + k) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            union { u32x4 u; bf16x8 b; } ua, uw;
            ua.u = av[j];
            uw.u = wv[j];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.b, uw.b, acc, 0, 0, 0);
        }
    }
    // D: lane holds rows m = 4 g + i, column n = r
#pragma unroll
    for (int i = 0; i < 4; ++i) red[w][(g * 4 + i) * 16 + r] = acc[i];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 256) {
        const int m = t >> 4;
        const long n = n0 + (t & 15);
        if (m < M && n < N) {
            float y = 0.f;
#pragma unroll
            for (int i = 0; i < NW; ++i) y += red[i][t];
            if (bias) y += bf2f(bias[n]);
            if (res) y = bf2f(f2bf(y)) + bf2f(res[(long)m * ldr + n]);      // as mantis_gemm_bf16_nt: the product is rounded, then the residual added
            C[(long)m * ldc + n] = f2bf(y);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ cache write
__global__ void kv_cache_write_kernel(bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                      const int* __restrict__ slot, const bf16_t* __restrict__ cosb, const bf16_t* __restrict__ sinb, long R,
                                      int rps, int H, int Hkv, int hd, int S_max) {
    const int half = hd >> 1, cph = half >> 3, nh = H + 2 * Hkv;
    const long total = R * nh * cph;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cph);
        const long t = i / cph;
        const int h = (int)(t % nh);
        const long r = t / nh;
        if (!cosb && h < H) continue;                        // copy only: q stays as it is
        bf16_t* p1 = qkv + r * ld + (long)h * hd + c * 8;
        bf16_t* p2 = p1 + half;
        u32x4 o1 = *reinterpret_cast<const u32x4*>(p1);
        u32x4 o2 = *reinterpret_cast<const u32x4*>(p2);
        if (cosb && h < H + Hkv) {
            const u32x4 a = o1, b = o2;
            const u32x4 vcs = *reinterpret_cast<const u32x4*>(cosb + r * half + c * 8);
            const u32x4 vsn = *reinterpret_cast<const u32x4*>(sinb + r * half + c * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x1[2] = {bf2f_lo(a[e]), bf2f_hi(a[e])};
                const float x2[2] = {bf2f_lo(b[e]), bf2f_hi(b[e])};
                const float cs[2] = {bf2f_lo(vcs[e]), bf2f_hi(vcs[e])};
                const float sn[2] = {bf2f_lo(vsn[e]), bf2f_hi(vsn[e])};
                float r1[2], r2[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    // rope_apply_kernel<1>: every product and the sum rounded to bf16 (modeling_llama.py:157-158)
                    r1[k] = bf2f(f2bf(x1[k] * cs[k])) - bf2f(f2bf(x2[k] * sn[k]));
                    r2[k] = bf2f(f2bf(x2[k] * cs[k])) + bf2f(f2bf(x1[k] * sn[k]));
                }
                o1[e] = pack_bf2(r1[0], r1[1]);
                o2[e] = pack_bf2(r2[0], r2[1]);
            }
        }
        if (h < H) {
            *reinterpret_cast<u32x4*>(p1) = o1;
            *reinterpret_cast<u32x4*>(p2) = o2;
            continue;
        }
        const int s = slot[r];
        if (s < 0 || s >= S_max) continue;
        const long b = r / rps;
        const int kvh = (h - H) % Hkv;
        bf16_t* dst = (h < H + Hkv ? kc : vc) + ((b * Hkv + kvh) * (long)S_max + s) * hd + c * 8;
        *reinterpret_cast<u32x4*>(dst) = o1;
        *reinterpret_cast<u32x4*>(dst + half) = o2;
    }
}

// ------------------------------------------------------------------------------------------------------------------ decode attention
#define DEC_M0 (-1.0e30f)       // running maximum of a row that has seen no live key (finite: exp(m - m') never meets inf - inf)

static inline int decode_cus() {
    static int cached = 0;
    if (cached == 0) {
        int dev = 0, n = 0;
        cached = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                  n > 0) ? n : 256;
    }
    return cached;
}
// the split count: a pure function of (B, Hkv, S_max, #CU): two workgroups per CU wanted, at least 128 keys per split, at most 64 splits
static inline int decode_splits(int B, int Hkv, int S_max) {
    const long wgs = (long)B * Hkv;
    long want = (2L * decode_cus() + wgs - 1) / wgs;
    const long maxs = (S_max + 127) / 128;
    if (want > maxs) want = maxs;
    if (want > 64) want = 64;
    return (int)(want < 1 ? 1 : want);
}
static inline int decode_chunk(int S_max, int splits) { return ((S_max + splits - 1) / splits + 63) / 64 * 64; }

template <int HD, int GT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, const int* __restrict__ kmask,
                                                          const int* __restrict__ n_keys, float* __restrict__ ws_o, float* __restrict__ ws_ml,
                                                          int H, int Hkv, int G, int S_max, int chunk, int splits, float scale) {
    constexpr int LPK = HD / 8;          // lanes per key row (16 bytes each)
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    constexpr int NGRP = 256 / LPK;
    __shared__ float s_acc[256][9];
    __shared__ float s_l[256];
    __shared__ float red[16];
    const int sp = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LPK, kg = lane / LPK;
    int nk = n_keys[b];
    nk = nk < S_max ? nk : S_max;
    const int s0 = sp * chunk;
    int s1 = s0 + chunk;
    s1 = s1 < nk ? s1 : nk;

    float qf[GT][8], acc[GT][8], m[GT], l[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        m[g] = DEC_M0;
        l[g] = 0.f;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (g < G) v = *reinterpret_cast<const u32x4*>(q + (long)b * ldq + (long)(kvh * G + g) * HD + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qf[g][2 * e] = bf2f_lo(v[e]) * scale;
            qf[g][2 * e + 1] = bf2f_hi(v[e]) * scale;
            acc[g][2 * e] = acc[g][2 * e + 1] = 0.f;
        }
    }
    const bf16_t* kb = kc + (long)(b * Hkv + kvh) * S_max * HD + c * 8;
    const bf16_t* vb = vc + (long)(b * Hkv + kvh) * S_max * HD + c * 8;
    const int* km = kmask ? kmask + (long)b * S_max : nullptr;
#pragma unroll 2
    for (int base = s0 + w * KPW; base < s1; base += 4 * KPW) {       // wave-uniform trip count: the shuffles below need every lane
        const int key = base + kg;
        const bool live = key < s1 && (!km || km[key] != 0);
        u32x4 kv4 = {0u, 0u, 0u, 0u}, vv4 = {0u, 0u, 0u, 0u};
        if (live) {
            kv4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (long)key * HD));
            vv4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (long)key * HD));
        }
        float kf[8], vf[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            kf[2 * e] = bf2f_lo(kv4[e]);
            kf[2 * e + 1] = bf2f_hi(kv4[e]);
            vf[2 * e] = bf2f_lo(vv4[e]);
            vf[2 * e + 1] = bf2f_hi(vv4[e]);
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s += qf[g][e] * kf[e];
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o);
            if (live) {
                const float mn = fmaxf(m[g], s);
                const float corr = __expf(m[g] - mn), p = __expf(s - mn);
                m[g] = mn;
                l[g] = l[g] * corr + p;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = acc[g][e] * corr + p * vf[e];
            }
        }
    }
    // merge the 256 / LPK key groups of the workgroup, one query head at a time, in group order
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        if (g < G) {                                                   // G is uniform over the grid
            const float mx = block_max(m[g], red);
            const float f = __expf(m[g] - mx);
#pragma unroll
            for (int e = 0; e < 8; ++e) s_acc[tid][e] = acc[g][e] * f;
            s_l[tid] = l[g] * f;
            __syncthreads();
            if (tid < HD) {
                const int cc = tid >> 3, e = tid & 7;
                float o = 0.f, ls = 0.f;
                for (int j = 0; j < NGRP; ++j) {
                    o += s_acc[j * LPK + cc][e];
                    ls += s_l[j * LPK];
                }
                const long row = ((long)b * H + (kvh * G + g)) * splits + sp;
                ws_o[row * HD + tid] = o;
                if (tid == 0) {
                    ws_ml[row * 2] = mx;
                    ws_ml[row * 2 + 1] = ls;
                }
            }
            __syncthreads();
        }
    }
}

template <int HD>
__global__ void attn_decode_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml, bf16_t* __restrict__ O, long ldo,
                                           int H, int splits) {
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (tid >= HD) return;
    const long base = ((long)b * H + h) * splits;
    float mx = DEC_M0;
    for (int s = 0; s < splits; ++s) mx = fmaxf(mx, ws_ml[(base + s) * 2]);
    float o = 0.f, ls = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float f = __expf(ws_ml[(base + s) * 2] - mx);
        ls += f * ws_ml[(base + s) * 2 + 1];
        o += f * ws_o[(base + s) * HD + tid];
    }
    O[(long)b * ldo + (long)h * HD + tid] = f2bf(ls > 0.f ? o / ls : 0.f);      // a row without a live key: zeros
}

template <int HD>
static int launch_attn_decode(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, const int* kmask, const int* n_keys, bf16_t* O,
                              long ldo, float* ws, int B, int H, int Hkv, int S_max, float scale, hipStream_t st) {
    const int G = H / Hkv;
    const int splits = decode_splits(B, Hkv, S_max), chunk = decode_chunk(S_max, splits);
    float* ws_o = ws;
    float* ws_ml = ws + (long)B * H * splits * HD;
    const dim3 grid(splits, Hkv, B);
#define DEC_LAUNCH(GT)                                                                                                                   \
    MANTIS_LAUNCH((attn_decode_kernel<HD, GT>), grid, dim3(256), 0, st, q, ldq, kc, vc, kmask, n_keys, ws_o, ws_ml, H, Hkv, G, S_max, chunk, \
                  splits, scale)
    if (G == 1) DEC_LAUNCH(1);
    else if (G <= 4) DEC_LAUNCH(4);
    else DEC_LAUNCH(8);
#undef DEC_LAUNCH
    int rc = mantis_check_launch();
    if (rc != MANTIS_OK) return rc;
    MANTIS_LAUNCH((attn_decode_combine_kernel<HD>), dim3(H, B), dim3(HD < 64 ? 64 : HD), 0, st, (const float*)ws_o, (const float*)ws_ml, O, ldo,
                  H, splits);
    return mantis_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------ argmax
__global__ __launch_bounds__(1024) void argmax_rows_kernel(const bf16_t* __restrict__ x, long ld, int V, long* __restrict__ out) {
    __shared__ float s_v[1024];
    __shared__ int s_i[1024];
    const int tid = threadIdx.x;
    const bf16_t* row = x + (long)blockIdx.x * ld;
    float best = 0.f;
    int bi = -1;
    for (int i = tid; i < V; i += 1024) {        // ascending i: a strict comparison keeps the lowest index of equal values
        const float v = bf2f(row[i]);
        if (bi < 0 || v > best) {
            best = v;
            bi = i;
        }
    }
    s_v[tid] = best;
    s_i[tid] = bi;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) {
            const float v2 = s_v[tid + off];
            const int i2 = s_i[tid + off];
            const float v1 = s_v[tid];
            const int i1 = s_i[tid];
            if (i2 >= 0 && (i1 < 0 || v2 > v1 || (v2 == v1 && i2 < i1))) {
                s_v[tid] = v2;
                s_i[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = (long)s_i[0];
}

// ------------------------------------------------------------------------------------------------------------------ greedy select
// argmax_rows_kernel's reduction (same strided scan, same tree, same tie rule) followed by one step of greedy search's bookkeeping for the
// row: pad fill of a finished row, the column write, the EOS test.  Row b's flags are read and written by thread 0 of workgroup b only.
__global__ __launch_bounds__(1024) void greedy_select_kernel(const bf16_t* __restrict__ x, long ld, int V, const long* __restrict__ eos_ids,
                                                             int n_eos, long pad_id, int* __restrict__ unfinished, int* __restrict__ finish_step,
                                                             long* __restrict__ out, long ldo, int step, long* __restrict__ next_tokens) {
    __shared__ float s_v[1024];
    __shared__ int s_i[1024];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const bf16_t* row = x + (long)b * ld;
    float best = 0.f;
    int bi = -1;
    for (int i = tid; i < V; i += 1024) {        // ascending i: a strict comparison keeps the lowest index of equal values
        const float v = bf2f(row[i]);
        if (bi < 0 || v > best) {
            best = v;
            bi = i;
        }
    }
    s_v[tid] = best;
    s_i[tid] = bi;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) {
            const float v2 = s_v[tid + off];
            const int i2 = s_i[tid + off];
            const float v1 = s_v[tid];
            const int i1 = s_i[tid];
            if (i2 >= 0 && (i1 < 0 || v2 > v1 || (v2 == v1 && i2 < i1))) {
                s_v[tid] = v2;
                s_i[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    long t = (long)s_i[0];
    if (n_eos > 0) {
        const bool live = unfinished[b] != 0;
        if (!live) t = pad_id;
        bool hit = false;
        for (int e = 0; e < n_eos; ++e) hit = hit || (eos_ids[e] == t);
        if (live && hit) {
            unfinished[b] = 0;
            finish_step[b] = step;
        }
    }
    out[(long)b * ldo + step] = t;
    next_tokens[b] = t;
}

extern "C" {

int mantis_linear_skinny_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                              const void* bias, const void* residual, int64_t ldr, void* stream) {
    if (M < 1 || M > 16 || N < 0 || K < 0) return MANTIS_EINVAL;
    if (K % 8 || lda % 8 || ldw % 8 || ((uintptr_t)A & 15) || ((uintptr_t)W & 15)) return MANTIS_EUNSUPPORTED;
    if (N == 0) return MANTIS_OK;
    const int strips = cdiv(N, 16);
    if (strips < 1024)      // few strips (N < 16 K rows): eight waves split K, for enough bytes in flight per CU
        MANTIS_LAUNCH((linear_skinny_kernel<8>), dim3(strips), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)A, (long)lda, (const bf16_t*)W,
                      (long)ldw, (bf16_t*)C, (long)ldc, M, N, K, (const bf16_t*)bias, (const bf16_t*)residual, (long)ldr);
    else
        MANTIS_LAUNCH((linear_skinny_kernel<4>), dim3(strips), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)A, (long)lda, (const bf16_t*)W,
                      (long)ldw, (bf16_t*)C, (long)ldc, M, N, K, (const bf16_t*)bias, (const bf16_t*)residual, (long)ldr);
    return mantis_check_launch();
}

int mantis_kv_cache_write(void* qkv, int64_t ld, void* k_cache, void* v_cache, const int32_t* slot, const void* cos_tab, const void* sin_tab,
                          int64_t R, int rows_per_sample, int H, int Hkv, int hd, int S_max, void* stream) {
    if (R < 0 || rows_per_sample < 1 || H < 1 || Hkv < 1 || S_max < 1 || (cos_tab == nullptr) != (sin_tab == nullptr) || !qkv || !k_cache ||
        !v_cache || !slot)
        return MANTIS_EINVAL;
    if (hd % 16 || ld % 8 || ((uintptr_t)qkv & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) || ((uintptr_t)cos_tab & 15) ||
        ((uintptr_t)sin_tab & 15))
        return MANTIS_EUNSUPPORTED;
    if (R == 0) return MANTIS_OK;
    const long total = R * (H + 2 * Hkv) * (hd / 16);
    long g = (total + 255) / 256;
    g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
    MANTIS_LAUNCH(kv_cache_write_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, (long)ld, (bf16_t*)k_cache,
                  (bf16_t*)v_cache, (const int*)slot, (const bf16_t*)cos_tab, (const bf16_t*)sin_tab, (long)R, rows_per_sample, H, Hkv, hd, S_max);
    return mantis_check_launch();
}

int mantis_attn_decode_splits(int B, int Hkv, int S_max) {
    if (B < 1 || Hkv < 1 || S_max < 1) return 1;
    return decode_splits(B, Hkv, S_max);
}

int mantis_attn_decode_workspace_bytes(int B, int H, int Hkv, int hd, int S_max) {
    if (B < 1 || H < 1 || Hkv < 1 || hd < 1 || S_max < 1) return 0;
    return (int)((long)B * H * decode_splits(B, Hkv, S_max) * (hd + 2) * (long)sizeof(float));
}

int mantis_attn_decode(const void* Q, int64_t ldq, const void* k_cache, const void* v_cache, const int32_t* kmask, const int32_t* n_keys,
                       void* O, int64_t ldo, void* workspace, int B, int H, int Hkv, int hd, int S_max, float scale, void* stream) {
    if (B < 1 || H < 1 || Hkv < 1 || S_max < 1 || H % Hkv || !workspace || !n_keys) return MANTIS_EINVAL;
    if (H / Hkv > 8 || ldq % 8 || B > 65535 || Hkv > 65535 || ((uintptr_t)Q & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15))
        return MANTIS_EUNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    switch (hd) {
        case 16:
            return launch_attn_decode<16>((const bf16_t*)Q, (long)ldq, (const bf16_t*)k_cache, (const bf16_t*)v_cache, (const int*)kmask,
                                          (const int*)n_keys, (bf16_t*)O, (long)ldo, (float*)workspace, B, H, Hkv, S_max, scale, st);
        case 64:
            return launch_attn_decode<64>((const bf16_t*)Q, (long)ldq, (const bf16_t*)k_cache, (const bf16_t*)v_cache, (const int*)kmask,
                                          (const int*)n_keys, (bf16_t*)O, (long)ldo, (float*)workspace, B, H, Hkv, S_max, scale, st);
        case 128:
            return launch_attn_decode<128>((const bf16_t*)Q, (long)ldq, (const bf16_t*)k_cache, (const bf16_t*)v_cache, (const int*)kmask,
                                           (const int*)n_keys, (bf16_t*)O, (long)ldo, (float*)workspace, B, H, Hkv, S_max, scale, st);
        default:
            return MANTIS_EUNSUPPORTED;
    }
}

int mantis_argmax_rows(const void* logits, int64_t ld, int B, int V, int64_t* out, void* stream) {
    if (B < 0 || V < 1) return MANTIS_EINVAL;
    if (B == 0) return MANTIS_OK;
    MANTIS_LAUNCH(argmax_rows_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld, V, (long*)out);
    return mantis_check_launch();
}

int mantis_greedy_select(const void* logits, int64_t ld, int B, int V, const int64_t* eos_ids, int n_eos, int64_t pad_id, int32_t* unfinished,
                         int32_t* finish_step, int64_t* out, int64_t ldo, int step, int64_t* next_tokens, void* stream) {
    if (B < 0 || V < 1 || n_eos < 0 || step < 0 || ldo < 1 || step >= ldo || ld < V || !logits || !out || !next_tokens) return MANTIS_EINVAL;
    if (n_eos > 0 && (!eos_ids || !unfinished || !finish_step)) return MANTIS_EINVAL;
    if (B == 0) return MANTIS_OK;
    MANTIS_LAUNCH(greedy_select_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld, V, (const long*)eos_ids,
                  n_eos, (long)pad_id, (int*)unfinished, (int*)finish_step, (long*)out, (long)ldo, step, (long*)next_tokens);
    return mantis_check_launch();
}

}  // extern "C"
