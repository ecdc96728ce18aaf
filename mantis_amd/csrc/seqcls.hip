// Sequence-classification / regression head for gfx950: pooled position, final RMSNorm + score linear + loss on the B pooled rows,
// and the backward of all of it.
//
// Replaces (reference): the tail of Idefics2ForSequenceClassification.forward -- score = nn.Linear(d, num_labels) over ALL [B, T]
// hidden states, the pad-token pooling rule, MSELoss / CrossEntropyLoss / BCEWithLogitsLoss (mean) -- and its autograd backward.
// Only the pooled row of each sample can reach the loss, so the [B, T, C] logits are never formed: one workgroup per sample reads its
// row of the PRE-norm decoder output, normalises it (fp32 statistics; the normalised row is rounded to bf16 twice, exactly as
// rmsnorm_fwd_kernel does), and takes C dot products of length d.
//
// These launches move B * d * 2 B of activations and C * d * 2 B of weights (C <= 128): microseconds, not tuned.  What matters:
// fp32 arithmetic, fixed summation orders (no atomics), bit-identical run to run.
#include "common.h"

#define SEQCLS_THREADS 256
#define SEQCLS_MAXC 128
#define SEQCLS_MAXD 8192

enum { SEQCLS_REGRESSION = 0, SEQCLS_SINGLE_LABEL = 1, SEQCLS_MULTI_LABEL = 2 };

// out[b] = (first t with ids[b, t] == pad_id) - 1  mod T   (T - 1 when the row has no pad id or starts with it); has_pad == 0: T - 1.
// One wave per row: every lane takes the first hit of its stride, the wave takes the minimum.
__global__ __launch_bounds__(64) void seqcls_pool_index_kernel(const int64_t* __restrict__ ids, int T, int64_t pad_id, int has_pad,
                                                               int* __restrict__ out) {
    const int b = blockIdx.x;
    int first = T;
    if (has_pad) {
        const int64_t* row = ids + (long)b * T;
        for (int t = threadIdx.x; t < T; t += 64)
            if (row[t] == pad_id) { first = t; break; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_xor(first, o);
        first = first < y ? first : y;
    }
    if (threadIdx.x == 0) out[b] = (first == T || first == 0) ? T - 1 : first - 1;
}

// One workgroup per sample.  labels: float [B, C] (regression, multi-label) or int32 [B] (single-label); nullptr = logits only.
// dlogits = d(gscale * mean loss) / d pooled logits, fp32 [B, C].  row_ws[b] = the sample's loss summed over its C entries;
// row_ws[B + b] = 1 where a class label is outside [0, C) (that sample adds neither loss nor gradient).
__global__ __launch_bounds__(SEQCLS_THREADS) void seqcls_head_fwd_kernel(
    const bf16_t* __restrict__ x, const int* __restrict__ pool, const bf16_t* __restrict__ norm_w, const bf16_t* __restrict__ score_w,
    const bf16_t* __restrict__ score_b, const void* __restrict__ labels, int problem, int B, int T, int d, int C, float eps, float gscale,
    int write_grad, bf16_t* __restrict__ nf, float* __restrict__ rstd_out, int* __restrict__ rows_out, float* __restrict__ pooled,
    float* __restrict__ dlogits, float* __restrict__ row_ws) {
    extern __shared__ u32x4 nfs[];                              // the normalised row, d bf16
    __shared__ float red[16];
    __shared__ float z[SEQCLS_MAXC];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int t = pool[b];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);                      // the index kernel never leaves [0, T); a foreign index stays in bounds
    const long row = (long)b * T + t;
    const bf16_t* xr = x + row * d;
    const int cpr = d >> 3;
    float ss = 0.f;
    for (int c = tid; c < cpr; c += SEQCLS_THREADS) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xr + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a0 = bf2f_lo(v[e]), a1 = bf2f_hi(v[e]);
            ss += a0 * a0 + a1 * a1;
        }
    }
    ss = block_sum(ss, red);
    const float rstd = rsqrtf(ss / (float)d + eps);
    if (tid == 0) { rstd_out[b] = rstd; rows_out[b] = (int)row; }
    bf16_t* nr = nf + (long)b * d;
    for (int c = tid; c < cpr; c += SEQCLS_THREADS) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(xr + c * 8);
        const u32x4 g = *reinterpret_cast<const u32x4*>(norm_w + c * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a0 = bf2f(f2bf(bf2f_lo(v[e]) * rstd)) * bf2f_lo(g[e]);
            const float a1 = bf2f(f2bf(bf2f_hi(v[e]) * rstd)) * bf2f_hi(g[e]);
            o[e] = pack_bf2(a0, a1);
        }
        *reinterpret_cast<u32x4*>(nr + c * 8) = o;             // kept for the backward
        nfs[c] = o;
    }
    __syncthreads();
    // score: wave wv takes classes wv, wv + 4, ... (a wave-uniform loop: wave_sum needs all 64 lanes)
    for (int c = wv; c < C; c += SEQCLS_THREADS / 64) {
        const bf16_t* wr = score_w + (long)c * d;
        float acc = 0.f;
        for (int k = lane; k < cpr; k += 64) {
            const u32x4 a = nfs[k];
            const u32x4 w = *reinterpret_cast<const u32x4*>(wr + k * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += bf2f_lo(a[e]) * bf2f_lo(w[e]) + bf2f_hi(a[e]) * bf2f_hi(w[e]);
        }
        acc = wave_sum(acc) + bf2f(score_b[c]);
        if (lane == 0) { z[c] = acc; pooled[(long)b * C + c] = acc; }
    }
    __syncthreads();
    if (!labels) return;
    const bool live = tid < C;
    const float zc = live ? z[tid] : 0.f;
    float loss_c = 0.f, g = 0.f;
    int bad = 0;
    if (problem == SEQCLS_REGRESSION) {
        const float y = live ? reinterpret_cast<const float*>(labels)[(long)b * C + tid] : 0.f;
        const float df = zc - y;
        loss_c = live ? df * df : 0.f;
        g = 2.f * df / ((float)B * (float)C);
    } else if (problem == SEQCLS_MULTI_LABEL) {
        const float y = live ? reinterpret_cast<const float*>(labels)[(long)b * C + tid] : 0.f;
        // BCE with logits, the stable form torch uses: max(z, 0) - z * y + log(1 + exp(-|z|))
        loss_c = live ? fmaxf(zc, 0.f) - zc * y + log1pf(expf(-fabsf(zc))) : 0.f;
        g = (1.f / (1.f + expf(-zc)) - y) / ((float)B * (float)C);
    } else {
        const int tgt = reinterpret_cast<const int*>(labels)[b];
        bad = (tgt < 0 || tgt >= C) ? 1 : 0;                    // block-uniform
        const float m = block_max(live ? zc : -INFINITY, red);
        const float s = block_sum(live ? expf(zc - m) : 0.f, red);
        const float lse = m + logf(s);
        loss_c = (live && !bad && tid == tgt) ? lse - zc : 0.f;
        g = bad ? 0.f : (expf(zc - lse) - (tid == tgt ? 1.f : 0.f)) / (float)B;
    }
    const float row_loss = block_sum(loss_c, red);
    if (tid == 0) { row_ws[b] = row_loss; row_ws[B + b] = bad ? 1.f : 0.f; }
    if (write_grad && live) dlogits[(long)b * C + tid] = g * gscale;
}

// loss = lscale * sum_b row_loss[b] / denom (b in index order), status[0] = number of samples with an out-of-range class label
__global__ void seqcls_finish_kernel(const float* __restrict__ row_ws, int B, float denom, float lscale, float* __restrict__ loss_out,
                                     int* __restrict__ status) {
    if (threadIdx.x != 0) return;
    float s = 0.f, bad = 0.f;
    for (int b = 0; b < B; ++b) { s += row_ws[b]; bad += row_ws[B + b]; }
    loss_out[0] = lscale * s / denom;
    status[0] = (int)(bad + 0.5f);
}

// dW[c, :] (+)= sum_b dlogits[b, c] * nf[b, :],  db[c] (+)= sum_b dlogits[b, c]   (b in index order).  One workgroup per class.
__global__ __launch_bounds__(SEQCLS_THREADS) void seqcls_dw_kernel(const float* __restrict__ dlogits, const bf16_t* __restrict__ nf,
                                                                   int B, int d, int C, bf16_t* __restrict__ dW, bf16_t* __restrict__ db,
                                                                   int accumulate) {
    const int c = blockIdx.x, cpr = d >> 3;
    for (int k = threadIdx.x; k < cpr; k += SEQCLS_THREADS) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) {
            const float g = dlogits[(long)b * C + c];
            const u32x4 a = *reinterpret_cast<const u32x4*>(nf + (long)b * d + k * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[2 * e] += g * bf2f_lo(a[e]); acc[2 * e + 1] += g * bf2f_hi(a[e]); }
        }
        bf16_t* out = dW + (long)c * d + k * 8;
        u32x4 o;
        if (accumulate) {
            const u32x4 p = *reinterpret_cast<const u32x4*>(out);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pack_bf2(acc[2 * e] + bf2f_lo(p[e]), acc[2 * e + 1] + bf2f_hi(p[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pack_bf2(acc[2 * e], acc[2 * e + 1]);
        }
        *reinterpret_cast<u32x4*>(out) = o;
    }
    if (db && threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dlogits[(long)b * C + c];
        if (accumulate) s += bf2f(db[c]);
        db[c] = f2bf(s);
    }
}

// One workgroup per sample: dnf = dlogits[b, :] . W (c in index order, kept in LDS as fp32), then the RMSNorm backward of the pooled row
//   dx = rstd * (g - xhat * mean(g * xhat)),  g = dnf * w, xhat = x * rstd;   dnorm partial[b, :] = dnf * xhat
__global__ __launch_bounds__(SEQCLS_THREADS) void seqcls_dx_kernel(const float* __restrict__ dlogits, const bf16_t* __restrict__ x,
                                                                   const int* __restrict__ rows, long n_rows,
                                                                   const float* __restrict__ rstd_in, const bf16_t* __restrict__ norm_w,
                                                                   const bf16_t* __restrict__ score_w, int d, int C,
                                                                   bf16_t* __restrict__ dx_rows, float* __restrict__ dnorm_part) {
    extern __shared__ float dnf[];                              // d floats
    __shared__ float red[16];
    __shared__ float gl[SEQCLS_MAXC];
    const int b = blockIdx.x, tid = threadIdx.x, cpr = d >> 3;
    if (tid < C) gl[tid] = dlogits[(long)b * C + tid];
    __syncthreads();
    long r = rows[b];
    r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);            // rows come from the forward kernel; a foreign index stays in bounds
    const bf16_t* xr = x + r * d;
    const float rstd = rstd_in[b];
    float dot = 0.f;
    for (int k = tid; k < cpr; k += SEQCLS_THREADS) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            const float g = gl[c];
            const u32x4 w = *reinterpret_cast<const u32x4*>(score_w + (long)c * d + k * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[2 * e] += g * bf2f_lo(w[e]); acc[2 * e + 1] += g * bf2f_hi(w[e]); }
        }
        const u32x4 vx = *reinterpret_cast<const u32x4*>(xr + k * 8);
        const u32x4 vw = *reinterpret_cast<const u32x4*>(norm_w + k * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x0 = bf2f_lo(vx[e]) * rstd, x1 = bf2f_hi(vx[e]) * rstd;
            dot += acc[2 * e] * bf2f_lo(vw[e]) * x0 + acc[2 * e + 1] * bf2f_hi(vw[e]) * x1;
            if (dnorm_part) {
                dnorm_part[(long)b * d + k * 8 + 2 * e] = acc[2 * e] * x0;
                dnorm_part[(long)b * d + k * 8 + 2 * e + 1] = acc[2 * e + 1] * x1;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) dnf[k * 8 + e] = acc[e];   // read back by the same thread below
    }
    dot = block_sum(dot, red) / (float)d;
    for (int k = tid; k < cpr; k += SEQCLS_THREADS) {
        const u32x4 vx = *reinterpret_cast<const u32x4*>(xr + k * 8);
        const u32x4 vw = *reinterpret_cast<const u32x4*>(norm_w + k * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x0 = bf2f_lo(vx[e]) * rstd, x1 = bf2f_hi(vx[e]) * rstd;
            const float a0 = rstd * (dnf[k * 8 + 2 * e] * bf2f_lo(vw[e]) - x0 * dot);
            const float a1 = rstd * (dnf[k * 8 + 2 * e + 1] * bf2f_hi(vw[e]) - x1 * dot);
            o[e] = pack_bf2(a0, a1);
        }
        *reinterpret_cast<u32x4*>(dx_rows + (long)b * d + k * 8) = o;
    }
}

// dnorm[j] (+)= sum_b part[b, j]   (b in index order)
__global__ __launch_bounds__(SEQCLS_THREADS) void seqcls_dnorm_kernel(const float* __restrict__ part, int B, int d, bf16_t* __restrict__ dnorm,
                                                                      int accumulate) {
    const int j = blockIdx.x * SEQCLS_THREADS + threadIdx.x;
    if (j >= d) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(long)b * d + j];
    if (accumulate) s += bf2f(dnorm[j]);
    dnorm[j] = f2bf(s);
}

static inline bool seqcls_shape_ok(int B, int d, int C) {
    return B >= 1 && C >= 1 && C <= SEQCLS_MAXC && d >= 8 && d % 8 == 0 && d <= SEQCLS_MAXD;
}

extern "C" {

int mantis_seqcls_pool_index(const int64_t* input_ids, int B, int T, int64_t pad_id, int has_pad, int32_t* out, void* stream) {
    if (B < 1 || T < 1) return MANTIS_EINVAL;
    MANTIS_LAUNCH(seqcls_pool_index_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, input_ids, T, pad_id, has_pad, out);
    return mantis_check_launch();
}

int mantis_seqcls_head_fwd(const void* x, const int32_t* pool, const void* norm_weight, const void* score_weight, const void* score_bias,
                           const void* labels, int problem_type, int B, int T, int d, int C, float eps, float grad_scale,
                           float loss_scale, int write_grad, void* nf, float* rstd, int32_t* rows, float* pooled_logits, float* dlogits,
                           float* row_ws, float* loss_out, int32_t* status_out, void* stream) {
    if (!seqcls_shape_ok(B, d, C) || T < 1 || problem_type < 0 || problem_type > 2) return MANTIS_EINVAL;
    if ((long)B * T >= (1L << 31)) return MANTIS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MANTIS_LAUNCH(seqcls_head_fwd_kernel, dim3(B), dim3(SEQCLS_THREADS), (size_t)d * 2, s, (const bf16_t*)x, pool,
                  (const bf16_t*)norm_weight, (const bf16_t*)score_weight, (const bf16_t*)score_bias, labels, problem_type, B, T, d, C, eps,
                  grad_scale, write_grad, (bf16_t*)nf, rstd, rows, pooled_logits, dlogits, row_ws);
    if (labels) {
        const float denom = problem_type == SEQCLS_SINGLE_LABEL ? (float)B : (float)B * (float)C;
        MANTIS_LAUNCH(seqcls_finish_kernel, dim3(1), dim3(64), 0, s, row_ws, B, denom, loss_scale, loss_out, status_out);
    }
    return mantis_check_launch();
}

int mantis_seqcls_head_bwd(const float* dlogits, const void* nf, const void* x, const int32_t* rows, int64_t n_rows, const float* rstd,
                           const void* norm_weight, const void* score_weight, int B, int d, int C, void* grad_score_weight,
                           void* grad_score_bias, void* grad_norm_weight, int accumulate, void* dx_rows, float* workspace, void* stream) {
    if (!seqcls_shape_ok(B, d, C) || n_rows < 1) return MANTIS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (grad_score_weight)
        MANTIS_LAUNCH(seqcls_dw_kernel, dim3(C), dim3(SEQCLS_THREADS), 0, s, dlogits, (const bf16_t*)nf, B, d, C, (bf16_t*)grad_score_weight,
                      (bf16_t*)grad_score_bias, accumulate);
    MANTIS_LAUNCH(seqcls_dx_kernel, dim3(B), dim3(SEQCLS_THREADS), (size_t)d * sizeof(float), s, dlogits, (const bf16_t*)x, rows,
                  (long)n_rows, rstd, (const bf16_t*)norm_weight, (const bf16_t*)score_weight, d, C, (bf16_t*)dx_rows,
                  grad_norm_weight ? workspace : nullptr);
    if (grad_norm_weight)
        MANTIS_LAUNCH(seqcls_dnorm_kernel, dim3(cdiv(d, SEQCLS_THREADS)), dim3(SEQCLS_THREADS), 0, s, workspace, B, d,
                      (bf16_t*)grad_norm_weight, accumulate);
    return mantis_check_launch();
}

}  // extern "C"
