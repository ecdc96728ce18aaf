// Flag bits and tile constants of the bf16 GEMM entry points (include/mantis_hip.h): plain defines, shared by the host-only planner
// (gemm_plan.h) and the kernels (gemm_ring.h)
#pragma once
#include "../../include/mantis_hip.h"  // the MANTIS_* return codes (plain C: this header and gemm_plan.h stay host-only)
#define BK 64
#define EPI_BIAS 1
#define EPI_ACT_SHIFT 1
#define EPI_ACT_MASK (7 << EPI_ACT_SHIFT)  // 0 none, 1 gelu(erf), 2 gelu(tanh), 3 quick_gelu
#define EPI_RESIDUAL 16
#define EPI_ACCUM 32
#define EPI_SWIGLU_BWD 64                   // C = [dgate | dup][M, 2N] from dact = A.B^T and residual = [gate | up][M, 2N] (ring kernel)
#define EPI_SUMSQ 128                        // ring16 kernels, through mantis_gemm_bf16_nt_sumsq: tile_sumsq[tile] = sum of squares of the stored tile
#define EPI_VARIANT_SHIFT 8                 // bits 8-11: tile variant (0 = auto)
#define EPI_VARIANT_MASK (15 << EPI_VARIANT_SHIFT)
#define EPI_A_KMAJOR 4096                   // A given as [K, M] (element (m,k) at A[k*lda + m])
#define EPI_B_KMAJOR 8192                   // B given as [K, N]
#define EPI_CUS_SHIFT 16                    // bits 16-27: CU budget this launch is planned for (0 = the default: MANTIS_GEMM_CUS or the whole device)
#define EPI_CUS_MASK (0xFFF << EPI_CUS_SHIFT)
#define EPI_SHARED_GPU 32768                 // the launch shares the GPU with long-running kernels of other queues (RCCL collectives under data parallelism): the
                                            // 176-row kernel then runs one tile per workgroup -- a persistent workgroup that has to wait for a CU someone else
                                            // holds would walk its whole static tile list late (the hardware's own dispatch degrades gracefully instead)
#define EPI_SK_INKERNEL 16384                // ring16 kernels: remainder tiles reduced by their last arriver inside the GEMM kernel (round 4) instead of by
                                            // gemm_ring16_finish_kernel -- same results bit for bit; tests and A/B measurements
#define PAIR_NONE 0                         // two-column forward fusions of the ring16 / 176-row epilogue (see ring16_epilogue)
#define PAIR_SWIGLU 1
#define PAIR_ROPE 2
