"""-m gpu: per-row / per-element parity of the row-wise kernels against float64, with the a-priori criteria of tests/local_error.py (second
half) on the inputs of tests/rowwise_cases.py.  tests/test_local_error_checker.py proves on the CPU that the fp32 oracle passes every
criterion on these very inputs and that seeded faults are rejected.  Each test prints `RATIO ...`: the worst error / bound and the share of
differing elements, collected in profiles/rowwise_error_ratios.md.

Kernel, template instantiation or branch -> the test id that runs it
  norm.hip
    rmsnorm_fwd_regs_kernel<NCH>, NCH = 1..8, 10, 12, 16       test_rmsnorm_fwd[regs{NCH}_d{512 NCH}]
      its `while (true)` re-load loop (rows > 8192)            test_rmsnorm_fwd[regs1_reload_loop_8197x512]
    rmsnorm_fwd_kernel (generic)                               test_rmsnorm_fwd[generic_d8 | _d520 | _d768 | _d4608]
      weights not 16-B aligned                                 test_rmsnorm_fwd[generic_d512_w_plus_8_bytes]
      its row loop (rows > 4096)                               test_rmsnorm_fwd[generic_row_loop_4101x520]
    rstd_out == nullptr, amax_parts (dirty buffer) both ways   every test_rmsnorm_fwd / test_rmsnorm_bwd case
    rmsnorm_bwd_kernel<2>                                      test_rmsnorm_bwd[bwd2_d8], [bwd2_d1024]
      its row loop, P = 512                                    the 4101-row entries of the two
    rmsnorm_bwd_kernel<8>                                      test_rmsnorm_bwd[bwd8_d1032], [bwd8_d3584], [bwd8_d4088]
    rmsnorm_bwd_kernel<16>                                     test_rmsnorm_bwd[bwd16_d4104], [bwd16_d8192]
    rmsnorm_bwd_d4096_kernel<false> / <true>                   test_rmsnorm_bwd[d4096_d4096]: rows 1, 3, 7, 121, 1025, 1027 leave slot 1 past the
                                                               end (rstd = 0); 1025, 1027 have niter > 1; 1027 an odd tail; <true> = the amax run
      dres == nullptr, grad_weight == nullptr, accumulate 0/1  dealt round-robin over the rows of every kernel (rowwise_cases.BWD_OPTIONS)
    reduce_partials_kernel  P = 1 (tail only), 16, 129 (unrolled body + tail), 512      rows 1 / 7, 121, 1025, 4101 of test_rmsnorm_bwd
    every row counted once                                     test_rmsnorm_bwd_one_hot_witness[4101x512], [1027x4096]
    layernorm_fwd_kernel                                       test_layernorm[d8 | 768 | 1024 | 1152 | 1280 | 8200]; row loop: d8 (4101 rows)
  ce.hip
    ce_count_kernel, ce_fwd_bwd_kernel, ce_finish_kernel       test_ce[V-kind]; V > 8192: the online (max, sum) rescale; partial last chunk: V = 1, 7,
                                                               9, 8193, 16389, 32002; ld > pad8(V), write_grad = 0, targets 0 / V - 1 / last chunk /
                                                               ignored / >= V in every case
      no usable row (0 / 0 -> NaN)                             test_ce_every_row_ignored
      a chunk of nothing but -inf                              test_ce_neg_inf_chunk[300], [16389]
  rope.hip
    rope_apply_kernel<1>, <-1>                                 test_rope_apply[hd-nheads-R]; cph = 1, 2, 5, 8; grid-stride loop: [128-64-1100]
    rope_table_kernel                                          test_rope_table[8 | 40 | 64]
    rope_table_sections_kernel                                 test_rope_table_sections[S-half]
  act.hip   colsum_partial_kernel, reduce_partials_kernel2     test_colsum[M]: ragged row blocks, the cap of 64 blocks (8193), ld > N, N around 64
  optim.hip sumsq_partial_kernel, sumsq_finish_kernel          test_sumsq[n]; the grid-stride loop: n = 8 (8192 x 256 + 3)
            sumsq_ranges_kernel                                test_sumsq_ranges
            sum_f32_kernel                                     test_sum_f32[n]
            clip_scale_kernel                                  test_clip_scale"""
import pytest

from tests import rowwise_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def K():
    import mantis_amd.hip_ops as k
    return k


def _report(name, stat):
    print(f"RATIO {name}: " + ", ".join(f"{k} {v:.4g}" for k, v in stat.items()))


@pytest.mark.parametrize("d,rows,w_off", [c[1:] for c in C.RMS_FWD_CASES], ids=[c[0] for c in C.RMS_FWD_CASES])
def test_rmsnorm_fwd(d, rows, w_off, request):
    _report(request.node.name, C.run_rmsnorm_fwd(K(), DEV, d, rows, w_off))


@pytest.mark.parametrize("d,sub", [c[1:] for c in C.RMS_BWD_CASES], ids=[c[0] for c in C.RMS_BWD_CASES])
def test_rmsnorm_bwd(d, sub, request):
    _report(request.node.name, C.run_rmsnorm_bwd(K(), DEV, d, sub))


@pytest.mark.parametrize("rows,d", C.RMS_BWD_WITNESS, ids=[f"{r}x{d}" for r, d in C.RMS_BWD_WITNESS])
def test_rmsnorm_bwd_one_hot_witness(rows, d):
    C.run_rmsnorm_bwd_witness(K(), DEV, rows, d)


@pytest.mark.parametrize("d,rows", C.LN_CASES, ids=[f"d{c[0]}" for c in C.LN_CASES])
def test_layernorm(d, rows, request):
    _report(request.node.name, C.run_layernorm(K(), DEV, d, rows))


@pytest.mark.parametrize("kind", C.CE_KINDS)
@pytest.mark.parametrize("V", C.CE_V)
def test_ce(V, kind, request):
    _report(request.node.name, C.run_ce(K(), DEV, V, kind))


def test_ce_every_row_ignored():
    C.run_ce_all_ignored(K(), DEV)


@pytest.mark.parametrize("V", C.CE_NEG_INF_V)
def test_ce_neg_inf_chunk(V, request):
    _report(request.node.name, C.run_ce_neg_inf(K(), DEV, V))


@pytest.mark.parametrize("hd,nheads,R_", C.ROPE_CASES)
def test_rope_apply(hd, nheads, R_, request):
    _report(request.node.name, C.run_rope_apply(K(), DEV, hd, nheads, R_))


@pytest.mark.parametrize("half", C.ROPE_TABLE_HALF)
def test_rope_table(half, request):
    _report(request.node.name, C.run_rope_table(K(), DEV, half))


@pytest.mark.parametrize("half", C.ROPE_TABLE_HALF)
@pytest.mark.parametrize("S", [3, 2])
def test_rope_table_sections(S, half, request):
    _report(request.node.name, C.run_rope_table_sections(K(), DEV, S, half))


@pytest.mark.parametrize("M", C.COLSUM_M)
def test_colsum(M, request):
    _report(request.node.name, C.run_colsum(K(), DEV, M))


@pytest.mark.parametrize("n", C.SUMSQ_N)
def test_sumsq(n, request):
    _report(request.node.name, C.run_sumsq(K(), DEV, n))


def test_sumsq_ranges(request):
    _report(request.node.name, C.run_sumsq_ranges(K(), DEV))


@pytest.mark.parametrize("n", C.SUM_F32_N)
def test_sum_f32(n, request):
    _report(request.node.name, C.run_sum_f32(K(), DEV, n))


def test_clip_scale(request):
    _report(request.node.name, C.run_clip_scale(K(), DEV))
