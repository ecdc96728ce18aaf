"""GPU: the records the instrumented wrappers of mantis_amd/hip_ops.py leave in LaunchContext.timer (bench.py reads them by position: x[0]..x[4],
then x[5] and x[6] where len(x) > 6).  One call per wrapper at the smallest shape that reaches its branch; every expected record is written out
as literals (kernel name, algorithmic flops and bytes, tag) from the formulas the wrappers carried before they shared one timer bracket.  The
bf16 GEMM family leaves 7-tuples (.., tag, stream), the fp8 and skinny launches 5-tuples; a declined fused launch leaves only its fallback's."""
import json

import pytest
import torch

from tests import gpu_checks
from tests.golden import make_gemm_plan as mk

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _k():
    from mantis_amd import hip_ops
    return hip_ops


def bf(*shape):
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    return (torch.randn(*shape, generator=g) * 0.25).to(torch.bfloat16).to(DEV)


def records(fn, **ctx):
    """The timer records of fn() under LaunchContext(timer=[], **ctx), each checked for its shape: two events with a positive elapsed time,
    and the current stream where the record carries one."""
    k = _k()
    timer = []
    with k.launch_context(k.LaunchContext(timer=timer, **ctx)):
        fn()
        stream = k._stream()
    torch.cuda.synchronize()
    out = []
    for r in timer:
        assert type(r) is tuple and len(r) in (5, 7), r
        assert r[3].elapsed_time(r[4]) > 0.0, r
        if len(r) == 7:
            assert r[6] == stream, r
        out.append(r[:3] + r[5:6])
    return out


class Collector:
    """Stands for optim.FusedAdamW.begin_fold(): slots of one device fp32 buffer, handed out in order."""

    def __init__(self, floats):
        self.buf = torch.zeros(floats, dtype=torch.float32, device=DEV)
        self.used, self.log = 0, []

    def take(self, grad, tiles):
        assert self.used + tiles <= self.buf.numel()
        slot = self.buf.data_ptr() + 4 * self.used
        self.used += tiles
        self.log.append(("take", tuple(grad.shape), tiles))
        return slot

    def give_back(self, grad, tiles):
        self.used -= tiles
        self.log.append(("give_back", tuple(grad.shape), tiles))


def test_gemm_nt_record():
    k = _k()
    a, b, bias, res = bf(300, 72), bf(200, 72), bf(200), bf(300, 200)
    assert records(lambda: k.gemm_nt(a, b, bias=bias, residual=res)) == [("gemm_nt_kernel", 8640000.0, 312000.0, (300, 200, 72, "NT", "bias+res"))]


def test_fused_forward_records_and_declined_shapes():
    k = _k()
    assert k.FUSE_FWD_EPILOGUES
    x, w_gu = bf(333, 64), bf(256, 64)                       # I = 128
    assert records(lambda: k.linear_gu_swiglu(x, w_gu)) == [("gemm_nt_kernel", 10911744.0, 331136.0, (333, 256, 64, "NT", "swiglu"))]
    w_qkv, bias = bf(512, 64), bf(512)                       # 2 query heads, 1 key / value head of 128
    cos, sin = bf(333, 64), bf(333, 64)
    assert records(lambda: k.linear_qkv_rope(x, w_qkv, bias, cos, sin, 3, 128)) == [
        ("gemm_nt_kernel", 21823488.0, 534400.0, (333, 512, 64, "NT", "rope+bias"))]
    # declined: N % 256 != 0 never reaches the fused entry; variant 12 does and comes back unsupported (csrc/gemm_plan.h, gemm_fused_choose).
    # Either way exactly the fallback's record (the pointwise kernel behind it leaves none)
    w384 = bf(384, 64)
    assert records(lambda: k.linear_gu_swiglu(x, w384)) == [("gemm_nt_kernel", 16367616.0, 347520.0, (333, 384, 64, "NT", "-"))]
    assert records(lambda: k.linear_gu_swiglu(x, w_gu, variant=12)) == [("gemm_nt_kernel", 10911744.0, 245888.0, (333, 256, 64, "NT", "-"))]
    assert records(lambda: k.linear_qkv_rope(x, w_qkv, bias, cos, sin, 3, 128, variant=12)) == [
        ("gemm_nt_kernel", 21823488.0, 449152.0, (333, 512, 64, "NT", "bias"))]


def test_linear_dx_swiglu_record():
    k = _k()
    dy, w_down, gu = bf(333, 64), bf(64, 176), bf(333, 352)
    assert records(lambda: k.linear_dx_swiglu(dy, w_down, gu)) == [("gemm_nt_kernel", 7501824.0, 534016.0, (333, 176, 64, "NN", "swiglu_bwd"))]


def test_fp8_and_skinny_records():
    k = _k()
    assert min(gpu_checks.FP8_GEMM_CASES, key=lambda c: c[0] * c[1] * c[2]) == (77, 40, 16, 1, "plain", 1)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    assert records(lambda: k.gemm_fp8_nt(u8(77, 16), one, u8(40, 16), one, k.FP8_E5M2, variant=1)) == [("gemm_fp8_nt_kernel", 98560.0, 8032.0)]
    gu = bf(300, 512)                                         # M = 300, d = 112, I = 256
    assert records(lambda: k.gemm_fp8_dx_swiglu(u8(300, 112), one, u8(256, 112), one, gu, k.FP8_E5M2)) == [
        ("gemm_fp8_nt_kernel", 17203200.0, 676672.0)]
    x, w = bf(3, 64), bf(64, 64)
    assert records(lambda: k.linear_skinny(x, w)) == [("linear_skinny_kernel", 24576.0, 8960.0)]


def test_weight_gradient_records():
    k = _k()
    with open(mk.FIXTURE) as f:
        table = json.load(f)["default"]
    # the smallest row of the planner's table whose weight-gradient (both operands K-major, with the sum of squares) entry is a ring16
    # kernel, 13 or 14, with N % 256 == 0: grad_w [384, 28672] over 64 rows
    rows = [(M * N * int(K), M, N, int(K)) for M, N in (map(int, mn.split(",")) for mn in table["rows"]) if N % 256 == 0
            for K in table["rows"][f"{M},{N}"] if mk.row(table, M, N, int(K), 0)["entries"][7] in "de"]
    assert min(rows)[1:] == (384, 28672, 64)
    dy, x, g = bf(64, 384), bf(64, 28672), torch.zeros(384, 28672, dtype=torch.bfloat16, device=DEV)
    assert records(lambda: k.linear_dw(dy, x, g, False)) == [("gemm_nt_kernel", 1409286144.0, 25739264.0, (384, 28672, 64, "TN", "-"))]
    col = Collector(224)
    assert records(lambda: k.linear_dw(dy, x, g, False), dw_sumsq=col) == [
        ("gemm_nt_kernel", 1409286144.0, 25739264.0, (384, 28672, 64, "TN", "sumsq"))]
    assert col.log == [("take", (384, 28672), 224)]
    assert records(lambda: k.linear_dw(dy, x, g, True), dw_sumsq=Collector(224)) == [
        ("gemm_nt_kernel", 1409286144.0, 47759360.0, (384, 28672, 64, "TN", "sumsq+acc"))]
    # the table's smallest paired win: two dW of [512, 256] over 512 rows (tests/test_gemm_plan_gpu.py)
    dy1, x1, dy2, x2 = bf(512, 512), bf(512, 256), bf(513, 512)[:512], bf(514, 256)[:512]
    g1, g2 = (torch.zeros(512, 256, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    assert records(lambda: k.linear_dw_pair(dy1, x1, g1, dy2, x2, g2, False)) == [
        ("gemm_nt_kernel", 268435456.0, 2097152.0, (512, 256, 512, "TN", "paired with 512x256x512"))]
    col = Collector(4)
    assert records(lambda: k.linear_dw_pair(dy1, x1, g1, dy2, x2, g2, True), dw_sumsq=col) == [
        ("gemm_nt_kernel", 268435456.0, 2621440.0, (512, 256, 512, "TN", "paired with 512x256x512+sumsq+acc"))]
    assert col.log == [("take", (512, 256), 2), ("take", (512, 256), 2)]
