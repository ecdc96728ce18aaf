"""-m gpu: localised-error parity of the GEMM, pointwise and attention kernels (tests/local_error.py; the checker itself is proven on the CPU
by tests/test_local_error_checker.py).  GEMM family and attention forward: every element inside the a-priori bound of the operator's
documented rounding chain (pass: worst ratio <= 1, printed per test; collected in profiles/local_error_ratios.md).  Pointwise kernels: every
bf16 bit pattern within 1 ulp of the correctly rounded fp64 value, or inside the fp32 floor c . 2^-24 . |x| of the cancelling tails with
c = 2 x the worst of the oracle's own fp32 evaluation (measured here on the CPU, never from the kernel).  Attention gradients: every
(row, head) within 3 x the worst (row, head) error of the CPU emulation of the kernels' rounding chain."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import llava_ref
from tests import local_error as LE
from tests.gpu_checks import _kmask, _segment_bounds, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def K():
    import mantis_amd.hip_ops as k
    return k


def _declined(e):
    from mantis_amd._lib import MantisHipError
    return isinstance(e, MantisHipError) and "rc=-2" in str(e)


# ------------------------------------------------------------------------------------------------------------- GEMM family
GEMM_SHAPES = [(77, 40, 8), (300, 200, 72), (257, 388, 1152), (353, 300, 200), (529, 776, 136), (1024, 302, 256)]
VARIANTS = [0, 1, 2, 12, 13, 14, 15]
EPILOGUES = ["plain", "bias", "res", "bias+res", "acc"]
N_ROUNDINGS = {"plain": 1, "bias": 1, "res": 2, "bias+res": 2, "acc": 2}


def _gemm_operands(M, N, K_, epi):
    a, b = rnd(M, K_, seed=1), rnd(N, K_, seed=2, scale=0.1)
    bias = rnd(N, seed=3) if "bias" in epi else None
    res = rnd(M, N, seed=4) if "res" in epi else None
    ldc = (N + 7) // 8 * 8 + 8
    c0 = rnd(M, ldc, seed=7) if epi == "acc" else None
    added = tuple(t for t in (None if bias is None else bias[None, :], res, None if c0 is None else c0[:, :N]) if t is not None)
    ref, _, bound = LE.gemm_bound(a, b, n_roundings=N_ROUNDINGS[epi], K=K_, added=added)
    return a, b, bias, res, c0, ref, bound


def _kmajor(x):
    """[R, K] -> the K-major copy [K, R] on the device, as a column window of a buffer whose row stride is a multiple of 8 (the way dW and
    dX consume activations as stored)"""
    buf = torch.zeros(x.shape[1], (x.shape[0] + 7) // 8 * 8 + 8, dtype=x.dtype)
    buf[:, : x.shape[0]] = x.t()
    return buf.to(DEV)[:, : x.shape[0]]


def _run_gemm(k, ad, bd, bias, res, c0, N, **kw):
    dv = lambda t: None if t is None else t.to(DEV)
    if c0 is None:
        return k.gemm_nt(ad, bd, bias=dv(bias), residual=dv(res), **kw)
    c = c0.to(DEV)
    k.gemm_nt(ad, bd, out=c[:, :N], accumulate=True, **kw)
    assert torch.equal(c[:, N:].cpu(), c0[:, N:]), "gemm wrote outside its N columns"
    return c[:, :N]


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_elementwise_bound(M, N, K_, epi):
    """every variant x operand layout the kernels accept, at shapes that own a ragged M tile, a ragged N tile (N % 4 != 0 or N % 16 != 0),
    a K tail, a single K-step and the 176 / 352 row seams"""
    k = K()
    a, b, bias, res, c0, ref, bound = _gemm_operands(M, N, K_, epi)
    lay = {(akm, bkm): (_kmajor(a) if akm else a.to(DEV), _kmajor(b) if bkm else b.to(DEV))
           for akm in (False, True) for bkm in (False, True)}
    worst, ran = 0.0, []
    for v in VARIANTS:
        for (akm, bkm), (ad, bd) in lay.items():
            try:
                out = _run_gemm(k, ad, bd, bias, res, c0, N, variant=v, a_kmajor=akm, b_kmajor=bkm)
            except Exception as e:          # a (variant, layout, alignment) the kernel declines
                if _declined(e):
                    continue
                raise
            worst = max(worst, LE.assert_elementwise(out, ref, bound, f"gemm {M}x{N}x{K_} {epi} v{v} akm={akm} bkm={bkm}"))
            ran.append((v, akm, bkm))
    # the only pair mantis_gemm_bf16_nt declines at these shapes (K % 8 == 0, strides % 8 == 0): the 176-row kernel with a K-major A
    want = [(v, akm, bkm) for v in VARIANTS for (akm, bkm) in lay if not (v == 15 and akm)]
    assert ran == want, f"launches declined: {sorted(set(want) - set(ran))}"
    print(f"RATIO gemm {M}x{N}x{K_} {epi}: worst {worst:.3f} over {len(ran)} (variant, layout) launches")


@pytest.mark.parametrize("variant", [0, 12, 13, 14, 15])
@pytest.mark.parametrize("K_", [1024, 2048])
def test_gemm_ksplit_remainder_elementwise(variant, K_, ksplit_ref):
    """the K-split remainder path, ALL rows against the bound.  2000 x 2100 is 8 x 9 = 72 tiles of 256 x 256, one incomplete round.  At
    K = 2048 the library's own plan (mantis_gemm_remainder_plan, the arithmetic the ring launch runs) splits every tile in S > 1 parts:
    asserted.  K = 1024, the smallest shape of check_gemm_ksplit_deterministic, has 16 K-steps, which the plan's cost model leaves whole
    (S = 1) -- it stays as the unsplit twin of the same grid.  Variant 15 (176-row tiles) has no K split (gemm.hip launches it without a
    workspace) and is held to the same bound on the same shapes."""
    import ctypes
    import numpy as np
    k = K()
    head = np.zeros(8 + 4 * 4096, dtype=np.int32)
    assert k._L.mantis_gemm_remainder_plan(2000, 2100, K_, 0, head.ctypes.data_as(ctypes.c_void_p), head.size) >= 8
    rem, S = int(head[2]), int(head[3])
    assert (S > 1 and rem == 72) if K_ == 2048 else S == 1, f"K = {K_}: remainder {rem}, S = {S}"
    a, b, ref, bound = ksplit_ref[K_]
    out = k.gemm_nt(a.to(DEV), b.to(DEV), variant=variant)
    worst = LE.assert_elementwise(out, ref, bound, f"gemm k-split 2000x2100x{K_} v{variant}")
    print(f"RATIO gemm k-split 2000x2100x{K_} v{variant} (S = {S}): worst {worst:.3f}")


@pytest.fixture(scope="module")
def ksplit_ref():
    refs = {}
    for K_ in (1024, 2048):
        a, b = rnd(2000, K_, seed=31), rnd(2100, K_, seed=32, scale=0.1)
        ref, _, bound = LE.gemm_bound(a, b, n_roundings=1, K=K_)
        refs[K_] = (a, b, ref, bound)
    return refs


@pytest.mark.parametrize("epi", ["plain", "bias+res", "acc"])
def test_gemm_persistent_176_elementwise(epi):
    """the persistent 176-row launch (8 CUs: 45 tiles, ~6 per workgroup) against the bound, both B layouts"""
    k = K()
    M, N, K_ = 1409, 1032, 520
    a, b, bias, res, c0, ref, bound = _gemm_operands(M, N, K_, epi)
    worst = 0.0
    for bkm in (False, True):
        out = _run_gemm(k, a.to(DEV), _kmajor(b) if bkm else b.to(DEV), bias, res, c0, N, variant=15, b_kmajor=bkm, cus=8)
        worst = max(worst, LE.assert_elementwise(out, ref, bound, f"persistent ring176 {epi} bkm={bkm}"))
    print(f"RATIO gemm persistent176 1409x1032x520 {epi}: worst {worst:.3f}")


@pytest.mark.parametrize("N,K_", [(300, 64), (352, 64), (64, 176), (6144, 4096)])
def test_linear_skinny_elementwise(N, K_):
    k = K()
    Np = k.pad8(N)
    w, bias = rnd(Np, K_, seed=N + K_, scale=0.05), rnd(Np, seed=1, scale=0.5)
    worst = 0.0
    for M in (1, 3, 16):
        x, res = rnd(M, K_, seed=M), rnd(M, Np, seed=M + 100)
        ref, _, bound = LE.gemm_bound(x, w[:N], n_roundings=1, K=K_)
        y = k.linear_skinny(x.to(DEV), w.to(DEV), n_valid=N, ldc=Np)
        worst = max(worst, LE.assert_elementwise(y[:, :N], ref, bound, f"skinny {M}x{N}x{K_}"))
        ref, _, bound = LE.gemm_bound(x, w[:N], n_roundings=2, K=K_, added=(bias[None, :N], res[:, :N]))
        y = k.linear_skinny(x.to(DEV), w.to(DEV), bias=bias.to(DEV), residual=res.to(DEV), n_valid=N, ldc=Np)
        worst = max(worst, LE.assert_elementwise(y[:, :N], ref, bound, f"skinny+bias+res {M}x{N}x{K_}"))
    print(f"RATIO linear_skinny {N}x{K_}: worst {worst:.3f}")


@pytest.mark.parametrize("M1,N1,M2,N2,Kd", [(512, 512, 1024, 256, 264), (300, 512, 520, 256, 1000), (2048, 2048, 4096, 4096, 136)])
def test_linear_dw_pair_elementwise(M1, N1, M2, N2, Kd):
    """the paired weight-gradient launch (mantis_gemm_bf16_tn_pair) at the no-split pairs: both outputs, with and without accumulation"""
    k = K()
    dy1, x1 = rnd(Kd, (M1 + 47) // 8 * 8, seed=91, scale=0.5), rnd(Kd, N1, seed=92, scale=0.5)
    dy2, x2 = rnd(Kd, (M2 + 7) // 8 * 8, seed=93, scale=0.5), rnd(Kd, N2, seed=94, scale=0.5)
    worst = 0.0
    for acc in (False, True):
        c1, c2 = rnd(M1, N1, seed=95), rnd(M2, N2, seed=96)
        g1, g2 = c1.clone().to(DEV), c2.clone().to(DEV)
        k.linear_dw_pair(dy1.to(DEV), x1.to(DEV), g1, dy2.to(DEV), x2.to(DEV), g2, acc)
        for g, dy, x, c, M in ((g1, dy1, x1, c1, M1), (g2, dy2, x2, c2, M2)):
            ref, _, bound = LE.gemm_bound(dy[:, :M].t(), x.t(), n_roundings=2 if acc else 1, K=Kd, added=c if acc else None)
            worst = max(worst, LE.assert_elementwise(g, ref, bound, f"dw pair {tuple(g.shape)} K={Kd} acc={acc}"))
    print(f"RATIO linear_dw_pair {M1}x{N1}+{M2}x{N2} K={Kd}: worst {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- pointwise
def _all_finite_bf16():
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    return x[torch.isfinite(x.float())]                 # 65280 patterns: both zeros, subnormals, every normal value


# the pointwise entry points take element counts / row widths that are multiples of 8 (16-byte accesses) and decline the rest: 263 x 248 =
# 65224 patterns in one call, the other 56 in a second (one short row).  act_fwd / act_bwd are flat over numel() / 8, so for them the two
# calls only give two element counts (one of them no multiple of the block); the 2-D shape matters for swiglu alone, whose gate | up rows
# have a stride.
ROWS, COLS = 263, 248


def _sig(x):
    return torch.sigmoid(x)                             # fp64, evaluated without overflow on either side


_K_TANH, _C_TANH = (2.0 / torch.pi) ** 0.5, 0.044715
ACT64 = {
    "gelu": lambda x: 0.5 * x * torch.erfc(-x / 2 ** 0.5),
    "gelu_pytorch_tanh": lambda x: x * _sig(2.0 * _K_TANH * (x + _C_TANH * x ** 3)),                        # 0.5 x (1 + tanh y) = x sigmoid(2 y)
    "quick_gelu": lambda x: x * _sig(1.702 * x),
    "silu": lambda x: x * _sig(x),
}


def _act_bwd64(x, kind):
    """closed-form derivatives; s (1 - s) is written s . sigmoid(-z) so that neither tail cancels"""
    if kind == "gelu":
        return 0.5 * torch.erfc(-x / 2 ** 0.5) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5
    if kind == "gelu_pytorch_tanh":
        z = 2.0 * _K_TANH * (x + _C_TANH * x ** 3)
        return _sig(z) + x * _sig(z) * _sig(-z) * 2.0 * _K_TANH * (1.0 + 3.0 * _C_TANH * x * x)
    a = 1.702 if kind == "quick_gelu" else 1.0
    return _sig(a * x) + a * x * _sig(a * x) * _sig(-a * x)


def _floor_c(err32, scale, ref64):
    """c = 2 x the worst |fp32 oracle - fp64| / (2^-24 . scale), over the patterns where the fp32 error is visible at bf16 resolution
    (more than 2^-9 |ref|: a quarter of an ulp at least) -- elsewhere the 1-ulp criterion decides and the floor has nothing to cover, and
    measuring there would let the patterns near x = 0 (error 2^-25 against a vanishing scale) set it.  0 when there is no such pattern."""
    ok = torch.isfinite(err32) & (scale > 0) & torch.isfinite(scale) & (err32 > 2.0 ** -9 * ref64.abs())
    return 2.0 * float((err32[ok] / (LE.U_F32 * scale[ok])).max()) if bool(ok.any()) else 0.0


RANGE_F32 = 2.0 ** -127      # 1 / (1 + e^-z) is exactly 0 in fp32 once e^-z overflows (z < -88.7): results under scale . 2^-127 may come out as 0


def _assert_pointwise(out, ref64, c, scale, what, x):
    """every pattern within 1 ulp of the correctly rounded value or inside the floor (c . 2^-24 + 2^-127) . scale.  -> (max ulp outside the
    floor, worst floor use, number of patterns that pass only through the 2^-127 range term).  The range term is an allowance beyond the
    c . 2^-24 form, so its use is pinned to its mechanism: a pattern that needs it must have come out as exactly 0."""
    floor = (c * LE.U_F32 + RANGE_F32) * scale
    ulp = LE.ulp_distance_bf16(out, ref64)
    err = (LE.f64(out) - ref64).abs()
    bad = (ulp > 1) & ~(err <= floor)
    need = torch.where(ulp > 1, err / floor.clamp_min(1e-300), torch.zeros_like(err))
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} patterns neither within 1 ulp nor inside the fp32 floor; first inputs "
                                 f"{x.flatten()[bad.flatten()][:6].tolist()} -> {out.flatten()[bad.flatten()][:6].tolist()} "
                                 f"(want {ref64.flatten()[bad.flatten()][:6].tolist()}); worst floor use {float(need.max()):.3g}")
    only_range = (ulp > 1) & (err > c * LE.U_F32 * scale) & ~bad
    assert not bool(out.flatten()[only_range.flatten()].any()), (f"{what}: {x.flatten()[only_range.flatten()][:6].tolist()} need the fp32 range "
                                                                 f"term without having come out as 0")
    return int(ulp[err > floor].max()) if bool((err > floor).any()) else 0, float(need.max()), int(only_range.sum())


def _two_calls(fn, x):
    """run fn on the ragged ROWS x COLS block and on the remainder; returns the flat result"""
    n = ROWS * COLS
    return torch.cat([fn(x[:n].reshape(ROWS, COLS)).reshape(-1), fn(x[n:].reshape(1, -1)).reshape(-1)])


@pytest.mark.parametrize("kind", ["gelu", "gelu_pytorch_tanh", "quick_gelu", "silu"])
def test_act_fwd_bwd_every_bf16_pattern(kind):
    """c = 2 x the worst fp32 error of the oracle's own evaluation (CPU, measured over every pattern where that error is visible at bf16
    resolution), in units of 2^-24 |x| (backward: |x . dy|, the same for dy = 1, -0.37, 3):
        forward   gelu 5.01   gelu_pytorch_tanh 0.99   quick_gelu 0   silu 0
        backward  gelu 0.17   gelu_pytorch_tanh 6.83   quick_gelu 0   silu 0
    (0: the oracle's fp32 error never shows at bf16 resolution, so only the 1-ulp criterion and the fp32 range term remain).  The kernel's
    own need is printed as `floor use` (<= 1 = inside the floor) with the number of patterns that pass through the range term alone;
    both are collected in profiles/local_error_ratios.md."""
    k = K()
    x = _all_finite_bf16()
    x64 = x.double()
    ref = ACT64[kind](x64)
    c = _floor_c((llava_ref.ACT[kind](x.float()).double() - ref).abs(), x64.abs(), ref)
    out = _two_calls(lambda t: k.act_fwd(t.contiguous().to(DEV), kind).cpu(), x)
    u, use, nr = _assert_pointwise(out, ref, c, x64.abs(), f"act_fwd {kind}", x)
    print(f"RATIO act_fwd {kind}: c = {c:.2f} (2 x oracle fp32 worst), kernel max ulp outside the floor {u}, floor use {use:.3f}, "
          f"{nr} patterns through the range term")
    g64 = _act_bwd64(x64, kind)
    for dyv in (1.0, -0.37, 3.0):
        dy = torch.full_like(x, dyv)
        ref = g64 * dy.double()
        scale = (x64 * dy.double()).abs()
        c = _floor_c((_oracle_bwd32(dy, x, kind) - ref).abs(), scale, ref)
        out = _two_calls(lambda t: k.act_bwd(torch.full_like(t, dyv).contiguous().to(DEV), t.contiguous().to(DEV), kind).cpu(), x)
        u, use, nr = _assert_pointwise(out, ref, c, scale, f"act_bwd {kind} dy={dyv}", x)
        print(f"RATIO act_bwd {kind} dy={dyv}: c = {c:.2f}, kernel max ulp outside the floor {u}, floor use {use:.3f}, {nr} patterns through the range term")


def _oracle_bwd32(dy, x, kind):
    """the oracle's act_bwd before its bf16 rounding (fp32 autograd of the same function)"""
    xf = x.float().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(llava_ref.ACT[kind](xf), xf, dy.float())
    return g.double()


@pytest.mark.parametrize("upv", [1.0, -2.5, 0.013])
def test_swiglu_fwd_bwd_every_gate_pattern(upv):
    """swiglu_fwd = bf16(bf16(silu(gate)) . up) (two roundings, as the reference's bf16 graph): the intermediate is the bf16 rounding of an
    fp32 silu, so both roundings of silu64 -+ its fp32 floor are admissible intermediates.  swiglu_bwd: one rounding of the fp32 value."""
    k = K()
    g = _all_finite_bf16()
    g64, u64 = g.double(), torch.full((g.numel(),), upv, dtype=torch.float64).to(BF).double()
    silu = ACT64["silu"](g64)
    # the kernel's fp32 silu: ~8 roundoffs of its own (exp, add, divide, multiply) + the exponent's argument, whose fp32 rounding costs
    # the exponential |g| . log2(e) . 2^-24 relatively (beyond |g| ~ 88 the exponential has saturated)
    # -- and 1 / (1 + e^-g) is 0 in fp32 once e^-g overflows (g < -88.7): silu values under |g| . 2^-127 may come out as 0
    fl = silu.abs() * (8.0 + 2.0 * g64.abs().clamp(max=128.0)) * LE.U_F32 + g64.abs() * 2.0 ** -127
    def fwd(t):
        gu = torch.cat([t, torch.full_like(t, upv)], dim=1).contiguous()
        return k.swiglu_fwd(gu.to(DEV)).cpu()
    out = _two_calls(fwd, g)
    lo, hi = (silu - fl).float().to(BF).double() * u64, (silu + fl).float().to(BF).double() * u64
    ulp = torch.minimum(LE.ulp_distance_bf16(out, lo), LE.ulp_distance_bf16(out, hi))
    o64 = out.double()
    bad = (ulp > 1) & ~((o64 >= torch.minimum(lo, hi)) & (o64 <= torch.maximum(lo, hi)))      # within 1 ulp of an admissible value, or between two
    assert not bool(bad.any()), (f"swiglu_fwd up={upv}: {int(bad.sum())} gate patterns off by more than 1 ulp; first {g[bad][:6].tolist()} -> "
                                 f"{out[bad][:6].tolist()} (want {lo[bad][:6].tolist()})")
    # how many patterns the fp32 allowance `fl` decides (not within 1 ulp of the correctly rounded two-rounding value on its own), and of
    # those how many need its range term: these must have come out as 0
    exact = silu.float().to(BF).double() * u64
    by_fl = LE.ulp_distance_bf16(out, exact) > 1
    fl0 = fl - g64.abs() * 2.0 ** -127
    lo0, hi0 = (silu - fl0).float().to(BF).double() * u64, (silu + fl0).float().to(BF).double() * u64
    ulp0 = torch.minimum(LE.ulp_distance_bf16(out, lo0), LE.ulp_distance_bf16(out, hi0))
    by_range = (ulp0 > 1) & ~((o64 >= torch.minimum(lo0, hi0)) & (o64 <= torch.maximum(lo0, hi0)))
    assert not bool(out[by_range].any()), f"swiglu_fwd up={upv}: gates {g[by_range][:6].tolist()} need the fp32 range term without having come out as 0"
    print(f"RATIO swiglu_fwd up={upv}: max ulp {int(ulp[~bad & (fl < 2.0 ** -20 * silu.abs())].max())}, {int(by_fl.sum())} patterns decided by "
          f"the fp32 allowance, {int(by_range.sum())} of them through the range term")
    s = _sig(g64)
    dsilu = s + silu * (1 - s)
    s32 = torch.sigmoid(g.float())
    for dv_ in (1.0, -0.37, 3.0):
        d64 = torch.full((g.numel(),), dv_, dtype=torch.float64).to(BF).double()
        ref = torch.cat([d64 * u64 * dsilu, d64 * silu])
        scale = torch.cat([(g64 * d64 * u64).abs(), (g64 * d64).abs()])
        o32 = torch.cat([d64.float() * u64.float() * (s32 + g.float() * s32 * (1 - s32)), d64.float() * (g.float() * s32)]).double()
        c = _floor_c((o32 - ref).abs(), scale, ref)
        def bwd(t):
            gu = torch.cat([t, torch.full_like(t, upv)], dim=1).contiguous()
            return k.swiglu_bwd(torch.full_like(t, dv_).contiguous().to(DEV), gu.to(DEV)).cpu()
        n = ROWS * COLS
        o1, o2 = bwd(g[:n].reshape(ROWS, COLS)), bwd(g[n:].reshape(1, -1))
        out = torch.cat([o1[:, :COLS].reshape(-1), o2[:, : o2.shape[1] // 2].reshape(-1), o1[:, COLS:].reshape(-1), o2[:, o2.shape[1] // 2:].reshape(-1)])
        u, use, nr = _assert_pointwise(out, ref, c, scale, f"swiglu_bwd up={upv} dact={dv_}", torch.cat([g, g]))
        print(f"RATIO swiglu_bwd up={upv} dact={dv_}: c = {c:.2f}, kernel max ulp outside the floor {u}, floor use {use:.3f}, {nr} patterns through the range term")


# ------------------------------------------------------------------------------------------------------------- attention
# (B, L, H, Hkv, hd, causal, mask, backward, cuts, window)
ATTN_CASES = [(2, 54, 4, 2, 16, True, "right", True, None, None), (2, 54, 4, 2, 16, True, "left", True, None, None),
              (1, 129, 2, 2, 64, True, "left", True, None, None), (1, 323, 12, 12, 64, True, None, True, None, None),
              (2, 193, 4, 2, 128, False, None, True, None, None), (1, 333, 14, 2, 128, True, "right", True, None, None),
              (2, 200, 7, 1, 128, True, None, True, None, None), (2, 80, 16, 4, 96, False, "right", True, None, None),
              (2, 391, 16, 16, 80, False, None, False, None, None),
              (1, 300, 8, 2, 128, True, None, True, [[70, 71, 200]], None),            # packed segments
              (1, 300, 8, 2, 128, True, None, True, None, 64),                        # sliding window
              (1, 300, 8, 2, 128, True, None, True, None, 1)]       # the smallest window: o = v, dV = group sum of dO, dQ = dK = 0 up to noise
_ATTN_IDS = ["B{}L{}H{}-{}hd{}c{}m{}b{}s{}w{}".format(*[("seg" if isinstance(x, list) else x) for x in c]) for c in ATTN_CASES]


@pytest.mark.parametrize("case", ATTN_CASES, ids=_ATTN_IDS)
def test_attention_self_localised(case):
    B, L, H, Hkv, hd, causal, mask, backward, cuts, window = case
    k = K()
    qkv = rnd(B * L, (H + 2 * Hkv) * hd, seed=L + hd + 1)
    do = rnd(B * L, H * hd, seed=L + 7)
    km = _kmask(B, L, mask, seed=L)
    if km is not None:
        do = do * km.reshape(B * L, 1).to(BF)
    ks, qe = _segment_bounds(B, L, cuts) if cuts is not None else (None, None)
    ref = LE.AttnCase(qkv, do if backward else None, B, L, H, Hkv, hd, causal, kmask=km, kstart=ks, window=window)
    dv = lambda t: None if t is None else t.to(DEV)
    qd = qkv.to(DEV)
    o, lse = k.attn_fwd(qd, B, L, H, Hkv, hd, dv(km), ref.scale, causal, kstart=dv(ks), window=window)
    what = f"attn B{B} L{L} H{H}/{Hkv} hd{hd} causal={causal} mask={mask} cuts={cuts} window={window}"
    worst = ref.check_forward(o, lse, what)
    print(f"RATIO {what} fwd: worst {worst:.3f}")
    if backward:
        d = k.attn_bwd(qd, o, do.to(DEV), lse, B, L, H, Hkv, hd, dv(km), ref.scale, causal, kstart=dv(ks), qend=dv(qe), window=window).cpu()
        got = ref.check_backward(d[:, : H * hd], d[:, H * hd: (H + Hkv) * hd], d[:, (H + Hkv) * hd:], what)
        bars = ref.backward_bars()
        print(f"RATIO {what} bwd: " + ", ".join(f"{n} {got[n]:.2e} (bar {bars[n][0]:.2e} = 3 x emulation {bars[n][1]:.2e})" if n in bars else
                                                f"{n} worst (row, head) norm / bound {got[n]:.3f}" for n in got))


@pytest.mark.parametrize("mode", ["1", "0"])
def test_attention_self_localised_with_forward_kernel_forced(mode):
    """the hd-128 forward has two kernels (MANTIS_ATTN_FWD64, read once per process): the group above once more under each, in a child"""
    if os.environ.get("MANTIS_LOCAL_ERROR_CHILD"):
        pytest.skip("already inside the forced-kernel child")
    env = dict(os.environ, MANTIS_ATTN_FWD64=mode, MANTIS_LOCAL_ERROR_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_attention_self_localised and hd128 and not forced"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    tail = (r.stdout + r.stderr)[-2500:]
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, tail


@pytest.mark.parametrize("B,Lq,Lk,H,Hkv,hd", [(2, 64, 80, 16, 4, 96), (2, 20, 300, 4, 1, 16)])
def test_attention_cross_localised(B, Lq, Lk, H, Hkv, hd):
    k = K()
    q, kv, do = rnd(B * Lq, H * hd, seed=Lq + hd), rnd(B * Lk, 2 * Hkv * hd, seed=Lk + hd + 1), rnd(B * Lq, H * hd, seed=Lq + 9)
    km = torch.ones(B, Lk, dtype=torch.int32)
    g = torch.Generator().manual_seed(Lk)
    for b in range(B):
        n = int(torch.randint(1, Lk // 2, (1,), generator=g))
        km[b, Lk // 3: Lk // 3 + n] = 0
    scale, rep = hd ** -0.5, H // Hkv
    refs, emus = [], []
    for b in range(B):
        qh = q[b * Lq:(b + 1) * Lq].reshape(Lq, H, hd).transpose(0, 1)
        kh = kv[b * Lk:(b + 1) * Lk, : Hkv * hd].reshape(Lk, Hkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
        vh = kv[b * Lk:(b + 1) * Lk, Hkv * hd:].reshape(Lk, Hkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
        dh = do[b * Lq:(b + 1) * Lq].reshape(Lq, H, hd).transpose(0, 1)
        ok = LE.allowed_mask(Lq, Lk, kmask=km[b])[None]
        refs.append((LE.attn_reference(qh, kh, vh, dh, scale, ok, rep), vh))
        emus.append(LE.attn_reference(qh, kh, vh, dh, scale, ok, rep, emulate=True))
    cat = lambda rs, n: torch.cat([LE.rows_major(r[n]) for r in rs], dim=0)
    qd, kvd, kmd = q.to(DEV), kv.to(DEV), km.to(DEV)
    o, lse = k.attn_fwd_cross(qd, kvd[:, : Hkv * hd], kvd[:, Hkv * hd:], B, Lq, Lk, H, Hkv, hd, kmd, scale)
    what = f"cross attn B{B} Lq{Lq} Lk{Lk} H{H}/{Hkv} hd{hd}"
    oref = cat([r for r, _ in refs], "o")
    bound = torch.cat([LE.rows_major(LE.attn_fwd_bound(r["p"], LE.f64(v), r["o"])) for r, v in refs], dim=0)
    worst = LE.assert_elementwise(o, oref, bound, f"{what} o", tile=(16, hd))
    dl = (LE.f64(lse) - torch.stack([r["lse"] for r, _ in refs])).abs().max()
    assert float(dl) <= LE.LSE_ABS_TOL, f"{what}: lse off by {float(dl):.3e}"
    dq, dkv = torch.empty_like(qd), torch.empty_like(kvd)
    k.attn_bwd_cross(qd, kvd[:, : Hkv * hd], kvd[:, Hkv * hd:], o, do.to(DEV), lse, dq, dkv[:, : Hkv * hd], dkv[:, Hkv * hd:], B, Lq, Lk, H, Hkv,
                     hd, kmd, scale)
    msg = []
    for name, heads, got, count in (("dq", H, dq, None), ("dk", Hkv, dkv[:, : Hkv * hd], km.reshape(-1).bool()),
                                    ("dv", Hkv, dkv[:, Hkv * hd:], km.reshape(-1).bool())):
        r64 = cat([r for r, _ in refs], name)
        err, _ = LE.attn_rowhead_error(cat(emus, name), r64, heads, hd)
        w = float(err.max() if count is None else torch.where(count[:, None].expand_as(err), err, torch.zeros_like(err)).max())
        e = LE.assert_rowhead(got, r64, heads, hd, LE.BWD_BAR_FACTOR * w, f"{what} {name}", count=count)
        msg.append(f"{name} {e:.2e} (bar {LE.BWD_BAR_FACTOR * w:.2e} = 3 x emulation {w:.2e})")
    print(f"RATIO {what}: fwd worst {worst:.3f}; " + ", ".join(msg))


@pytest.mark.parametrize("G", [1, 4, 7])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_attention_decode_localised(hd, G):
    """more than one split, key counts straddling a split boundary, with and without a key mask: per (sample, head), not the flat norm"""
    k = K()
    B, Hkv, S_max = 2, 2, 1024
    H, scale = G * Hkv, hd ** -0.5
    kc, vc, q = rnd(B, Hkv, S_max, hd, seed=hd + G), rnd(B, Hkv, S_max, hd, seed=hd + G + 1), rnd(B, H * hd, seed=B)
    splits, chunk = k.attn_decode_splits(B, Hkv, S_max)
    assert splits > 1 and chunk + 1 <= S_max, (splits, chunk)
    kmask = (torch.rand(B, S_max, generator=torch.Generator().manual_seed(7)) > 0.3).to(torch.int32)
    worst = 0.0
    for counts in ((chunk - 1, chunk), (chunk + 1, S_max)):
        n_keys = torch.tensor(counts, dtype=torch.int32)
        for km in (None, kmask):
            o = k.attn_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), None if km is None else km.to(DEV), n_keys.to(DEV), H, Hkv, hd, scale)
            for b in range(B):
                live = torch.arange(S_max) < counts[b]
                if km is not None:
                    live = live & (km[b] != 0)
                qh = q[b].reshape(H, 1, hd)
                kh, vh = kc[b].repeat_interleave(G, dim=0), vc[b].repeat_interleave(G, dim=0)
                r = LE.attn_reference(qh, kh, vh, None, scale, live[None, None, :])
                bound = LE.attn_fwd_bound(r["p"], LE.f64(vh), r["o"])
                what = f"attn_decode hd{hd} G{G} keys {counts[b]} mask={km is not None} sample {b}"
                worst = max(worst, LE.assert_elementwise(o[b].reshape(H, hd), r["o"][:, 0], bound[:, 0], what, tile=(1, hd)))
                # P stays in fp32 in this kernel: the output's own rounding (2^-8 per element) + the same 2^-8 allowance for the fp32
                # score / exp / split-merge path as in the elementwise bound
                err, _ = LE.attn_rowhead_error(o[b:b + 1], LE.rows_major(r["o"]), H, hd)
                assert float(err.max()) <= 2 * LE.U_BF16, f"{what}: worst head rel-L2 {float(err.max()):.3e}"
    print(f"RATIO attn_decode hd{hd} G{G} splits {splits}: worst {worst:.3f}")
