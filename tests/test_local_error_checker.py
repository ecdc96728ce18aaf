"""CPU proof that the localised checks of tests/local_error.py discriminate: a CPU emulation of each operator's documented rounding chain
passes them at ratio <= 1 with the constants as derived, every seeded fault (a K tail dropped in a ragged corner, stale tail columns, a
column strip missing one K-step, a zero row, a causal mask off by one, a stale running max, a masked key let through, a zero dK row) is
rejected -- and the faults that motivated the module are accepted by the whole-tensor `close(...)` of tests/gpu_checks.py."""
import pytest
import torch

from tests import local_error as LE
from tests.gpu_checks import _kmask, close, rnd

BF = torch.bfloat16
GEMM_SHAPES = [(1000, 4304, 1152), (300, 200, 72), (257, 388, 1152), (77, 40, 8)]
OLD_CLOSE_ACCEPTS = {((1000, 4304, 1152), "k_tail_corner"), ((1000, 4304, 1152), "stale_tail_block"), ((257, 388, 1152), "k_tail_corner")}
GEMM_FAULTS = ["k_tail_corner", "stale_tail_block", "strip_missing_k_step", "last_row_zero"]


def _gemm_fault(name, clean, a, b):
    M, K = a.shape
    N = b.shape[0]
    out = clean.clone()
    af, bf = a.float(), b.float()
    if name == "k_tail_corner":             # the last 8 k dropped in the ragged bottom-right 16 x 16 corner
        kk = max(K - 8, 0)
        out[M - 16:, N - 16:] = (af[M - 16:, :kk] @ bf[N - 16:, :kk].t()).to(BF)
    elif name == "stale_tail_block":        # a 16 x 4 block of stale values (another tile's) in the tail columns
        r0 = (M // 2) // 16 * 16
        out[r0:r0 + 16, N - 4:] = clean[0:16, 0:4]
    elif name == "strip_missing_k_step":    # a whole 16-column strip missing one 32-wide K-step, every row
        c0 = (N // 2) // 16 * 16
        k0 = (K // 2) // 32 * 32
        keep = torch.ones(K, dtype=torch.bool)
        keep[k0:k0 + 32] = False
        out[:, c0:c0 + 16] = (af[:, keep] @ bf[c0:c0 + 16][:, keep].t()).to(BF)
    elif name == "last_row_zero":
        out[M - 1] = 0
    return out


@pytest.fixture(scope="module", params=GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def gemm_case(request):
    M, N, K = request.param
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1)
    clean = (a.float() @ b.float().t()).to(BF)                      # the documented chain: fp32 accumulation, one bf16 rounding
    ref, _, bound = LE.gemm_bound(a, b, n_roundings=1, K=K)
    return request.param, a, b, clean, ref, bound


def test_gemm_clean_emulation_fits_the_bound(gemm_case):
    shape, a, b, clean, ref, bound = gemm_case
    worst = LE.assert_elementwise(clean, ref, bound, f"emulated gemm {shape}")
    print(f"gemm {shape} plain: emulation worst ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fault", GEMM_FAULTS)
def test_gemm_seeded_fault_is_rejected(gemm_case, fault):
    shape, a, b, clean, ref, bound = gemm_case
    bad = _gemm_fault(fault, clean, a, b)
    assert not torch.equal(bad, clean)
    with pytest.raises(AssertionError, match="over the bound"):
        LE.assert_elementwise(bad, ref, bound, f"{fault} {shape}")
    if (shape, fault) in OLD_CLOSE_ACCEPTS:                        # the reason this module exists
        close(bad, a.float() @ b.float().t(), 1e-2, f"old bar, {fault} {shape}")


@pytest.mark.parametrize("epi,n_roundings", [("bias", 1), ("res", 2), ("bias+res", 2), ("acc", 2)])
def test_gemm_epilogue_chains_fit_their_bounds(epi, n_roundings):
    """oracle/ops_ref.py gemm_nt restates the kernels' chains (bias into the fp32 accumulator; product rounded, then the residual added;
    accumulate reads bf16 C): each fits its bound, and the residual chain does NOT fit the one-rounding bound everywhere."""
    from oracle import ops_ref as R
    M, N, K = 300, 200, 72
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1)
    bias = rnd(N, seed=3) if "bias" in epi else None
    res = rnd(M, N, seed=4) if "res" in epi else None
    c0 = rnd(M, N, seed=7) if epi == "acc" else None
    out = R.gemm_nt(a, b, bias=bias, residual=res, out=None if c0 is None else c0.clone(), accumulate=c0 is not None)
    added = tuple(t for t in (None if bias is None else bias[None, :], res, c0) if t is not None)
    ref, _, bound = LE.gemm_bound(a, b, n_roundings=n_roundings, K=K, added=added)
    worst = LE.assert_elementwise(out, ref, bound, f"oracle gemm {epi}")
    print(f"gemm 300x200x72 {epi}: oracle chain worst ratio {worst:.3f}")
    bad = out.clone()
    bad[M - 1] = 0
    with pytest.raises(AssertionError):
        LE.assert_elementwise(bad, ref, bound, f"last row zero, {epi}")


def test_ulp_distance():
    x = torch.tensor([1.0, 1.0 + 2 ** -7, -1.0, 0.0, 3.0e38, 1e-40], dtype=torch.float64)
    same = x.to(torch.float32).to(BF)
    assert int(LE.ulp_distance_bf16(same, x).max()) == 0
    up = (same.view(torch.int16) + 1).view(BF)                      # one ulp away from zero
    assert LE.ulp_distance_bf16(up, x).tolist() == [1, 1, 1, 1, 1, 1]
    assert int(LE.ulp_distance_bf16(torch.tensor([-0.0], dtype=BF), torch.tensor([0.0], dtype=torch.float64))[0]) == 0
    assert int(LE.ulp_distance_bf16(torch.tensor([2.0 ** -126], dtype=BF), torch.tensor([-(2.0 ** -126)], dtype=torch.float64))[0]) == 2 * 0x80
    assert int(LE.ulp_distance_bf16(torch.tensor([float("nan")], dtype=BF), torch.tensor([1.0], dtype=torch.float64))[0]) >= 1 << 20


# ------------------------------------------------------------------------------------------------------------- attention
ATTN_CASES = [(2, 197, 12, 12, 64, True, None), (1, 129, 2, 2, 64, True, "left")]
OLD_CLOSE_ACCEPTS_ATTN = {"causal_off_by_one", "stale_running_max"}      # at the first case (the table's)


class _Attn:
    def __init__(self, B, L, H, Hkv, hd, causal, mask):
        self.geom = (B, L, H, Hkv, hd)
        self.causal = causal
        self.qkv = rnd(B * L, (H + 2 * Hkv) * hd, seed=L + hd + 1)
        self.km = _kmask(B, L, mask, seed=L)
        do = rnd(B * L, H * hd, seed=L + 7)
        self.do = do if self.km is None else do * self.km.reshape(B * L, 1).to(BF)
        self.case = LE.AttnCase(self.qkv, self.do, B, L, H, Hkv, hd, causal, kmask=self.km)
        emu = self.case.emulation()
        self.o, self.lse = self.case.rows(emu, "o"), self.case.lse(emu)
        self.dq, self.dk, self.dv = (self.case.rows(emu, n) for n in ("dq", "dk", "dv"))

    def emulate(self, allowed_of):
        """the emulation with another visibility mask: allowed_of(b, ok [1, L, L]) -> [H or 1, L, L]"""
        B, L, H, Hkv, hd = self.geom
        res = [LE.attn_reference(q, k, v, self.case.do[b], self.case.scale, allowed_of(b, ok), H // Hkv, emulate=True)
               for b, (q, k, v, ok) in enumerate(self.case.probs)]
        return {n: self.case.rows(res, n) for n in ("o", "dq", "dk", "dv")} | {"lse": self.case.lse(res)}

    def counted_rows(self, b=0):
        """rows of sample b that have a live key"""
        return torch.isfinite(self.case.lse(self.case.ref)[b, 0]).nonzero()[:, 0]


@pytest.fixture(scope="module", params=ATTN_CASES, ids=lambda c: "B{}L{}H{}/{}hd{}c{}m{}".format(*c))
def attn(request):
    return _Attn(*request.param)


def _old_forward_close(A, o, lse):
    """today's whole-tensor forward check (tests/gpu_checks.py check_attn_fwd) against the oracle's attn_fwd"""
    from oracle import ops_ref as R
    B, L, H, Hkv, hd = A.geom
    oref, lref = R.attn_fwd(A.qkv, B, L, H, Hkv, hd, A.km, hd ** -0.5, A.causal)
    valid = torch.isfinite(lref)
    vo = valid.transpose(1, 2).reshape(B * L, H, 1).expand(B * L, H, hd).reshape(B * L, H * hd)
    close(o.float() * vo, oref.float() * vo, 2e-2, "old attn_fwd bar")


def test_attention_clean_emulation_fits(attn):
    worst = attn.case.check_forward(attn.o, attn.lse, "emulated attention")
    bars = attn.case.backward_bars()
    got = attn.case.check_backward(attn.dq, attn.dk, attn.dv, "emulated attention")
    print(f"attention {attn.geom}: forward worst ratio {worst:.3f}; emulation worst (row, head) error / bar: "
          + ", ".join(f"{n} {bars[n][1]:.2e} / {bars[n][0]:.2e}" for n in bars))
    assert worst <= 1.0 and all(got[n] <= bars[n][0] for n in bars)
    _old_forward_close(attn, attn.o, attn.lse)


def _off_by_one(A):
    """causal mask off by one (`>=` for `>`: the diagonal key hidden) on the last L % 64 query rows, all heads"""
    B, L = A.geom[:2]
    def allowed(b, ok):
        ok = ok.clone()
        for i in range(L - L % 64, L):
            ok[0, i, i] = False
        return ok
    return A.emulate(allowed)


def test_attention_causal_off_by_one_is_rejected(attn):
    bad = _off_by_one(attn)
    assert not torch.equal(bad["o"], attn.o)
    with pytest.raises(AssertionError):
        attn.case.check_forward(bad["o"], bad["lse"], "causal off by one")
    with pytest.raises(AssertionError, match="over the bound"):         # the output alone gives it away, without the lse
        attn.case.check_forward(bad["o"], attn.lse, "causal off by one, o only")
    with pytest.raises(AssertionError, match="dq"):
        attn.case.check_backward(bad["dq"], attn.dk, attn.dv, "causal off by one")
    with pytest.raises(AssertionError, match="dk"):
        attn.case.check_backward(attn.dq, bad["dk"], attn.dv, "causal off by one")
    if attn.km is None:
        _old_forward_close(attn, bad["o"], bad["lse"])


def test_attention_stale_running_max_is_rejected(attn):
    """16 rows of one head scaled by 1.08"""
    B, L, H, Hkv, hd = attn.geom
    bad = attn.o.clone()
    rows = slice(B * L - 16, B * L)
    bad[rows, (H - 1) * hd:] = (bad[rows, (H - 1) * hd:].float() * 1.08).to(BF)
    with pytest.raises(AssertionError, match="over the bound"):
        attn.case.check_forward(bad, attn.lse, "stale running max")
    if attn.km is None:
        _old_forward_close(attn, bad, attn.lse)


def test_attention_last_row_zero_is_rejected(attn):
    bad = attn.o.clone()
    bad[-1] = 0
    with pytest.raises(AssertionError, match="over the bound"):
        attn.case.check_forward(bad, attn.lse, "last row zero")
    for name in ("dq", "dk", "dv"):
        g = {n: getattr(attn, n).clone() for n in ("dq", "dk", "dv")}
        g[name][-1] = 0
        with pytest.raises(AssertionError, match=name):
            attn.case.check_backward(g["dq"], g["dk"], g["dv"], "last row zero")


def test_attention_masked_key_let_through_is_rejected(attn):
    """one masked key visible to ONE (row, head): the middle row that has a live key, and of its masked keys the one with the largest
    score (a leaked key whose weight is below the bf16 resolution of the output changes nothing any output check could see)"""
    B, L, H, Hkv, hd = attn.geom
    live = attn.counted_rows(0)
    i = int(live[len(live) // 2])
    q, k, _, ok = attn.case.probs[0]
    s = (q[H - 1, i].double() @ k[H - 1].double().t()).masked_fill(ok[0, i], float("-inf"))
    j = int(s.argmax())
    assert not bool(ok[0, i, j])
    def allowed(b, ok):
        ok = ok.expand(H, L, L).clone()
        if b == 0:
            ok[H - 1, i, j] = True
        return ok
    bad = attn.emulate(allowed)
    assert not torch.equal(bad["o"][i], attn.o[i]) and torch.equal(bad["o"][:i], attn.o[:i])
    with pytest.raises(AssertionError):
        attn.case.check_forward(bad["o"], bad["lse"], "masked key let through")
    with pytest.raises(AssertionError, match="over the bound"):
        attn.case.check_forward(bad["o"], attn.lse, "masked key let through, o only")


def test_attention_dk_row_head_zero_is_rejected(attn):
    """one (key row, kv head) of dK zero; one (row, head) of dQ zero"""
    B, L, H, Hkv, hd = attn.geom
    i = int(attn.counted_rows(0)[3])
    bad = attn.dk.clone()
    bad[i, (Hkv - 1) * hd:] = 0
    with pytest.raises(AssertionError, match="dk"):
        attn.case.check_backward(attn.dq, bad, attn.dv, "dk row-head zero")
    bad = attn.dq.clone()
    bad[i, :hd] = 0
    with pytest.raises(AssertionError, match="dq"):
        attn.case.check_backward(bad, attn.dk, attn.dv, "dq row-head zero")
    from tests.gpu_checks import rel
    if attn.km is None:
        assert rel(bad, attn.case.rows(attn.case.ref, "dq")) <= 3e-2        # the old whole-tensor gradient bar accepts it


def test_rowhead_floor_share_is_asserted():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(200, 4 * 8, dtype=torch.float64, generator=g)
    ref[:10] *= 1e-3                                                # 5 % of the rows near-cancelling ...
    out = ref + 1e-4 * torch.randn(200, 4 * 8, dtype=torch.float64, generator=g)     # ... and only the floor keeps them under the bar
    with pytest.raises(AssertionError, match="floor"):
        LE.assert_rowhead(out, ref, 4, 8, 1e-2, "floor share")


def test_rowhead_zero_reference_pairs_are_held_absolutely():
    """a (row, head) whose reference is exactly zero (one visible key: dQ = 0) has no verdict without the floor, so fp32 noise there is no
    verdict the floor changed -- and anything that is not noise there still fails against the floored denominator"""
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(50, 4 * 8, dtype=torch.float64, generator=g)
    ref[0] = 0                                                      # 4 of 200 pairs: 2 %
    out = ref.clone()
    out[0] = 1e-7 * torch.randn(4 * 8, dtype=torch.float64, generator=g)
    err, raw = LE.attn_rowhead_error(out, ref, 4, 8)
    assert bool(torch.isnan(raw[0]).all()) and bool(torch.isfinite(raw[1:]).all())
    assert LE.floor_verdict_share(err, raw, 1e-2) == 0.0
    assert LE.assert_rowhead(out, ref, 4, 8, 1e-2, "zero reference, noise") < 1e-6
    out[0, 8:16] = 0.05 * torch.randn(8, dtype=torch.float64, generator=g)         # one head of the zero row: a real value
    with pytest.raises(AssertionError, match=r"row 0, head 1"):
        LE.assert_rowhead(out, ref, 4, 8, 1e-2, "zero reference, a value")


def test_single_key_window_backward_is_held_absolutely():
    """window = 1: the reference of dQ and dK is zero everywhere, so they are bounded a priori per (row, head); dV keeps its relative bar"""
    B, L, H, Hkv, hd = 1, 70, 4, 2, 128
    qkv, do = rnd(B * L, (H + 2 * Hkv) * hd, seed=11), rnd(B * L, H * hd, seed=12)
    case = LE.AttnCase(qkv, do, B, L, H, Hkv, hd, True, window=1)
    emu = case.emulation()
    dq, dk, dv = (case.rows(emu, n) for n in ("dq", "dk", "dv"))
    assert set(case.backward_bars()) == {"dv"}
    got = case.check_backward(dq, dk, dv, "window 1")
    print(f"window 1 emulation: dq / dk worst norm over bound {got['dq']:.3f} / {got['dk']:.3f}, dv {got['dv']:.2e}")
    assert got["dq"] <= 1.0 and got["dk"] <= 1.0
    assert torch.equal(dv, case.rows(case.ref, "dv").to(BF).to(dv.dtype))           # dV = the group sum of dO, rounded once
    for name in ("dq", "dk"):
        g = dict(dq=dq.clone(), dk=dk.clone(), dv=dv)
        g[name][37, hd: 2 * hd] = 1e-3 * rnd(hd, seed=13).to(g[name].dtype)          # 1e-3 of a typical gradient in one (row, head)
        with pytest.raises(AssertionError, match=name):
            case.check_backward(g["dq"], g["dk"], g["dv"], "window 1, a value")
    bad = dv.clone()
    bad[69, :hd] = 0
    with pytest.raises(AssertionError, match="dv"):
        case.check_backward(dq, dk, bad, "window 1, dv row-head zero")


# ------------------------------------------------------------------------------------------------------------- row-wise kernels
# (a) the fp32 oracle passes every criterion on the exact inputs of tests/test_rowwise_local_error_gpu.py (tests/rowwise_cases.py holds
# both); (b) every seeded fault, applied to a CPU emulation of the kernel's arithmetic, is rejected.
from oracle import ops_ref as OR          # noqa: E402
from tests import rowwise_cases as C      # noqa: E402

CPU = "cpu"


@pytest.mark.parametrize("d,rows,w_off", [c[1:] for c in C.RMS_FWD_CASES], ids=[c[0] for c in C.RMS_FWD_CASES])
def test_oracle_passes_rmsnorm_fwd(d, rows, w_off):
    print(C.run_rmsnorm_fwd(OR, CPU, d, rows, w_off))


@pytest.mark.parametrize("d,sub", [c[1:] for c in C.RMS_BWD_CASES], ids=[c[0] for c in C.RMS_BWD_CASES])
def test_oracle_passes_rmsnorm_bwd(d, sub):
    print(C.run_rmsnorm_bwd(OR, CPU, d, sub))


@pytest.mark.parametrize("rows,d", C.RMS_BWD_WITNESS)
def test_oracle_passes_rmsnorm_bwd_witness(rows, d):
    C.run_rmsnorm_bwd_witness(OR, CPU, rows, d)


@pytest.mark.parametrize("d,rows", C.LN_CASES, ids=[f"d{c[0]}" for c in C.LN_CASES])
def test_oracle_passes_layernorm(d, rows):
    print(C.run_layernorm(OR, CPU, d, rows))


@pytest.mark.parametrize("V", C.CE_V)
def test_oracle_passes_ce(V):
    for kind in C.CE_KINDS:
        print(kind, C.run_ce(OR, CPU, V, kind))


def test_oracle_passes_ce_edge_rows():
    C.run_ce_all_ignored(OR, CPU)
    for V in C.CE_NEG_INF_V:
        C.run_ce_neg_inf(OR, CPU, V)


@pytest.mark.parametrize("hd,nheads,R_", C.ROPE_CASES)
def test_oracle_passes_rope_apply(hd, nheads, R_):
    stat = C.run_rope_apply(OR, CPU, hd, nheads, R_)
    assert stat["bwd_share"] == 0.0, stat             # the cap of 0.1 % is held by the reference alone


@pytest.mark.parametrize("half", C.ROPE_TABLE_HALF)
def test_oracle_passes_rope_tables(half):
    for stat in (C.run_rope_table(OR, CPU, half), C.run_rope_table_sections(OR, CPU, 3, half), C.run_rope_table_sections(OR, CPU, 2, half)):
        assert stat["share"] == 0.0, stat


def test_oracle_passes_reductions():
    for M in C.COLSUM_M:
        C.run_colsum(OR, CPU, M)
    for n in C.SUMSQ_N:
        C.run_sumsq(OR, CPU, n)
    C.run_sumsq_ranges(OR, CPU)
    for n in C.SUM_F32_N:
        C.run_sum_f32(OR, CPU, n)
    C.run_clip_scale(OR, CPU)


def _bf(t):
    return t.to(BF).float()


# ---- RMSNorm forward
def _emu_rmsnorm_fwd(x, w, eps, fault=None):
    xf, wf, d = x.float(), w.float(), x.shape[1]
    ms = xf.pow(2).mean(-1)
    if fault == "row_denominator":                      # one row normalised with d + 8 in the denominator
        ms[x.shape[0] // 2] = xf[x.shape[0] // 2].pow(2).sum() / (d + 8)
    rstd = torch.rsqrt(ms + eps)
    if fault == "single_rounding":
        return (xf * rstd[:, None] * wf).to(BF), rstd
    n = _bf(xf * rstd[:, None])
    y = (n * wf).to(BF)
    if fault == "neighbour_weights":                    # one 8-chunk scaled by its neighbour's weights
        c = d // 16 * 8
        y[:, c:c + 8] = (n[:, c:c + 8] * wf[c + 8:c + 16]).to(BF)
    return y, rstd


@pytest.mark.parametrize("rows,d", [(323, 768), (37, 3584), (16, 8192)])
def test_rmsnorm_fwd_emulation_differs_nowhere(rows, d):
    x, w = rnd(rows, d, seed=1), C._weight(d, 2)
    stat = LE.check_rmsnorm_fwd(*_emu_rmsnorm_fwd(x, w, 1e-5), x, w, 1e-5, f"emulation {rows}x{d}")
    assert stat["share"] == 0.0 and stat["ulp"] == 0, stat


@pytest.mark.parametrize("fault", ["single_rounding", "row_denominator", "neighbour_weights"])
def test_rmsnorm_fwd_seeded_fault_is_rejected(fault):
    x, w = rnd(323, 768, seed=1), C._weight(768, 2)
    y, rstd = _emu_rmsnorm_fwd(x, w, 1e-5, fault)
    with pytest.raises(AssertionError, match="rmsnorm y"):
        LE.check_rmsnorm_fwd(y, None, x, w, 1e-5, "rmsnorm")            # the output alone gives it away
    if fault == "row_denominator":
        with pytest.raises(AssertionError, match="rstd"):
            LE.check_rmsnorm_fwd(_emu_rmsnorm_fwd(x, w, 1e-5)[0], rstd, x, w, 1e-5, "rmsnorm")
    if fault == "single_rounding":                                       # the reason: the whole-tensor bar lets it through
        close(y, OR.rmsnorm_fwd(x, w, 1e-5)[0], 4e-3, "old bar, single rounding")


# ---- RMSNorm backward
def _emu_rmsnorm_bwd(dy, x, w, rstd, dres, g0, fault=None):
    rows, d = x.shape
    xf, g = x.float(), dy.float() * w.float()
    xhat = xf * rstd[:, None]
    prod = g * xhat
    dot = (prod[:, :-8] if fault == "dot_last_chunk" else prod).sum(-1, keepdim=True) / d
    add = dres.float().clone()
    if fault == "dres_last_row":
        add[-1] = 0
    dx = (rstd[:, None] * (g - xhat * dot) + add).to(BF)
    t = dy.float() * xhat
    if fault == "dw_row":
        t[rows // 2] = 0
    if fault == "dw_partial_row":                       # one workgroup's partial row: 8 rows
        t[8:16] = 0
    gw = t.sum(0) + g0.float()
    if fault == "dw_swap":
        j = d // 2
        gw[[j, j + 8]] = gw[[j + 8, j]]
    return dx, gw.to(BF)


@pytest.fixture(scope="module")
def rms_bwd_case():
    rows, d = 323, 768
    x, w, dy, dres, g0 = rnd(rows, d, seed=1), C._weight(d, 2), rnd(rows, d, seed=3), rnd(rows, d, seed=4), rnd(d, seed=5)
    rstd = LE.rmsnorm_fwd_reference(x, w, 1e-5)[1].float()
    return (dy, x, w, rstd, dres, g0), LE.rmsnorm_bwd_reference(dy, x, w, rstd, dres, g0, True)


@pytest.mark.parametrize("fault", [None, "dot_last_chunk", "dres_last_row", "dw_row", "dw_partial_row", "dw_swap"])
def test_rmsnorm_bwd_seeded_fault_is_rejected(rms_bwd_case, fault):
    args, ref = rms_bwd_case
    dx, gw = _emu_rmsnorm_bwd(*args, fault=fault)
    hits = []
    for name, out in (("dx", dx), ("dw", gw)):
        try:
            LE.assert_bounded(out, ref[name], ref[name + "_bound"], name)
        except AssertionError:
            hits.append(name)
    assert hits == ([] if fault is None else ["dw"] if fault.startswith("dw") else ["dx"]), hits


@pytest.mark.parametrize("rows,d", C.RMS_BWD_WITNESS)
def test_rmsnorm_bwd_witness_sees_a_row_counted_twice(rows, d):
    class Twice:
        @staticmethod
        def rmsnorm_bwd(dy, x, w, rstd, dres, g, acc, amax_parts=None):
            dy = dy.clone()
            dy[rows - 1] *= 2                           # the last row's contribution added twice
            return OR.rmsnorm_bwd(dy, x, w, rstd, dres, g, acc)
    with pytest.raises(AssertionError, match="witness"):
        C.run_rmsnorm_bwd_witness(Twice, CPU, rows, d)


# ---- LayerNorm
def _emu_layernorm(x, w, b, eps, fault=None):
    xf, wf, bf_ = x.float(), w.float(), b.float().clone()
    mean = xf.mean(-1, keepdim=True)
    if fault == "one_pass_variance":                    # fp32 E[x^2] - mean^2: cancels catastrophically at mean 30, std 1
        var = (xf * xf).mean(-1, keepdim=True) - mean * mean
    else:
        var = (xf - mean).pow(2).mean(-1, keepdim=True)
    if fault == "bias_shift":                           # the bias of one chunk read 8 elements further
        c = x.shape[1] // 16 * 8
        bf_[c:c + 8] = b.float()[c + 8:c + 16]
    return ((xf - mean) * torch.rsqrt(var + eps) * wf + bf_).to(BF)


@pytest.mark.parametrize("rows,d", [(5, 768), (37, 768), (323, 1152)])      # the first is a GPU case as it stands
@pytest.mark.parametrize("fault", [None, "one_pass_variance", "bias_shift"])
def test_layernorm_seeded_fault_is_rejected(fault, rows, d):
    """the one-pass variance errs by about 2^-24 . mean^2 / var relative, the bound's mean term allows (d / 64 + 6) . 2^-24 . mean absolute:
    at mean 30 the fault stands out by a factor 30 / (d / 64 + 6) -- clear at d = 768, 10 elements of 3840 over the bound, thin at 5 x 1152,
    where it takes more rows to meet an element next to a rounding tie"""
    x, w, b = C.ln_inputs(rows, d)
    ref, bound = LE.layernorm_reference(x, w, b, 1e-6)
    y = _emu_layernorm(x, w, b, 1e-6, fault)
    if fault is None:
        LE.assert_bounded(y, ref, bound, "layernorm emulation")
        return
    with pytest.raises(AssertionError, match="over the bound"):
        LE.assert_bounded(y, ref, bound, fault)


# ---- cross-entropy
def _emu_ce(x0, tgt, V, fault=None):
    """ce.hip in fp32 with its thread layout: thread t of 1024 owns the 8-chunks t, t + 1024, ... and keeps an online (max, sum)"""
    R_, Vp = x0.shape[0], C.pad8(V)
    xf = x0.float()[:, :Vp]
    seen = Vp if fault == "pad_in_lse" else V
    trips = -(-(Vp // 8) // 1024)
    buf = torch.full((R_, trips * 8192), float("-inf"))
    buf[:, :seen] = xf[:, :seen]
    buf = buf.reshape(R_, trips, 1024, 8)
    m, s = torch.full((R_, 1024), float("-inf")), torch.zeros(R_, 1024)
    for i in range(trips):
        c = buf[:, i]
        nm = torch.maximum(m, c.amax(-1))
        acc = torch.exp(c - nm[..., None]).nan_to_num(0.0).sum(-1)
        s = s * (1.0 if fault == "no_rescale" else torch.exp(m - nm).nan_to_num(0.0)) + acc
        m = nm
    gm = m.amax(-1, keepdim=True)
    lse = gm[:, 0] + torch.log((s * torch.exp(m - gm).nan_to_num(0.0)).sum(-1))
    t = tgt.long()
    valid = (t >= 0) & (t < V)
    sc = C.GSCALE / (R_ if fault == "scale_by_rows" else int(valid.sum()))
    g = torch.zeros(R_, Vp)
    g[:, :V] = torch.exp(xf[:, :V] - lse[:, None])
    hot = torch.where(t + 1 < V, t + 1, t - 1) if fault == "target_off_by_one" else t
    g[torch.arange(R_)[valid], hot[valid]] -= 1.0
    g = g * sc * valid[:, None]
    return g.to(BF), torch.where(valid, lse, torch.zeros_like(lse))


@pytest.mark.parametrize("V,kind", [(300, "normal3"), (16389, "ramp_up"), (32002, "ramp_down")])
@pytest.mark.parametrize("fault", [None, "pad_in_lse", "no_rescale", "scale_by_rows", "target_off_by_one"])
def test_ce_seeded_fault_is_rejected(fault, V, kind):
    tgt = C.ce_targets(V)
    x0 = C.ce_logits(V, kind, tgt, C.pad8(V) + 24)
    ref = LE.ce_reference(x0, tgt, V, C.GSCALE)
    dl, lse = _emu_ce(x0, tgt, V, fault)
    hits = []
    for name, check in (("lse", lambda: LE.assert_bounded(lse, ref["lse"], ref["lse_bound"] * ref["valid"], "lse", tile=(1, 1))),
                        ("dl", lambda: LE.assert_bounded(dl, ref["dlogits"], ref["dl_bound"], "dlogits"))):
        try:
            check()
        except AssertionError:
            hits.append(name)
    if fault is None:
        assert hits == []
    elif fault == "no_rescale" and (V <= 8192 or kind == "ramp_down"):
        assert hits == []                               # one chunk per thread, or a maximum that never rises: the rescale is idle -- which is
    elif fault == "pad_in_lse" and V % 8 == 0:          # why the GPU cases carry V > 8192 with a rising ramp, and V % 8 != 0
        assert hits == []
    elif fault in ("pad_in_lse", "no_rescale"):
        assert hits == ["lse", "dl"]
    else:
        assert hits == ["dl"]


# ---- RoPE
def _emu_rope(x, cos, sin, nheads, hd, backward=False, fault=None):
    if fault == "table_row_shift":                      # row r rotated with table row r + 1
        cos, sin = cos.roll(-1, 0), sin.roll(-1, 0)
    out = OR.rope_apply_(x.clone(), cos, sin, nheads, hd, backward=backward)
    half = hd // 2
    if fault == "sine_sign_one_head":
        h = nheads - 1
        out[:, h * hd:(h + 1) * hd] = OR.rope_apply_(x[:, h * hd:(h + 1) * hd].clone(), cos, -sin, 1, hd, backward=backward)
    if fault == "single_rounding":
        v = x.float().reshape(x.shape[0], nheads, hd)
        x1, x2, c, s = v[..., :half], v[..., half:], cos.float()[:, None], sin.float()[:, None]
        out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(x.shape[0], -1).to(BF)
    return out


@pytest.mark.parametrize("hd", [16, 80, 128])
@pytest.mark.parametrize("fault", ["sine_sign_one_head", "table_row_shift", "single_rounding"])
def test_rope_seeded_fault_is_rejected(fault, hd):
    nheads, R_ = 6, 77
    cos, sin = OR.rope_table(C.rope_positions(R_, hd), C.inv_freq(hd // 2))
    x = rnd(R_, nheads * hd, seed=hd)
    with pytest.raises(AssertionError, match="not bit-equal"):
        LE.assert_bit_equal(_emu_rope(x, cos, sin, nheads, hd, fault=fault), OR.rope_apply_(x.clone(), cos, sin, nheads, hd), fault)
    if fault != "single_rounding":                      # the backward has one rounding by design
        with pytest.raises(AssertionError):
            LE.assert_ulp(_emu_rope(x, cos, sin, nheads, hd, True, fault), LE.rope_bwd_reference(x, cos, sin, nheads, hd), 1, 1e-3, fault)
    cref, _ = LE.rope_table_reference(C.rope_positions(R_, hd)[:, None].expand(R_, hd // 2), C.inv_freq(hd // 2))
    with pytest.raises(AssertionError):                 # and the table criterion sees a table shifted by one row
        LE.assert_ulp(cos.roll(-1, 0), cref, 1, 1e-3, "shifted table")


# ---- colsum
@pytest.mark.parametrize("fault", [None, "last_row_block", "accumulate_ignored"])
@pytest.mark.parametrize("M,N", [(129, 65), (777, 300), (8193, 64)])
def test_colsum_seeded_fault_is_rejected(M, N, fault):
    x, g0 = rnd(M, N, seed=M + N), rnd(N, seed=N)
    ref, bound = LE.colsum_reference(x, g0, True)
    P = min(64, -(-M // 128))
    keep = M - (M - (P - 1) * -(-M // P)) if fault == "last_row_block" else M
    out = (x.float()[:keep].sum(0) + (0 if fault == "accumulate_ignored" else g0.float())).to(BF)
    if fault is None:
        LE.assert_bounded(out, ref, bound, "colsum emulation", tile=(1, 64))
        return
    with pytest.raises(AssertionError, match="over the bound"):
        LE.assert_bounded(out, ref, bound, fault, tile=(1, 64))


def test_exact_witnesses_see_a_row_counted_twice():
    class Twice:
        @staticmethod
        def colsum(x, grad, accumulate):
            OR.colsum(torch.cat([x, x[-1:]]) if bool(((x == 0) | (x == 1)).all()) else x, grad, accumulate)      # the witness input only

        @staticmethod
        def grad_sumsq(x, out, accumulate=False, ws=None):
            OR.grad_sumsq(torch.cat([x, x[-8:]]) if bool((x.abs() == 1).all()) else x, out, accumulate)
    with pytest.raises(AssertionError, match="witness"):
        C.run_colsum(Twice, CPU, 129)
    with pytest.raises(AssertionError, match="witness"):
        C.run_sumsq(Twice, CPU, 8000)
