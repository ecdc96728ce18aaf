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
