"""Localised-error checks for the kernel parity tests (pure torch, imports no GPU code).

A whole-tensor relative L2 norm at 1e-2 ... 3e-2 leaves a factor 6 ... 18 over the bf16 noise of these operators (about 1.7e-3), and a
fault confined to a tile edge, a K tail, a ragged strip or one (row, head) hides in it.  The checks below bound every ELEMENT of a GEMM /
attention forward a priori from the documented rounding chain, and every (row, head) of the attention gradients relatively, and on failure
say where (row, col, 16x16 tile) the worst violations sit.  tests/test_local_error_checker.py proves on the CPU that they discriminate;
tests/test_kernel_local_error_gpu.py applies them to the kernels.

Number formats: bf16 has an 8-bit significand, unit roundoff u = 2^-8 (half an ulp, relative); round-to-nearest gives
|fl(x) - x| <= u / (1 + u) |x|, which is what absorbs the second-order terms of a two-rounding chain into "n . u".  fp32: 2^-24."""
import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24


def f64(t):
    return t.detach().cpu().to(torch.float64)


def gemm_bound(a, b, *, n_roundings, K, added=None):
    """(ref64, absdot, bound) for out = round(A . B^T [+ added]) with bf16 operands a [M, K], b [N, K].

        bound = n_roundings . 2^-8 . (scale + acc) + acc,      acc = 2 . K . 2^-24 . (|A| . |B|^T + sum |added|)
        scale = |A . B^T| + sum |added|                        (= |ref| for the plain epilogue)

    Derivation.  bf16 x bf16 products are exact in fp32 (8 + 8 significand bits).  K fp32 additions in ANY order (MFMA blocks, K-split
    slabs, a bias added to the fp32 accumulator) cost at most K . 2^-24 . sum|a||b| to first order; the factor 2 covers an MFMA adder that
    does not round to nearest (truncation doubles the roundoff) and the second-order terms.  That is `acc`, the error of the fp32 value the
    epilogue sees.  Every bf16 rounding of the operator's documented chain then costs u . |value rounded| <= u . (scale + acc):
      * plain, bias (bias joins the fp32 accumulator: oracle/ops_ref.py gemm_nt, csrc/gemm_ring.h gemm_epilogue): n_roundings = 1;
      * residual ("the product is rounded, then the residual added": gemm_ring.h `x = bf2f(f2bf(x)) + bf2f(res)`, decode.hip:69) and
        bias + residual: n_roundings = 2, `added` = (bias, residual) -- the value rounded first (product + bias) and the result are both
        <= scale in magnitude, and with the sharper u / (1 + u) the two roundings stay under 2 u . scale;
      * accumulate (reads bf16 C, adds, rounds): n_roundings = 2, `added` = the C read.
    `added`: one tensor or a tuple of tensors ([M, N] or broadcastable), everything the epilogue adds to the product.  The terms enter the
    scale by their ABSOLUTE values one by one: bias and residual may cancel in the result while the intermediate that was rounded is large."""
    a64, b64 = f64(a), f64(b)
    prod = a64 @ b64.t()
    absdot = a64.abs() @ b64.abs().t()
    terms = () if added is None else (added if isinstance(added, (tuple, list)) else (added,))
    ref, addabs = prod.clone(), torch.zeros_like(prod)
    for t in terms:
        ref += f64(t)
        addabs += f64(t).abs()
    acc = 2.0 * K * U_F32 * (absdot + addabs)
    bound = n_roundings * U_BF16 * (prod.abs() + addabs + acc) + acc
    return ref, absdot, bound


def violation_report(ratio, tile=(16, 16), first=6):
    """(worst ratio, (row, col), violation count, [tile coordinates of the first few violating tiles]) of a 2-D ratio tensor"""
    flat = int(ratio.argmax())
    r, c = divmod(flat, ratio.shape[1])
    bad = (ratio > 1.0) | ~torch.isfinite(ratio)
    idx = bad.nonzero()
    tiles = []
    for i, j in idx.tolist():
        t = (i // tile[0], j // tile[1])
        if t not in tiles:
            tiles.append(t)
            if len(tiles) == first:
                break
    return float(ratio.max()), (r, c), int(bad.sum()), tiles


def assert_elementwise(out, ref64, bound, what, tile=(16, 16)):
    """max |out - ref| / bound <= 1 over every element; returns the worst ratio.  The failure message carries the worst ratio, its
    (row, col), the number of violations and the tile coordinates of the first few violating tiles: a seam, a tail or a strip."""
    o = f64(out)
    assert o.shape == ref64.shape == bound.shape, f"{what}: shapes {tuple(o.shape)} {tuple(ref64.shape)} {tuple(bound.shape)}"
    ratio = (o - ref64).abs() / bound.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where((o == ref64) & torch.isfinite(o), torch.zeros_like(ratio), ratio)        # bound == 0: only an exact value passes
    if ratio.numel() == 0:
        return 0.0
    worst, (r, c), nbad, tiles = violation_report(ratio, tile)
    assert nbad == 0, (f"{what}: worst |out - ref| / bound = {worst:.3g} at (row {r}, col {c}); {nbad} of {ratio.numel()} elements over "
                       f"the bound; first violating {tile[0]}x{tile[1]} tiles (tile row, tile col): {tiles}")
    return worst


def ulp_distance_bf16(out, ref64):
    """Distance of `out` (bf16 values) from the correctly rounded bf16 of ref64, in bf16 ulps (signed-magnitude integer order; 0 = the
    kernel returned the correctly rounded value).  Non-finite on either side: 0 if identical bit patterns, else a huge distance."""
    def order(t):
        bits = t.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(bits >= 0x8000, 0x8000 - bits, bits)          # -x -> -(magnitude bits); +-0 -> 0
    o = out.detach().cpu().to(torch.bfloat16)
    r = ref64.detach().cpu().to(torch.float64).to(torch.float32).to(torch.bfloat16)   # fp64 -> fp32 is exact enough: see below
    # double rounding fp64 -> fp32 -> bf16 can differ from fp64 -> bf16 only when the fp64 value sits within 2^-29 (relative) of a bf16
    # tie; such a value is within half an ulp of both neighbours, so the distance measured against either is <= 1 where it should be.
    d = (order(o) - order(r)).abs()
    same = o.view(torch.int16) == r.view(torch.int16)
    fin = torch.isfinite(o.float()) & torch.isfinite(r.float())
    return torch.where(fin | same, d, torch.full_like(d, 1 << 20))


# ------------------------------------------------------------------------------------------------------------- attention
FLOOR_MULT = 0.25


def attn_rowhead_error(out, ref64, H, hd, floor_mult=FLOOR_MULT):
    """Relative L2 error per (row, head) of out [rows, H * hd] against ref64 -> (floored [rows, H] float64, unfloored [rows, H]).  The
    denominator is max(|ref row-head|, floor_mult . median |ref row-head|): a near-cancelling row (the second query row of a causal sample:
    its dQ is the difference of two nearly equal terms, and the bf16 rounding of O in rowsum(dO . O) is most of it) is measured against a
    quarter of the typical row instead of against itself, so it cannot dominate.

    A pair whose reference is EXACTLY zero has no relative error of its own, and its unfloored entry is NaN: "no verdict without the
    floor".  These pairs are structural, not near-cancelling: a query row with one visible key (the first live row of a causal sample,
    of a packed segment or of a window; a one-row segment also for dK) has P = 1 and dS = P (dP - rowsum(dO . O)) = 0 in exact arithmetic,
    for every head and whatever the seed, while an implementation leaves fp32 noise there (dP comes out of an MFMA, the row sum out of
    another summation order).  They are still held to the bar against the floored denominator, i.e. absolutely."""
    o = f64(out).reshape(-1, H, hd)
    r = ref64.reshape(-1, H, hd)
    num = (o - r).norm(dim=-1)
    den = r.norm(dim=-1)
    live = den[den > 0]
    floor = floor_mult * float(live.median()) if live.numel() else 0.0
    bad = ~torch.isfinite(o).all(dim=-1)
    inf = torch.full_like(num, float("inf"))
    err = torch.where(bad, inf, num / den.clamp_min(max(floor, 1e-300)))
    raw = torch.where(bad, inf, num / den.clamp_min(1e-300))
    raw = torch.where(~bad & (den == 0), torch.full_like(num, float("nan")), raw)
    return err, raw


def floor_verdict_flips(err, raw, bar, count=None):
    """bool [rows, H]: the counted pairs whose verdict at `bar` the denominator floor changes (over without it, within with it).  A pair
    with an exactly zero reference has no verdict without the floor (NaN, attn_rowhead_error), so there is none to change."""
    flip = (raw > bar) & (err <= bar)                                   # NaN > bar is False
    return flip if count is None else flip & count


def floor_verdict_share(err, raw, bar, count=None):
    """share of the counted (row, head) pairs whose verdict at `bar` the denominator floor changes"""
    flip = floor_verdict_flips(err, raw, bar, count)
    return float(flip.sum()) / max(1, flip.numel() if count is None else int(count.sum()))


def assert_rowhead(out, ref64, H, hd, bar, what, count=None, max_floored=0.01):
    """every counted (row, head) of `out` within `bar` of ref64 (attn_rowhead_error); count: bool [rows] or [rows, H] of the pairs that
    count (fully masked query rows are don't-care).  The floor may change the verdict of at most 1 % of the pairs.  Returns the worst error."""
    err, raw = attn_rowhead_error(out, ref64, H, hd)
    c = torch.ones_like(err, dtype=torch.bool) if count is None else (count if count.dim() == 2 else count[:, None].expand_as(err))
    err = torch.where(c, err, torch.zeros_like(err))
    nbad = int((err > bar).sum())
    r, h = divmod(int(err.argmax()), err.shape[1])
    bad_rows = sorted(set((err > bar).nonzero()[:, 0].tolist()))[:8]
    assert nbad == 0, (f"{what}: worst (row, head) rel-L2 = {float(err.max()):.3e} > {bar:.3e} at (row {r}, head {h}); {nbad} pairs over; "
                       f"first rows: {bad_rows}")
    flips = floor_verdict_flips(err, raw, bar, c)
    share = float(flips.sum()) / max(1, int(c.sum()))
    assert share <= max_floored, (f"{what}: the denominator floor changes the verdict of {share:.2%} of the (row, head) pairs (> {max_floored:.0%}); "
                                  f"first (row, head, unfloored error): {[(i, j, float(raw[i, j])) for i, j in flips.nonzero().tolist()[:8]]}")
    return float(err.max())


C_P = 2.0


def attn_fwd_bound(p64, v64, ref64, c_p=C_P):
    """Elementwise bound of the attention forward: |o - ref| <= c_p . 2^-8 . sum_j p_ij |v_jd| + 2^-8 |ref|.

    p64 [..., Lq, Lk] the fp64 softmax, v64 [..., Lk, hd] the values of the same heads, ref64 = p64 @ v64.  c_p counts the roundings on the
    P / normaliser path the kernels document (csrc/attn_fwd_body.inc, attn_fwd64_body.inc, attn_common.h):
      1   P (the exponentials relative to the running max -- <= 1, or <= 256 under attn_fwd64's lazily raised max: the same RELATIVE
          precision) is rounded to bf16 by pack_frag / pack_bf2 (round-to-nearest-even, common.h) for the P.V MFMA: 2^-8 . sum p |v|;
      1   the normaliser: l = sum p is kept in fp32 from the UNROUNDED exponentials and the running max, rescales (alpha) and 1 / l are
          fp32 too -- no bf16 rounding, but the fp32 errors of the scores (hd products), of exp2 (the hardware approximation) and of the
          l / alpha chain scale with |s| and the key count; one more 2^-8 = 2^16 fp32 roundoffs bounds them for hd <= 128 and |s| . (hd +
          keys) well under 2^16 (the test shapes: < 3e4);
      0   Q is NOT pre-scaled in bf16: the scale is folded into the fp32 scores (`s * c`, `fma(s, c, -m)`); the decode kernel scales q in
          fp32 too and keeps P in fp32 (it stays inside this bound with room to spare).
    The last term is the bf16 rounding of the output."""
    return c_p * U_BF16 * (p64 @ v64.abs()) + U_BF16 * ref64.abs()


def allowed_mask(Lq, Lk, causal=False, kmask=None, kstart=None, window=None):
    """bool [Lq, Lk]: key j visible to query i (one sample): causal j <= i, key mask, packed-sample start j >= kstart[i], sliding window
    i - window < j."""
    i = torch.arange(Lq)[:, None]
    j = torch.arange(Lk)[None, :]
    ok = torch.ones(Lq, Lk, dtype=torch.bool)
    if causal:
        ok &= j <= i
    if kmask is not None:
        ok &= (kmask != 0)[None, :]
    if kstart is not None:
        ok &= j >= kstart.long()[:, None]
    if window is not None:
        ok &= j > i - window
    return ok


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def attn_problem(qkv, B, L, H, Hkv, hd, causal, kmask=None, kstart=None, window=None):
    """Split a fused q|k|v [B*L, (H + 2 Hkv) hd] into per-sample head-major tensors with k / v repeated per query head, plus the mask.
    -> list over samples of (q [H, L, hd], k [H, L, hd], v [H, L, hd], allowed [1, L, L])"""
    rep = H // Hkv
    out = []
    for b in range(B):
        x = qkv[b * L:(b + 1) * L]
        q = x[:, : H * hd].reshape(L, H, hd).transpose(0, 1)
        k = x[:, H * hd: (H + Hkv) * hd].reshape(L, Hkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
        v = x[:, (H + Hkv) * hd:].reshape(L, Hkv, hd).transpose(0, 1).repeat_interleave(rep, dim=0)
        ok = allowed_mask(L, L, causal, None if kmask is None else kmask[b], None if kstart is None else kstart[b], window)
        out.append((q, k, v, ok[None]))
    return out


def attn_reference(q, k, v, do, scale, allowed, rep=1, emulate=False):
    """Forward and backward of one attention problem (q [H, Lq, hd], k / v [H, Lk, hd] repeated per query head, do [H, Lq, hd] or None).

    emulate=False: everything in fp64 from the bf16 inputs -- the reference.
    emulate=True: the kernels' documented rounding chain on the CPU (fp32 arithmetic, bf16 where the kernels round):
      forward   P -> bf16 for P.V, l from the unrounded P, O -> bf16                     (attn_fwd_body.inc)
      backward  P recomputed from the fp32 lse, dsum = rowsum(dO . O) from the bf16 O in fp32, P -> bf16 for dV = P^T dO,
                dS = P (dP - dsum) scale -> bf16 for dQ = dS K and dK = dS^T Q           (attn_bwd_dq_body.inc, attn_bwd_dkv_body.inc: pack_frag)
                dQ -> bf16; dK / dV of each query head -> bf16 in the GQA workspace, summed over the group -> bf16 (rep > 1), else -> bf16.
    -> dict o, lse, p (fp64 softmax, reference only) and, with do, dq [H, Lq, hd], dk / dv [H / rep, Lk, hd]"""
    dt = torch.float32 if emulate else torch.float64
    qf, kf, vf = q.to(dt), k.to(dt), v.to(dt)
    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None]).nan_to_num(0.0)
    res = {}
    if emulate:
        m = s.amax(dim=-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        pu = torch.exp(s - m)                                   # relative to the row max, as the kernels hold it
        l = pu.sum(-1, keepdim=True)
        o = (_bf(pu) @ vf) / l.clamp_min(1e-30)
        o = _bf(torch.where(l > 0, o, torch.zeros_like(o)))
    else:
        o = p @ vf
        res["p"] = p
    res["o"] = o
    res["lse"] = torch.where(torch.isinf(lse) & (lse < 0), torch.full_like(lse, float("inf")), lse)
    if do is None:
        return res
    dO = do.to(dt)
    dsum = (dO * o).sum(-1, keepdim=True)
    dP = dO @ vf.transpose(-1, -2)
    dS = p * (dP - dsum) * scale
    pr, dSr = (_bf(p), _bf(dS)) if emulate else (p, dS)
    dq = dSr @ kf
    dk = dSr.transpose(-1, -2) @ qf
    dv = pr.transpose(-1, -2) @ dO
    Hh = q.shape[0]
    if rep > 1:
        if emulate:
            dk, dv = _bf(dk), _bf(dv)
        dk = dk.reshape(Hh // rep, rep, *dk.shape[1:]).sum(1)
        dv = dv.reshape(Hh // rep, rep, *dv.shape[1:]).sum(1)
    if emulate:
        dq, dk, dv = _bf(dq), _bf(dk), _bf(dv)
    res.update(dq=dq, dk=dk, dv=dv)
    return res


def rows_major(x):
    """[H, L, hd] -> [L, H * hd] (the kernels' row layout)"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


# ------------------------------------------------------------------------------------------------------------- whole-case helpers
LSE_ABS_TOL = 2e-3
BWD_BAR_FACTOR = 3.0      # bar of the gradients = 3 x the emulation's worst (row, head) error: a different summation order over <= 391 keys


class AttnCase:
    """fp64 reference (and, lazily, the bf16 emulation) of one self-attention case on the fused q|k|v layout, computed once and shared by
    the forward and backward checks.  Fully masked query rows (no live key) are don't-care in the forward; the gradients of masked (pad)
    rows are don't-care in the backward -- the same set as the whole-tensor checks of tests/gpu_checks.py."""

    def __init__(self, qkv, do, B, L, H, Hkv, hd, causal, kmask=None, kstart=None, window=None, scale=None):
        self.B, self.L, self.H, self.Hkv, self.hd = B, L, H, Hkv, hd
        self.scale = hd ** -0.5 if scale is None else scale
        self.kmask, self.window = kmask, window
        self.probs = attn_problem(qkv, B, L, H, Hkv, hd, causal, kmask, kstart, window)
        self.do = None if do is None else [do[b * L:(b + 1) * L].reshape(L, H, hd).transpose(0, 1) for b in range(B)]
        self.ref = [attn_reference(q, k, v, None if self.do is None else self.do[b], self.scale, ok, H // Hkv)
                    for b, (q, k, v, ok) in enumerate(self.probs)]
        self._emu = None

    def emulation(self):
        if self._emu is None:
            self._emu = [attn_reference(q, k, v, None if self.do is None else self.do[b], self.scale, ok, self.H // self.Hkv, emulate=True)
                         for b, (q, k, v, ok) in enumerate(self.probs)]
        return self._emu

    def rows(self, results, name):
        """[B*L, heads * hd] of a per-sample result list"""
        return torch.cat([rows_major(r[name]) for r in results], dim=0)

    def lse(self, results):
        return torch.stack([r["lse"] for r in results])                     # [B, H, L]

    def check_forward(self, o, lse, what):
        """elementwise bound on o (every row with a live key) and |lse - ref| <= 2e-3 per element; returns the worst o ratio"""
        ref = self.rows(self.ref, "o")
        bound = torch.cat([rows_major(attn_fwd_bound(r["p"], f64(v), r["o"])) for r, (_, _, v, _) in zip(self.ref, self.probs)], dim=0)
        lref = self.lse(self.ref)
        valid = torch.isfinite(lref)                                        # [B, H, L]
        vo = valid.transpose(1, 2).reshape(self.B * self.L, self.H, 1).expand(-1, -1, self.hd).reshape(self.B * self.L, -1)
        o64 = torch.where(vo, f64(o), ref)
        worst = assert_elementwise(o64, ref, bound, f"{what} o", tile=(16, self.hd))
        d = torch.where(valid, (f64(lse) - lref).abs(), torch.zeros_like(lref))
        d = torch.where(valid & ~torch.isfinite(f64(lse)), torch.full_like(d, float("inf")), d)
        b, rem = divmod(int(d.argmax()), self.H * self.L)
        h, r = divmod(rem, self.L)
        assert float(d.max()) <= LSE_ABS_TOL, f"{what} lse: worst |lse - ref| = {float(d.max()):.3e} > {LSE_ABS_TOL} at (b {b}, head {h}, row {r})"
        return worst

    def grad_count(self):
        """bool [B*L]: rows whose gradients count"""
        if self.kmask is None:
            return torch.ones(self.B * self.L, dtype=torch.bool)
        return (self.kmask != 0).reshape(-1)

    def single_key(self):
        """window = 1 (unmasked): every query row sees only its own key, so dQ = dK = 0 exactly and dV is the group sum of dO"""
        return self.window == 1 and self.kmask is None

    def single_key_bounds(self):
        """(dq [B*L, H], dk [B*L, Hkv]): a-priori bound of the L2 norm of every (row, head) of dQ / dK when each query sees one key.
        There P = 1 and dS = (dP - D) . scale with dP = dO . v (an MFMA sum over hd) and D = rowsum(dO . O), O = v exactly: two fp32 sums
        of the same hd products in different orders, each within 2 . hd . 2^-24 . sum |dO| |v| (the `acc` of gemm_bound), so
        |dS| <= 4 . hd . 2^-24 . sum |dO| |v| . scale.  dS is rounded to bf16, multiplied by the key (dQ) or the query (dK, summed over
        the query heads of the group) and rounded again: two more factors (1 + 2^-8)."""
        dq, dk = [], []
        rep = self.H // self.Hkv
        for (q, k, v, _), do in zip(self.probs, self.do):
            ds = 4.0 * self.hd * U_F32 * (f64(do).abs() * f64(v).abs()).sum(-1) * self.scale * (1 + U_BF16) ** 2      # [H, L]
            dq.append((ds * f64(k).norm(dim=-1)).t())
            dk.append((ds * f64(q).norm(dim=-1)).reshape(self.Hkv, rep, -1).sum(1).t())
        return torch.cat(dq), torch.cat(dk)

    def backward_bars(self):
        """{name: (bar, emulation's worst (row, head) error)} for dq, dk, dv (dv alone when every query sees one key)"""
        emu, bars = self.emulation(), {}
        for name, heads in (("dq", self.H), ("dk", self.Hkv), ("dv", self.Hkv)):
            if self.single_key() and name != "dv":
                continue
            err, raw = attn_rowhead_error(self.rows(emu, name), self.rows(self.ref, name), heads, self.hd)
            c = self.grad_count()[:, None].expand_as(err)
            w = float(torch.where(c, err, torch.zeros_like(err)).max())
            share = floor_verdict_share(err, raw, BWD_BAR_FACTOR * w, c)
            assert share <= 0.01, f"{name}: the denominator floor changes the verdict of {share:.2%} of the emulation's (row, head) pairs"
            bars[name] = (BWD_BAR_FACTOR * w, w)
        return bars

    def check_backward(self, dq, dk, dv, what):
        """per-(row, head) error of dq, dk, dv within 3 x the emulation's worst; returns {name: worst error}.  When every query sees one
        key the reference of dQ and dK is zero everywhere and no relative error exists: their (row, head) norms are held to
        single_key_bounds instead, and the value returned for them is the worst norm / bound."""
        bars, worst = self.backward_bars(), {}
        zero = dict(zip(("dq", "dk"), self.single_key_bounds())) if self.single_key() else {}
        for name, heads, t in (("dq", self.H, dq), ("dk", self.Hkv, dk), ("dv", self.Hkv, dv)):
            if name in zero:
                assert not bool(self.rows(self.ref, name).any())
                norm = f64(t).reshape(-1, heads, self.hd).norm(dim=-1)
                worst[name] = assert_elementwise(norm, torch.zeros_like(norm), zero[name], f"{what} {name} (row, head) norm", tile=(16, heads))
                continue
            worst[name] = assert_rowhead(t, self.rows(self.ref, name), heads, self.hd, bars[name][0], f"{what} {name}", count=self.grad_count())
        return worst


# ------------------------------------------------------------------------------------------------------------- row-wise kernels
# norm.hip, ce.hip, rope.hip and the colsum / sumsq / sum_f32 / clip_scale reductions (tests/rowwise_cases.py holds the inputs,
# tests/test_rowwise_local_error_gpu.py applies the criteria to the kernels, tests/test_local_error_checker.py proves them on the CPU).
# Every bound has the form
#       half a bf16 ulp of the float64 reference   (the one rounding of the stored value)
#     + c . 2^-24 . sum of the |terms| the fp32 value is made of
# with c the number of fp32 roundings on the longest path to the value: pointwise operations plus the longest chain of additions any term
# passes through (Higham: a sum evaluated in ANY order errs by at most depth . u . sum |x_i| to first order).  Fused multiply-adds
# (-ffp-contract=fast) only remove roundings.  Nothing here was fitted to a kernel's output.
def bf16_round(t64):
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    return t64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def half_ulp_bf16(ref64):
    """half the spacing of bf16 at |ref| (8-bit significand: 2^(e - 8) for 2^e <= |ref| < 2^(e+1)); subnormal spacing below 2^-126"""
    _, e = torch.frexp(ref64.abs().clamp_min(2.0 ** -126))               # |ref| = m . 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(ref64), e - 9)


def as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(t.shape[0], -1)


def assert_bounded(out, ref64, bound, what, tile=(1, 8)):
    """assert_elementwise on [rows, cols] (or flat) data with the row-wise kernels' natural tile: one row x one 8-element chunk"""
    return assert_elementwise(as2d(out), as2d(ref64), as2d(bound), what, tile=tile)


def assert_ulp(out, ref64, max_ulp, max_share, what, tile=(1, 8)):
    """every element of `out` within max_ulp bf16 ulps of the correctly rounded ref64 and at most max_share of them different at all.
    -> (worst distance, share that differs).  The failure names row and 8-chunk (violation_report)."""
    d = as2d(ulp_distance_bf16(out, ref64)).to(torch.float64)
    if d.numel() == 0:
        return 0, 0.0
    worst, (r, c), nbad, tiles = violation_report(d / max(max_ulp, 0.5), tile)
    far = int((d > max_ulp).sum())
    assert far == 0, (f"{what}: {far} of {d.numel()} elements more than {max_ulp} bf16 ulp from the reference; worst {int(d.max())} ulp at "
                      f"(row {r}, col {c}); first violating (row, chunk): {tiles}")
    share = float((d > 0).sum()) / d.numel()
    rows = sorted(set((d > 0).nonzero()[:, 0].tolist()))[:8]
    assert share <= max_share, (f"{what}: {share:.3%} of the elements differ from the reference (cap {max_share:.1%}); worst {int(d.max())} "
                                f"ulp at (row {r}, col {c}); first rows: {rows}")
    return int(d.max()), share


def assert_bit_equal(out, ref, what, tile=(1, 8)):
    o, r = as2d(out.detach().cpu()), as2d(ref.detach().cpu())
    assert o.dtype == r.dtype and o.shape == r.shape, f"{what}: {o.dtype} {tuple(o.shape)} vs {r.dtype} {tuple(r.shape)}"
    ne = o.contiguous().view(torch.int16) != r.contiguous().view(torch.int16) if o.dtype == torch.bfloat16 else (o != r) & ~(o.isnan() & r.isnan())
    if bool(ne.any()):
        _, (i, j), nbad, tiles = violation_report(ne.to(torch.float64) * 2.0, tile)
        raise AssertionError(f"{what}: {nbad} of {ne.numel()} elements not bit-equal, first worst at (row {i}, col {j}): {float(o[i, j])} vs "
                             f"{float(r[i, j])}; first (row, chunk): {tiles}")


def assert_relative(value, ref, rel, what):
    value, ref = float(value), float(ref)
    err = abs(value - ref)
    assert err <= rel * abs(ref) and value == value, f"{what}: {value!r} vs {ref!r}: relative error {err / max(abs(ref), 1e-300):.3e} > {rel:.3e}"
    return err / (rel * abs(ref)) if ref else 0.0


# ---- RMSNorm
def rstd_rel_bound(d):
    """relative error of rstd = rsqrtf(ss / d + eps) against float64: d / 64 squares added per lane (the squares of bf16 values are exact),
    six levels of the wave reduction, and 6 for the division, the eps addition and rsqrtf (2 ulp, halved by the square root's
    derivative but counted whole)"""
    return (d / 64 + 12) * U_F32


def rmsnorm_fwd_reference(x, w, eps):
    """(y, rstd) of the documented chain bf16(bf16(x . rstd) . w) with float64 statistics; eps as the fp32 value the kernel receives"""
    x64 = f64(x)
    rstd = (x64.pow(2).mean(-1) + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()
    return bf16_round(bf16_round(x64 * rstd[:, None]) * f64(w)), rstd


def check_rmsnorm_fwd(y, rstd, x, w, eps, what, ref=None):
    """y within 2 bf16 ulp everywhere and different on at most 0.1 %; rstd (when returned) relative within rstd_rel_bound(d).
    -> dict(ulp, share, rstd = worst error / bound)"""
    yref, r64 = rmsnorm_fwd_reference(x, w, eps) if ref is None else ref
    ulp, share = assert_ulp(y, yref, 2, 1e-3, f"{what} y")
    stat = dict(ulp=ulp, share=share, rstd=0.0)
    if rstd is not None:
        assert rstd.dtype == torch.float32
        stat["rstd"] = assert_bounded(rstd, r64, rstd_rel_bound(x.shape[1]) * r64, f"{what} rstd", tile=(1, 1))
    return stat


def rmsnorm_bwd_dw_n_add(rows, d):
    """Longest chain of fp32 roundings a term dy . xhat passes through on its way into dW[j] (csrc/norm.hip):
         2                    xhat = x . rstd and the product dy . xhat
       + rows per accumulator one wave (generic kernels: P . 8 waves stride the rows) or one row slot (d = 4096: P . 2 slots) adds its rows
                              in turn into a register
       + fold                 the 8 waves of a workgroup add into one LDS row in wave order: 7;  d = 4096: slot 1 onto slot 0: 1
       + ceil(P / 16)         reduce_partials_kernel: row group g adds partial rows g, g + 16, ... in order
       + 16                   the 16 group sums, added in order onto 0
       + 1                    the old gradient under `accumulate`
    with P = min(512, ceil(rows / 8)) workgroups = partial rows (mantis_rmsnorm_bwd_partials)."""
    P = min(512, max(1, -(-rows // 8)))
    per_acc, fold = (-(-rows // (2 * P)), 1) if d == 4096 else (-(-rows // (8 * P)), 7)
    return 2 + per_acc + fold + -(-P // 16) + 16 + 1


def rmsnorm_bwd_reference(dy, x, w, rstd, dres, g0, accumulate):
    """float64 dx and dW from the DEVICE's rstd, with their bounds -> dict(dx, dx_bound, dw, dw_bound).

    dx = rstd . (g - xhat . dot) + dres,  g = dy . w,  xhat = x . rstd,  dot = mean(g . xhat).  Roundings on the longest path, the one through
    the dot: xhat 1, g 1, the product 1, d / 64 additions per lane, 6 reduction levels, the division 1 -- d / 64 + 6 for the chain plus
    4 -- then xhat . dot, the subtraction, the factor rstd and the residual: 4 more, and 2 for the second-order terms: c = d / 64 + 6 + 10.
    The d = 4096 kernel adds the four waves' sums of a row in order: + 4.  Each rounding is relative to a partial result that is no larger
    than the sum of the |terms| it is made of, which is what multiplies c."""
    d = x.shape[1]
    r = f64(rstd)[:, None]
    g, xhat = f64(dy) * f64(w), f64(x) * r
    dot = (g * xhat).mean(-1, keepdim=True)
    dx = r * (g - xhat * dot)
    mag = (r * g).abs() + (r * xhat).abs() * (dot.abs() + (g * xhat).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + f64(dres)
        mag = mag + f64(dres).abs()
    c = d / 64 + 6 + 10 + (4 if d == 4096 else 0)
    res = dict(dx=dx, dx_bound=half_ulp_bf16(dx) + c * U_F32 * mag)
    t = f64(dy) * xhat
    dw, mag = t.sum(0), t.abs().sum(0)
    if accumulate:
        dw, mag = dw + f64(g0), mag + f64(g0).abs()
    res.update(dw=dw, dw_bound=half_ulp_bf16(dw) + rmsnorm_bwd_dw_n_add(x.shape[0], d) * U_F32 * mag)
    return res


# ---- LayerNorm
def layernorm_reference(x, w, b, eps):
    """float64 y = (x - mean) . rstd . w + b and its bound
         half ulp + c . 2^-24 . (|x - mean| . rstd . |w| + |b|) + rstd . |w| . (d / 64 + 6) . 2^-24 . mean |x|.
    c = d / 64 + 16: rstd carries the chain of the squared deviations (d / 64 per lane + 6 levels; the deviation and its square 2, the
    division, the eps addition and rsqrtf 4) and the value four pointwise roundings (x - mean, . rstd, . w, + b), 2 for second order.
    The last term is the error of the mean itself (the same chain over the |x|), which enters y through x - mean without the factor
    |x - mean|: it is what bounds a row whose deviations cancel (a constant row)."""
    d = x.shape[1]
    x64, w64, b64 = f64(x), f64(w), f64(b)
    mean = x64.mean(-1, keepdim=True)
    dev = x64 - mean
    rstd = (dev.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()
    ref = dev * rstd * w64 + b64
    bound = (half_ulp_bf16(ref) + (d / 64 + 16) * U_F32 * (dev.abs() * rstd * w64.abs() + b64.abs())
             + rstd * w64.abs() * (d / 64 + 6) * U_F32 * x64.abs().mean(-1, keepdim=True))
    return ref, bound


# ---- cross-entropy
def ce_reference(logits, targets, V, grad_scale):
    """float64 reference of ce.hip on logits [R, ld] (columns < V count) -> dict
         valid [R], count = [valid rows, rows with a target >= V], lse [R] (0 on rows that are not valid), lse_bound [R], loss (mean over
         the valid rows, NaN without one), dlogits [R, pad8(V)] (zero on rows that are not valid and on columns >= V), dl_bound.

    lse_bound = (V / 1024 + 16) . 2^-24 . max(1, |lse|) + E,   E = (2 . range + 8 + 2 . ceil(V / 8192)) . 2^-24,
    range = the row's largest minus its smallest finite logit.  The first term: a thread adds 8 . ceil(V / 8192) exponentials, then the
    wave and block reductions and logf.  E is what __expf costs: it evaluates exp2(x . log2 e), and the fp32 rounding of that product is
    an ABSOLUTE error |x| . 2^-24 of the exponent, i.e. a RELATIVE error |x| . 2^-24 of the exponential, |x| <= range (1 more for the
    exp2 itself); the rescale factors __expf(m - nm) of a thread and __expf(m - gm) of the block reduction cost the same and their
    arguments telescope to at most `range` again (2 . range in all), with one ulp each for the ceil(V / 8192) + 1 rescales and the
    subtractions: 8 + 2 . ceil(V / 8192) covers them.  A relative error of the sum is an absolute error of its logarithm.

    dl_bound = half ulp + c . 2^-24 . sc . (p . (1 + |x - lse|) + onehot),  sc = grad_scale / count,  c = lse_bound / 2^-24 + 4 per row:
    p = __expf(x - lse) inherits the absolute error of lse and of the subtraction as a relative error (|x - lse| . 2^-24 twice: the
    subtraction and the log2 e product), 1 for exp2, then `- 1` at the target, `. sc` and sc's own division: 4.  The bound is absolute at
    the target, where p - 1 cancels: its terms p and onehot enter by their absolute values.  2^-126 on top: fp32 results below the
    smallest normal number may be flushed to zero (p . sc reaches 1e-38 at the far end of an 80-wide ramp)."""
    R_, Vp = logits.shape[0], (V + 7) // 8 * 8
    x = f64(logits)[:, :V]
    t = targets.cpu().long()
    valid = (t >= 0) & (t < V)
    cnt = int(valid.sum())
    lse = torch.logsumexp(x, dim=-1)
    fin = torch.isfinite(x)
    rng = torch.where(fin, x, torch.full_like(x, -1e300)).amax(-1) - torch.where(fin, x, torch.full_like(x, 1e300)).amin(-1)
    e_exp = (2 * rng + 8 + 2 * -(-V // 8192)) * U_F32
    lse_bound = (V / 1024 + 16) * U_F32 * lse.abs().clamp_min(1.0) + e_exp
    picked = x.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
    sc = grad_scale / cnt if cnt else 0.0
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x)
    onehot[torch.arange(R_)[valid], t[valid]] = 1.0
    dl = torch.zeros(R_, Vp, dtype=torch.float64)
    dl[:, :V] = (p - onehot) * sc * valid[:, None]
    dist = torch.where(fin, (x - lse[:, None]).abs(), torch.zeros_like(x))
    c = lse_bound / U_F32 + 4
    bound = torch.zeros_like(dl)
    bound[:, :V] = c[:, None] * U_F32 * sc * (p * (1 + dist) + onehot) * valid[:, None]
    bound = bound + (half_ulp_bf16(dl) + 2.0 ** -126) * (dl != 0)
    return dict(valid=valid, count=[cnt, int((t >= V).sum())], lse=torch.where(valid, lse, torch.zeros_like(lse)), lse_bound=lse_bound,
                loss=loss, dlogits=dl, dl_bound=bound)


# ---- RoPE
def rope_table_reference(pos_rows, inv_freq):
    """float64 cos / sin of the fp32 product float(pos) . inv_freq (one IEEE multiplication: the same on every machine); pos_rows [R, half]
    holds the position each (row, frequency) reads (rope_table: pos[:, None]; sections: pos[sec[j], r])"""
    f = (pos_rows.to(torch.float32) * inv_freq.to(torch.float32)[None]).to(torch.float64)
    return f.cos(), f.sin()


def rope_bwd_reference(x, cos, sin, nheads, hd):
    """float64 transpose of the rotation on the first nheads . hd columns -> [R, nheads . hd]"""
    Rr, half = x.shape[0], hd // 2
    v = f64(x)[:, : nheads * hd].reshape(Rr, nheads, hd)
    x1, x2 = v[..., :half], v[..., half:]
    c, s = f64(cos)[:, None, :], f64(sin)[:, None, :]
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], dim=-1).reshape(Rr, nheads * hd)


# ---- reductions
def colsum_n_add(M):
    """act.hip: P = min(64, ceil(M / 128)) row blocks of rpb = ceil(M / P) rows; a thread adds every fourth row of its block
    (ceil(rpb / 4)), the four row lanes are added (3), reduce_partials_kernel2 adds the P partial rows in order (P), then the old
    gradient under `accumulate` (1)"""
    P = min(64, max(1, -(-M // 128)))
    return -(-(-(-M // P)) // 4) + 3 + P + 1


def colsum_reference(x, g0, accumulate):
    x64 = f64(x)
    ref, mag = x64.sum(0), x64.abs().sum(0)
    if accumulate:
        ref, mag = ref + f64(g0), mag + f64(g0).abs()
    return ref, half_ulp_bf16(ref) + colsum_n_add(x.shape[0]) * U_F32 * mag


BLOCK_SUM_ADDS = 12      # common.h block_sum: six levels inside a wave, six more over the (at most 16) wave sums


def sumsq_n_add(n):
    """optim.hip mantis_sumsq: 8192 x 256 threads stride the n / 8 chunks, 8 additions per chunk (squares of bf16 values are exact in
    fp32), block_sum; sumsq_finish_kernel: 1024 threads add 8 partials each, block_sum, and the accumulate"""
    return 8 * max(1, -(-(n // 8) // (8192 * 256))) + BLOCK_SUM_ADDS + 8 + BLOCK_SUM_ADDS + 1


def sumsq_range_n_add(n):
    """sumsq_ranges_kernel: one 1024-thread workgroup per range"""
    return 8 * max(1, -(-(n // 8) // 1024)) + BLOCK_SUM_ADDS


def sum_f32_n_add(n):
    """sum_f32_kernel: 1024 threads stride the array, block_sum, the accumulate"""
    return max(1, -(-n // 1024)) + BLOCK_SUM_ADDS + 1


def clip_scale_reference(sumsq, max_norm):
    """float64 (scale, norm) from the fp32 sum the kernel read; held to 4 . 2^-24: sqrtf, the 1e-6 addition, the division, and one for
    max_norm and 1e-6 being passed as fp32"""
    s = float(sumsq)
    norm = s ** 0.5
    return min(1.0, float(torch.tensor(max_norm, dtype=torch.float32)) / (norm + float(torch.tensor(1e-6, dtype=torch.float32)))), norm
