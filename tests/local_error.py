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
