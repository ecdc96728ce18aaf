"""Inputs and criterion runs of the row-wise parity checks (norm.hip, ce.hip, rope.hip, colsum, sumsq, sum_f32, clip_scale).

Every run_* function takes the backend (`ops`: mantis_amd.hip_ops on the GPU, oracle.ops_ref on the CPU -- same signatures) and the device,
builds the seeded inputs on the CPU, calls the backend and asserts the a-priori criteria of tests/local_error.py.  The GPU tests
(tests/test_rowwise_local_error_gpu.py) and the CPU proof that the fp32 oracle passes on the very same inputs
(tests/test_local_error_checker.py) are both parametrised from the case lists below, so neither can drift from the other."""
import torch

from tests import local_error as LE
from tests.gpu_checks import rnd

BF = torch.bfloat16
DIRTY = 3e38           # pre-fill of an amax_parts buffer: any entry the kernel leaves behind shows in parts.max()


def dv(t, dev):
    return None if t is None else t.to(dev)


def pad8(n):
    return (n + 7) // 8 * 8


def _weight(d, seed):
    return (1 + 0.1 * rnd(d, seed=seed).float()).to(BF)


def _amax_rerun(ops, dev, run, out, what):
    """the same launch with an amax_parts buffer full of 3e38: the output bit-equal, parts.max() == max |out| (so every entry from the
    grid size to 2048 was cleared and every workgroup stored its own)"""
    parts = ops.amax_parts_buffer(dev)
    parts.fill_(DIRTY)
    again = run(parts)
    LE.assert_bit_equal(again, out, f"{what}: output with amax_parts")
    got, want = float(parts.max()), float(out.float().abs().max())
    assert got == want, f"{what}: amax_parts.max() = {got!r}, max |out| = {want!r}"


# ------------------------------------------------------------------------------------------------------------- RMSNorm forward
REGS_D = [512 * n for n in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16)]          # rmsnorm_fwd_regs_kernel<NCH>, every instantiation
GENERIC_D = [8, 520, 768, 4608]                                           # rmsnorm_fwd_kernel (4608 = 9 x 512 is not instantiated)
SMALL_ROWS = (1, 5, 37)
# (id, d, rows tuple, weight offset in elements)
RMS_FWD_CASES = ([(f"regs{d // 512}_d{d}", d, SMALL_ROWS, 0) for d in REGS_D] + [(f"generic_d{d}", d, SMALL_ROWS, 0) for d in GENERIC_D]
                 + [("generic_d512_w_plus_8_bytes", 512, SMALL_ROWS, 4),      # 8-byte aligned weights: the launcher must leave the 16-B regs kernel
                    ("regs1_reload_loop_8197x512", 512, (8197,), 0),          # > 4 x 2048 rows: the `while (true)` re-load of the regs kernel
                    ("generic_row_loop_4101x520", 520, (4101,), 0)])          # > 4 x 1024 rows: the generic kernel's row loop


def run_rmsnorm_fwd(ops, dev, d, rows_list, w_off, eps=1e-5):
    stat = dict(ulp=0, share=0.0, rstd=0.0)
    for rows in rows_list:
        what = f"rmsnorm_fwd {rows}x{d}" + (f" w+{2 * w_off}B" if w_off else "")
        x, w = rnd(rows, d, seed=rows + d), _weight(d, d + 1)
        wbuf = torch.zeros(d + 8, dtype=BF)
        wbuf[w_off:w_off + d] = w
        xd, wd = x.to(dev), wbuf.to(dev)[w_off:w_off + d]
        ref = LE.rmsnorm_fwd_reference(x, w, eps)
        y, rstd = ops.rmsnorm_fwd(xd, wd, eps)
        s = LE.check_rmsnorm_fwd(y, rstd, x, w, eps, what, ref=ref)
        y2, none = ops.rmsnorm_fwd(xd, wd, eps, want_rstd=False)
        assert none is None
        LE.assert_bit_equal(y2, y, f"{what}: want_rstd=False")
        _amax_rerun(ops, dev, lambda parts: ops.rmsnorm_fwd(xd, wd, eps, amax_parts=parts)[0], y, what)
        stat = {k: max(stat[k], s[k]) for k in stat}
    return stat


# ------------------------------------------------------------------------------------------------------------- RMSNorm backward
# (dres given, grad_w mode): every value of either at every kernel -- the six combinations are dealt round-robin over the (d, rows) pairs
# of a kernel, and every kernel has at least six pairs.
BWD_OPTIONS = [(True, "acc"), (False, "new"), (True, None), (False, "acc"), (True, "new"), (False, None)]
BWD_ROWS = (1, 7, 121, 1025)                  # P = 1, 1, 16, 129 partial rows: reduce_partials' tail only, exactly 16, unrolled body + tail
BWD_KERNELS = [("bwd2", [(8, BWD_ROWS + (4101,)), (1024, BWD_ROWS + (4101,))]),            # 4101 rows: P = 512 and the row loop
               ("bwd8", [(1032, BWD_ROWS), (3584, BWD_ROWS), (4088, BWD_ROWS)]),
               ("d4096", [(4096, (1, 2, 3, 7, 121, 1025, 1027))]),                         # slot 1 past the end, niter > 1, odd tail
               ("bwd16", [(4104, BWD_ROWS), (8192, BWD_ROWS)])]


def _bwd_cases():
    cases = []
    for kern, shapes in BWD_KERNELS:
        i = 0
        for d, rows_list in shapes:
            sub = []
            for rows in rows_list:
                sub.append((rows,) + BWD_OPTIONS[i % len(BWD_OPTIONS)])
                i += 1
            cases.append((f"{kern}_d{d}", d, tuple(sub)))
        assert i >= len(BWD_OPTIONS)
    return cases


RMS_BWD_CASES = _bwd_cases()                  # (id, d, ((rows, dres given, grad mode), ...))
RMS_BWD_WITNESS = [(4101, 512), (1027, 4096)]


def run_rmsnorm_bwd(ops, dev, d, sub):
    stat = dict(dx=0.0, dw=0.0)
    for rows, with_dres, gmode in sub:
        what = f"rmsnorm_bwd {rows}x{d} dres={with_dres} grad_w={gmode}"
        x, w, dy = rnd(rows, d, seed=rows + d), _weight(d, d + 1), rnd(rows, d, seed=rows + d + 2)
        rstd = LE.rmsnorm_fwd_reference(x, w, 1e-5)[1].to(torch.float32)          # the rstd handed to the kernel IS the reference's
        dres = rnd(rows, d, seed=rows + d + 3) if with_dres else None
        g0 = rnd(d, seed=d + 4)
        ref = LE.rmsnorm_bwd_reference(dy, x, w, rstd, dres, g0, gmode == "acc")
        xd, wd, dyd, rd, dresd = x.to(dev), w.to(dev), dy.to(dev), rstd.to(dev), dv(dres, dev)

        def run(parts=None, keep=None):
            g = None if gmode is None else g0.to(dev).clone()
            dx = ops.rmsnorm_bwd(dyd, xd, wd, rd, dresd, g, gmode == "acc", amax_parts=parts)
            if keep is not None:
                keep.append(g)
            return dx
        gs = []
        dx = run(keep=gs)
        stat["dx"] = max(stat["dx"], LE.assert_bounded(dx, ref["dx"], ref["dx_bound"], f"{what} dx"))
        if gmode is not None:
            stat["dw"] = max(stat["dw"], LE.assert_bounded(gs[0], ref["dw"], ref["dw_bound"], f"{what} dW"))
        _amax_rerun(ops, dev, lambda parts: run(parts, gs), dx, what)
        if gmode is not None:
            LE.assert_bit_equal(gs[1], gs[0], f"{what}: dW with amax_parts")
    return stat


def run_rmsnorm_bwd_witness(ops, dev, rows, d):
    """every row counted once: rstd = 1, x = w = 1, dy[r, r % d] = 1 -> dW[j] = the number of rows r with r % d == j, an integer <= 9"""
    r = torch.arange(rows)
    dy = torch.zeros(rows, d, dtype=BF)
    dy[r, r % d] = 1
    want = torch.bincount(r % d, minlength=d).to(torch.float32)
    assert float(want.max()) <= 9
    g = torch.full((d,), 7.0, dtype=BF).to(dev)
    ones = torch.ones(rows, d, dtype=BF).to(dev)
    ops.rmsnorm_bwd(dy.to(dev), ones, torch.ones(d, dtype=BF).to(dev), torch.ones(rows).to(dev), None, g, False)
    LE.assert_bit_equal(g.float(), want, f"rmsnorm_bwd one-hot witness {rows}x{d}")


# ------------------------------------------------------------------------------------------------------------- LayerNorm
# (d, rows tuple): every d at 1 and 5 rows; 4101 rows (> 4 x 1024: the row loop) at d = 8
LN_CASES = [(8, (1, 5, 4101)), (768, (1, 5)), (1024, (1, 5)), (1152, (1, 5)), (1280, (1, 5)), (8200, (1, 5))]


def ln_inputs(rows, d):
    """mean 30, std 1 (the one-pass variance E[x^2] - mean^2 loses everything here), one constant row among the random ones"""
    x = (30 + rnd(rows, d, seed=rows + d, dtype=torch.float32)).to(BF)
    if rows > 1:
        x[rows // 2] = 30.0
    return x, rnd(d, seed=d + 1), rnd(d, seed=d + 2)


def run_layernorm(ops, dev, d, rows_list):
    worst = 0.0
    for rows in rows_list:
        x, w, b = ln_inputs(rows, d)
        for eps in (1e-6, 1e-5):
            ref, bound = LE.layernorm_reference(x, w, b, eps)
            y = ops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), eps)
            worst = max(worst, LE.assert_bounded(y, ref, bound, f"layernorm {rows}x{d} eps={eps}"))
    return dict(y=worst)


# ------------------------------------------------------------------------------------------------------------- cross-entropy
CE_V = [1, 7, 8, 9, 300, 8192, 8193, 16389, 32002]         # > 8192: a thread owns more than one chunk and the online rescale works
CE_KINDS = ["normal3", "ramp_up", "ramp_down", "dominant"]
SENTINEL, GARBAGE = -7.25, 3e38
GSCALE, LSCALE = 0.25, 0.5


def ce_targets(V):
    """first and last column, the first column of the (partial) last chunk, two ignored, two out of range: one row each (seven rows: the
    six of the plan cannot hold the seven targets it lists)"""
    return torch.tensor([0, V - 1, (V - 1) // 8 * 8, -100, -1, V, V + 5], dtype=torch.int32)


def ce_logits(V, kind, tgt, ld):
    R_ = tgt.numel()
    x = torch.full((R_, ld), SENTINEL, dtype=BF)
    x[:, V:pad8(V)] = GARBAGE                  # large and finite: a missing tail mask turns the row's lse into inf
    if kind == "normal3":
        x[:, :V] = rnd(R_, V, seed=V, scale=3.0)
    elif kind in ("ramp_up", "ramp_down"):      # every thread's running maximum rises (or never does) chunk by chunk
        ramp = torch.linspace(-40.0, 40.0, V) if V > 1 else torch.zeros(1)
        x[:, :V] = (ramp if kind == "ramp_up" else ramp.flip(0)).to(BF)[None]
    else:
        x[:, :V] = rnd(R_, V, seed=V + 1, scale=3.0)
        t = tgt.long().clamp(0, V - 1)
        x[torch.arange(R_), t] = 60.0
    return x


def check_ce(ops, dev, x0, tgt, V, what, want_count=None):
    """one launch with write_grad=False (logits untouched), one with it; every criterion of LE.ce_reference.  -> stats"""
    ref = LE.ce_reference(x0, tgt, V, GSCALE)
    Vp, ld = pad8(V), x0.shape[1]
    td = tgt.to(dev)
    x = x0.to(dev, copy=True)
    lse0 = torch.full((x0.shape[0],), 123.0).to(dev)
    loss0, cnt0 = ops.ce_fwd_bwd(x, td, V, GSCALE, LSCALE, write_grad=False, row_lse=lse0)
    LE.assert_bit_equal(x, x0, f"{what}: write_grad=False left the logits")
    lse = torch.full((x0.shape[0],), 123.0).to(dev)
    loss, cnt = ops.ce_fwd_bwd(x, td, V, GSCALE, LSCALE, row_lse=lse)
    assert cnt.cpu().tolist() == ref["count"] == cnt0.cpu().tolist(), f"{what}: count {cnt.cpu().tolist()} vs {ref['count']}"
    if want_count is not None:
        assert ref["count"] == want_count
    LE.assert_bit_equal(lse, lse0, f"{what}: row lse of the two launches")
    stat = dict(lse=LE.assert_bounded(lse, ref["lse"], ref["lse_bound"] * ref["valid"], f"{what} row lse", tile=(1, 1)))
    if ref["count"][0]:
        want = LSCALE * float(ref["loss"])
        for l in (loss, loss0):
            assert abs(float(l.cpu()) - want) <= 2e-4 * abs(want) + 1e-6, f"{what}: loss {float(l.cpu())} vs {want}"
    else:
        assert bool(loss.cpu().isnan()) and bool(loss0.cpu().isnan()), f"{what}: loss without a valid row must be NaN, got {float(loss.cpu())}"
    xc = x.cpu()
    stat["dl"] = LE.assert_bounded(xc[:, :Vp], ref["dlogits"], ref["dl_bound"], f"{what} dlogits")
    dead = ~ref["valid"]
    assert not bool(xc[dead][:, :Vp].float().ne(0).any()), f"{what}: rows without a usable target must be zero over pad8(V) columns"
    LE.assert_bit_equal(xc[:, Vp:], x0[:, Vp:], f"{what}: columns from pad8(V) to ld")
    return stat


def run_ce(ops, dev, V, kind):
    stat = dict(lse=0.0, dl=0.0)
    tgt = ce_targets(V)
    for ld in (pad8(V), pad8(V) + 24):
        s = check_ce(ops, dev, ce_logits(V, kind, tgt, ld), tgt, V, f"ce V={V} ld={ld} {kind}", want_count=[3, 2])
        stat = {k: max(stat[k], s[k]) for k in stat}
    return stat


def run_ce_all_ignored(ops, dev, V=300):
    tgt = torch.tensor([-100, -1, V, -100, V + 5, -100, -100], dtype=torch.int32)
    x0 = ce_logits(V, "normal3", tgt, pad8(V) + 24)
    stat = check_ce(ops, dev, x0, tgt, V, f"ce V={V} every row ignored", want_count=[0, 2])
    return stat


CE_NEG_INF_V = [300, 16389]


def run_ce_neg_inf(ops, dev, V):
    """columns 8..15 are -inf (a masked vocabulary range), the targets elsewhere: torch's logsumexp is finite, and so must the kernel's be.
    At V > 8200 the thread that owns chunk 1 meets it with its running maximum still -inf and goes on to a finite chunk."""
    tgt = torch.tensor([0, V - 1, (V - 1) // 8 * 8, -100, 16, 7, V], dtype=torch.int32)
    x0 = ce_logits(V, "normal3", tgt, pad8(V))
    x0[:, 8:16] = float("-inf")
    return check_ce(ops, dev, x0, tgt, V, f"ce V={V} columns 8..15 = -inf", want_count=[5, 1])


# ------------------------------------------------------------------------------------------------------------- RoPE
# (hd, nheads, R): hd 80 is Qwen2-VL's vision head (5 chunks per half head); the last case has 1100 x 64 x 8 = 563200 work items, more than
# the 2048 x 256 threads of the capped grid: the grid-stride loop
ROPE_CASES = [(hd, nh, R_) for hd in (16, 32, 80, 128) for nh in (1, 6) for R_ in (1, 77)] + [(128, 64, 1100)]
ROPE_TABLE_HALF = [8, 40, 64]


def inv_freq(half, base=500000.0):
    return 1.0 / (base ** (torch.arange(0, 2 * half, 2, dtype=torch.float32) / (2 * half)))


def rope_positions(n, seed):
    pos = torch.randint(0, 131072, (n,), generator=torch.Generator().manual_seed(seed))
    pos[:3] = torch.tensor([0, 1, 131071])[: min(3, n)]
    return pos


def run_rope_apply(ops, dev, hd, nheads, R_):
    from oracle import ops_ref
    half = hd // 2
    cos, sin = ops_ref.rope_table(rope_positions(R_, hd), inv_freq(half))
    cd, sd = cos.to(dev), sin.to(dev)
    stat = dict(bwd_ulp=0, bwd_share=0.0)
    for spare in (0, hd + 8):                   # exact, or the V columns of a fused projection plus 8 spare: all of them untouched
        x0 = rnd(R_, nheads * hd + spare, seed=hd + nheads + R_)
        what = f"rope hd={hd} nheads={nheads} R={R_} ld={x0.shape[1]}"
        fwd = ops.rope_apply_(x0.to(dev, copy=True), cd, sd, nheads, hd).cpu()
        LE.assert_bit_equal(fwd, ops_ref.rope_apply_(x0.clone(), cos, sin, nheads, hd), f"{what} forward")
        bwd = ops.rope_apply_(x0.to(dev, copy=True), cd, sd, nheads, hd, backward=True).cpu()
        ulp, share = LE.assert_ulp(bwd[:, : nheads * hd], LE.rope_bwd_reference(x0, cos, sin, nheads, hd), 1, 1e-3, f"{what} backward")
        LE.assert_bit_equal(bwd[:, nheads * hd:], x0[:, nheads * hd:], f"{what} backward: columns past the heads")
        stat = dict(bwd_ulp=max(stat["bwd_ulp"], ulp), bwd_share=max(stat["bwd_share"], share))
    return stat


def _check_table(cos, sin, pos_rows, inv, what):
    cref, sref = LE.rope_table_reference(pos_rows, inv)
    uc, sc = LE.assert_ulp(cos, cref, 1, 1e-3, f"{what} cos")
    us, ss = LE.assert_ulp(sin, sref, 1, 1e-3, f"{what} sin")
    return dict(ulp=max(uc, us), share=max(sc, ss))


def run_rope_table(ops, dev, half, R_=300):
    pos, inv = rope_positions(R_, half), inv_freq(half)
    cos, sin = ops.rope_table(pos.to(dev), inv.to(dev))
    return _check_table(cos, sin, pos[:, None].expand(R_, half), inv, f"rope_table half={half}")


def run_rope_table_sections(ops, dev, S, half, R_=300):
    """S = 3: Qwen2-VL's multimodal sections (temporal / height / width in thirds of the frequencies); S = 2: its vision tower, inv_freq = [f | f]"""
    pos = torch.stack([rope_positions(R_, 10 * S + s).roll(s) for s in range(S)])
    if S == 2:
        inv, sec = inv_freq(half // 2, 10000.0).repeat(2), (torch.arange(half) >= half // 2).to(torch.int32)
    else:
        inv, sec = inv_freq(half, 1000000.0), (torch.arange(half) * S // half).to(torch.int32)
    cos, sin = ops.rope_table_sections(pos.to(dev), inv.to(dev), sec.to(dev))
    return _check_table(cos, sin, pos[sec.long()].t(), inv, f"rope_table_sections S={S} half={half}")


# ------------------------------------------------------------------------------------------------------------- reductions
COLSUM_M = [1, 3, 127, 128, 129, 777, 8193]          # one row block, the 128-row seam, ragged blocks, 8193: the cap of 64 blocks
COLSUM_N = [1, 63, 64, 65, 300]                      # around the 64-column workgroup
SUMSQ_N = [8, 8000, 8 * (8192 * 256 + 3)]            # the last: three chunks into the second trip of the grid-stride loop
SUM_F32_N = [1, 1023, 1024, 1025, 100000]


def run_colsum(ops, dev, M):
    worst = 0.0
    for N in COLSUM_N:
        wide = rnd(M, N + 11, seed=M + N)
        x = wide[:, 3:3 + N]                          # a column slice: ld > N, the first element 6 bytes into the row
        g0 = rnd(N, seed=N)
        for acc in (False, True):
            ref, bound = LE.colsum_reference(x, g0, acc)
            g = g0.to(dev).clone()
            ops.colsum(wide.to(dev)[:, 3:3 + N], g, acc)
            worst = max(worst, LE.assert_bounded(g, ref, bound, f"colsum {M}x{N} accumulate={acc}", tile=(1, 64)))
        m = torch.arange(M)                           # every row counted once: x[m, m % N] = 1
        hot = torch.zeros(M, N + 11, dtype=BF)
        hot[m, 3 + m % N] = 1
        want = torch.bincount(m % N, minlength=N).to(torch.float64)
        if float(want.max()) <= 256:                  # integers a bf16 holds exactly
            g = torch.full((N,), 7.0, dtype=BF).to(dev)
            ops.colsum(hot.to(dev)[:, 3:3 + N], g, False)
            LE.assert_bit_equal(g.double(), want, f"colsum one-hot witness {M}x{N}", tile=(1, 64))
    return dict(colsum=worst)


def run_sumsq(ops, dev, n, witness=True):
    x = rnd(n, seed=n % 1000, scale=0.01)
    ref = float(LE.f64(x).pow(2).sum())
    stat = {}
    for acc in (False, True):
        out = torch.full((1,), 0.5).to(dev)
        ops.grad_sumsq(x.to(dev), out, acc)
        want = ref + (0.5 if acc else 0.0)
        stat[f"acc{int(acc)}"] = LE.assert_relative(out.cpu(), want, LE.sumsq_n_add(n) * LE.U_F32, f"sumsq n={n} accumulate={acc}")
    if witness:                                       # x = +-1: the sum of squares is n exactly (n < 2^24, or a multiple of 8 below 2^27)
        pm = torch.where(torch.arange(n) % 3 == 0, -1.0, 1.0).to(BF)
        out = torch.zeros(1).to(dev)
        ops.grad_sumsq(pm.to(dev), out, False)
        assert float(out.cpu()) == float(n), f"sumsq witness n={n}: {float(out.cpu())!r}"
    return stat


def run_sumsq_ranges(ops, dev):
    lens = [0, 8, 8 * 1025]                           # nothing, one chunk, one chunk into the second trip of the 1024 threads
    offs = [0, 8, 16]
    x = rnd(16 + lens[-1], seed=5, scale=0.01)
    out = torch.full((3,), 9.0).to(dev)
    ops.sumsq_ranges(x.to(dev), torch.tensor(list(zip(offs, lens)), dtype=torch.int64).to(dev), out)
    stat = {}
    for i, (o, n) in enumerate(zip(offs, lens)):
        ref = float(LE.f64(x[o:o + n]).pow(2).sum())
        stat[f"len{n}"] = LE.assert_relative(out[i].cpu(), ref, LE.sumsq_range_n_add(n) * LE.U_F32, f"sumsq_ranges len={n}")
    return stat


def run_sum_f32(ops, dev, n):
    x = rnd(n, seed=n, dtype=torch.float32).abs()     # non-negative (tile sums of squares): sum |x| = the sum, the bound is relative
    ref = float(x.double().sum())
    stat = {}
    for acc in (False, True):
        out = torch.full((1,), 0.5).to(dev)
        ops.sum_f32(x.to(dev), out, acc)
        stat[f"acc{int(acc)}"] = LE.assert_relative(out.cpu(), ref + (0.5 if acc else 0.0), LE.sum_f32_n_add(n) * LE.U_F32,
                                                    f"sum_f32 n={n} accumulate={acc}")
    return stat


def run_clip_scale(ops, dev):
    stat = {}
    for s, max_norm in ((0.3, 1.0), (7.7, 1.0), (123456.0, 0.5), (0.0, 1.0)):       # below, above, far above max_norm; no gradient at all
        ss = torch.tensor([s], dtype=torch.float32)
        scale, norm = ops.clip_scale(ss.to(dev), max_norm)
        sref, nref = LE.clip_scale_reference(ss, max_norm)
        stat[f"s{s}"] = LE.assert_relative(scale.cpu(), sref, 4 * LE.U_F32, f"clip_scale sumsq={s} max_norm={max_norm}")
        assert abs(float(norm.cpu()) - nref) <= 4 * LE.U_F32 * nref, f"clip_scale norm sumsq={s}: {float(norm.cpu())} vs {nref}"
    assert float(ops.clip_scale(torch.zeros(1).to(dev), 1.0)[0].cpu()) == 1.0
    return stat
