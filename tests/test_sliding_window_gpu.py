"""-m gpu: sliding-window attention (Mistral, query q attends keys q - W < k <= q) on the gfx950 kernels.

Kernel level: mantis_attn_fwd_window / mantis_attn_bwd_window against oracle.ops_ref.attn_fwd / attn_bwd with the window written as
per-query lower key bounds kstart[q] = max(sample start, q - W + 1) -- every kernel branch: the 64-row hd-128 forward (L >= 1024), the
32-row forward, the dQ kernel, the grouped dK/dV kernel (hd 128, G = 4) and the per-query-head dK/dV kernel with its workspace and group
reduction; key masks with rows whose whole window is padding; packed segments.  Model level: the Idefics2 step against the reference's
windowed fixture, the full-width reduced-depth step at T = 8192, W = 4096 against the oracle with windowed attention, and activation
checkpointing with the window engaged at the full width."""

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests import helpers as Hh

DEV = "cuda"
BF = torch.bfloat16
pytestmark = pytest.mark.gpu


def K():
    import mantis_amd.hip_ops as k
    return k


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def key_mask(B, L, pads):
    """pads: per row (left, right) padding lengths -> int32 [B, L] or None."""
    if pads is None:
        return None
    m = torch.ones(B, L, dtype=torch.int32)
    for b, (lp, rp) in enumerate(pads):
        m[b, :lp] = 0
        if rp:
            m[b, L - rp:] = 0
    return m


def bounds(B, L, W, cuts):
    """(segment kstart, segment qend or None, windowed kstart for the oracle)."""
    pos = torch.arange(L, dtype=torch.int32)
    ks = torch.zeros(B, L, dtype=torch.int32)
    qe = torch.full((B, L), L, dtype=torch.int32)
    for b, cs in enumerate(cuts or []):
        edges = [0] + list(cs) + [L]
        for a, e in zip(edges[:-1], edges[1:]):
            ks[b, a:e] = a
            qe[b, a:e] = e
    kw = torch.maximum(ks, pos[None] - W + 1)
    return (ks, qe, kw) if cuts else (None, None, kw)


def group_cols(H, Hkv, hd, g):
    G = H // Hkv
    return (list(range(g * G * hd, (g + 1) * G * hd)), list(range(H * hd + g * hd, H * hd + (g + 1) * hd)),
            list(range((H + Hkv) * hd + g * hd, (H + Hkv) * hd + (g + 1) * hd)))


def run_window(B, L, H, Hkv, hd, W, pads=None, cuts=None, no_workspace=False, seed=0):
    k = K()
    qkv = rnd(B * L, (H + 2 * Hkv) * hd, seed=seed + L)
    do = rnd(B * L, H * hd, seed=seed + L + 1)
    km = key_mask(B, L, pads)
    if km is not None:
        do = do * km.reshape(B * L, 1).to(BF)
    ks, qe, kw = bounds(B, L, W, cuts)
    dv = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    qd, dod = qkv.to(DEV), do.to(DEV)
    scale = hd ** -0.5
    o, lse = k.attn_fwd(qd, B, L, H, Hkv, hd, dv(km), scale, True, kstart=dv(ks), window=W)
    d = k.attn_bwd(qd, o, dod, lse, B, L, H, Hkv, hd, dv(km), scale, True, kstart=dv(ks), qend=dv(qe), no_workspace=no_workspace,
                   window=W)
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and torch.isfinite(d.float()).all(), "non-finite output or gradient"
    return qkv, do, km, kw, o, lse, d


def check_against_oracle(B, L, H, Hkv, hd, W, pads=None, cuts=None, no_workspace=False):
    """Two KV groups (the first and the last) through the oracle on the device, with the window as kstart."""
    qkv, do, km, kw, o, lse, d = run_window(B, L, H, Hkv, hd, W, pads, cuts, no_workspace)
    G = H // Hkv
    scale = hd ** -0.5
    for g in sorted({0, Hkv - 1}):
        qc, kc, vc = group_cols(H, Hkv, hd, g)
        cols = torch.tensor(qc + kc + vc)
        sub = qkv[:, cols].to(DEV)
        dsub = do[:, torch.tensor(qc)].to(DEV)
        with torch.device(DEV):
            oref, lref = R.attn_fwd(sub, B, L, G, 1, hd, None if km is None else km.to(DEV), scale, True, kstart=kw.to(DEV))
            dref = R.attn_bwd(sub, oref, dsub, lref, B, L, G, 1, hd, None if km is None else km.to(DEV), scale, True, kstart=kw.to(DEV))
        valid = torch.isfinite(lref).transpose(1, 2).reshape(B * L, G, 1).expand(B * L, G, hd).reshape(B * L, G * hd)
        oc = o[:, torch.tensor(qc, device=DEV)].float()
        what = f"B{B} L{L} H{H}/{Hkv} hd{hd} W{W} pads{pads} cuts{cuts} group{g}"
        assert (oc[~valid] == 0).all(), f"{what}: rows that see no key must give 0"
        r = rel(oc * valid, oref.float() * valid)
        assert r <= 2e-2, f"{what}: o rel_l2 {r:.3e}"
        lsel = lse[:, g * G:(g + 1) * G]
        fin = torch.isfinite(lref)
        assert torch.equal(torch.isfinite(lsel), fin), f"{what}: lse finiteness"
        assert rel(lsel[fin], lref[fin]) <= 2e-3, what
        dv_norm = float(dref[:, (G + 1) * hd:].float().norm())
        for name, dc, rc in (("dq", qc, slice(0, G * hd)), ("dk", kc, slice(G * hd, (G + 1) * hd)),
                             ("dv", vc, slice((G + 1) * hd, (G + 2) * hd))):
            got = d[:, torch.tensor(dc, device=DEV)].float()
            if W == 1 and name != "dv":
                # one visible key per query: softmax has no gradient w.r.t. its only score, dQ = dK = 0 up to the rounding of
                # D = rowsum(dO * O) against dP -- both sides are noise, so bound them against the gradient that carries signal (dV)
                assert float(got.norm()) <= 5e-2 * dv_norm and float(dref[:, rc].norm()) <= 5e-2 * dv_norm, f"{what}: {name}"
                continue
            r = rel(got, dref[:, rc].float())
            assert r <= 3e-2, f"{what}: {name} rel_l2 {r:.3e}"
    return o, d


MISTRAL = [(2, L, 32, 8, 128, W) for L in (4097, 8192) for W in (4096, 4000, 100, 1)]


@pytest.mark.parametrize("B,L,H,Hkv,hd,W", MISTRAL)
def test_window_mistral_geometry(B, L, H, Hkv, hd, W):
    """64-row forward, dQ, grouped dK/dV (G = 4) at Mistral's 32/8 x 128."""
    check_against_oracle(B, L, H, Hkv, hd, W)


# (B, L, H, Hkv, hd, W, pads, no_workspace): masks, the 32-row forward (hd 128 below L = 1024, hd 64), the per-query-head dK/dV with its
# workspace + reduction (G = 1, G = 3 at hd 128, G = 4 at hd 64) and the group kernel without a workspace (G = 2)
SMALL = [(2, 700, 32, 8, 128, 100, None, False),
         (2, 700, 32, 8, 128, 100, [(0, 250), (0, 30)], False),         # row 0: the last 150 queries see only padding
         (2, 700, 8, 2, 128, 100, [(150, 0), (0, 0)], False),           # left padding
         (2, 700, 8, 8, 64, 100, [(0, 0), (0, 260)], False),
         (2, 1100, 8, 2, 64, 300, [(0, 400), (20, 0)], False),
         (1, 1100, 6, 2, 128, 90, [(0, 200)], False),
         (2, 600, 8, 8, 128, 64, [(0, 100), (0, 0)], False),
         (1, 900, 4, 2, 128, 130, [(0, 180)], True)]


@pytest.mark.parametrize("B,L,H,Hkv,hd,W,pads,no_ws", SMALL)
def test_window_masks_and_kernel_paths(B, L, H, Hkv, hd, W, pads, no_ws):
    check_against_oracle(B, L, H, Hkv, hd, W, pads, no_workspace=no_ws)


@pytest.mark.parametrize("L,H,Hkv,hd,W,cuts", [(1200, 8, 2, 128, 100, [300, 310, 900]), (700, 4, 4, 64, 80, [100, 110, 600]),
                                                (1300, 8, 2, 64, 150, [300, 310, 900])])
def test_window_with_packed_segments(L, H, Hkv, hd, W, cuts):
    """Packed samples under the window: per sample, q - W < k <= q; the second segment -- longer than W -- equals that segment run alone
    with the window."""
    o, _ = check_against_oracle(1, L, H, Hkv, hd, W, cuts=[cuts])
    a, e = cuts[1], cuts[2]
    assert e - a > W and e <= L
    qkv = rnd(L, (H + 2 * Hkv) * hd, seed=L)
    o1, _ = K().attn_fwd(qkv[a:e].to(DEV), 1, e - a, H, Hkv, hd, None, hd ** -0.5, True, window=W)
    r = rel(o[a:e].float(), o1.float())
    assert r <= 1e-2, r


@pytest.mark.parametrize("B,L,H,Hkv,hd", [(2, 700, 8, 2, 128), (1, 1100, 32, 8, 128), (2, 300, 8, 8, 64), (1, 500, 6, 2, 128)])
def test_window_not_shorter_than_row_is_plain_causal_bitwise(B, L, H, Hkv, hd, monkeypatch):
    """The window entries with window >= L run the plain causal kernels: the same bits as mantis_attn_fwd / mantis_attn_bwd."""
    k = K()
    monkeypatch.setattr(k, "window_engaged", lambda window, Lseq: window is not None)     # call the window entries whatever the length
    qkv = rnd(B * L, (H + 2 * Hkv) * hd, seed=5).to(DEV)
    do = rnd(B * L, H * hd, seed=6).to(DEV)
    km = key_mask(B, L, [(0, 17)] + [(0, 0)] * (B - 1)).to(DEV)
    s = hd ** -0.5
    o0, l0 = k.attn_fwd(qkv, B, L, H, Hkv, hd, km, s, True)
    d0 = k.attn_bwd(qkv, o0, do, l0, B, L, H, Hkv, hd, km, s, True)
    for W in (L, L + 5):
        o1, l1 = k.attn_fwd(qkv, B, L, H, Hkv, hd, km, s, True, window=W)
        d1 = k.attn_bwd(qkv, o1, do, l1, B, L, H, Hkv, hd, km, s, True, window=W)
        assert torch.equal(o0, o1) and torch.equal(l0, l1) and torch.equal(d0, d1), W


def _idefics2_window_model(window):
    from mantis_amd.configuration_idefics2 import Idefics2Config
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
    meta, sd = Hh.golden_cfg_and_weights("idefics2")
    meta["text"] = dict(meta["text"], sliding_window=window)
    model = Idefics2ForConditionalGeneration(Idefics2Config.from_oracle_meta(meta), device=DEV, init=None)
    model.load_reference_state_dict(sd)
    return model


def test_idefics2_step_matches_windowed_reference(monkeypatch):
    """The Idefics2 step on the HIP kernels with the text model's sliding window (W = 24, T = 100, a row padded by more than W) against
    the reference's windowed fixture: the loss within a quarter of what the window moves it, and the oracle restated with the window --
    which reproduces the fixture on the CPU (tests/test_sliding_window.py) -- activation by activation and gradient by gradient."""
    import oracle.idefics2_ref as O
    from tests.test_sliding_window import FIXTURE, windowed_attention
    z = np.load(FIXTURE)
    W = int(z["sliding_window"])
    zz = Hh.ZDict({k: z[k] for k in ("input_ids", "attention_mask", "labels")})
    zz["pixel_values"] = z["pixel_values"].astype(np.float32)
    model = _idefics2_window_model(W)
    assert model._ensure_grad_arena()
    rec = {}
    out = model.engine.step_from_batch(Hh.idefics2_batch(zz), compute_grads=True, overwrite_grads=True, need_logits=True, record=rec)
    torch.cuda.synchronize()
    loss = float(out["loss"].float().cpu())
    gap = abs(float(z["loss"]) - float(z["loss_nowindow"]))
    assert abs(loss - float(z["loss"])) < 0.25 * gap, (loss, float(z["loss"]), float(z["loss_nowindow"]))
    monkeypatch.setattr(O, "attention", windowed_attention(W))
    Hh.check_idefics2_step_against_oracle(model, Hh.build_idefics2_oracle_bf16(), zz, out, rec)
    for name, p in model.named_parameters():      # and against the reference's own fp32 gradients
        if p.requires_grad and "grad." + name in z.files and np.linalg.norm(z["grad." + name]) > 1e-12:
            g = p.grad.float().cpu().numpy()
            assert Hh.cosine(g, z["grad." + name]) >= 0.99, name


def test_idefics2_full_width_window_checkpointing_bitwise():
    """Mantis-8B-Idefics2 at full width, reduced depth, one 8192-token row (W = 4096 engaged): `gradient_checkpointing_enable()` gives the
    same loss and gradient arena bit for bit, and the window changes the step (against sliding_window=None on the same weights)."""
    from mantis_amd import configuration_idefics2 as C
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
    from mantis_amd.trainer import MantisHipTrainer
    import bench
    cfg = C.mantis_8b_idefics2()
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    cfg.perceiver_config.resampler_depth = 1
    model = Idefics2ForConditionalGeneration(cfg, device=DEV, seed=0)
    batch = bench.synthetic_batch_idefics2(cfg, 1, 8192, 2, 448, 0)
    tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
    res = []
    for on in (False, True):
        (model.gradient_checkpointing_enable if on else model.gradient_checkpointing_disable)()
        for p in model.parameters():
            p.grad = None
        loss = tr.training_step(model, batch)
        torch.cuda.synchronize()
        res.append((loss.clone(), model.grad_arena.clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    assert torch.equal(res[0][1], res[1][1]), "gradients differ with activation checkpointing under the window"
    model.gradient_checkpointing_disable()
    model.config.text_config.sliding_window = None
    for p in model.parameters():
        p.grad = None
    l_full = tr.training_step(model, batch)
    torch.cuda.synchronize()
    assert not torch.equal(l_full, res[0][0]), "the window did not change the 8192-token step"


def test_idefics2_full_width_window_vs_oracle(monkeypatch):
    """Mantis-8B-Idefics2 at FULL WIDTH, reduced depth (SigLIP-so400m NaViT 448^2, perceiver 16/4 x 96, Mistral 4096 / 14336 with 32/8 x 128
    heads, V = 32003), one 8192-token row with the preset's W = 4096 engaged -- the 64-row forward and the grouped dK/dV window kernels inside
    the real decoder -- against the Idefics2 oracle (fp32, on the device) with its attention restated with the window, on the same
    bf16-rounded weights: loss, decoder layer outputs, and every gradient at SURVEY 8c's bars (0.999 / 2e-2, relaxed only where the
    reference's own bf16 run deviates more at full width: tests/golden/bf16_envelope.json, as the window-less full-width check)."""
    import oracle.idefics2_ref as O
    from mantis_amd import configuration_idefics2 as C
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
    from oracle.idefics2_ref import Idefics2Ref
    from tests.test_sliding_window import windowed_attention
    import bench
    cfg = C.mantis_8b_idefics2()
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    cfg.perceiver_config.resampler_depth = 1
    W, T = cfg.text_config.sliding_window, 8192
    assert W == 4096
    model = Idefics2ForConditionalGeneration(cfg, device=DEV, seed=0)
    batch = bench.synthetic_batch_idefics2(cfg, 1, T, 2, 448, 0)
    assert model._ensure_grad_arena()
    rec = {}
    out = model.engine.step_from_batch(batch, compute_grads=True, overwrite_grads=True, need_logits=False, record=rec)
    torch.cuda.synchronize()
    loss = float(out["loss"].float().cpu().reshape(-1)[0])
    grads = {n: p.grad.float().cpu().numpy() for n, p in model.named_parameters() if p.requires_grad}
    layers = {k: v.float().cpu().numpy() for k, v in rec.items() if k.startswith("llm_layer")}
    del out, rec
    meta = dict(vision=cfg.vision_config.to_dict(), perceiver=cfg.perceiver_config.to_dict(), text=cfg.text_config.to_dict(),
                image_token_id=cfg.image_token_id)
    monkeypatch.setattr(O, "attention", windowed_attention(W))
    with torch.device(DEV):
        oracle = Idefics2Ref({n: p.detach().float() for n, p in model.named_parameters()}, meta)
        orec = {}
        oloss, _ = oracle.forward(batch["input_ids"].to(DEV), batch["pixel_values"].to(DEV), None, batch["attention_mask"].to(DEV),
                                  batch["labels"].to(DEV), record=orec)
        oloss.backward()
    torch.cuda.synchronize()
    assert abs(loss - float(oloss)) <= 5e-3 * abs(float(oloss)), (loss, float(oloss))
    am = batch["attention_mask"].numpy().astype(bool)
    for k, a in layers.items():
        r = Hh.rel_l2(a[am], orec[k].detach().float().cpu().numpy()[am])
        assert r < 3e-2, (k, r)
    env = Hh.bf16_envelope("oracle_bf16:idefics2_full_width")
    worst_c, worst_r, n = 1.0, 0.0, 0
    for name, g in grads.items():
        og = oracle.w[name].grad
        if og is None:
            assert not g.any(), name
            continue
        og = og.float().cpu().numpy()
        if np.linalg.norm(og) < 1e-12:
            assert np.linalg.norm(g) < 1e-6, name
            continue
        c, r = Hh.cosine(g, og), Hh.rel_l2(g, og)
        cbar, rbar = Hh.envelope_bars(env, name)
        assert c >= cbar and r <= rbar, (name, c, r, cbar, rbar)
        worst_c, worst_r, n = min(worst_c, c), max(worst_r, r), n + 1
    assert n >= 20
    print(f"idefics2 full width, T {T}, W {W} vs windowed oracle: loss {loss:.5f} / {float(oloss):.5f}, {n} gradients, "
          f"worst cosine {worst_c:.5f}, worst rel-L2 {worst_r:.4f}", flush=True)
