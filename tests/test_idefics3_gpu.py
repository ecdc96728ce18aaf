"""-m gpu: the Idefics3 path on the gfx950 kernels.

Kernel level: mantis_pixel_shuffle against the closed form, bit for bit (a copy is a copy), and its unsupported codes.  Model level: the
reference's fixtures through engine.step_from_batch against the bf16 restatement (tests/idefics3_ref.py) at the project's bars (loss rtol
5e-3, GRAD_COS / GRAD_REL); a full-width, reduced-depth step against the restatement with per-tensor bars max(2e-2, ENVELOPE_FACTOR x the
reference's own bf16 deviation) from tests/golden/idefics3/bf16_envelope.json; bitwise determinism; FusedAdamW against torch AdamW."""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import idefics3_ref as R

DEV = "cuda"
BF = torch.bfloat16
pytestmark = pytest.mark.gpu


def K():
    import mantis_amd.hip_ops as k
    return k


# ----------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("I,H,C,s", [(3, 4, 64, 2), (2, 8, 64, 4), (1, 27, 64, 3), (8, 26, 1152, 2)])
def test_pixel_shuffle_kernel_equals_the_closed_form_bit_for_bit(I, H, C, s):
    k = K()
    x = torch.randn(I, H * H, C, generator=torch.Generator().manual_seed(I * 1000 + H)).to(BF)
    want = R.pixel_shuffle_closed_form(x, s)
    got = k.pixel_shuffle(x.reshape(I * H * H, C).to(DEV), I, H, s)
    torch.cuda.synchronize()
    assert got.shape == (I * (H // s) ** 2, s * s * C) and got.is_contiguous()
    assert torch.equal(got.cpu().view(torch.int16), want.reshape(got.shape).view(torch.int16))
    # a strided input (rows of a wider buffer) reads the same elements
    wide = torch.zeros(I * H * H, C + 16, dtype=BF, device=DEV)
    wide[:, :C] = x.reshape(I * H * H, C).to(DEV)
    got2 = k.pixel_shuffle(wide[:, :C], I, H, s)
    torch.cuda.synchronize()
    assert torch.equal(got2, got)


def test_pixel_shuffle_kernel_refuses_what_it_does_not_cover():
    from mantis_amd._lib import MantisHipError
    k = K()
    with pytest.raises(MantisHipError, match="rc=-2"):                      # C % 8 != 0
        k.pixel_shuffle(torch.zeros(16, 12, dtype=BF, device=DEV), 1, 4, 2)
    with pytest.raises(MantisHipError, match="rc=-2"):                      # H % s != 0
        k.pixel_shuffle(torch.zeros(16, 64, dtype=BF, device=DEV), 1, 4, 3)
    with pytest.raises(ValueError):                                         # row count is not I * H * H
        k.pixel_shuffle(torch.zeros(15, 64, dtype=BF, device=DEV), 1, 4, 2)
    with pytest.raises(ValueError):                                         # a host tensor never reaches the kernel
        k.pixel_shuffle(torch.zeros(16, 64, dtype=BF), 1, 4, 2)


# ----------------------------------------------------------------------------------------------------------- the step on the fixtures
@pytest.mark.parametrize("case", R.CASES)
def test_step_matches_restatement(case):
    z = R.load_case(case)
    model = R.build_product(DEV, case)
    oracle = R.Idefics3Ref.from_golden(case, bf16_weights=True)
    assert model._ensure_grad_arena()
    rec = {}
    out = model.engine.step_from_batch(R.batch(z), compute_grads=True, overwrite_grads=True, need_logits=True, record=rec)
    torch.cuda.synchronize()
    rep = Hh.check_idefics2_step_against_oracle(model, oracle, z, out, rec, loss_rtol=5e-3, grad_cos=Hh.GRAD_COS, grad_rel=Hh.GRAD_REL)
    loss, ref, alt = float(out["loss"].cpu()), float(z["loss"]), float(z["loss_ignoring_image_labels"])
    print(f"    idefics3 {case}: loss {loss:.5f} (reference fp32 {ref:.5f}, image labels ignored {alt:.5f}); worst gradient cosine "
          f"{min(c for c, _ in rep.values()):.5f}, worst rel {max(r for _, r in rep.values()):.4f}", flush=True)
    assert abs(loss - ref) < 0.03 * ref
    # integers exact: cross-entropy rows / targets are the reference's (image_token_id labels counted), one slot per token
    ids, am, lab = z["input_ids"], z["attention_mask"], z["labels"]
    B, T = ids.shape
    valid = (am != 0) & (lab != -100)
    valid[:, 0] = False
    bb, tt = np.nonzero(valid)
    plan = out["plan"]
    assert np.array_equal(plan.ce_row.cpu().numpy()[: bb.size], bb * T + tt - 1)
    assert np.array_equal(plan.ce_tgt.cpu().numpy()[: bb.size], lab[bb, tt])
    if "pixel_values" in z.files:
        bi, ti = np.nonzero(ids == model.config.image_token_id)
        assert np.array_equal(plan.img_slot.cpu().numpy(), bi * T + ti)


def test_forward_and_autograd_bridge_on_the_device():
    z = R.load_case("b2_padimg_rightpad")
    model = R.build_product(DEV)
    model.eval()
    with torch.no_grad():
        out = model(**R.batch(z))
    am = z["attention_mask"].astype(bool)
    assert Hh.rel_l2(out.logits.cpu().numpy()[am], z["logits"][am]) < 3e-2
    assert abs(float(out.loss) - float(z["loss"])) <= 5e-3 * float(z["loss"])
    model.train()
    loss = model(**R.batch(z)).loss
    loss.backward()
    torch.cuda.synchronize()
    g = model._param(R.PROJ).grad.float().cpu().numpy()
    assert Hh.cosine(g, z["grad." + R.PROJ]) >= Hh.GRAD_COS


# ----------------------------------------------------------------------------------------------------------- full width
@pytest.fixture(scope="module")
def full_width():
    """8B widths (SigLIP-so400m/14 at 364^2 -> 676 patches -> 169 rows of 4608 per tile; Llama-3-8B 4096 / 14336, V = 128259), tower depth
    2, decoder depth 2; B = 2 with three and two tiles, T = 1024, right padding, every <image> run whole."""
    from mantis_amd.configuration_idefics3 import idefics3_8b_llama3
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    cfg = idefics3_8b_llama3()
    cfg.vision_config.num_hidden_layers = 2
    cfg.text_config.num_hidden_layers = 2
    model = Idefics3ForConditionalGeneration(cfg, device=DEV, seed=0)
    return model, cfg, R.full_width_batch(cfg)


def test_full_width_step_vs_restatement(full_width):
    model, cfg, batch = full_width
    oracle = R.Idefics3Ref({n: p.detach().float().cpu() for n, p in model.named_parameters()}, cfg.to_oracle_meta())
    z = Hh.ZDict(input_ids=batch["input_ids"].numpy(), attention_mask=batch["attention_mask"].numpy(), labels=batch["labels"].numpy(),
                 pixel_values=batch["pixel_values"].numpy())
    assert model._ensure_grad_arena()
    rec = {}
    out = model.engine.step_from_batch(batch, compute_grads=True, overwrite_grads=True, need_logits=True, record=rec)
    torch.cuda.synchronize()
    # integers exact
    ids, am, lab = z["input_ids"], z["attention_mask"], z["labels"]
    B, T = ids.shape
    valid = (am != 0) & (lab != -100)
    valid[:, 0] = False
    bb, tt = np.nonzero(valid)
    plan = out["plan"]
    assert np.array_equal(plan.ce_row.cpu().numpy()[: bb.size], bb * T + tt - 1)
    assert np.array_equal(plan.ce_tgt.cpu().numpy()[: bb.size], lab[bb, tt])
    bi, ti = np.nonzero(ids == cfg.image_token_id)
    assert bi.size == 5 * 169 and np.array_equal(plan.img_slot.cpu().numpy(), bi * T + ti)
    assert np.array_equal(plan.kmask.cpu().numpy() != 0, am != 0)
    assert np.array_equal(plan.position_ids.cpu().numpy(), np.broadcast_to(np.arange(T), (B, T)))
    # per-tensor bars: max(2e-2, ENVELOPE_FACTOR x the reference's own bf16 deviation at this geometry) -- helpers.envelope_bars
    env = R.bf16_envelope("oracle_bf16:idefics3_full_width")
    try:
        rep = Hh.check_idefics2_step_against_oracle(model, oracle, z, out, rec, loss_rtol=5e-3, envelope=env)
    finally:
        last = Hh.GRAD_REPORTS[-1][1] if Hh.GRAD_REPORTS else {}
        for n, (c, r) in sorted(last.items(), key=lambda kv: -kv[1][1])[:6]:
            print(f"    {n}: cos {c:.5f} rel {r:.4f} (bars {Hh.envelope_bars(env, n)})", flush=True)
    print(f"    idefics3 full width vs restatement: loss {float(out['loss'].cpu()):.5f}; worst gradient cosine "
          f"{min(c for c, _ in rep.values()):.5f}, worst rel {max(r for _, r in rep.values()):.4f}", flush=True)
    assert len(rep) == sum(1 for _, p in model.named_parameters() if p.requires_grad)


def test_full_width_step_is_bitwise_reproducible(full_width):
    import math
    from mantis_amd.trainer import MantisHipTrainer
    model, cfg, batch = full_width
    tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
    for p in model.parameters():
        p.grad = None
    l1 = tr.training_step(model, batch)
    g1 = model.grad_arena.clone()
    for p in model.parameters():
        p.grad = None
    l2 = tr.training_step(model, batch)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, model.grad_arena), "the Idefics3 step is not bitwise reproducible"
    assert math.isfinite(float(l1)) and 10.5 < float(l1) < 14.5, float(l1)        # ~ln(128259) = 11.76 (+ logit variance) at random init


# ----------------------------------------------------------------------------------------------------------- optimizer
def test_fused_adamw_step_matches_torch_adamw():
    """`FusedAdamW` after Idefics3 steps against torch.optim.AdamW + clip_grad_norm_ on fp32 copies of the restatement's weights (the same
    bf16-exact values), fed the product's bf16 gradients, at the bars of helpers.check_fused_optimizer_vs_torch: gradient norm within 1e-3,
    fp32 masters within 2e-5 relative, bf16 parameters = bf16(torch's fp32 parameters) up to one rounding."""
    from mantis_amd.optim import FusedAdamW
    from mantis_amd.trainer import MantisHipTrainer
    model = R.build_product(DEV)
    oracle = R.Idefics3Ref.from_golden(bf16_weights=True)
    tr = MantisHipTrainer(model, 1)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    tp = {n: torch.nn.Parameter(oracle.w[n].detach().clone()) for n in names}
    for n in names:
        assert torch.equal(tp[n].detach(), model._param(n).detach().float().cpu()), n
    topt = torch.optim.AdamW(list(tp.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for i, case in enumerate(["b2_padimg_rightpad", "b1_label_quirk", "b1_text_only"]):
        tr.training_step(model, R.batch(R.load_case(case)))
        for n in names:
            tp[n].grad = model._param(n).grad.detach().float().cpu().clone()
        total = torch.nn.utils.clip_grad_norm_(list(tp.values()), 1.0)
        norm = opt.clip_grad_norm(1.0)
        assert abs(float(norm) - float(total)) <= 1e-3 * float(total)
        topt.step()
        opt.step()
        opt.zero_grad(set_to_none=True)
        flat_ref = torch.zeros(model.grad_arena.numel())
        for n in names:
            flat_ref[model._grad_offs[n]: model._grad_offs[n] + tp[n].numel()] = tp[n].detach().reshape(-1)
        err = Hh.rel_l2(opt.master.cpu().numpy(), flat_ref.numpy())
        assert err < 2e-5, (i, err)
        for n in names:
            got = model._param(n).detach().float().cpu()
            assert torch.equal(got, tp[n].detach().to(torch.bfloat16).float()) or Hh.rel_l2(got.numpy(), tp[n].detach().numpy()) < 4e-3, n
