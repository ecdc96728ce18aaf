"""CPU: the Idefics3 path.
  * the restatement (tests/idefics3_ref.py) against the fixtures recorded from the reference class (tests/golden/make_golden_idefics3.py),
    at the bars of tests/test_idefics2_oracle.py;
  * the PRODUCT's host logic (mantis_amd/modeling_idefics3.py over the Idefics2 engine) with the oracle's operator restatement in place
    of the HIP backend, against the same fixtures at the bars of tests/test_idefics2_host_logic.py;
  * the public contract: parameter names, the loss rule, refusals, autograd bridge, checkpointing, gradient buckets, the C-ABI entry."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import idefics3_ref as R

CASES = R.CASES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cpu_backend(monkeypatch):
    import mantis_amd.modeling_idefics2 as mod
    import mantis_amd.modeling_idefics3  # noqa: F401
    monkeypatch.setattr(mod, "K", R.backend())
    return mod


# ----------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference(case):
    z = R.load_case(case)
    m = R.Idefics3Ref.from_golden(case)
    rec = {}
    pv = z["pixel_values"] if "pixel_values" in z.files else None
    pm = z["pixel_attention_mask"] if "pixel_attention_mask" in z.files else None
    loss, logits = m.forward(z["input_ids"], pv, pm, z["attention_mask"], z["labels"], record=rec)
    loss.backward()
    seen = 0
    for k in ("vision_last_hidden_state", "connector_out", "merged_embeds", "llm_layer0_out", "llm_layer1_out"):
        if k in z.files:
            assert np.allclose(rec[k].detach().numpy(), z[k], atol=2e-5, rtol=1e-4), (k, Hh.rel_l2(rec[k].detach().numpy(), z[k]))
            seen += 1
    assert seen == (2 if pv is None else 5)
    am = z["attention_mask"].astype(bool)
    assert np.allclose(logits.detach().numpy()[am], z["logits"][am], atol=2e-5, rtol=1e-4)
    assert abs(float(loss) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"])) + 1e-6
    n = 0
    for k in z.files:
        if k.startswith("grad."):
            g = m.w[k[5:]].grad
            assert g is not None, k
            assert Hh.rel_l2(g.numpy(), z[k]) < 1e-4 or np.abs(z[k]).max() < 1e-7, (k, Hh.rel_l2(g.numpy(), z[k]))
            n += 1
    assert n >= 21
    assert all(t.grad is None for k, t in m.w.items() if k.startswith("model.vision_model."))
    # the other loss rule, from the same logits
    alt, _ = m.forward(z["input_ids"], pv, pm, z["attention_mask"], z["labels"], ignore_image_labels=True)
    assert abs(float(alt) - float(z["loss_ignoring_image_labels"])) <= 1e-5 * float(alt)


@pytest.mark.parametrize("s,H", [(2, 4), (2, 26), (3, 27), (4, 8)])
def test_pixel_shuffle_restatement_equals_the_closed_form(s, H):
    x = torch.randn(3, H * H, 16, generator=torch.Generator().manual_seed(s * 100 + H))
    want = R.pixel_shuffle_closed_form(x, s)
    assert torch.equal(R.pixel_shuffle_ref(x, s), want)
    got = R.pixel_shuffle(x.reshape(3 * H * H, 16), 3, H, s)
    assert got.shape == (3 * (H // s) ** 2, s * s * 16) and torch.equal(got, want.reshape(got.shape))
    with pytest.raises(RuntimeError):
        R.pixel_shuffle(x.reshape(3 * H * H, 16), 3, H, H + 1)


def test_fixtures_pin_the_loss_rule():
    """Every case with images counts labels equal to image_token_id; the pin case holds -100 AND image_token_id at attended positions."""
    meta, _ = R.golden_cfg_and_weights()
    IMG = meta["image_token_id"]
    for case in CASES:
        z = R.load_case(case)
        if "pixel_values" in z.files:
            assert abs(float(z["loss"]) - float(z["loss_ignoring_image_labels"])) > 1e-3 * float(z["loss"]), case
    z = R.load_case("b1_label_quirk")
    att = z["attention_mask"][:, 1:] != 0
    lab = z["labels"][:, 1:][att]
    assert (lab == -100).any() and (lab == IMG).any()
    assert ((z["labels"] == -100) & (z["input_ids"] == IMG)).any()          # some <image> positions ARE ignored: by -100, not by id


# ----------------------------------------------------------------------------------------------------------- the product on the CPU backend
@pytest.mark.parametrize("case", CASES)
def test_step_matches_restatement_and_reference(cpu_backend, case):
    z = R.load_case(case)
    model = R.build_product("cpu", case)
    oracle = R.Idefics3Ref.from_golden(case, bf16_weights=True)
    assert model._ensure_grad_arena()
    rec = {}
    out = model.engine.step_from_batch(R.batch(z), compute_grads=True, overwrite_grads=True, need_logits=True, record=rec)
    Hh.check_idefics2_step_against_oracle(model, oracle, z, out, rec)
    assert abs(float(out["loss"]) - float(z["loss"])) < 0.03 * float(z["loss"])          # vs the reference's own fp32 loss
    # integers of the plan: one slot per token, <image> tokens take the image rows in row-major order, arange positions
    ids, am = z["input_ids"], z["attention_mask"]
    B, T = ids.shape
    plan = out["plan"]
    IMG = model.config.image_token_id
    assert plan.L == T and np.array_equal(plan.position_ids.numpy(), np.broadcast_to(np.arange(T), (B, T)))
    assert np.array_equal(plan.kmask.numpy() != 0, am != 0)
    if "pixel_values" in z.files:
        bi, ti = np.nonzero(ids == IMG)
        assert np.array_equal(plan.img_slot.numpy(), bi * T + ti)
    # cross-entropy lists: exactly the reference's targets (attended, label != -100, t >= 1), image_token_id labels included
    valid = (am != 0) & (z["labels"] != -100)
    valid[:, 0] = False
    bb, tt = np.nonzero(valid)
    n = bb.size
    row, tgt = plan.ce_row.numpy(), plan.ce_tgt.numpy()
    assert row.size % 8 == 0 and np.array_equal(row[:n], bb * T + tt - 1) and np.array_equal(tgt[:n], z["labels"][bb, tt])
    assert (row[n:] == -1).all() and (tgt[n:] == -100).all()
    for n_, p in model.named_parameters():
        if n_.startswith("model.vision_model."):
            assert p.grad is None


@pytest.mark.parametrize("case", ["b1_img2", "b1_label_quirk", "b2_padimg_rightpad"])
def test_loss_counts_image_token_labels(cpu_backend, case):
    """modeling_idefics3.py:1186-1198: CrossEntropyLoss() ignores -100 only.  The product matches `loss`, not the loss with the
    image_token_id labels ignored (what the Idefics2 path would compute)."""
    z = R.load_case(case)
    model = R.build_product("cpu", case)
    model.eval()
    with torch.no_grad():
        out = model(**R.batch(z))
    loss, ref, alt = float(out.loss), float(z["loss"]), float(z["loss_ignoring_image_labels"])
    assert abs(loss - ref) <= 5e-3 * ref, (loss, ref)
    assert abs(loss - ref) < 0.25 * abs(alt - ref), (loss, ref, alt)
    assert out.logits.shape == z["logits"].shape and out.logits.dtype == torch.float32


def test_state_dict_names_match_reference():
    model = R.build_product("cpu")
    _, sd = R.golden_cfg_and_weights()
    names = {n for n, _ in model.named_parameters()}
    assert names == set(sd)
    assert "model.connector.modality_projection.proj.weight" in names and "lm_head.weight" in names
    assert not any(n.endswith("proj.bias") and "connector" in n for n in names)
    for n, p in model.named_parameters():
        assert tuple(p.shape) == tuple(sd[n].shape), n
        assert torch.equal(p.detach().float(), torch.from_numpy(sd[n])), n          # the recorded weights are bf16-exact
        assert p.requires_grad == (not n.startswith("model.vision_model.")), n


def test_grad_buckets_cover_every_trainable_parameter_once(cpu_backend):
    z = R.load_case("b1_img2")
    model = R.build_product("cpu")
    b = model.grad_buckets()
    assert sum(v.numel() for v in b.values()) == model.grad_arena.numel()
    spans = sorted((v.data_ptr(), v.numel()) for v in b.values())
    assert spans[0][0] == model.grad_arena.data_ptr()
    for (p0, n0), (p1, _) in zip(spans, spans[1:]):
        assert p0 + 2 * n0 == p1, "buckets overlap or leave a gap"
    for n, p in model.named_parameters():
        if p.requires_grad:
            a = model._grad_views[n].data_ptr()
            assert sum(1 for p0, n0 in spans if p0 <= a < p0 + 2 * n0) == 1, n
    seen = []
    model.engine.step_from_batch(R.batch(z), compute_grads=True, overwrite_grads=True, on_bucket_ready=seen.append)
    assert set(seen) == set(b) and len(seen) == len(b) and seen[0] == "head" and seen[-1] == "front"


def test_refusals(cpu_backend):
    z = R.load_case("b1_img2")
    model = R.build_product("cpu")
    b = R.batch(z)
    for kw in (dict(past_key_values=()), dict(use_cache=True), dict(inputs_embeds=torch.zeros(1, 26, 64)),
               dict(image_hidden_states=torch.zeros(2, 4, 64)), dict(output_attentions=True), dict(output_hidden_states=True),
               dict(position_ids=torch.arange(26)[None])):
        with pytest.raises(NotImplementedError):
            model(**{**b, **kw})
    for prec in ("fp8", "fp8_rowwise"):
        with pytest.raises(NotImplementedError, match="fp8"):
            model.set_precision(prec)
    assert model.set_precision("bf16") is model
    # one <image> token fewer than image hidden states
    bad = dict(b, input_ids=b["input_ids"].clone())
    bad["input_ids"][0, 3] = 5
    with pytest.raises(ValueError):
        model.engine.step_from_batch(bad, compute_grads=False)
    # a non-square padded pixel tensor, and a patch grid the scale factor does not divide: the reference would mis-shape silently
    with pytest.raises(ValueError, match="square"):
        model.engine.step_from_batch(dict(b, pixel_values=torch.randn(1, 2, 3, 56, 28)), compute_grads=False)
    with pytest.raises(ValueError, match="scale_factor"):
        model.engine.step_from_batch(dict(b, pixel_values=torch.randn(1, 2, 3, 42, 42)), compute_grads=False)
    # packed rows: refused by name on every route (engine keyword, batch key, the trainer's segment ids and its 4-D packed mask)
    seg = torch.zeros_like(b["input_ids"], dtype=torch.int32)
    seg[0, 13:] = 1
    with pytest.raises(NotImplementedError, match="segment_ids"):
        model.engine.step_from_batch(b, compute_grads=False, segment_ids=seg)
    with pytest.raises(NotImplementedError, match="segment_ids"):
        model.engine.step_from_batch(dict(b, segment_ids=seg), compute_grads=False)
    from mantis_amd.trainer import MantisHipTrainer
    with pytest.raises(NotImplementedError, match="segment_ids"):
        MantisHipTrainer(model, gradient_accumulation_steps=1).training_step(model, dict(b, segment_ids=seg))
    # a counted label outside the vocabulary
    lab = b["labels"].clone()
    lab[0, 20] = 300
    with pytest.raises(IndexError):
        model.engine.step_from_batch(dict(b, labels=lab), compute_grads=False)
    from mantis_amd.configuration_idefics3 import Idefics3Config
    with pytest.raises(NotImplementedError):
        Idefics3Config(text_config=dict(rope_scaling=dict(rope_type="llama3", factor=8.0)))
    with pytest.raises(NotImplementedError):
        Idefics3Config(text_config=dict(model_type="mistral"))


def test_config_defaults_and_preset():
    from mantis_amd.configuration_idefics3 import Idefics3Config, idefics3_8b_llama3
    c = Idefics3Config()
    assert (c.image_token_id, c.scale_factor, c.pad_token_id) == (128257, 2, 128002)
    assert (c.vision_config.hidden_size, c.vision_config.patch_size, c.text_config.rms_norm_eps) == (1152, 32, 1e-5)
    c = idefics3_8b_llama3()
    vc, tc = c.vision_config, c.text_config
    assert vc.image_size == 364 and (vc.image_size // vc.patch_size // c.scale_factor) ** 2 == 169
    assert (tc.hidden_size, tc.num_key_value_heads, tc.head_dim, tc.sliding_window) == (4096, 8, 128, None)


def test_loss_backward_through_the_autograd_bridge(cpu_backend):
    """Stock `model(**batch).loss.backward()` callers: same loss and bit-identical gradients as MantisHipTrainer.training_step."""
    from mantis_amd.trainer import MantisHipTrainer
    z = R.load_case("b2_padimg_rightpad")
    ref = R.build_product("cpu")
    l_ref = MantisHipTrainer(ref, gradient_accumulation_steps=1).training_step(ref, R.batch(z))
    model = R.build_product("cpu")
    model.train()
    out = model(**R.batch(z))
    assert out.logits is None and out.loss.requires_grad
    out.loss.backward()
    assert torch.equal(out.loss.detach(), l_ref) and torch.equal(model.grad_arena, ref.grad_arena)
    for p in model.parameters():
        p.grad = None
    model(**R.batch(z)).loss.backward()
    assert torch.equal(model.grad_arena, ref.grad_arena)
    assert type(out).__name__ == "Idefics3CausalLMOutputWithPast"


def test_trainer_accumulates_and_text_only_zeroes_the_connector(cpu_backend):
    from mantis_amd.trainer import MantisHipTrainer
    z = R.load_case("b2_padimg_rightpad")
    model = R.build_product("cpu")
    tr = MantisHipTrainer(model, gradient_accumulation_steps=2)
    l1 = tr.training_step(model, R.batch(z))
    g1 = model.grad_arena.float().clone()
    l2 = tr.training_step(model, R.batch(z))
    assert l1.dim() == 0 and abs(float(l1) - float(z["loss"]) / 2) < 0.03 * float(z["loss"]) and torch.equal(l1, l2)
    assert Hh.rel_l2(model.grad_arena.float().numpy(), 2 * g1.numpy()) < 2e-2
    model = R.build_product("cpu")
    model._ensure_grad_arena()
    model.engine.step_from_batch(R.batch(R.load_case("b1_img2")), compute_grads=True, overwrite_grads=True)
    assert model._param(R.PROJ).grad.abs().max() > 0
    model.engine.step_from_batch(R.batch(R.load_case("b1_text_only")), compute_grads=True, overwrite_grads=True)
    assert not model._param(R.PROJ).grad.any()


def test_activation_checkpointing_is_bit_identical(cpu_backend):
    z = R.load_case(CASES[0])
    res = []
    for on in (False, True):
        model = R.build_product("cpu")
        if on:
            model.gradient_checkpointing_enable()
        model._ensure_grad_arena()
        out = model.engine.step_from_batch(R.batch(z), compute_grads=True, overwrite_grads=True)
        res.append((float(out["loss"]), model.grad_arena.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


def test_fused_adamw_is_built_over_the_arena():
    from mantis_amd.optim import FusedAdamW
    model = R.build_product("cpu")
    model._ensure_grad_arena()
    opt = FusedAdamW(model, lr=1e-3)
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == n


def test_pixel_shuffle_symbol_is_declared_and_bound():
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from mantis_amd import _lib
    src = open(os.path.join(ROOT, "include", "mantis_hip.h")).read()
    assert re.search(r"\bint\s+mantis_pixel_shuffle\s*\(", src)
    assert len(_lib.SIGNATURES["mantis_pixel_shuffle"]) == 9
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mantis_pixel_shuffle")
    from mantis_amd import hip_ops
    assert callable(hip_ops.pixel_shuffle)
    # argument checks run on the host, before any launch
    L = _lib.load()
    assert L.mantis_pixel_shuffle(None, 12, None, 48, 1, 4, 12, 2, None) == -2          # C % 8
    assert L.mantis_pixel_shuffle(None, 16, None, 144, 1, 4, 16, 3, None) == -2         # H % s
    assert L.mantis_pixel_shuffle(None, 8, None, 64, 1, 4, 16, 2, None) == -1           # row stride shorter than a row
    assert L.mantis_pixel_shuffle(None, 16, None, 64, 0, 4, 16, 2, None) == 0           # no image: nothing launched


def test_bf16_envelope_covers_every_case_and_trainable_tensor():
    """tests/golden/idefics3/bf16_envelope.json: the reference's own bf16-vs-fp32 deviation, measured on the reference class (tiny cases) and
    on the pinned restatement (full width) -- never on the product.  The GPU check takes its per-tensor bars from it."""
    model = R.build_product("cpu")
    train = {n for n, p in model.named_parameters() if p.requires_grad}
    for case in CASES:
        env = R.bf16_envelope("reference_bf16:" + case)
        want = train - ({R.PROJ} if case == "b1_text_only" else set())
        assert set(env) == want, (case, set(env) ^ want)
        assert all(c > 0.99 and 0.0 <= r < 0.1 for c, r in env.values()), case
    env = R.bf16_envelope("oracle_bf16:idefics3_full_width")
    assert set(env) == train and all(c > 0.99 and 0.0 <= r < 0.1 for c, r in env.values())
