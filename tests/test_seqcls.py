"""CPU: sequence classification / regression on the Idefics2 path (`Idefics2ForSequenceClassification`).

The test-side fp32 restatement (tests/seqcls_ref.py) against the fixtures recorded from the reference class; the pooled-position rule
as host arithmetic; arena / config / state-dict / error contract of the product class; `collate_classification`; and the product's
host logic (engine step, trainer, evaluation forward) with the operators restated in torch in place of the HIP backend."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import seqcls_ref as S

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["idefics2_seqcls_regression_c5", "idefics2_seqcls_regression_c1", "idefics2_seqcls_single_label_c5",
         "idefics2_seqcls_multi_label_c5", "idefics2_seqcls_regression_c5_leftpad"]


def fixture(case):
    z = np.load(os.path.join(G, case + ".npz"))
    return z, int(z["num_labels"]), str(z["problem_type"]), int(z["pad_token_id"])


def reference_weights(z, bf16=False):
    """the reference class's state_dict: backbone of weights_idefics2.npz (without lm_head) + the fixture's score head"""
    meta, sd = Hh.golden_cfg_and_weights("idefics2")
    sd = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    sd["score.weight"], sd["score.bias"] = z["weight.score.weight"], z["weight.score.bias"]
    if bf16:
        sd = {k: torch.from_numpy(v).to(torch.bfloat16).float() for k, v in sd.items()}
    return meta, sd


def build_ref(case, bf16=False):
    z, C, problem, pad = fixture(case)
    meta, sd = reference_weights(z, bf16)
    return z, S.Idefics2SeqClsRef(sd, meta, C, problem, pad)


def build_product(case, device="cpu"):
    from mantis_amd.configuration_idefics2 import Idefics2Config
    from mantis_amd.modeling_idefics2 import Idefics2ForSequenceClassification
    z, C, problem, pad = fixture(case)
    meta, sd = reference_weights(z)
    cfg = Idefics2Config.from_oracle_meta(dict(meta, num_labels=C, problem_type=problem, pad_token_id=pad))
    model = Idefics2ForSequenceClassification(cfg, device=device, init=None)
    model.load_reference_state_dict(sd)
    return z, model


def batch_of(z):
    return dict(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
                labels=torch.from_numpy(z["labels"]), pixel_values=torch.from_numpy(z["pixel_values"].astype(np.float32)),
                pixel_attention_mask=None)


# The fixtures' gradients are rounded to 14 mantissa bits: every element moves by at most 2^-15 of itself, so a tensor's rel-L2 moves
# by at most 2^-15; the oracle-vs-golden bar of tests/test_idefics2_oracle.py (1e-4) is widened by exactly that.
GRAD_BAR = 1e-4 + 2.0 ** -15


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference_fixture(case):
    z, ref = build_ref(case)
    loss, pooled, pos = ref.forward(z["input_ids"], z["pixel_values"].astype(np.float32), None, z["attention_mask"], z["labels"])
    loss.backward()
    assert np.array_equal(pos.numpy(), z["pooled_positions"])
    assert np.allclose(pooled.detach().numpy(), z["logits"], atol=1e-5, rtol=0), np.abs(pooled.detach().numpy() - z["logits"]).max()
    assert abs(float(loss) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
    n = 0
    for k in z.files:
        if k.startswith("grad."):
            g = ref.w[k[5:]].grad
            assert g is not None, k
            assert Hh.rel_l2(g.numpy(), z[k]) < GRAD_BAR or np.abs(z[k]).max() < 1e-7, (k, Hh.rel_l2(g.numpy(), z[k]))
            n += 1
    assert n == 47 and "grad.score.weight" in z.files and "grad.score.bias" in z.files
    assert all(t.grad is None for k, t in ref.w.items() if k.startswith("model.vision_model."))


def test_left_padded_row_pools_the_last_position():
    z, _, _, _ = fixture("idefics2_seqcls_regression_c5_leftpad")
    assert z["attention_mask"][1, 0] == 0 and z["pooled_positions"].tolist() == [27, 27]
    z, _, _, _ = fixture("idefics2_seqcls_regression_c5")
    assert z["pooled_positions"].tolist() == [27, 22]


POOL_ROWS = {"no pad": [5, 6, 7, 8, 9, 3], "right pad": [5, 6, 7, 0, 0, 0], "left pad": [0, 0, 5, 6, 7, 8],
             "pad id mid-row": [5, 0, 7, 8, 0, 0], "all pad": [0, 0, 0, 0, 0, 0], "pad last": [5, 6, 7, 8, 9, 0]}


def test_pool_position_rule_is_the_references_arithmetic():
    from mantis_amd import decoder as D
    ids = torch.tensor(list(POOL_ROWS.values()), dtype=torch.int64)
    want = (torch.eq(ids, 0).int().argmax(-1) - 1) % ids.shape[-1]
    assert want.tolist() == [5, 2, 5, 0, 5, 4]
    assert D.seqcls_pool_positions(ids, 0).tolist() == want.tolist()
    assert S.pool_positions(ids, 0).tolist() == want.tolist()
    assert S.SeqclsOps.seqcls_pool_index(ids, 0).tolist() == want.tolist()
    assert D.seqcls_pool_positions(ids[:1], None).tolist() == [5]
    with pytest.raises(ValueError, match="Cannot handle batch sizes > 1 if no padding token is defined"):
        D.seqcls_pool_positions(ids[:2], None)


def test_arena_has_score_and_no_lm_head():
    z, model = build_product("idefics2_seqcls_regression_c5")
    names = [n for n, _ in model.named_parameters()]
    assert "lm_head.weight" not in names and names[-2:] == ["score.weight", "score.bias"]
    assert tuple(model.score.weight.shape) == (5, 64) and tuple(model.score.bias.shape) == (5,)
    _, sd = reference_weights(z)
    assert set(names) == set(sd)                                         # the reference class's state_dict, key for key
    assert np.array_equal(model.score.weight.detach().float().numpy(),
                          torch.from_numpy(sd["score.weight"]).to(torch.bfloat16).float().numpy())
    with pytest.raises(KeyError):
        model.load_reference_state_dict(dict(sd, **{"lm_head.weight": np.zeros((300, 64), np.float32)}))
    buckets = model.grad_buckets()
    head = buckets["head"]
    off = model._grad_offs
    assert head.data_ptr() == model.grad_arena[off["model.text_model.norm.weight"]:].data_ptr()
    assert head.numel() == model.grad_arena.numel() - off["model.text_model.norm.weight"]        # final norm + score.weight + score.bias
    assert off["score.bias"] > off["score.weight"] > off["model.text_model.norm.weight"]
    assert sum(b.numel() for b in buckets.values()) == model.grad_arena.numel()
    assert all(p.grad is None for n, p in model.named_parameters() if n.startswith("model.vision_model."))


def test_generation_class_is_unchanged():
    model = Hh.build_idefics2_product("cpu")
    names = [n for n, _ in model.named_parameters()]
    assert names[-1] == "lm_head.weight" and not any(n.startswith("score.") for n in names)


def test_config_fields_round_trip_and_validation():
    from mantis_amd.configuration_idefics2 import Idefics2Config, mantis_8b_idefics2
    meta, _ = Hh.golden_cfg_and_weights("idefics2")
    cfg = Idefics2Config.from_oracle_meta(dict(meta, num_labels=5, problem_type="regression", pad_token_id=0))
    assert (cfg.num_labels, cfg.problem_type, cfg.pad_token_id) == (5, "regression", 0)
    d = cfg.to_dict()
    again = Idefics2Config(**d)
    assert again.to_dict() == d and again.num_labels == 5 and again.problem_type == "regression" and again.pad_token_id == 0
    plain = Idefics2Config.from_oracle_meta(meta)
    assert (plain.num_labels, plain.problem_type, plain.pad_token_id) == (2, None, None)         # HF PretrainedConfig's defaults
    big = mantis_8b_idefics2(num_labels=5, problem_type="regression")
    assert big.num_labels == 5 and big.problem_type == "regression" and big.text_config.hidden_size == 4096
    with pytest.raises(ValueError):
        Idefics2Config.from_oracle_meta(dict(meta, problem_type="ranking"))
    with pytest.raises(ValueError):
        Idefics2Config.from_oracle_meta(dict(meta, num_labels=0))


def test_num_labels_outside_the_supported_range_is_refused():
    from mantis_amd.configuration_idefics2 import Idefics2Config
    from mantis_amd.modeling_idefics2 import Idefics2ForSequenceClassification
    meta, _ = Hh.golden_cfg_and_weights("idefics2")
    with pytest.raises(ValueError, match="num_labels"):
        Idefics2ForSequenceClassification(Idefics2Config.from_oracle_meta(dict(meta, num_labels=129)), device="cpu", init=None)
    Idefics2ForSequenceClassification(Idefics2Config.from_oracle_meta(dict(meta, num_labels=128)), device="cpu", init=None)


def test_problem_type_inference_and_label_checks():
    from mantis_amd.configuration_idefics2 import Idefics2Config
    from mantis_amd.modeling_idefics2 import Idefics2ForSequenceClassification
    meta, _ = Hh.golden_cfg_and_weights("idefics2")

    def make(C, problem=None):
        return Idefics2ForSequenceClassification(Idefics2Config.from_oracle_meta(dict(meta, num_labels=C, problem_type=problem, pad_token_id=0)),
                                                 device="cpu", init=None)
    m = make(1)
    lab, problem = m.prepare_labels(torch.tensor([1.5, 2.5]), 2)
    assert problem == "regression" and m.config.problem_type == "regression" and tuple(lab.shape) == (2, 1) and lab.dtype == torch.float32
    m = make(5)
    lab, problem = m.prepare_labels(torch.tensor([1, 4]), 2)
    assert problem == "single_label_classification" and lab.dtype == torch.int32 and tuple(lab.shape) == (2,)
    m = make(5)
    lab, problem = m.prepare_labels(torch.rand(2, 5), 2)
    assert problem == "multi_label_classification" and tuple(lab.shape) == (2, 5)
    assert m.prepare_labels(torch.rand(2, 5).double(), 2)[1] == "multi_label_classification"      # inferred once, then kept
    m = make(5, "regression")
    for bad in (torch.tensor([[1, 2, 3, 4, 5]] * 2), torch.rand(2, 4), torch.rand(2), torch.rand(3, 5)):
        with pytest.raises(ValueError):
            m.prepare_labels(bad, 2)
    m = make(5, "single_label_classification")
    for bad in (torch.rand(2), torch.tensor([[1, 2], [3, 4]])):
        with pytest.raises(ValueError):
            m.prepare_labels(bad, 2)
    for bad in (torch.tensor([1, 5]), torch.tensor([-1, 0])):
        with pytest.raises(IndexError):
            m.prepare_labels(bad, 2)


def test_collate_classification_two_ragged_samples():
    from mantis_amd.data import collate_classification
    a = dict(input_ids=torch.tensor([[5, 6, 7, 8, 9]]), attention_mask=torch.ones(1, 5, dtype=torch.int64),
             labels=torch.tensor([[1.0, 2.0, 3.0]]), pixel_values=torch.ones(1, 2, 3, 4, 4))
    b = dict(input_ids=torch.tensor([[5, 6, 7]]), attention_mask=torch.ones(1, 3, dtype=torch.int64),
             labels=torch.tensor([[4.0, 5.0, 6.0]]), pixel_values=2 * torch.ones(1, 1, 3, 4, 4))
    out = collate_classification([a, b], pad_token_id=0)
    assert out["input_ids"].tolist() == [[5, 6, 7, 8, 9], [5, 6, 7, 0, 0]] and out["input_ids"].dtype == torch.int64
    assert out["attention_mask"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 0]]
    assert out["labels"].dtype == torch.float32 and out["labels"].tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert tuple(out["pixel_values"].shape) == (2, 2, 3, 4, 4)
    assert float(out["pixel_values"][1, 0].min()) == 2.0 and not out["pixel_values"][1, 1].any()       # missing image = all-zero padding image
    assert S.pool_positions(out["input_ids"], 0).tolist() == [4, 2]
    ints = collate_classification([dict(input_ids=[1, 2], labels=torch.tensor([3])), dict(input_ids=[1], labels=torch.tensor([0]))], 0)
    assert ints["labels"].tolist() == [3, 0] and ints["labels"].dtype == torch.int64 and ints["pixel_values"] is None


# ---------------------------------------------------------------------------------------------------- product host logic on the CPU
@pytest.fixture()
def cpu_backend(monkeypatch):
    import mantis_amd.modeling_idefics2 as mod
    monkeypatch.setattr(mod, "K", S.SeqclsOps)
    return mod


def check_step(model, ref, z, out):
    """bf16 product step vs the fp32 restatement on the same bf16-rounded weights: SURVEY 8c's bars (tests/helpers.py)."""
    ref.zero_grad()
    oloss, opooled, opos = ref.forward(z["input_ids"], z["pixel_values"].astype(np.float32), None, z["attention_mask"], z["labels"])
    oloss.backward()
    assert np.array_equal(out["pooled_positions"].cpu().numpy(), opos.cpu().numpy())
    loss = float(out["loss"].float().cpu().reshape(-1)[0])
    assert abs(loss - float(oloss)) <= 5e-3 * abs(float(oloss)), (loss, float(oloss))
    lg, ol = out["logits"].float().cpu().numpy(), opooled.detach().cpu().numpy()
    assert np.abs(lg - ol).max() <= 3e-2 * np.sqrt((ol ** 2).mean()), (lg, ol)
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        og = ref.w[name].grad
        g = p.grad.float().cpu().numpy()
        assert og is not None, name
        og = og.cpu().numpy()
        if np.linalg.norm(og) < 1e-12:
            assert np.linalg.norm(g) < 1e-6, name
            continue
        c, r = Hh.cosine(g, og), Hh.rel_l2(g, og)
        assert c >= Hh.GRAD_COS and r <= Hh.GRAD_REL, (name, c, r)


@pytest.mark.parametrize("case", CASES)
def test_product_step_matches_restatement_on_cpu_operators(cpu_backend, case):
    z, model = build_product(case)
    _, ref = build_ref(case, bf16=True)
    assert model._ensure_grad_arena()
    out = model.engine.step_from_batch(batch_of(z), compute_grads=True, overwrite_grads=True)
    assert out["logits"].dtype == torch.float32 and tuple(out["logits"].shape) == (2, int(z["num_labels"]))
    check_step(model, ref, z, out)
    assert abs(float(out["loss"]) - float(z["loss"])) < 0.03 * abs(float(z["loss"]))          # vs the reference's own fp32 loss


def test_forward_surface_train_eval_and_refusals(cpu_backend):
    from mantis_amd.modeling_idefics2 import SequenceClassifierOutputWithPast
    z, model = build_product("idefics2_seqcls_regression_c5")
    b = batch_of(z)
    out = model(**b)
    assert isinstance(out, SequenceClassifierOutputWithPast) and out.loss.requires_grad and tuple(out.logits.shape) == (2, 5)
    out.loss.backward()
    g = model.grad_arena.clone()
    assert float(g.float().abs().sum()) > 0
    model.eval()
    with torch.no_grad():
        ev = model(**b)
        tup = model(**b, return_dict=False)
    assert torch.equal(ev.logits, out.logits) and torch.equal(ev.loss, out.loss.detach())
    assert torch.equal(model.grad_arena, g)                                # evaluation leaves the gradients alone
    assert len(tup) == 2 and torch.equal(tup[1], ev.logits)
    nolab = model(**dict(b, labels=None))
    assert nolab.loss is None and torch.equal(nolab.logits, ev.logits)
    model.train()
    with pytest.raises(NotImplementedError):
        model.engine.step_from_batch(dict(b, segment_ids=torch.zeros(2, 28, dtype=torch.int32)), compute_grads=False)
    for kw in (dict(inputs_embeds=torch.zeros(2, 28, 64)), dict(use_cache=True), dict(past_key_values=()), dict(output_hidden_states=True)):
        with pytest.raises(NotImplementedError):
            model(**dict(b, **kw))
    model.config.pad_token_id = None
    with pytest.raises(ValueError, match="Cannot handle batch sizes > 1"):
        model(**b)


def test_trainer_accumulates_and_the_optimizer_covers_the_head(cpu_backend):
    from mantis_amd.trainer import MantisHipTrainer
    z, model = build_product("idefics2_seqcls_regression_c5")
    tr = MantisHipTrainer(model, gradient_accumulation_steps=2)
    l1 = tr.training_step(model, batch_of(z))
    g1 = model.grad_arena.float().clone()
    l2 = tr.training_step(model, batch_of(z))
    assert l1.dim() == 0 and not l1.requires_grad and torch.equal(l1, l2)
    assert abs(float(l1) - float(z["loss"]) / 2) < 0.03 * float(z["loss"])
    assert Hh.rel_l2(model.grad_arena.float().numpy(), 2 * g1.numpy()) < 2e-2
    assert {"score.weight", "score.bias"} <= set(model._grad_key)          # what FusedAdamW lays its state out by
