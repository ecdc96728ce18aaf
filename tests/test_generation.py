"""CPU: the host logic of greedy generation (mantis_amd/generation.py, decoder.layer_decode, LlavaForConditionalGeneration.generate)
driven through the oracle's operator restatement + the fp32 restatements of the four decode operators (tests/generation_ref.py),
against what the reference class computes (tests/golden/generation/llava_generate_*.npz, recorded by tests/golden/make_golden_generation.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import generation_ref as GR
from tests import helpers as Hh

FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(Hh.G, "generation", "llava_generate_*.npz")))
EXPECTED = ["llava_generate_b1_img2", "llava_generate_b1_img4_first", "llava_generate_b1_text_only", "llava_generate_b2_eos",
            "llava_generate_b2_leftpad"]


@pytest.fixture()
def backend32(monkeypatch):
    import mantis_amd.engine as eng
    monkeypatch.setattr(eng, "K", GR.backend(fp32_tables=True))


@pytest.fixture()
def backend16(monkeypatch):
    import mantis_amd.engine as eng
    monkeypatch.setattr(eng, "K", GR.backend())


def _model32():
    model, _, sd = Hh.build_product_model("siglip", "cpu")
    return GR.fp32_model(model, sd)


def _inputs(z):
    eos = int(z["eos_token_id"])
    return dict(input_ids=torch.from_numpy(z["input_ids"]), pixel_values=Hh.pixels_list(z), attention_mask=torch.from_numpy(z["attention_mask"]),
                max_new_tokens=int(z["n_steps"])), (None if eos < 0 else eos), int(z["pad_token_id"])


def test_fixtures_make_token_equality_a_fair_demand():
    """every step of every row of every committed fixture: fp32 top-2 margin > 2 x eps, eps = 1.5 x the reference's own bf16 deviation"""
    assert FIXTURES == EXPECTED
    for case in FIXTURES:
        z = Hh.load_case("generation/" + case)
        n, B = int(z["n_steps"]), z["input_ids"].shape[0]
        assert n >= 12 and z["tokens"].shape == (B, n) and z["logits"].shape[:2] == (n, B) and z["logits_bf16"].shape == z["logits"].shape
        delta = float(np.abs(z["logits_bf16"] - z["logits"]).max())
        assert delta == float(z["delta"]) and delta > 0
        top = np.sort(z["logits"], axis=-1)
        margins = top[..., -1] - top[..., -2]
        assert np.allclose(margins, z["margins"]) and margins.min() > 2 * Hh.ENVELOPE_FACTOR * delta, (case, margins.min(), delta)
        assert np.array_equal(z["logits"].argmax(-1).T, z["tokens"])
    z = Hh.load_case("generation/llava_generate_b2_eos")
    seq, T = z["sequences"], z["input_ids"].shape[1]
    stop = [int(np.argmax(seq[b, T:] == int(z["eos_token_id"]))) if (seq[b, T:] == int(z["eos_token_id"])).any() else -1 for b in range(2)]
    assert min(stop) >= 0 and stop[0] != stop[1], "the rows must stop at different steps"
    early = int(np.argmin(stop))
    assert (seq[early, T + stop[early] + 1:] == int(z["pad_token_id"])).all() and seq.shape[1] == T + max(stop) + 1
    assert int(z["input_ids"][0, 0]) != 298 and int(Hh.load_case("generation/llava_generate_b1_img4_first")["input_ids"][0, 0]) == 298


@pytest.mark.parametrize("case", EXPECTED)
def test_generate_reproduces_the_reference(backend32, case):
    z = Hh.load_case("generation/" + case)
    model = _model32()
    kw, eos, pad = _inputs(z)
    out = model.generate(**kw, eos_token_id=eos, pad_token_id=pad)
    assert out.dtype == torch.int64 and np.array_equal(out.numpy(), z["sequences"])
    lg = GR.teacher_forced_logits(model, kw["input_ids"], kw["attention_mask"], kw["pixel_values"], torch.from_numpy(z["tokens"]))
    assert np.abs(lg.numpy() - z["logits"]).max() <= 1e-4


@pytest.mark.parametrize("case", ["llava_generate_b2_leftpad", "llava_generate_b1_text_only"])
def test_cached_decode_equals_cache_free_forward(backend32, case):
    z = Hh.load_case("generation/" + case)
    model = _model32()
    kw, _, _ = _inputs(z)
    out = model.generate(**kw)
    lg = GR.teacher_forced_logits(model, kw["input_ids"], kw["attention_mask"], kw["pixel_values"], out[:, kw["input_ids"].shape[1]:])
    ids, am = kw["input_ids"], kw["attention_mask"]
    for step in range(kw["max_new_tokens"]):
        ref = model(input_ids=ids, pixel_values=kw["pixel_values"], attention_mask=am, return_logits=True).logits[:, -1].float()
        assert (ref - lg[step]).abs().max() <= 1e-4, step
        ids = torch.cat([ids, ref.argmax(-1)[:, None]], 1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], 1)
    assert torch.equal(ids, out)


def test_bf16_host_path_reproduces_the_tokens(backend16):
    """the product's own storage precision (bf16 arena, bf16 RoPE tables) through the same host logic: logits within eps, tokens equal"""
    for case in EXPECTED:
        z = Hh.load_case("generation/" + case)
        model, _, _ = Hh.build_product_model("siglip", "cpu")
        kw, eos, pad = _inputs(z)
        lg = GR.teacher_forced_logits(model, kw["input_ids"], kw["attention_mask"], kw["pixel_values"], torch.from_numpy(z["tokens"]))
        assert np.abs(lg.numpy() - z["logits"]).max() <= Hh.ENVELOPE_FACTOR * float(z["delta"])
        assert np.array_equal(model.generate(**kw, eos_token_id=eos, pad_token_id=pad).numpy(), z["sequences"])


def test_eos_pad_fill_max_length_and_terminator_list(backend32):
    z = Hh.load_case("generation/llava_generate_b2_eos")
    model = _model32()
    kw, eos, pad = _inputs(z)
    T = kw["input_ids"].shape[1]
    want = z["sequences"]
    assert np.array_equal(model.generate(**kw, eos_token_id=[eos, 297], pad_token_id=pad).numpy(), want)       # chat_mllava passes a list
    assert np.array_equal(model.generate(**kw, eos_token_id=torch.tensor([eos])).numpy(), want)                # pad from the config
    free = np.concatenate([z["input_ids"], z["tokens"]], 1)
    assert np.array_equal(model.generate(**kw).numpy(), free)                                                  # no EOS: the length limit
    kw.pop("max_new_tokens")
    out = model.generate(**kw, max_length=T + 5)
    assert np.array_equal(out.numpy(), free[:, : T + 5])
    out = model.generate(**kw, max_length=T + 5, max_new_tokens=3)                                             # max_new_tokens wins
    assert out.shape[1] == T + 3
    model.config.pad_token_id = None                                                                           # HF: pad falls back to the first EOS
    out = model.generate(**kw, max_length=T + 12, eos_token_id=eos).numpy()
    exp = want.copy()
    exp[:, T:] = np.where(want[:, T:] == pad, eos, want[:, T:])
    assert np.array_equal(out, exp)
    with pytest.raises(ValueError):
        model.generate(**kw, max_length=T)


def test_streamer_call_sequence(backend32):
    z = Hh.load_case("generation/llava_generate_b1_img2")
    model = _model32()
    kw, _, _ = _inputs(z)

    class Streamer:
        def __init__(self):
            self.calls = []

        def put(self, v):
            self.calls.append(("put", v.clone()))

        def end(self):
            self.calls.append(("end", None))
    s = Streamer()
    out = model.generate(**kw, streamer=s)
    n = kw["max_new_tokens"]
    assert [c[0] for c in s.calls] == ["put"] * (n + 1) + ["end"]
    assert torch.equal(s.calls[0][1], kw["input_ids"])                      # the prompt first, as HF does
    assert torch.equal(torch.stack([c[1] for c in s.calls[1:-1]], 1), out[:, kw["input_ids"].shape[1]:])


def test_refusals(backend32):
    z = Hh.load_case("generation/llava_generate_b2_leftpad")
    model = _model32()
    kw, _, _ = _inputs(z)
    for bad in (dict(do_sample=True), dict(num_beams=4), dict(temperature=0.7), dict(top_p=0.9), dict(repetition_penalty=1.2),
                dict(logits_processor=[object()]), dict(assistant_model=object()), dict(return_dict_in_generate=True), dict(frobnicate=1)):
        with pytest.raises(NotImplementedError, match=next(iter(bad))):
            model.generate(**kw, **bad)
    model.generate(**dict(kw, max_new_tokens=1), do_sample=False, num_beams=1, use_cache=True, temperature=None)      # what chat_mllava may pass along
    # right-padded batch of unequal lengths
    ids, am = kw["input_ids"].flip(1), kw["attention_mask"].flip(1)
    assert int(am[1, -1]) == 0
    with pytest.raises(ValueError, match="[Ll][Ee][Ff][Tt]"):
        model.generate(ids, pixel_values=kw["pixel_values"], attention_mask=am, max_new_tokens=2)
    # a padded text-only batch: refused by name, nothing dropped silently
    with pytest.raises(NotImplementedError, match="TEXT-ONLY"):
        model.generate(kw["input_ids"].clamp(max=200), attention_mask=kw["attention_mask"], max_new_tokens=2)
    for hook in ("_teacher", "_logits_out"):                       # no test hooks inside the public call
        with pytest.raises(NotImplementedError, match=hook):
            model.generate(**kw, **{hook: None})
    # forward() keeps refusing the cache arguments and now points to generate()
    with pytest.raises(NotImplementedError, match="generate"):
        model(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], pixel_values=kw["pixel_values"], use_cache=True)
    with pytest.raises(NotImplementedError):
        model(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], past_key_values=((None, None),))


def test_other_families_still_refuse():
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
    from mantis_amd.modeling_qwen2_vl import Qwen2VLForConditionalGeneration
    for cls in (Idefics2ForConditionalGeneration, Qwen2VLForConditionalGeneration):
        assert not hasattr(cls, "generate")
    ids = torch.zeros((1, 4), dtype=torch.int64)
    for model in (Hh.build_idefics2_product("cpu"), Hh.build_qwen2vl_product("cpu")):
        with pytest.raises(NotImplementedError):
            model(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True)


def test_decoder_forward_default_path_is_untouched(backend16):
    """the kv_sink hook: its default leaves the evaluation forward's results as they were; with a sink the same hidden states come back"""
    import mantis_amd.engine as eng
    z = Hh.load_case("siglip_b2_equal_nopad")
    model, _, _ = Hh.build_product_model("siglip", "cpu")
    args = (torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]), None, Hh.pixels_list(z))
    rec = {}
    model.engine.step(*args, compute_grads=False, need_logits=True, record=rec)
    seen = []
    out = model.engine.step(*args, compute_grads=False, kv_sink=lambda i, qkv: seen.append((i, qkv.shape)))
    tc = model.config.text_config
    assert [i for i, _ in seen] == list(range(tc.num_hidden_layers))
    last = rec[f"llm_layer{tc.num_hidden_layers - 1}_out"]
    assert torch.equal(out["hidden"].view(last.shape), last)
    with pytest.raises(ValueError):
        model.engine.step(*args, compute_grads=True, kv_sink=lambda i, qkv: None)
