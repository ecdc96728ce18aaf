"""CPU: the host logic of greedy generation on the Idefics3 path (mantis_amd/generation.py, the prefill hooks of Idefics2Engine.step,
Idefics3ForConditionalGeneration.generate) driven through the oracle's operator restatement + the decode operators + a restatement of the
select kernel (tests/generation_select_ref.py), against what the reference class computes
(tests/golden/generation/idefics3_generate_*.npz, recorded by tests/golden/make_golden_idefics3_generation.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import generation_ref as GR
from tests import generation_select_ref as S
from tests import helpers as Hh
from tests import idefics3_ref as R

IMG = 298


@pytest.fixture()
def backend32(monkeypatch):
    import mantis_amd.modeling_idefics2 as mod
    monkeypatch.setattr(mod, "K", S.backend(fp32_tables=True))


@pytest.fixture()
def backend16(monkeypatch):
    import mantis_amd.modeling_idefics2 as mod
    monkeypatch.setattr(mod, "K", S.backend())


def _model32():
    _, sd = R.golden_cfg_and_weights()
    return GR.fp32_model(R.build_product("cpu"), sd)


class Streamer:
    def __init__(self):
        self.calls = []

    def put(self, v):
        self.calls.append(("put", v.clone()))

    def end(self):
        self.calls.append(("end", None))


def test_fixtures_make_token_equality_a_fair_demand():
    """every step of every row of every committed fixture: fp32 top-2 margin > 2 x eps, eps = 1.5 x the reference's own bf16 deviation;
    no generated token is the image placeholder or the pad id"""
    found = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(Hh.G, "generation", "idefics3_generate_*.npz")))
    assert found == sorted("idefics3_generate_" + c for c in S.CASES)
    for case in S.CASES:
        z = S.load(case)
        n, B = int(z["n_steps"]), z["input_ids"].shape[0]
        assert n == 12 and z["tokens"].shape == (B, n) and z["logits"].shape[:2] == (n, B) and z["logits_bf16"].shape == z["logits"].shape
        delta = float(np.abs(z["logits_bf16"] - z["logits"]).max())
        assert delta == float(z["delta"]) and delta > 0
        top = np.sort(z["logits"], axis=-1)
        margins = top[..., -1] - top[..., -2]
        assert np.allclose(margins, z["margins"]) and margins.min() > 2 * Hh.ENVELOPE_FACTOR * delta, (case, margins.min(), delta)
        assert np.array_equal(z["logits"].argmax(-1).T, z["tokens"])
        assert not np.isin(z["tokens"], [IMG, int(z["pad_token_id"])]).any()
        assert os.path.getsize(os.path.join(Hh.G, "generation", f"idefics3_generate_{case}.npz")) < (1 << 20)
    # what each case is there for
    assert S.load("b1_img2")["input_ids"].shape[0] == 1 and int((S.load("b1_img2")["input_ids"] == IMG).sum()) == 8
    for c in ("b1_text_only", "b2_text_leftpad"):
        assert "pixel_values" not in S.load(c).files and not (S.load(c)["input_ids"] == IMG).any()
    z = S.load("b2_leftpad")
    assert (z["input_ids"] == IMG).sum(1).tolist() == [8, 4] and int(z["attention_mask"][1, 0]) == 0 and z["attention_mask"][:, -1].all()
    assert not z["pixel_values"][1, 1].any() and not z["pixel_attention_mask"][1, 1].any() and z["pixel_values"][1, 0].any()
    z = S.load("b2_text_leftpad")
    assert z["input_ids"].shape[0] == 2 and (z["attention_mask"][1] == 0).any() and z["attention_mask"][:, -1].all()
    z = S.load("b2_eos")
    seq, T, eos = z["sequences"], z["input_ids"].shape[1], int(z["eos_token_id"])
    stop = [int(np.argmax(seq[b, T:] == eos)) if (seq[b, T:] == eos).any() else -1 for b in range(2)]
    assert min(stop) >= 0 and stop[0] != stop[1] and max(stop) < 11, "the rows must stop at different steps, both before step 12"
    early = int(np.argmin(stop))
    assert (seq[early, T + stop[early] + 1:] == int(z["pad_token_id"])).all() and seq.shape[1] == T + max(stop) + 1


@pytest.mark.parametrize("case", S.CASES)
def test_generate_reproduces_the_reference(backend32, case):
    z = S.load(case)
    model = _model32()
    kw, eos, pad = S.inputs(z)
    out = model.generate(**kw, eos_token_id=eos, pad_token_id=pad)
    assert out.dtype == torch.int64 and np.array_equal(out.numpy(), z["sequences"])
    lg = S.teacher_forced_logits(model, kw, torch.from_numpy(z["tokens"]))
    assert np.abs(lg.numpy() - z["logits"]).max() <= 1e-4


def test_bf16_host_path_reproduces_the_tokens(backend16):
    """the product's own storage precision (bf16 arena, bf16 RoPE tables) through the same host logic: logits within eps, tokens equal"""
    for case in S.CASES:
        z = S.load(case)
        model = R.build_product("cpu")
        kw, eos, pad = S.inputs(z)
        lg = S.teacher_forced_logits(model, kw, torch.from_numpy(z["tokens"]))
        assert np.abs(lg.numpy() - z["logits"]).max() <= Hh.ENVELOPE_FACTOR * float(z["delta"]), case
        assert np.array_equal(model.generate(**kw, eos_token_id=eos, pad_token_id=pad).numpy(), z["sequences"]), case


@pytest.mark.parametrize("case", ["b2_leftpad", "b2_text_leftpad"])
def test_cached_decode_equals_cache_free_step(backend32, case):
    z = S.load(case)
    model = _model32()
    kw, _, _ = S.inputs(z)
    out = model.generate(**kw)
    T = kw["input_ids"].shape[1]
    lg = S.teacher_forced_logits(model, kw, out[:, T:])
    ids, am = kw["input_ids"], kw["attention_mask"]
    for step in range(kw["max_new_tokens"]):
        ref = S.cache_free_logits(model, kw, ids, am)
        assert (ref - lg[step]).abs().max() <= 1e-4, step
        ids = torch.cat([ids, ref.argmax(-1)[:, None]], 1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], 1)
    assert torch.equal(ids, out)


@pytest.mark.parametrize("k", [1, 3, 5, 12])
def test_read_back_interval_changes_neither_result_nor_bound(backend32, monkeypatch, k):
    from mantis_amd import generation as Gn
    z = S.load("b2_eos")
    model = _model32()
    kw, eos, pad = S.inputs(z)
    T = kw["input_ids"].shape[1]
    last_finish = z["sequences"].shape[1] - T - 1          # the step at which the last row emits its EOS
    calls = []
    real = Gn.decode_step
    monkeypatch.setattr(Gn, "decode_step", lambda *a, **kw_: (calls.append(1), real(*a, **kw_))[1])
    out = Gn.generate(model, **kw, eos_token_id=eos, pad_token_id=pad, eos_check_every=k)
    assert np.array_equal(out.numpy(), z["sequences"])
    print(f"k = {k}: {len(calls)} decode steps, last finish step {last_finish}")
    assert last_finish <= len(calls) <= min(last_finish + k - 1, kw["max_new_tokens"] - 1)
    # with a streamer the interval is 1 whatever was asked for: the stream ends exactly where HF's does
    calls.clear()
    s = Streamer()
    out = Gn.generate(model, **kw, eos_token_id=eos, pad_token_id=pad, eos_check_every=k, streamer=s)
    n = z["sequences"].shape[1] - T
    assert np.array_equal(out.numpy(), z["sequences"]) and len(calls) == last_finish
    assert [c[0] for c in s.calls] == ["put"] * (n + 1) + ["end"]
    assert torch.equal(s.calls[0][1], kw["input_ids"])
    assert torch.equal(torch.stack([c[1] for c in s.calls[1:-1]], 1), out[:, T:])
    with pytest.raises(ValueError):
        Gn.generate(model, **kw, eos_token_id=eos, pad_token_id=pad, eos_check_every=0)


def test_no_eos_never_reads_back_and_runs_to_the_limit(backend32):
    z = S.load("b2_eos")
    model = _model32()
    kw, _, _ = S.inputs(z)
    assert np.array_equal(model.generate(**kw).numpy(), np.concatenate([z["input_ids"], z["tokens"]], 1))


def test_composition_fallback_gives_the_same_sequences(monkeypatch):
    """a backend without greedy_select: the loop runs generation.select_composition, the definition the kernel is tested against"""
    import mantis_amd.modeling_idefics2 as mod
    from mantis_amd import generation as Gn
    be = S.backend(fp32_tables=True, with_select=False)
    assert not hasattr(be, "greedy_select")
    monkeypatch.setattr(mod, "K", be)
    used = []
    real = Gn.select_composition
    monkeypatch.setattr(Gn, "select_composition", lambda *a: (used.append(1), real(*a))[1])
    model = _model32()
    for case in S.CASES:
        z = S.load(case)
        kw, eos, pad = S.inputs(z)
        assert np.array_equal(model.generate(**kw, eos_token_id=eos, pad_token_id=pad).numpy(), z["sequences"]), case
    assert used
    z = S.load("b2_eos")
    kw, eos, pad = S.inputs(z)
    assert np.array_equal(Gn.generate(model, **kw, eos_token_id=eos, pad_token_id=pad, eos_check_every=5).numpy(), z["sequences"])


def test_select_restatement_equals_the_composition():
    """the two CPU statements of one step (row-by-row restatement, operator composition) agree, flags included"""
    from mantis_amd import generation as Gn
    K = GR.backend()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 304, generator=g).to(torch.bfloat16)
    x[:, 300:] = 100.0
    x[0, 7] = x[0, 200] = 50.0
    x[1, 299] = 60.0
    eos = torch.tensor([7, 299, 0], dtype=torch.int64)
    res = []
    for fn in (S.greedy_select, lambda *a: Gn.select_composition(K, *a)):
        unf = torch.tensor([1, 1, 0, 1], dtype=torch.int32)
        fin = torch.tensor([-1, -1, 2, -1], dtype=torch.int32)
        out = torch.full((4, 9), -7, dtype=torch.int64)
        nxt = torch.zeros(4, dtype=torch.int64)
        fn(x, 300, eos, 0, unf, fin, out, 5, nxt)
        res.append((unf, fin, out, nxt))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    unf, fin, out, nxt = res[0]
    assert unf.tolist()[:3] == [0, 0, 0] and fin.tolist()[:3] == [5, 5, 2] and nxt.tolist()[:3] == [7, 299, 0]
    assert (out[:, :5] == -7).all() and (out[:, 6:] == -7).all() and torch.equal(out[:, 5], nxt)


def test_engine_step_hooks(backend16):
    """kv_sink=None and position_ids=None leave the evaluation forward bit for bit; a sink sees every layer once; the refusals"""
    z = R.load_case("b2_padimg_rightpad")
    b = R.batch(z)
    model = R.build_product("cpu")
    args = (b["input_ids"], b["attention_mask"], None, b["pixel_values"], b["pixel_attention_mask"])
    rec, rec2 = {}, {}
    model.engine.step(*args, compute_grads=False, need_logits=True, record=rec)
    base = model.engine.step(*args, compute_grads=False, need_logits=True, record=rec2, kv_sink=None, position_ids=None)
    tc = model.config.text_config
    last = rec[f"llm_layer{tc.num_hidden_layers - 1}_out"]
    assert torch.equal(rec2[f"llm_layer{tc.num_hidden_layers - 1}_out"], last)
    B, T = b["input_ids"].shape
    assert torch.equal(base["plan"].position_ids, torch.arange(T)[None].expand(B, T))
    seen = []
    out = model.engine.step(*args, compute_grads=False, kv_sink=lambda i, qkv: seen.append((i, tuple(qkv.shape))))
    assert [i for i, _ in seen] == list(range(tc.num_hidden_layers)) and all(s[0] == B * T for _, s in seen)
    assert sorted(out) == ["L", "hidden", "plan"] and out["L"] == T and torch.equal(out["hidden"].view(last.shape), last)
    # explicit positions equal to the default give the same bits; others move the result
    ar = torch.arange(T)[None].expand(B, T)
    same = model.engine.step(*args, compute_grads=False, kv_sink=lambda i, qkv: None, position_ids=ar)
    assert torch.equal(same["hidden"], out["hidden"])
    moved = model.engine.step(*args, compute_grads=False, kv_sink=lambda i, qkv: None, position_ids=ar * 2)
    assert torch.equal(moved["plan"].position_ids, ar * 2) and not torch.equal(moved["hidden"], out["hidden"])
    with pytest.raises(ValueError):
        model.engine.step(*args, compute_grads=True, kv_sink=lambda i, qkv: None)
    with pytest.raises(ValueError):
        model.engine.step(b["input_ids"], b["attention_mask"], b["labels"], b["pixel_values"], b["pixel_attention_mask"],
                          compute_grads=False, kv_sink=lambda i, qkv: None)
    with pytest.raises(ValueError):
        model.engine.step(*args, compute_grads=False, position_ids=ar[:, :-1])


def test_refusals(backend32):
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    assert not hasattr(Idefics2ForConditionalGeneration, "generate") and "generate" in vars(Idefics3ForConditionalGeneration)
    z = S.load("b2_leftpad")
    model = _model32()
    kw, _, _ = S.inputs(z)
    for bad in (dict(do_sample=True), dict(num_beams=4), dict(frobnicate=1), dict(eos_check_every=4), dict(return_dict_in_generate=True)):
        with pytest.raises(NotImplementedError, match=next(iter(bad))):
            model.generate(**kw, **bad)
    model.generate(**dict(kw, max_new_tokens=1), do_sample=False, num_beams=1, use_cache=True)      # what idefics3_eval.py passes along
    # right-padded batch of unequal lengths
    ids, am = kw["input_ids"].flip(1), kw["attention_mask"].flip(1)
    assert int(am[1, -1]) == 0
    with pytest.raises(ValueError, match="[Ll][Ee][Ff][Tt]"):
        model.generate(ids, pixel_values=kw["pixel_values"], pixel_attention_mask=kw["pixel_attention_mask"], attention_mask=am,
                       max_new_tokens=2)
    with pytest.raises(ValueError, match="masked"):
        model.generate(ids[1:], attention_mask=am[1:], max_new_tokens=2)
    # fp8 is refused by name on this path, so generate never meets an fp8 decoder; a would-be one is refused too
    with pytest.raises(NotImplementedError, match="fp8"):
        model.set_precision("fp8")
    model.engine.w8 = object()
    with pytest.raises(NotImplementedError, match="bf16"):
        model.generate(**kw)
    model.engine.w8 = None
    # forward() keeps refusing the cache arguments and explicit positions
    with pytest.raises(NotImplementedError):
        model(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], pixel_values=kw["pixel_values"], use_cache=True)
    with pytest.raises(NotImplementedError):
        model(input_ids=kw["input_ids"], attention_mask=kw["attention_mask"], position_ids=S.positions(kw["attention_mask"]))


def test_llava_method_does_not_expose_the_loop_keywords(monkeypatch):
    import mantis_amd.engine as eng
    monkeypatch.setattr(eng, "K", GR.backend(fp32_tables=True))
    model, _, sd = Hh.build_product_model("siglip", "cpu")
    z = Hh.load_case("generation/llava_generate_b1_text_only")
    for bad in ("eos_check_every", "pixel_attention_mask"):
        with pytest.raises(NotImplementedError, match=bad):
            model.generate(torch.from_numpy(z["input_ids"]), max_new_tokens=1, **{bad: 1})


def test_greedy_select_symbol_is_declared_and_bound():
    from mantis_amd import _lib
    hdr = open(os.path.join(os.path.dirname(Hh.G), "..", "include", "mantis_hip.h")).read()
    assert "int mantis_greedy_select(" in hdr and len(_lib.SIGNATURES["mantis_greedy_select"]) == 14
    assert hasattr(_lib.load(), "mantis_greedy_select")
