"""GPU: the select kernel of csrc/decode.hip (`hip_ops.greedy_select`) against its definition (`generation.select_composition` on the same
tensors: integer outputs, so equality is exact), and `Idefics3ForConditionalGeneration.generate` on the kernels against the reference's
record (tests/golden/generation/idefics3_generate_*.npz: teacher-forced logits within eps = 1.5 x the reference's own bf16 deviation,
free-running tokens exactly) and against the engine's own cache-free step at full width."""
import numpy as np
import pytest
import torch

from tests import generation_select_ref as S
from tests import helpers as Hh
from tests import idefics3_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
COS, REL = 0.999, 2e-2
PAD = 2
SENTINEL = -7


def _k():
    from mantis_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------------------------ the select kernel
def _logits(B, V, ld, shift):
    """row b is of kind (b + shift) % 4: 0 random, 1 all equal (-> index 0), 2 a three-way tie at 5, a middle column and V - 1 (-> 5),
    3 the maximum in column V - 1.  The pad columns [V, ld) hold 100.0 and must be ignored."""
    g = torch.Generator().manual_seed(1000 * B + V + shift)
    x = torch.randn(B, ld, generator=g).to(torch.bfloat16)
    mid = 77777 if V > 77777 else 77
    want = {}
    for b in range(B):
        kind = (b + shift) % 4
        if kind == 1:
            x[b, :V] = 1.0
            want[b] = 0
        elif kind == 2:
            x[b, 5] = x[b, mid] = x[b, V - 1] = 50.0
            want[b] = 5
        elif kind == 3:
            x[b, V - 1] = 60.0
            want[b] = V - 1
    x[:, V:] = 100.0
    return x.to(DEV), want


def _state(B, step):
    """rows with b % 3 == 1 are already finished (at step 2, or at 0 when the call is for step 0 itself -- an earlier call's work)"""
    unf = torch.ones(B, dtype=torch.int32)
    fin = torch.full((B,), -1, dtype=torch.int32)
    for b in range(1, B, 3):
        unf[b] = 0
        fin[b] = min(2, step)
    buf = torch.full((B, 12), SENTINEL, dtype=torch.int64)          # row stride 12 > the 9 columns of `out`
    return unf.to(DEV), fin.to(DEV), buf.to(DEV), torch.full((B,), SENTINEL, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("V", [300, 128258])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_greedy_select_equals_the_composition(B, V):
    from mantis_amd import generation as Gn
    K = _k()
    ld = 304 if V == 300 else K.pad8(V)
    assert ld > V
    n_checked = 0
    for shift in range(4):
        x, want = _logits(B, V, ld, shift)
        arg = x[:, :V].float().argmax(-1)
        for b, t in want.items():
            assert int(arg[b]) == t
        for n_eos in (0, 1, 3):
            # 1: the token row 0 is about to choose (a live row finishing now); 3: the pad id inside the list, row 0's token, and the
            # last row's token (or one nobody chooses, where that row is already finished)
            eos = None if n_eos == 0 else torch.tensor([int(arg[0])] if n_eos == 1 else [PAD, int(arg[0]), int(arg[B - 1])],
                                                       dtype=torch.int64, device=DEV)
            for step in (0, 5):
                got, ref = _state(B, step), _state(B, step)
                K.greedy_select(x, V, eos, PAD, got[0], got[1], got[2][:, :9], step, got[3])
                Gn.select_composition(K, x, V, eos, PAD, ref[0], ref[1], ref[2][:, :9], step, ref[3])
                for a, b_, name in zip(got, ref, ("unfinished", "finish_step", "out", "next_tokens")):
                    assert torch.equal(a, b_), (name, B, V, shift, n_eos, step, a.tolist(), b_.tolist())
                unf, fin, buf, nxt = (t.cpu() for t in got)
                # only column `step` of `out` may change; nothing past its 9 columns
                assert (buf[:, :step] == SENTINEL).all() and (buf[:, step + 1:] == SENTINEL).all() and torch.equal(buf[:, step], nxt)
                for b in range(B):
                    was_finished = n_eos > 0 and b % 3 == 1
                    if was_finished:                    # gets the pad id and keeps its finish step, also where the pad id is an EOS
                        assert int(nxt[b]) == PAD and int(unf[b]) == 0 and int(fin[b]) == min(2, step)
                    else:
                        assert int(nxt[b]) == int(arg[b])
                        if n_eos > 0:                   # (without an EOS the flags stay as they were: checked below)
                            hits = int(arg[b]) in eos.tolist()
                            assert int(unf[b]) == (0 if hits else 1) and int(fin[b]) == (step if hits else -1)
                if n_eos == 0:                          # without an EOS the flags are not touched (here: not even read)
                    s0 = _state(B, step)
                    assert torch.equal(got[0], s0[0]) and torch.equal(got[1], s0[1])
                else:
                    assert int(fin[0]) == step, "row 0 finishes now"
                again = _state(B, step)
                K.greedy_select(x, V, eos, PAD, again[0], again[1], again[2][:, :9], step, again[3])
                assert all(torch.equal(a, b_) for a, b_ in zip(got, again)), "a second call on the same inputs differs"
                n_checked += 1
    assert n_checked == 24


def test_greedy_select_refuses_what_it_does_not_cover():
    K = _k()
    x, _ = _logits(2, 300, 304, 0)
    unf, fin, buf, nxt = _state(2, 0)
    eos = torch.tensor([1], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        K.greedy_select(x, 300, eos, PAD, unf, fin, buf[:, :9], 9, nxt)                     # step outside out
    with pytest.raises(ValueError):
        K.greedy_select(x, 305, eos, PAD, unf, fin, buf[:, :9], 0, nxt)                     # V past the row
    with pytest.raises(ValueError):
        K.greedy_select(x, 300, eos, PAD, unf.to(torch.int64), fin, buf[:, :9], 0, nxt)     # flags must be int32
    with pytest.raises(ValueError):
        K.greedy_select(x, 300, eos.cpu(), PAD, unf, fin, buf[:, :9], 0, nxt)               # the EOS list lives on the device
    assert (buf == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ model level
def _gen(model, kw, **more):
    return model.generate(kw["input_ids"], pixel_values=kw["pixel_values"], pixel_attention_mask=kw["pixel_attention_mask"],
                          attention_mask=kw["attention_mask"], max_new_tokens=kw["max_new_tokens"], **more)


@pytest.mark.parametrize("case", S.CASES)
def test_generate_matches_reference_record(case):
    z = S.load(case)
    model = R.build_product(DEV)
    kw, eos, pad = S.inputs(z)
    eps = Hh.ENVELOPE_FACTOR * float(z["delta"])
    lg = S.teacher_forced_logits(model, kw, torch.from_numpy(z["tokens"]))
    err = np.abs(lg.numpy() - z["logits"])
    print(f"{case}: teacher-forced max |logit error| per step {err.max(axis=(1, 2)).round(4).tolist()} (eps {eps:.4f})")
    assert err.max() <= eps, (case, float(err.max()), eps)
    model.eval()
    out = _gen(model, kw, eos_token_id=eos, pad_token_id=pad)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), z["sequences"]), case
    model.train()
    again = _gen(model, kw, eos_token_id=eos, pad_token_id=pad)
    assert model.training and torch.equal(out, again), "two runs differ"


def test_read_back_interval_does_not_change_the_result():
    from mantis_amd import generation as Gn
    z = S.load("b2_eos")
    model = R.build_product(DEV)
    kw, eos, pad = S.inputs(z)
    outs = [Gn.generate(model, **kw, eos_token_id=eos, pad_token_id=pad, eos_check_every=k) for k in (1, 5)]
    assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy(), z["sequences"])


def test_generate_inside_training_loop_leaves_the_step_untouched():
    from mantis_amd.trainer import MantisHipTrainer
    batch = R.batch(R.load_case("b2_padimg_rightpad"))
    kw, _, _ = S.inputs(S.load("b2_leftpad"))
    res = []
    for with_generate in (False, True):
        model = R.build_product(DEV)
        tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
        tr.training_step(model, batch)
        for p in model.parameters():
            p.grad = None
        if with_generate:
            _gen(model, kw)
            assert model.training
        loss = tr.training_step(model, batch)
        res.append((loss.clone(), model.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def _bars(got, ref, what):
    a, b = got.float().reshape(-1).double(), ref.float().reshape(-1).double()
    cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
    rel = float((a - b).norm() / (b.norm() + 1e-30))
    print(f"{what}: cosine {cos:.6f} rel-L2 {rel:.5f}")
    assert cos >= COS and rel <= REL, (what, cos, rel)


def test_cached_decode_matches_cache_free_step_at_full_width():
    """The widths of `idefics3_full_width_vs_oracle` (SigLIP-so400m/14, Llama-3-8B 4096 / 14336, V = 128259) with the decoder cut to 2
    layers and the tower to 1; B = 2 left-padded with 2 and 1 images (the unused slot zero-filled), 16 new tokens.  The prompt is kept
    under 300 tokens, so the tiles are 224 x 224 (16 x 16 patches -> 64 <image> tokens each; a full 364 x 364 tile alone takes 169):
    T = 208.  The tokens come from the engine's cache-free evaluation step at the generation positions (argmax of the last row, the
    sequence grown by one each step) and are FED to the cached path; every step's cached-decode logits against that step's cache-free
    logits -- two paths through different kernels."""
    from mantis_amd import generation as Gn
    from mantis_amd.configuration_idefics3 import idefics3_8b_llama3
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    cfg = idefics3_8b_llama3()
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    model = Idefics3ForConditionalGeneration(cfg, device=DEV, seed=0)
    model.eval()
    V, n_new, side, n_tok = cfg.text_config.vocab_size, 16, 224, 64
    assert (side // cfg.vision_config.patch_size // cfg.scale_factor) ** 2 == n_tok
    T = 208
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 120000, (2, T), generator=g)
    ids[ids == cfg.image_token_id] = 7
    am = torch.ones_like(ids)
    ids[1, :70] = cfg.pad_token_id
    am[1, :70] = 0
    ids[0, 4: 4 + n_tok] = ids[0, 90: 90 + n_tok] = ids[1, 100: 100 + n_tok] = cfg.image_token_id
    pix = torch.zeros(2, 2, 3, side, side)
    pix[0] = torch.randn(2, 3, side, side, generator=g).to(torch.bfloat16).float()
    pix[1, 0] = torch.randn(3, side, side, generator=g).to(torch.bfloat16).float()
    kw = dict(pixel_values=pix, pixel_attention_mask=None)
    with torch.no_grad():
        cache, logits = Gn.prefill(model, ids, am, pix, n_new)
        assert cache.L == T and cache.position.tolist() == [T, T - 70]
        cur_ids, cur_am = ids, am
        for step in range(n_new):
            ref = S.cache_free_logits(model, kw, cur_ids, cur_am)
            _bars(logits[:, :V], ref, f"full-width step {step}")
            nxt = ref[:, :120000].argmax(-1)
            cur_ids = torch.cat([cur_ids, nxt.cpu()[:, None]], 1)
            cur_am = torch.cat([cur_am, torch.ones_like(cur_am[:, :1])], 1)
            if step + 1 < n_new:
                logits = Gn.decode_step(model, cache, nxt)
