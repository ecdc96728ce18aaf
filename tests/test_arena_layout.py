"""Placement rules of the flat parameter / gradient arenas (`mantis_amd/arena.py`; round 4): every parameter starts on a
256-byte boundary -- the forward GEMMs fetch weights in 128-byte row segments, and a 16-byte aligned arena left every decoder weight of
Mantis-8B 96 bytes into a cache line (profiles/r04_experiments.md 12) -- except the later members of a fused projection, which must
stay adjacent (zero-copy q|k|v / gate|up views); DP buckets tile the gradient arena; the optimizer's segments cover every trainable
parameter exactly once.  CPU only: layouts are host logic."""
import pytest
import torch

from tests import helpers as Hh

BUILDERS = {
    "llava_siglip": lambda: Hh.build_product_model("siglip", "cpu")[0],
    "llava_clip": lambda: Hh.build_product_model("clip", "cpu")[0],
    "idefics2": lambda: Hh.build_idefics2_product("cpu"),
    "qwen2vl": lambda: Hh.build_qwen2vl_product("cpu"),
}


@pytest.fixture(params=list(BUILDERS))
def model(request):
    return BUILDERS[request.param]()


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def test_parameters_start_on_256_byte_boundaries_and_views_are_the_arena(model):
    from mantis_amd.arena import ARENA_ALIGN
    assert ARENA_ALIGN == 128
    base = model.arena.data_ptr()
    end = 0
    for name, shape in model._specs:
        off = model._offs[name]
        p = model._param(name)
        assert p.data_ptr() == base + 2 * off and tuple(p.shape) == tuple(shape), name
        assert off >= end, name                                           # no overlap, arena order
        if name.endswith(model.adjacent_suffixes):
            assert off == end, f"{name}: a fused projection's member must directly follow its predecessor"
        else:
            assert off % ARENA_ALIGN == 0, f"{name} starts {2 * (off % ARENA_ALIGN)} bytes into a 256-byte block"
            assert off - end < ARENA_ALIGN
        end = off + (_numel(shape) + 7) // 8 * 8
    assert model.arena.numel() == end
    # what lies between parameters is zero and stays out of every view
    mask = torch.ones(model.arena.numel(), dtype=torch.bool)
    for name, shape in model._specs:
        mask[model._offs[name]: model._offs[name] + _numel(shape)] = False
    assert float(model.arena[mask].float().abs().sum()) == 0.0


def test_headline_geometry_puts_every_decoder_weight_on_a_line_boundary():
    """The case that cost 6.7 ms per step: Mantis-8B-SigLIP-Llama-3's specs (no tensors are allocated here)."""
    from mantis_amd.configuration_llava import mantis_8b_siglip_llama3
    from mantis_amd import modeling_llava as ml
    from mantis_amd.arena import ArenaModule
    specs = ml._param_specs(mantis_8b_siglip_llama3())
    offs, total = ArenaModule._place(ml.LlavaForConditionalGeneration, [(n, _numel(s)) for n, s in specs])
    two_d = [n for n, s in specs if len(s) == 2 and n.startswith(("language_model", "multi_modal_projector"))]
    assert len(two_d) > 200 and all((2 * offs[n]) % 128 == 0 for n in two_d)
    # round 3's rule (16-byte alignment) reproduces the defect: 96 bytes into a line from the projector on
    off8, o = {}, 0
    for n, s in specs:
        off8[n] = o
        o += (_numel(s) + 7) // 8 * 8
    assert {(2 * off8[n]) % 128 for n in two_d} == {96}
    assert total - o < 128 * len(specs)


def test_gradient_buckets_tile_the_gradient_arena(model):
    model._ensure_grad_arena()
    buckets = model.grad_buckets()
    base = model.grad_arena.data_ptr()
    spans = sorted((b.data_ptr() - base, b.numel() * 2) for b in buckets.values())
    pos = 0
    for start, nbytes in spans:
        assert start == pos, "buckets must be contiguous and non-overlapping"
        pos += nbytes
    assert pos == model.grad_arena.numel() * 2
    assert all(o % 128 == 0 or n.endswith(model.adjacent_suffixes) for n, o in model._grad_offs.items())


def test_optimizer_segments_cover_every_trainable_parameter_once(model, monkeypatch):
    from mantis_amd.optim import FusedAdamW
    import mantis_amd.optim as opt_mod
    from oracle import ops_ref
    monkeypatch.setattr(opt_mod, "K", ops_ref)      # construction and `opt.master` (joined on demand) run on the oracle's operators
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, no_decay=lambda n: model._param(n).dim() <= 1)
    cover_p = torch.zeros(model.arena.numel(), dtype=torch.int32)
    cover_g = torch.zeros(model.grad_arena.numel(), dtype=torch.int32)
    for p_off, g_off, cnt, _ in opt._segments:
        cover_p[p_off:p_off + cnt] += 1
        cover_g[g_off:g_off + cnt] += 1
    assert int(cover_p.max()) <= 1 and int(cover_g.max()) <= 1
    for n in opt._names:
        k = model._param(n).numel()
        assert bool((cover_p[model._offs[n]: model._offs[n] + k] == 1).all()), n
        assert bool((cover_g[model._grad_offs[n]: model._grad_offs[n] + k] == 1).all()), n
    # a segment never reaches into a frozen parameter
    frozen = [n for n, _ in model._specs if n not in set(opt._names)]
    for n in frozen:
        k = model._param(n).numel()
        assert int(cover_p[model._offs[n]: model._offs[n] + k].sum()) == 0, n
    # the fp32 masters mirror the parameters in the gradient arena's layout, zeros elsewhere
    ref = torch.zeros(model.grad_arena.numel())
    for n in opt._names:
        ref[model._grad_offs[n]: model._grad_offs[n] + model._param(n).numel()] = model._param(n).detach().float().reshape(-1)
    assert torch.equal(opt.master.cpu(), ref)


def test_arena_alignment_variable_is_validated(monkeypatch):
    """MANTIS_ARENA_ALIGN (round-4 advisor finding): 0 used to end in a ZeroDivisionError in _place(), a value that is not a multiple of 8
    broke the 16-byte alignment the GEMM / AdamW / sum-of-squares kernels assume."""
    import pytest
    from mantis_amd import arena
    for bad in ("0", "4", "12", "-8", "lots"):
        monkeypatch.setenv("MANTIS_ARENA_ALIGN", bad)
        with pytest.raises(ValueError):
            arena._arena_align()
    for good, want in (("8", 8), ("128", 128), ("256", 256)):
        monkeypatch.setenv("MANTIS_ARENA_ALIGN", good)
        assert arena._arena_align() == want
    monkeypatch.delenv("MANTIS_ARENA_ALIGN")
    assert arena._arena_align() == 128


def test_optimizer_state_records_the_alignment_it_was_laid_out_with(monkeypatch):
    """A FusedAdamW checkpoint belongs to the arena layout it was written under: the alignment is part of the state and a mismatch is
    reported as such (it used to surface as a tensor-shape mismatch)."""
    import pytest
    import mantis_amd.engine as eng
    import mantis_amd.optim as opt
    from oracle import ops_ref
    from tests import helpers as Hh
    monkeypatch.setattr(eng, "K", ops_ref)
    monkeypatch.setattr(opt, "K", ops_ref)
    model, _, _ = Hh.build_product_model("siglip", "cpu")
    o = opt.FusedAdamW(model, lr=1e-3)
    sd = o.state_dict()
    assert sd["arena_align"] == opt.ARENA_ALIGN
    o.load_state_dict(sd)                                       # round trip
    with pytest.raises(ValueError, match="aligned to 8 elements"):
        o.load_state_dict(dict(sd, arena_align=8))


@pytest.fixture(scope="module")
def layout_fixture():
    import json
    import os
    with open(os.path.join(Hh.G, "arena_layout.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["llava_siglip", "llava_clip", "idefics2", "idefics2_seqcls", "qwen2vl", "idefics3"])
def test_layout_buckets_and_init_match_the_recorded_fixture(layout_fixture, name):
    """Every parameter's (name, shape, offset), every gradient bucket's (key, offset, numel) and the arena bytes after
    `reset_parameters(0)` equal what tests/golden/make_arena_layout.py recorded: the shared plumbing (mantis_amd/backbone.py, arena.py) must
    not move a tensor, a bucket or a drawn value.  Lists are compared, not digests, so a mismatch names the tensor."""
    from tests.golden import make_arena_layout as mk
    assert torch.__version__ == layout_fixture["torch_version"], (
        f"tests/golden/arena_layout.json was recorded with torch {layout_fixture['torch_version']}, this is {torch.__version__}: the seed-0 "
        "digests depend on torch's CPU generator -- run tests/golden/make_arena_layout.py again (on a commit whose layout is known good)")
    want = layout_fixture["models"][name]
    got = mk.record(mk.builders()[name]())
    assert got["layout"] == want["layout"]
    assert got["buckets"] == want["buckets"]
    assert (got["arena_numel"], got["grad_arena_numel"]) == (want["arena_numel"], want["grad_arena_numel"])
    assert got["init_sha256"] == want["init_sha256"]
