"""Arena layout, gradient buckets and seed-0 initialisation of every model class at the tiny test geometries, recorded as a fixture
(tests/golden/arena_layout.json) so that a change of the host-side plumbing which moves a parameter, a bucket or a drawn value shows up
as a readable difference (tests/test_arena_layout.py::test_layout_buckets_and_init_match_the_recorded_fixture).

Per model: `layout` = [name, shape, offset in the parameter arena] in arena order; `buckets` = [key, offset in the gradient arena,
numel] in `grad_buckets()` order (key = "head" / "front" / ["layer", i, "down" | "gu" | "attn"]); `init_sha256` = sha256 of the arena's
bytes after `reset_parameters(0)` on the CPU.  The digest depends on torch's CPU generator, so the file also records `torch_version`;
on another torch version the test fails and asks for this script to be run again -- on a commit whose layout is known to be right.

    python tests/golden/make_arena_layout.py        (from the repository root; CPU only, a few seconds)"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arena_layout.json")


def _seqcls():
    from tests import helpers as Hh
    from mantis_amd.configuration_idefics2 import Idefics2Config
    from mantis_amd.modeling_idefics2 import Idefics2ForSequenceClassification
    meta, _ = Hh.golden_cfg_and_weights("idefics2")
    cfg = Idefics2Config.from_oracle_meta(dict(meta, num_labels=5, problem_type="regression", pad_token_id=0))
    return Idefics2ForSequenceClassification(cfg, device="cpu", init=None)


def builders():
    from tests import helpers as Hh
    from tests import idefics3_ref
    return {
        "llava_siglip": lambda: Hh.build_product_model("siglip", "cpu")[0],
        "llava_clip": lambda: Hh.build_product_model("clip", "cpu")[0],
        "idefics2": lambda: Hh.build_idefics2_product("cpu"),
        "idefics2_seqcls": _seqcls,
        "qwen2vl": lambda: Hh.build_qwen2vl_product("cpu"),
        "idefics3": lambda: idefics3_ref.build_product("cpu"),
    }


def record(model):
    """What the fixture holds for one model (JSON-ready: lists, ints, strings).  Overwrites the model's parameters."""
    layout = [[name, list(shape), model._offs[name]] for name, shape in model._specs]
    buckets = model.grad_buckets()
    base = model.grad_arena.data_ptr()
    size = model.grad_arena.element_size()
    bk = [[list(k) if isinstance(k, tuple) else k, (b.data_ptr() - base) // size, b.numel()] for k, b in buckets.items()]
    model.reset_parameters(0)
    digest = hashlib.sha256(model.arena.view(torch.int16).numpy().tobytes()).hexdigest()
    return dict(arena_numel=model.arena.numel(), grad_arena_numel=model.grad_arena.numel(), layout=layout, buckets=bk, init_sha256=digest)


def _dumps(out):
    """JSON with one tensor / one bucket per line, so that a diff of the fixture reads like a diff of the layout"""
    def rows(v):
        return "[\n" + ",\n".join(json.dumps(r) for r in v) + "\n]"
    models = ",\n".join(
        json.dumps(name) + ": {" + ", ".join(json.dumps(k) + ": " + (rows(v) if isinstance(v, list) else json.dumps(v)) for k, v in m.items()) + "}"
        for name, m in out["models"].items())
    head = ", ".join(json.dumps(k) + ": " + json.dumps(v) for k, v in out.items() if k != "models")
    return "{" + head + ',\n"models": {\n' + models + "\n}}"


def main():
    out = {"__doc__": "written by tests/golden/make_arena_layout.py (see its docstring)", "torch_version": torch.__version__,
           "models": {name: record(build()) for name, build in builders().items()}}
    with open(OUT, "w") as f:
        f.write(_dumps(out) + "\n")
    print(f"wrote {OUT}: " + ", ".join(f"{k} ({len(v['layout'])} tensors, {len(v['buckets'])} buckets)" for k, v in out["models"].items()))


if __name__ == "__main__":
    main()
