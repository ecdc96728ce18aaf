"""CPU: the C-ABI library loads and exports every symbol include/mantis_hip.h declares (no compute without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "mantis_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\bint\s+(mantis_\w+)\s*\(", _header())))


def _prototypes():
    """name -> the ctypes class of every parameter, from the header's prototypes: a `*` is c_void_p, int64_t c_int64, int / int32_t c_int,
    float c_float; anything else is an error (the binding table would have no word for it)."""
    scalars = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int, "float": ctypes.c_float}
    out = {}
    for name, params in re.findall(r"\bint\s+(mantis_\w+)\s*\(([^)]*)\)\s*;", _header()):
        assert name not in out, f"{name} is declared twice"
        out[name] = []
        for param in (x.strip() for x in params.split(",")):
            if param == "void" and params.strip() == "void":
                continue
            words = [w for w in re.findall(r"\w+", param) if w != "const"]
            if "*" in param:
                out[name].append(ctypes.c_void_p)
            else:
                assert len(words) == 2 and words[0] in scalars, f"{name}: cannot classify the parameter {param!r}"
                out[name].append(scalars[words[0]])
    return out


def test_library_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    from mantis_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mantis_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes binding table and header disagree"


def test_ctypes_table_matches_every_prototype():
    """_lib.SIGNATURES is written out by hand (nothing is parsed at import): every list equals what the header declares, entry by entry."""
    from mantis_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == _declared() == sorted(_lib.SIGNATURES)
    for name, argtypes in _lib.SIGNATURES.items():
        assert argtypes == protos[name], (name, [t.__name__ for t in argtypes], [t.__name__ for t in protos[name]])


def _defines(path, prefix):
    """name -> int of the plain `#define <prefix>... <integer>` lines of a C source"""
    src = open(os.path.join(ROOT, "mantis_amd", "csrc", path)).read()
    return {n: int(v, 0) for n, v in re.findall(r"^#define\s+(%s\w*)\s+(\d+|0x[0-9a-fA-F]+)\s*(?://.*)?$" % prefix, src, flags=re.M)}


def test_gemm_flag_constants_equal_the_c_side():
    """hip_ops states the flag bits once, under the C side's names: every constant of a name csrc/gemm_flags.h or csrc/gemm_fp8.hip defines has
    that value, the fifteen the wrappers build their words from exist, and the fused entry's own two bits are the ones gemm_fused_choose decodes."""
    import __graft_entry__
    __graft_entry__.build()
    from mantis_amd import hip_ops as k
    c_side = {**_defines("gemm_flags.h", "EPI_"), **_defines("gemm_fp8.hip", "F8_EPI_")}
    used = ("EPI_BIAS EPI_ACT_SHIFT EPI_RESIDUAL EPI_ACCUM EPI_SWIGLU_BWD EPI_VARIANT_SHIFT EPI_A_KMAJOR EPI_B_KMAJOR EPI_SK_INKERNEL EPI_SHARED_GPU "
            "EPI_CUS_SHIFT F8_EPI_BIAS F8_EPI_RESIDUAL F8_EPI_ACCUM F8_EPI_VECSCALE").split()
    for n in used:
        assert n in c_side, f"{n} is not a plain define of the C side"
        assert getattr(k, n) == c_side[n], (n, getattr(k, n), c_side[n])
    for n, v in c_side.items():
        if hasattr(k, n):
            assert getattr(k, n) == v, (n, getattr(k, n), v)
    plan = open(os.path.join(ROOT, "mantis_amd", "csrc", "gemm_plan.h")).read()
    body = plan[plan.index("gemm_fused_choose("):]
    decoded = dict((flag, int(bit)) for bit, flag in re.findall(r"\(variant & (\d+)\) \? (EPI_\w+) : 0", body[:body.index("\n}\n")]))
    assert decoded == {"EPI_SK_INKERNEL": k.FUSED_SK_INKERNEL, "EPI_SHARED_GPU": k.FUSED_SHARED_GPU}
    assert (k.FUSED_SK_INKERNEL, k.FUSED_SHARED_GPU) == (64, 128)
    assert not any(hasattr(k, n) for n in ("CUS_SHIFT", "SK_INKERNEL", "SHARED_GPU")), "the unprefixed names are gone, not aliased"


def test_wrappers_hand_the_library_the_recorded_words():
    """Every argument word of the GEMM-family wrappers (flags, strides, shapes, NULLs, the collector's take / give_back order) equals
    tests/golden/hip_ops_calls.json, recorded from the wrappers before the flag bits had names (tests/golden/make_hip_ops_calls.py)."""
    import json
    import __graft_entry__
    __graft_entry__.build()
    from mantis_amd import hip_ops as k
    from tests.golden import make_hip_ops_calls as mk
    with open(mk.FIXTURE) as f:
        want = json.load(f)
    saved = {n: getattr(k, n) for n in mk.PATCHED}
    got = mk.record(k)
    assert all(getattr(k, n) is saved[n] for n in mk.PATCHED), "the recorder left a stand-in in hip_ops"
    assert list(got) == list(want) == ["neutral", "cus240_shared"]
    for ctx in want:
        assert [r["case"] for r in got[ctx]] == [r["case"] for r in want[ctx]]
        for g, w in zip(got[ctx], want[ctx]):
            assert g["calls"] == w["calls"], (ctx, w["case"])
    assert len(want["neutral"]) >= 50


def test_no_oracle_import_in_product():
    """The product package must not reach the oracle (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "mantis_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            txt = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in txt and "from oracle" not in txt, fn


def test_gemm_tile_heuristic_is_exposed_and_sane():
    """mantis_gemm_pick_variant is pure host arithmetic (no GPU needed): 12 = 256x256 ring kernel, 1 = 128x128 generic kernel."""
    from mantis_amd import _lib
    L = _lib.load()
    assert L.mantis_gemm_pick_variant(5624, 28672, 4096) == 12      # gate|up projection of the 8B step
    assert L.mantis_gemm_pick_variant(28672, 4096, 5624) == 12      # its weight gradient
    assert L.mantis_gemm_pick_variant(300, 200, 72) == 1            # small: generic kernel
    assert L.mantis_gemm_pick_variant(4608, 1152, 1152) == 1        # ViT out-projection: 90 big tiles would idle most CUs


def test_library_path_override(monkeypatch, tmp_path):
    """MANTIS_HIP_LIB points the loader at another build (A/B runs); a missing file fails loudly, never falls back."""
    import importlib
    import pytest
    from mantis_amd import _lib
    monkeypatch.setenv("MANTIS_HIP_LIB", str(tmp_path / "nope.so"))
    m = importlib.reload(_lib)
    try:
        with pytest.raises(ImportError):
            m.load()
    finally:
        monkeypatch.delenv("MANTIS_HIP_LIB")
        importlib.reload(_lib)
