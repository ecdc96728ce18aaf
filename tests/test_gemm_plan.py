"""CPU: every decision of the bf16 GEMM planner (csrc/gemm_plan.h: tile variant per entry point and layout, K split, balanced remainder round,
176-row tile, paired dW, workspace, operand checks) equals tests/golden/gemm_plan.json.  The dump program (tools/gemm_plan_dump.cpp) is built
from the header alone with the host compiler -- no device code, no GPU -- and run over the full sweep with the default environment and over
the reduced sweep once per value of each MANTIS_GEMM_* switch.  A planner edit that moves any decision fails here and names the entry; an
intended change re-records the fixture (tests/golden/make_gemm_plan.py)."""
import json

import pytest

from tests.golden import make_gemm_plan as mk


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return mk.build(str(tmp_path_factory.mktemp("gemm_plan")))       # a missing compiler is an error, not a skip


@pytest.fixture(scope="module")
def golden():
    with open(mk.FIXTURE) as f:
        return json.load(f)


def _flat(section):
    """{"M,N": {"K": [row per budget]}} -> {"M,N,K,#i": row}; flat sections as they are."""
    out = {}
    for k, v in section.items():
        if isinstance(v, dict):
            for k2, rows in v.items():
                out.update({f"{k},{k2},#{i}": r for i, r in enumerate(rows)})
        else:
            out[k] = v
    return out


def _same(got, want, where):
    assert sorted(got) == sorted(want), where
    for section in want:
        if isinstance(want[section], dict):
            g, w = _flat(got[section]), _flat(want[section])
            assert sorted(g) == sorted(w), (where, section)
            bad = [(k, g[k], w[k]) for k in w if g[k] != w[k]]
            assert not bad, f"{where}: {len(bad)} entries of {section!r} differ, first (key, got, recorded): {bad[:3]}"
        else:
            assert got[section] == want[section], (where, section)


def test_default_environment_full_sweep(exe, golden):
    want = golden["default"]
    assert len(_flat(want["rows"])) == 11 * 11 * 12 * 2 and len(want["more"]) == 3 * 4 * 4 * 2 + 5 and want["dev_cus"] == 256
    _same(mk.run(exe), want, "default")


@pytest.mark.parametrize("switch", [f"{k}={v}" for k, v in mk.ENV])
def test_each_environment_switch_reduced_sweep(exe, golden, switch):
    k, v = switch.split("=")
    _same(mk.run(exe, True, {k: v}), golden["env"][switch], switch)


def test_the_sweep_holds_the_remainder_plan_tests_shapes(golden):
    from tests.test_gemm_remainder_plan import SHAPES
    for M, N, K, cus in SHAPES:
        assert mk.row(golden["default"], M, N, K, cus)["pick"] in (1, 12)
