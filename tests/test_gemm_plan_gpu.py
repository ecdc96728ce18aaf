"""GPU: what the planner decides on the CPU (csrc/gemm_plan.h, held to tests/golden/gemm_plan.json by tests/test_gemm_plan.py) is what launches.
For one shape per planner outcome -- the entry of the recorded table with the smallest M * N * K -- the library's own plan on this device equals
the recorded row, and a launch with variant 0 is bit-identical to a launch that names the variant the table predicts (the K split is the
planner's for both; naming the variant pins the kernel).  A handful of small GEMM launches each."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests.golden import make_gemm_plan as mk

pytestmark = pytest.mark.gpu

# outcome: (M, N, K, A K-major, B K-major, variant).  From the table's rows with budget 0 (plain entry point): variant 1; 13; 14 without a
# split; 14 with an equal split (S = 6 x 4 remainder tiles); 14 with the balanced round (10 remainder tiles x 448 K-steps in 256 ranges, B
# K-major: the NT layout of that size goes to 13); 15.
OUTCOMES = {
    "variant_1": (256, 256, 64, False, False, 1),
    "variant_13": (384, 384, 25600, False, False, 13),
    "variant_14_no_split": (8192, 1152, 64, False, False, 14),
    "variant_14_equal_split": (384, 384, 4096, False, False, 14),
    "variant_14_balanced_round": (384, 1152, 28672, False, True, 14),
    "variant_15": (8192, 1152, 504, False, False, 15),
}
PAIR = ((512, 256), (512, 256), 512)          # the smallest paired-dW win of the table: two dW of [512, 256] over 512 rows


@pytest.fixture(scope="module")
def table():
    with open(mk.FIXTURE) as f:
        return json.load(f)["default"]


def _rand(*shape):
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    return (torch.randn(*shape, generator=g) * 0.5).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("outcome", list(OUTCOMES))
def test_auto_launch_is_the_predicted_variant_bit_for_bit(table, outcome):
    from mantis_amd import _lib, hip_ops as k
    M, N, K, akm, bkm, variant = OUTCOMES[outcome]
    L = _lib.load()
    if L.mantis_gemm_cu_budget(0) != table["dev_cus"]:
        pytest.fail(f"the table is recorded for {table['dev_cus']} CUs, this device plans for {L.mantis_gemm_cu_budget(0)}")
    row = mk.row(table, M, N, K, 0)
    assert row["entries"][2 * akm + bkm] == "0123456789abcdef"[variant], (outcome, row)
    buf = np.zeros(8 + 4 * 1024, dtype=np.int32)
    assert L.mantis_gemm_remainder_plan(M, N, K, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.size) >= 8
    tiles, full, rem, S, units, tails, nwg, nk = buf[:8].tolist()
    want = [row[f] for f in ("pick", "S", "full", "rem", "units", "tails", "nwg")]
    assert [L.mantis_gemm_pick_variant(M, N, K), S, full, rem, units, tails, nwg] == want, (outcome, buf[:8].tolist(), row)
    assert L.mantis_gemm_workspace_bytes(M, N, K) == (table["ws_bytes"] if row["needs_ws"] else 0)
    if outcome == "variant_14_no_split":
        assert S == 1
    if outcome == "variant_14_equal_split":
        assert S > 1 and units == 0
    if outcome == "variant_14_balanced_round":
        assert S > 1 and units == table["dev_cus"]
    a = _rand(K, M) if akm else _rand(M, K)
    b = _rand(K, N) if bkm else _rand(N, K)
    auto = k.gemm_nt(a, b, a_kmajor=akm, b_kmajor=bkm)
    named = k.gemm_nt(a, b, a_kmajor=akm, b_kmajor=bkm, variant=variant)
    again = k.gemm_nt(a, b, a_kmajor=akm, b_kmajor=bkm)
    torch.cuda.synchronize()
    assert torch.equal(auto, named), f"{outcome}: variant 0 did not launch what variant {variant} launches"
    assert torch.equal(auto, again)
    ref = (a.float().t() if akm else a.float()) @ (b.float() if bkm else b.float().t())
    # bf16 result of an fp32 accumulation: half an ulp of the result (2^-9 relative) + the fp32 summation error, well inside 2^-7 of the largest value
    assert float((auto.float() - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -7


def test_paired_dw_win_is_one_launch_of_whole_variant_14_tiles(table):
    from mantis_amd import hip_ops as k
    (M1, N1), (M2, N2), K = PAIR
    shapes = [tuple(s) for s in table["pair_shapes"]]
    i, j = shapes.index((M1, N1)), shapes.index((M2, N2))
    assert table["pairs"][f"{K},0"][i * len(shapes) + j] == "1"
    assert k.dw_pair_wins(M1, N1, M2, N2, K)
    dy1, x1, dy2, x2 = _rand(K, M1), _rand(K, N1), _rand(K + 1, M2)[:K], _rand(K + 2, N2)[:K]
    g1, g2 = torch.zeros(M1, N1, dtype=torch.bfloat16, device="cuda"), torch.zeros(M2, N2, dtype=torch.bfloat16, device="cuda")
    k.linear_dw_pair(dy1, x1, g1, dy2, x2, g2, False)
    # neither shape has a K-split remainder (2 tiles x 8 K-steps): the paired grid runs the same whole tiles as variant 14
    w1 = k.gemm_nt(dy1, x1, a_kmajor=True, b_kmajor=True, variant=14)
    w2 = k.gemm_nt(dy2, x2, a_kmajor=True, b_kmajor=True, variant=14)
    torch.cuda.synchronize()
    assert torch.equal(g1, w1) and torch.equal(g2, w2)
