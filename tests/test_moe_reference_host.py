"""tests/moe_reference.py and the bounds of tests/test_moe_ops_gpu.py proved without a GPU.

The emulation (moe_reference.emulated_device) stands in for the device: unmutated it must pass every assertion of the GPU
file on every case of the GPU file, and each of six mutations of it — the kernel errors the model-level MoE tests cannot
see — must break the bound it is aimed at, on the case the GPU file would catch it with."""
import numpy as np
import pytest

import moe_reference as R
from test_moe_ops_gpu import MOE_RATIO_BOUND, EXPERT_CASES

DENSE = {i + 1: c for i, c in enumerate(R.DENSE_CASES)}      # numbered as the list in test_moe_ops_gpu.py


@pytest.mark.parametrize("M,E,k", R.ROUTING_CASES)
def test_unmutated_routing_passes(M, E, k):
    inp = R.crafted_routing_inputs(M, E, k)
    kinds = [R.ROW_KINDS[r % 4] for r in range(M)]
    lg = R.router_logits(inp["x"], inp["router"])
    assert np.array_equal(lg, inp["router"][np.arange(M) % 64].astype(np.float64))        # one router entry per logit
    gaps = np.abs(lg[:, :, None] - lg[:, None, :])
    assert ((gaps == 0) | (gaps >= 0.125)).all() and np.abs(lg).max() <= 4.0
    srt = -np.sort(-lg, axis=1)
    for r, kind in enumerate(kinds):       # the rows carry the ties they are named for
        if kind == "boundary_tie" and k < E:
            assert srt[r, k - 1] == srt[r, k]
        if kind == "inner_tie" and k >= 2:
            assert srt[r, 0] == srt[r, 1]
        if kind == "all_equal":
            assert (lg[r] == lg[r, 0]).all()
        if kind == "distinct":
            assert np.unique(lg[r]).size == E
    for form in ("dense_fused", "plan"):
        R.check_routing_exact(inp, R.emulated_device(inp, form))
    rnd = R.random_inputs(M, E, k, 64, 64)
    R.check_routing_random(rnd, R.emulated_device(rnd, "dense"))


@pytest.mark.parametrize("name,inp,forms", EXPERT_CASES, ids=[c[0] for c in EXPERT_CASES])
def test_unmutated_experts_pass(name, inp, forms):
    inp = inp()
    for form in sorted({"dense" if f in R.DENSE_FORMS else "plan" for f, _ in forms}):
        out = R.emulated_device(inp, form)
        R.check_routing_random(inp, out)
        ratio = R.check_experts(inp, out, MOE_RATIO_BOUND, name)
        assert np.abs(ratio - 1.0).max() <= 1e-3        # (the stand-in is the emulation rounded to fp32)


@pytest.mark.parametrize("skew", R.SKEWS)
def test_skew_inputs_route_as_dictated(skew):
    inp = R.skew_inputs(skew)
    gate = R.route(R.router_logits(inp["x"], inp["router"]), 2)
    assert [tuple(np.flatnonzero(g)) for g in gate] == [tuple(sorted(p)) for p in inp["picks"]]
    picked = (gate != 0).sum(0)
    if skew == "two_experts":
        assert list(np.flatnonzero(picked)) == [2, 5]
    elif skew == "one_token_each":
        assert (picked[2:] == 1).all() and np.flatnonzero(gate[:, 7]).tolist() == [19]
    else:
        assert np.flatnonzero(gate[:, 0]).tolist() == [0]
    R.check_experts(inp, R.emulated_device(inp, "dense"), MOE_RATIO_BOUND, skew)


def mutated(inp, form="dense_fused", gate=None, w_out=None):
    """the stand-in device with its expert stage run on a mutated gate matrix or down weight (what it REPORTS is unmutated)"""
    out = R.emulated_device(inp, form)
    out["y"] = R.experts_emulated(inp["x"], inp["w_in"], inp["w_out"] if w_out is None else w_out,
                                  out["gate"] if gate is None else gate, form).astype(np.float32)
    return out


def test_mutation_a_dropped_pair():
    inp = R.random_inputs(*DENSE[1])
    out = R.emulated_device(inp, "dense_fused")
    g = out["gate"].copy()
    g[0, np.flatnonzero(g[0])[-1]] = 0.0
    with pytest.raises(AssertionError):
        R.check_experts(inp, mutated(inp, gate=g), MOE_RATIO_BOUND)


def test_mutation_b_no_renormalisation():
    inp = R.random_inputs(*DENSE[1])
    out = R.emulated_device(inp, "dense_fused")
    out["gate"] = np.where(out["gate"] != 0, R.softmax(out["router_logits"]), 0.0).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_routing_random(inp, out)
    crafted = R.crafted_routing_inputs(3, 8, 2)
    out = R.emulated_device(crafted, "dense_fused")
    out["gate"] = np.where(out["gate"] != 0, R.softmax(out["router_logits"]), 0.0).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_routing_exact(crafted, out)


def test_mutation_c_tie_to_the_higher_index():
    inp = R.crafted_routing_inputs(3, 8, 2)
    out = R.emulated_device(inp, "dense_fused")
    lg = out["router_logits"][0]                       # row 0: a two-way tie across the top-k boundary
    lo = int(np.flatnonzero(out["gate"][0])[np.argmin(lg[np.flatnonzero(out["gate"][0])])])
    twins = [e for e in np.flatnonzero(lg == lg[lo]) if e != lo]
    assert len(twins) == 1 and twins[0] > lo and out["gate"][0, twins[0]] == 0
    out["gate"][0, twins[0]], out["gate"][0, lo] = out["gate"][0, lo], 0.0      # same weights: only the selection tells
    with pytest.raises(AssertionError, match="selection"):
        R.check_routing_exact(inp, out)
    R.check_routing_random(inp, out)                   # (and the random-input assertions cannot: why the crafted case exists)


def test_mutation_d_last_k_step_of_one_expert():
    inp = R.random_inputs(*DENSE[2])                    # I = 96: three k-steps, the ragged tail of the down loop
    w = inp["w_out"].copy()
    w[3, :, 64:] = 0.0
    assert R.emulated_device(inp, "dense")["gate"][:, 3].any()
    with pytest.raises(AssertionError):
        R.check_experts(inp, mutated(inp, w_out=w), MOE_RATIO_BOUND)


def test_mutation_e_block_31_of_32():
    inp = R.random_inputs(*DENSE[8])                    # I = 4096 at U = 4: 32 blocks of 128 columns
    w = inp["w_out"].copy()
    w[1, :, 31 * 128:] = 0.0
    assert R.emulated_device(inp, "dense")["gate"][:, 1].any()
    with pytest.raises(AssertionError):
        R.check_experts(inp, mutated(inp, w_out=w), MOE_RATIO_BOUND)


def test_mutation_f_gate_row_off_by_one():
    inp = R.random_inputs(*DENSE[4])                    # M = 17: the last row is alone in its 16-row tile
    out = R.emulated_device(inp, "dense_fused")
    g = out["gate"].copy()
    g[-1] = g[-2]
    assert not np.array_equal(out["gate"][-1], out["gate"][-2])
    with pytest.raises(AssertionError):
        R.check_experts(inp, mutated(inp, gate=g), MOE_RATIO_BOUND)
