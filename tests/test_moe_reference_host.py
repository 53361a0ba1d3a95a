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


# ---- quantized experts: tests/test_moe_q_ops_gpu.py proved without a GPU ------------------------------------------------
# The stand-in (moe_reference.emulated_device_q) reports W~ of the mirror and computes with it: unmutated it passes every
# check of every case and format, its h at a ratio of exactly 1.  Each mutation below makes it COMPUTE with what a wrong
# kernel would read — while it still reports the right W~, as a device whose decode kernel is wrong and whose dequantize
# kernel is right would — and must fail the check aimed at it.
import dense_reference as D
from test_int4_weights_gpu import bf16_rne
from test_kv_fp8_gpu import VALUES
from test_moe_q_ops_gpu import ALL_Q_CASES, MOE_Q_RATIO_BOUND, chain_gu, inputs

QB = MOE_Q_RATIO_BOUND
CHECK_H = lambda q, o: R.check_h(q, o, QB)
CHECK_DOWN = lambda q, o: R.check_down(q, o)
CHECK_Y = lambda q, o: R.check_experts(q, o, QB)


@pytest.mark.parametrize("name,fmt,shape,g,crafted,forms", ALL_Q_CASES, ids=[c[0] for c in ALL_Q_CASES])
def test_unmutated_q_passes(name, fmt, shape, g, crafted, forms):
    q = inputs(shape, fmt, g, crafted)
    assert np.array_equal(bf16_rne(q["w_in"]).view(np.uint32), q["w_in"].view(np.uint32))          # W~ is exact in bf16
    assert np.array_equal(bf16_rne(q["w_out"]).view(np.uint32), q["w_out"].view(np.uint32))
    for form in sorted({"dense" if f in R.DENSE_FORMS else "plan" for f, _ in forms}):
        out = R.emulated_device_q(q, form)
        ratio = R.check_all_q(q, out, QB, name)
        assert np.abs(ratio - 1.0).max() <= 1e-3        # (y of the stand-in is the emulation rounded to fp32)
        if form == "dense":
            assert set(R.h_ratio(q, out).values()) == {1.0}       # (its h IS the emulation)


def chain_standin(q, ran, form, mut=None):
    """dense_reference.emulated_moe_device with the outputs the quantized op adds: W~ as reported, h from the same scales"""
    out = D.emulated_moe_device(q, ran, form, mut)
    out.update(wt_in=q["w_in"].copy(), wt_out=q["w_out"].copy())
    rs_u = np.roll(out["rs1"], -1, 0) if mut == "neighbour_rstd" else out["rs1"]
    out["h"] = R.emulated_h(q, out["gate"], gu=chain_gu(q, dict(out, rs1=rs_u)))
    return out


def check_chain(q, out):
    R.check_wt(out, q)
    D.check_moe_chain(q, out, QB)
    R.check_h(q, out, QB, "", chain_gu(q, out))
    R.check_down(q, out, "", base=out["x1"], alpha=float(np.float32(D.alphas(q)[0])))


CHAIN_Q = [c for c in D.MOE_Q_CASES if c[3] == {}]       # (the stand-in does not depend on the routing form)


@pytest.mark.parametrize("fmt,g,M,keys,form,ran,shape", CHAIN_Q, ids=[f"{c[0]}-M{c[2]}-E{c[6]['E']}" for c in CHAIN_Q])
def test_unmutated_chain_q_passes(fmt, g, M, keys, form, ran, shape):
    q = D.moe_inputs_q(M, fmt, g, shape)
    out = chain_standin(q, ran, form)
    check_chain(q, out)
    assert set(R.h_ratio(q, out, chain_gu(q, out)).values()) == {1.0}


def q_case(fmt, number):
    shape, g = R.Q_CASES[number - 1]
    return inputs(shape, fmt, g, number in R.Q_CRAFTED)


def fails(q, compute_with, checks, form="dense_fused", **kw):
    """the stand-in computing with the mutated experts passes check_wt (it reports the right W~) and fails each check"""
    for key, w in compute_with.items():
        assert not np.array_equal(w, q[key]), "the mutation changed nothing"
    out = R.emulated_device_q(q, form, compute_with, **kw)
    R.check_wt(out, q)
    for check in checks:
        with pytest.raises(AssertionError):
            check(q, out)


def rows2d(q, key):
    E, N, K = q[key].shape
    return R.mirror(q["fmt"])(q["raw_" + key[2:]].reshape(E * N, K), q["g"]), (E, N, K)


def nibbles(packed):
    c = np.empty((packed.shape[0], 2 * packed.shape[1]), np.float32)
    c[:, 0::2], c[:, 1::2] = packed & 15, packed >> 4
    return c


def first_live_expert(q):
    return int(np.flatnonzero(R.emulated_device(q, "dense")["gate"].any(0))[0])


def test_q_mutation_a_fp8_down_scale_rows_of_the_next_expert():
    q = q_case("fp8", 4)
    m, (E, H, I) = rows2d(q, "w_out")
    s = np.roll(m["s"].reshape(E, H), -1, 0)
    w = bf16_rne(VALUES[m["codes"]].astype(np.float32).reshape(E, H, I) * s[:, :, None])
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y])


def test_q_mutation_b_fp8_up_scales_not_following_the_interleave():
    q = q_case("fp8", 2)
    m, (E, N, K) = rows2d(q, "w_in")
    I = N // 2
    idx = np.concatenate([np.r_[16 * b:16 * b + 16, I + 16 * b:I + 16 * b + 16] for b in range(I // 16)])     # device row p holds row idx[p]
    s = m["s"].reshape(E, N).copy()
    s[:, idx] = m["s"].reshape(E, N)          # ... and is scaled by the scale of row p
    w = bf16_rne(VALUES[m["codes"]].astype(np.float32).reshape(E, N, K) * s[:, :, None])
    fails(q, dict(w_in=w), [CHECK_H])


def test_q_mutation_c_mxfp4_last_block_scale_from_the_next_expert():
    q = q_case("mxfp4", 2)
    m, (E, H, I) = rows2d(q, "w_out")
    s = m["s"].reshape(E, H, I // 32).astype(np.int32)
    w = q["w_out"].copy()
    w[:-1, :, -32:] = np.ldexp(w[:-1, :, -32:], (s[1:, :, 0] - s[:-1, :, -1])[:, :, None])
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y])


def test_q_mutation_d_int4_group_words_shifted_across_the_expert_boundary():
    q = q_case("int4", 2)                              # I = 96, g = 32: the last of three groups takes the next expert's first word
    m, (E, H, I) = rows2d(q, "w_out")
    g = q["g"]
    s, z = m["s"].astype(np.float32).reshape(E, H, I // g), m["z"].astype(np.float32).reshape(E, H, I // g)
    code = nibbles(m["codes"]).reshape(E, H, I)
    w = q["w_out"].copy()
    w[:-1, :, -g:] = bf16_rne(s[1:, :, :1] * (code[:-1, :, -g:] - z[1:, :, :1]))
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y])


def test_q_mutation_e_int4_zero_point_of_one_group_read_as_0():
    q = q_case("int4", 1)
    m, (E, N, K) = rows2d(q, "w_in")
    e, r = first_live_expert(q), 7                     # one group of one gate row of a live expert
    g = q["g"]
    assert m["z"].reshape(E, N, K // g)[e, r, 0] != 0
    w = q["w_in"].copy()
    w[e, r, :g] = bf16_rne(m["s"].astype(np.float32).reshape(E, N, K // g)[e, r, 0] * nibbles(m["codes"]).reshape(E, N, K)[e, r, :g])
    fails(q, dict(w_in=w), [CHECK_H])


@pytest.mark.parametrize("fmt", ["mxfp4", "int4"])
def test_q_mutation_f_nibble_order_swapped_in_one_k_step(fmt):
    q = q_case(fmt, 3)                                 # I = 32: the down matrix of an expert is one k-step
    e = first_live_expert(q)
    w = q["w_out"].copy()
    w[e, :, 0:32:2], w[e, :, 1:32:2] = q["w_out"][e, :, 1:32:2], q["w_out"][e, :, 0:32:2]
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y])
    w = q["w_in"].copy()                               # ... and the first k-step of its up matrix
    w[e, :, 0:32:2], w[e, :, 1:32:2] = q["w_in"][e, :, 1:32:2], q["w_in"][e, :, 0:32:2]
    fails(q, dict(w_in=w), [CHECK_H])


def test_q_mutation_g_last_k_step_dropped_at_one_k_step_per_register_set():
    shape, g, form = R.Q_MASK_EDGES["int4"][0]          # 33 rows, I = 1024: 32 blocks of one k-step
    q = inputs(shape, "int4", g)
    w = q["w_out"].copy()
    w[first_live_expert(q), :, -32:] = 0.0
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y], form="dense")


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_q_mutation_h_neighbour_rstd_in_the_deferred_chain(fmt):
    assert "neighbour_rstd" in D.MOE_MUTATIONS
    _, g, M, _, form, ran, shape = next(c for c in D.MOE_Q_CASES if c[0] == fmt and c[2] == 16)
    q = D.moe_inputs_q(M, fmt, g, shape)
    out = chain_standin(q, ran, form, "neighbour_rstd")
    R.check_wt(out, q)
    with pytest.raises(AssertionError):
        D.check_moe_chain(q, out, QB)
    with pytest.raises(AssertionError):
        R.check_h(q, out, QB, "", chain_gu(q, out))


def test_q_mutation_i_untouched_expert_read_as_0_instead_of_skipped():
    q = q_case("mxfp4", 1)                              # one row, two of eight experts live
    out = R.emulated_device_q(q, "dense_fused", untouched=0.0)
    R.check_experts(q, out, QB)                         # (y cannot tell)
    with pytest.raises(AssertionError, match="picked by no row"):
        R.check_h(q, out, QB)


def test_q_mutation_j_int4_pad_word_applied_to_a_real_row():
    q = q_case("int4", 4)
    m, (E, H, I) = rows2d(q, "w_out")
    e = first_live_expert(q)
    w = q["w_out"].copy()
    w[e, 3] = bf16_rne(nibbles(m["codes"]).reshape(E, H, I)[e, 3])          # {s = 1, z = 0}: W~ = q
    fails(q, dict(w_out=w), [CHECK_DOWN, CHECK_Y])


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_unmutated_q_skews_and_routing_pass(fmt):
    for skew in R.SKEWS:
        q = inputs(None, fmt, 64, False, skew)
        out = R.emulated_device_q(q, "dense")
        assert [tuple(np.flatnonzero(g)) for g in out["gate"]] == [tuple(sorted(p)) for p in q["picks"]]
        R.check_all_q(q, out, QB, skew)
    for M, E, k in R.ROUTING_CASES:
        q = inputs((M, E, k), fmt, 64, False, "routing")
        for form in ("dense_fused", "plan"):
            out = R.emulated_device_q(q, form)
            R.check_routing_exact(q, out)
            R.check_wt(out, q)
            base = R.emulated_device(dict(q, w_in=q["raw_in"], w_out=q["raw_out"]), form)       # the bf16-expert call
            assert np.array_equal(out["router_logits"], base["router_logits"]) and np.array_equal(out["gate"], base["gate"])
