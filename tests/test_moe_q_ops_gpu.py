"""The MoE block with QUANTIZED experts (fp8 e4m3 row scales, MXFP4 e8m0 block scales, INT4 group words) stage by stage,
through nvl_op_moe_stages_q / nvl_op_dense_moe_stages_q (ops.moe_stages / ops.dense_moe_stages with expert_format=...)
against the float64 statement of tests/moe_reference.py — what tests/test_moe_ops_gpu.py does for bf16 experts.

The op builds the experts the way a model gets them: the upload quantizer, then nvl_finalize's own code (one function,
shared), so gather_rows_q's interleave of codes and scales, the three moe_cat_down_w* kernels, the per-expert fp8 scale
rows and the registration for the decode dispatch are the model's.  The reference computes with W~ of the bit-exact numpy
mirrors (ref_w8 / ref_mx / ref_gq), so quantization error is not in any figure here.  Per call:
  form     the literal each case must report, derived from moe_dense_ok and the launchers' conditions (a silent fallback
           to "plan" cannot pass for the decode kernels);
  W~       wt_in / wt_out — the device's codes and scales after finalize, read back through the grouped forms' dequantize
           kernels — equal the mirror bit for bit (check_wt);
  routing  as the bf16 file holds it, and bit-identical to the bf16-expert call on the crafted inputs;
  h        the dense forms' intermediate after the up projection, copied between the two launches: untouched experts still
           hold the NaN pre-fill, live experts are finite and exactly 0 where the gate is 0, each picked (row, expert) within
           MOE_Q_RATIO_BOUND x the emulation's own error (check_h);
  down     y against the down projection of the DEVICE'S OWN h: exact operands, so only fp32 summation error, under a
           worst-case bound (check_down) — a wrong up result cannot mask or be blamed on the down projection;
  y        per row within MOE_Q_RATIO_BOUND x the emulation's error, both references fed the device's gate (check_experts).
No row, expert or case is left out for a near-tie.

What the model-level tests (tiny granite_moe, final logits at 1.5e-2 of the largest) cannot see and these can: an expert's
scale row taken from its neighbour, a group word or block scale shifted across an expert boundary of the concatenated down
matrix, a dropped zero point, a skipped last k-step, the full live-block mask (cases 8, 9 and the 33-row edges), the wide up
form (case 6), E = 5, 6, 40 and I = 32, 96, 160, and the deferred FFN norm on quantized experts (test_moe_chain_q).
tests/test_moe_reference_host.py shows on the CPU that each of those mutations fails the check aimed at it.

MOE_Q_RATIO_BOUND = 1.25 x the largest ratio (h or y) measured on the MI355X over all cases of this file
(profiles/moe_q_op_tests.txt, written by scripts/moe_op_figures.py), never above 2 — the rule of MOE_RATIO_BOUND."""
import functools

import numpy as np
import pytest

import dense_reference as D
import moe_reference as R
from test_dense_ops_gpu import DENSE_RATIO_BOUND
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu

MOE_Q_RATIO_BOUND = 1.341        # 1.25 x the largest measured device / emulation rms ratio, 1.0725 (profiles/moe_q_op_tests.txt: h of mxfp4-6)

DENSE2 = [("dense_fused", {}), ("dense", {31: 0})]
SORTED2 = [("plan", {22: 0}), ("grouped", {22: 0, 8: 0})]
ALL4 = DENSE2 + SORTED2
PREFILL3 = [("grouped", {}), ("grouped", {17: 256}), ("grouped", {16: 0})]


@functools.lru_cache(maxsize=None)
def inputs(shape, fmt, g, crafted=False, kind="random"):
    """the inputs of a case with W~ in w_in / w_out: computed once, shared by the tests that need them, never modified"""
    if kind == "random":
        inp = R.random_inputs(*shape)
    elif kind == "routing":
        inp = R.crafted_routing_inputs(*shape)
    else:
        inp = R.skew_inputs(kind)
    return R.quantized(inp, fmt, g, crafted)


def forms_of(i):
    """cases 1-5 in all four forms; case 6 also with the narrow up form"""
    return ALL4 if i <= 5 else DENSE2 + ([("dense_fused", {2: 1})] if i == 6 else [])


EXPERT_Q_CASES = [(f"{fmt}-{i}-" + "x".join(map(str, shape)), fmt, shape, g, i in R.Q_CRAFTED, forms_of(i))
                  for fmt in R.FORMATS for i, (shape, g) in enumerate(R.Q_CASES, 1)]
EDGE_Q_CASES = [(f"{fmt}-" + "x".join(map(str, shape)) + f"-{form}", fmt, shape, g, False, DENSE2 if form == "dense" else [("plan", {})])
                for fmt in R.FORMATS for shape, g, form in R.Q_MASK_EDGES[fmt]]
PREFILL_Q_CASES = [(f"{fmt}-" + "x".join(map(str, shape)) + "-prefill", fmt, shape, 64, False, PREFILL3)
                   for fmt in R.FORMATS for shape in R.PREFILL_CASES]
ALL_Q_CASES = EXPERT_Q_CASES + EDGE_Q_CASES + PREFILL_Q_CASES


def run(gpu, q, form, keys, fmt=None):
    """one call on the unquantized experts, which the op quantizes itself (fmt "bf16": the bf16-expert call on the same inputs)"""
    with Tuning(gpu, keys):
        out = gpu.ops.moe_stages(q["x"], q["router"], q["raw_in"], q["raw_out"], q["k"], expert_format=fmt or q["fmt"],
                                 group_size=q["g"] if fmt is None else 0)
    assert out["form"] == form, (out["form"], form, keys)
    return out


def expert_outputs(gpu, name, q, forms):
    """every form of a case with all of its checks, then the forms against each other -> [(form, keys, out, ratios)]"""
    outs = []
    for form, keys in forms:
        out = run(gpu, q, form, keys)
        ratio = R.check_all_q(q, out, MOE_Q_RATIO_BOUND, f"{name} {keys}")
        outs.append((form, keys, out, ratio))
    dense = [o for f, _, o, _ in outs if f in R.DENSE_FORMS]
    for o in dense[1:]:        # the two dense routings (and the two up forms) pick the same experts
        assert np.array_equal(o["gate"] != 0, dense[0]["gate"] != 0), name
    prefill = [o for f, keys, o, _ in outs if f == "grouped" and not (22 in keys)]
    for o in prefill[1:]:      # keys 16 / 17: the same rows bit for bit, as for bf16 experts
        assert np.array_equal(o["y"], prefill[0]["y"]), name
    return outs


@pytest.mark.parametrize("name,fmt,shape,g,crafted,forms", ALL_Q_CASES, ids=[c[0] for c in ALL_Q_CASES])
def test_experts_q(gpu, name, fmt, shape, g, crafted, forms):
    expert_outputs(gpu, name, inputs(shape, fmt, g, crafted), forms)


@pytest.mark.parametrize("skew", R.SKEWS)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_skew_q(gpu, fmt, skew):
    q = inputs(None, fmt, 64, False, skew)
    for form, keys, out, _ in expert_outputs(gpu, f"{fmt} {skew}", q, DENSE2):
        assert [tuple(np.flatnonzero(g)) for g in out["gate"]] == [tuple(sorted(p)) for p in q["picks"]]


@pytest.mark.parametrize("M,E,k", R.ROUTING_CASES)
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_routing_untouched_by_the_expert_format(gpu, fmt, M, E, k):
    """the crafted ties in every form: exact, and logits and gate bit-identical to the bf16-expert call on the same inputs"""
    q = inputs((M, E, k), fmt, 64, False, "routing")
    for form, keys in ALL4:
        out, base = run(gpu, q, form, keys), run(gpu, q, form, keys, fmt="bf16")
        R.check_routing_exact(q, out)
        assert np.array_equal(out["router_logits"].view(np.uint32), base["router_logits"].view(np.uint32)), (form, "logits")
        assert np.array_equal(out["gate"].view(np.uint32), base["gate"].view(np.uint32)), (form, "gate")
        assert np.isfinite(out["y"]).all()
        R.check_wt(out, q)


CHAIN_IDS = [f"{fmt}-g{g}-M{M}-{form}-E{s['E']}" for fmt, g, M, _, form, _, s in D.MOE_Q_CASES]


def chain_gu(q, out):
    """[g | u] of the deferred chain: rstd[m] x (the device's operand . W~_in^T) — the scale after the product"""
    rstd = D.rstd_of(out["rs1"], out["op1"].shape[1], q["norm_eps"])
    return lambda e, rows, rounded: (out["op1"].astype(np.float64)[rows] @ q["w_in"][e].astype(np.float64).T) * rstd[rows, None]


@pytest.mark.parametrize("fmt,g,M,keys,form,ran,shape", D.MOE_Q_CASES, ids=CHAIN_IDS)
def test_moe_chain_q(gpu, fmt, g, M, keys, form, ran, shape):
    """O projection as the producer of the FFN norm -> moe(deferred_norm) on quantized experts: the up accumulators take
    rstd[m] after the product, on top of the format's own scales"""
    q = D.moe_inputs_q(M, fmt, g, shape)
    with Tuning(gpu, keys):
        out = gpu.ops.dense_moe_stages(q["x"], q["attn_out"], q["wo"], q["norm_w"], q["router"], q["raw_in"], q["raw_out"],
                                       q["next_norm_w"], q["k"], norm_eps=q["norm_eps"], expert_format=fmt, group_size=g)
    name = f"moe-q {fmt} M={M} {form}"
    print(name, out["form"], out["ran"])
    assert out["form"] == form and out["ran"] == ran, (out["form"], out["ran"], ran)
    R.check_wt(out, q)
    D.check_moe_chain(q, out, DENSE_RATIO_BOUND, name)
    R.check_h(q, out, MOE_Q_RATIO_BOUND, name, chain_gu(q, out))
    R.check_down(q, out, name, base=out["x1"], alpha=float(np.float32(D.alphas(q)[0])))
