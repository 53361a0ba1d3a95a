"""The MoE block stage by stage through nvl_op_moe_stages (ops.moe_stages: moe() set up as a layer of the model has it, so
rows <= 64 take the decode "dense-masked" form) against the float64 statement of tests/moe_reference.py.

Every stage is compared with the reference FED THE DEVICE'S OWN OUTPUT of the stage before: the routing reference runs on
the device's router logits, the expert references on the device's gate matrix.  No row is ever left out for a near-tie.
Every test asserts the form that ran (out["form"]), so a fallback cannot pass for the form under test, and the op fills
every scratch buffer with NaN first, so y is finite only if nothing unwritten was read.

Bounds.  Router logits: bit-exact on the crafted inputs (one-hot x, router entries multiples of 1/8: a logit is one router
entry in every path), 2e-5 of the largest logit on random inputs (test_ops_gpu.py's F32_TOL).  Routing weights and row
sums: 1e-5 of the row maximum (the bound test_softmax holds the fp32 softmax to); selection: exact on the crafted inputs,
chosen >= unchosen - 1e-5 max|logit| on random ones.  Experts: per row m, rms(y_dev[m] - y_f64[m]) <= MOE_RATIO_BOUND x
rms(y_emulated[m] - y_f64[m]), the emulation (moe_reference.experts_emulated) being float64 with a bf16 rounding at each of
the kernels' operand points.  MOE_RATIO_BOUND = 1.25 x the largest ratio measured on the MI355X over all cases of this
file (profiles/moe_op_tests.txt, written by scripts/moe_op_figures.py), and never above 2 — the rule of
test_mamba_ops_gpu.py's SSD bound.  tests/test_moe_reference_host.py shows on the CPU that each bound fails under the
mutation it is aimed at.

The gaps of the model-level suite (the tiny granite_moe model and one Granite-1B-shaped comparison, both on final logits
at a whole-tensor tolerance; test_ops_gpu.py::test_moe never reaches the dense form and drops unclear rows) and the test
here that closes each:
 1. a token losing one of its experts, an unrenormalised gate          -> test_routing_*, test_experts (per-row ratio)
 2. a tie broken the wrong way                                          -> test_routing_exact (crafted ties, all forms)
 3. a last k-step / a block of the down projection dropped              -> test_experts cases 2, 5, 8, 9, 10
 4. E = 5, 6, 40, 64: slice and wave layouts of the down projection     -> test_experts cases 2, 3, 4, 5
 5. I = 32, 96: an expert shorter than a block, a ragged tail           -> test_experts cases 2, 3
 6. the 32-block edge of the live mask and moe_dense_ok's division      -> test_experts cases 8, 9, 10 and the refused ones
 7. the M = 16/17 and 32/33 switches of MT and U                        -> test_experts cases 3, 4, 8, 9
 8. an expert picked only by the last row; untouched experts            -> test_skew
 9. the two dense routings against each other                           -> test_experts (cross-form gate pattern)
What test_experts case 2 found: E = 5 gives one K slice, for which the down kernel adds into x itself and writes no
partial, while moe() still announced one pending slice — the next norm added the unwritten moe_part rows (NaN here, a
stale layer's partials in a model).  moe() now leaves nothing pending for one slice.

Quantized experts (fp8, MXFP4, INT4) have this file's cases and checks, plus W~ and h, in tests/test_moe_q_ops_gpu.py; the
deferred_norm input path (it needs the preceding O projection) is test_dense_ops_gpu.py::test_moe_chain.  Out of scope: the
key-33 deferred-norm producer form of the down projection (off by default).  The sorted forms' cases with I % 64 == 32 (I = 96, 32, 160 — widths nvl_create refuses,
their grouped GEMMs stream K in 64-wide tiles) run on experts zero-padded by 32 columns inside the op."""
import numpy as np
import pytest

import moe_reference as R

pytestmark = pytest.mark.gpu

MOE_RATIO_BOUND = 1.254          # 1.25 x the largest measured device / emulation rms ratio, 1.0033 (profiles/moe_op_tests.txt)

DENSE2 = [("dense_fused", {}), ("dense", {31: 0})]
SORTED2 = [("plan", {22: 0}), ("grouped", {22: 0, 8: 0})]
ALL4 = DENSE2 + SORTED2


def _case(shape, forms, tag=""):
    return ("x".join(map(str, shape)) + tag, lambda: R.random_inputs(*shape), forms)


EXPERT_CASES = (
    [_case(c, ALL4 if i < 5 else DENSE2 + ([("dense_fused", {2: 1})] if i == 5 else [])) for i, c in enumerate(R.DENSE_CASES)]
    + [_case(c, [("plan", {})], "-refused") for c in R.REFUSED_CASES]
    + [_case(c, [("grouped", {}), ("grouped", {17: 256}), ("grouped", {16: 0})], "-prefill") for c in R.PREFILL_CASES])


class Tuning:
    """nvl_set_tuning keys for a block, restored afterwards"""
    def __init__(self, gpu, keys):
        self.lib, self.keys, self.old = gpu.lib(), keys, {}

    def __enter__(self):
        for key, value in self.keys.items():
            self.old[key] = self.lib.nvl_set_tuning(key, value)

    def __exit__(self, *exc):
        for key, value in self.old.items():
            self.lib.nvl_set_tuning(key, value)


def run(gpu, inp, form, keys):
    with Tuning(gpu, keys):
        out = gpu.ops.moe_stages(inp["x"], inp["router"], inp["w_in"], inp["w_out"], inp["k"])
    assert out["form"] == form, (out["form"], form, keys)
    return out


@pytest.mark.parametrize("M,E,k", R.ROUTING_CASES)
def test_routing_exact(gpu, M, E, k):
    inp = R.crafted_routing_inputs(M, E, k)
    for form, keys in ALL4:
        out = run(gpu, inp, form, keys)
        R.check_routing_exact(inp, out)
        assert np.isfinite(out["y"]).all()


@pytest.mark.parametrize("M,E,k", R.ROUTING_CASES)
def test_routing_random(gpu, M, E, k):
    inp = R.random_inputs(M, E, k, 64, 64)
    for form, keys in ALL4:
        R.check_routing_random(inp, run(gpu, inp, form, keys))


def expert_outputs(gpu, name, inp, forms):
    """every form of a case, checked at the routing stage and across forms -> [(form, keys, out)]"""
    outs = []
    for form, keys in forms:
        out = run(gpu, inp, form, keys)
        R.check_routing_random(inp, out)
        outs.append((form, keys, out))
    dense = [o for f, _, o in outs if f in R.DENSE_FORMS]
    for o in dense[1:]:        # the two dense routings (and the two up forms) pick the same experts
        assert np.array_equal(o["gate"] != 0, dense[0]["gate"] != 0), name
    prefill = [o for f, keys, o in outs if f == "grouped" and not (22 in keys)]
    for o in prefill[1:]:      # keys 16 / 17: the same rows bit for bit, as test_ops_gpu.py::test_moe holds them
        assert np.array_equal(o["y"], prefill[0]["y"]), name
    return outs


@pytest.mark.parametrize("name,inp,forms", EXPERT_CASES, ids=[c[0] for c in EXPERT_CASES])
def test_experts(gpu, name, inp, forms):
    inp = inp()
    for form, keys, out in expert_outputs(gpu, name, inp, forms):
        R.check_experts(inp, out, MOE_RATIO_BOUND, f"{name} {keys}")


@pytest.mark.parametrize("skew", R.SKEWS)
def test_skew(gpu, skew):
    inp = R.skew_inputs(skew)
    for form, keys, out in expert_outputs(gpu, skew, inp, DENSE2):
        assert [tuple(np.flatnonzero(g)) for g in out["gate"]] == [tuple(sorted(p)) for p in inp["picks"]]
        R.check_experts(inp, out, MOE_RATIO_BOUND, f"{skew} {keys}")
