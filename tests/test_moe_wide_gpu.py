"""More than 64 experts through ops.moe_stages: elem.h moe_route_row_wide in the two-launch decode route (router GEMM + moe_plan_wide_kernel,
"plan"; the default, key 31 = 0 or 1), the one-launch route behind tuning key 31 = 2 (gemm.h moe_router_plan_kernel,
"plan") and the prefill route (moe_route_wide / hist / scan / scatter kernels, "grouped"), against tests/moe_reference.py.
E = 80: two experts per lane with a partly filled second slot; 128: both slots full; 256: four per lane.  M = 1, 17 (a second,
ragged row tile), 64 (the PLAN limit), 80 (past it).  Bounds: test_moe_ops_gpu.py's, unchanged."""
import numpy as np
import pytest

import moe_reference as R
from test_moe_ops_gpu import MOE_RATIO_BOUND, run
from test_moe_wide_host import wide_routing_inputs

pytestmark = pytest.mark.gpu

CASES = [(M, E, k, 64) for E in (80, 128, 256) for k in (1, 8) for M in (1, 17, 64)] + [(80, 128, 8, 128)]


@pytest.mark.parametrize("M,E,k,H", CASES)
def test_wide_routing_and_experts(gpu, M, E, k, H):
    form = "plan" if M <= 64 else "grouped"
    crafted, rnd = wide_routing_inputs(M, E, k, H), R.random_inputs(M, E, k, H, 64)
    outs = []
    for key31 in (2, 0):
        out = run(gpu, crafted, form, {31: key31})
        R.check_routing_exact(crafted, out)              # every row: the crafted logits are exact in bf16
        assert np.isfinite(out["y"]).all()
        outs.append(out)
        out = run(gpu, rnd, form, {31: key31})
        R.check_routing_random(rnd, out)
        R.check_experts(rnd, out, MOE_RATIO_BOUND, f"{M}x{E}x{k} key31={key31}")
    for name in ("router_logits", "gate", "y"):           # one launch and two: the same ids, weights and rows, bit for bit
        assert np.array_equal(outs[0][name], outs[1][name]), name
    if M <= 64:                                           # and the prefill kernels route the same way
        out = run(gpu, crafted, "grouped", {8: 0})
        R.check_routing_exact(crafted, out)
        assert np.array_equal(out["gate"], outs[0]["gate"])
