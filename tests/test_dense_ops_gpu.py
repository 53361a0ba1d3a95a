"""The dense layer tail stage by stage through nvl_op_dense_stages (ops.dense_stages: layer_tail() — the code forward()
runs from the O projection to the end of a layer — under tail_plan()'s own decisions, on workspaces sized as nvl_create
sizes them) against the float64 statement of tests/dense_reference.py.

Every stage is compared with the reference FED THE DEVICE'S OWN OUTPUT of the stage before, so no error is charged twice
and no row is left out.  Every case asserts what ran (out["ran"]: producer or not, half tiles, the launch form, the slices
left pending, the norm launches, the norm kernel that consumed a pending add, the partials per row) against literals
worked out by hand in dense_reference.CASES, so a fallback cannot pass for the form under test, and the op fills every
scratch buffer and output with NaN first, so a stage is finite only if nothing unwritten was read.

Bounds: dense_reference's docstring.  Derived: xn_raw bit for bit, each x^2 partial to (n + 1) 2^-24, rstd to 1e-6, the
exact family's x1 / xn_raw / partials with np.array_equal, its x2 to the fp32 dot product bound, its h to half a bf16 ulp
plus 4 x the error of a float32 evaluation, yn to test_ops_gpu.py's F32_TOL of the float64 product of its own operands.
Measured: per row and stage rms(dev - f64) <= DENSE_RATIO_BOUND x rms(emulated - f64), DENSE_RATIO_BOUND = 1.25 x the
largest ratio measured on the MI355X over all cases of this file (profiles/dense_op_tests.txt, written by
scripts/dense_op_figures.py), never above 2.  tests/test_dense_reference_host.py shows on the CPU that each check fails
under the mutation it is aimed at.

The gaps of the model-level suite (final logits at 2e-2 of the maximum; test_depth_parity_gpu.py at M = 1 and 24 of one
width, its emulator rounding bf16(x w / rms), not the deferred path's bf16(x w); test_ops_gpu.py::test_ffn / test_matmul*
never reaching a producer, a consumer, a slice or a pending add) and the case here that closes each:
 1. a lost x^2 tile (0.4 % of rstd at H = 2048), a tile read at the wrong stride   -> partial / rstd checks of every deferred case
 2. the second 64-row group reading the first group's rstd                         -> llama-M65 / M100 / M128 (and -serial), h
 3. a bias added once per slice; a slice nobody wrote                              -> gpt2-*, *-key1=*, tile-* (x1, x2; NaN fill)
 4. a row >= M of a padded tile leaking into row M - 1; rows swapped across tiles   -> exact family at M = 5, 17, 33, 100, 130
 5. alpha on the wrong term, alpha skipped on a pending add                         -> *-alpha0.22*, *-alpha0.5*, falcon-*-mults
 6. the M = 16 / 17, 32 / 33, 64 / 65, 128 / 129 switches of half tiles, MT, U, groups -> llama-M*
 7. defer_half's answer at H / 16 = 256                                             -> wide-H4096-M8
 8. the last layer's two forms (final norm carried; rows_idx + pending slices)      -> llama-last-*
 9. the parallel block's order and its one pending projection                       -> falcon-*
10. the tile kernel's split-K and both norm kernels that sum it                     -> tile-M130, tile-M520 (and tile-M520-fused;
    with the split off 130 rows take the decode kernel's 64-row groups: groups-M130-key26=0)
11. the MoE consumers of the deferred operand: the routing kernel's own loop over the partials, the router GEMM, the
    expert up projection (set_deferred_in), four slices pending in moe_part          -> test_moe_chain (ops.dense_moe_stages)
What the key 3 = 2 / 3 cases found: the producer of those forms has no m_split and so never runs on half tiles — it writes
H / 16 partials per row — while every consumer asked defer_half(), which at <= 16 rows answered "H / 8 per row": rows 1..15
summed their neighbours' partials (row 0 got its own 16 and row 1's).  defer_half() now answers no under those keys.
"""
import numpy as np
import pytest

import dense_reference as R
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu

DENSE_RATIO_BOUND = 1.266        # 1.25 x the largest measured device / emulation rms ratio, 1.0125 (profiles/dense_op_tests.txt: h of tile-M520)

PARAMS = [(name, fam) for name, c in R.CASES.items() for fam in c["families"]]


def run(gpu, name, fam):
    inp = R.make_inputs(name, fam)
    pos, kw = R.op_args(inp)
    with Tuning(gpu, R.CASES[name]["keys"]):
        out = gpu.ops.dense_stages(*pos, **kw)
    return inp, out


@pytest.mark.parametrize("name,fam", PARAMS, ids=[f"{n}-{f}" for n, f in PARAMS])
def test_dense_stages(gpu, name, fam):
    inp, out = run(gpu, name, fam)
    print(name, fam, out["ran"])
    assert out["ran"] == R.CASES[name]["ran"], (name, out["ran"], R.CASES[name]["ran"])
    R.check_stages(inp, out, DENSE_RATIO_BOUND, f"{name} {fam}")


def test_last_rows_form_completes_only_the_rows_it_reads(gpu):
    """llama-last-rows: the rows_idx form of norm_row_kernel adds the two pending FFN-down slices into the three rows it
    normalises and into no other: there x still lacks the FFN-down product (x_end = x1), and yn has three rows."""
    inp, out = run(gpu, "llama-last-rows", "exact")
    rows = np.asarray(inp["last_rows"])
    rest = np.setdiff1d(np.arange(inp["x"].shape[0]), rows)
    assert out["yn"].shape == (3, 1003) and out["op2"].shape == (3, 256)
    assert np.array_equal(out["x_end"][rows], out["x2"][rows])
    assert np.array_equal(out["x_end"][rest], out["x1"][rest])
    assert not np.array_equal(out["x2"][rest], out["x1"][rest])


MOE_PARAMS = [(M, keys, form) for M, keys, form, _ in R.MOE_CASES]


@pytest.mark.parametrize("M,keys,form", MOE_PARAMS, ids=[f"M{M}-{form}" for M, _, form in MOE_PARAMS])
def test_moe_chain(gpu, M, keys, form):
    """O projection as the producer of the FFN norm -> moe(deferred_norm): the routing kernel's own loop over the partials
    (key 31 = 1) and the router GEMM's deferred_rstd (key 31 = 0), set_deferred_in on the expert up projection, the down
    projection's four slices pending in moe_part."""
    ran = next(c[3] for c in R.MOE_CASES if c[0] == M and c[2] == form)
    inp = R.moe_inputs(M)
    with Tuning(gpu, keys):
        out = gpu.ops.dense_moe_stages(inp["x"], inp["attn_out"], inp["wo"], inp["norm_w"], inp["router"], inp["w_in"], inp["w_out"],
                                       inp["next_norm_w"], inp["k"], norm_eps=inp["norm_eps"])
    print(M, keys, out["form"], out["ran"])
    assert out["form"] == form and out["ran"] == ran, (out["form"], out["ran"], ran)
    R.check_moe_chain(inp, out, DENSE_RATIO_BOUND, f"moe M={M} {form}")
