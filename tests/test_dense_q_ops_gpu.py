"""The dense layer tail with QUANTIZED weights (fp8 e4m3 row scales, MXFP4 e8m0 block scales, INT4 group words at g = 32,
64, 128) stage by stage, through nvl_op_dense_stages with the longer struct (ops.dense_stages(..., weight_format=...))
against the float64 statement of tests/dense_reference.py — what tests/test_dense_ops_gpu.py does for bf16 weights.

The op builds the layer the way a model gets it: wo, w1, w2 (and wn where a model quantizes it: the next layer's QKV, the
fp8 LM head) through the upload quantizer, then nvl_finalize's own fuse_w1 (the SwiGLU interleave of codes AND scales) and
its registration for gemm()'s dispatch, so the same layer_tail() runs on the WF_FP8 / WF_MXFP4 / WF_INT4 instances of the
decode kernels — deferred-RMSNorm producers (EPI_RESID with rs_out: half tiles, m_split, 64-row groups) and consumers (rs_in
on the narrow and the wide kernels), split-K slices, SwiGLU / GELU epilogues with their biases — and, above the decode
forms, on dequantize + the tile kernel.  The reference computes with W~ of the bit-exact numpy mirrors (ref_w8 / ref_mx /
ref_gq), so quantization error is in no figure.  Per case x family x format:
  ran    equals the literal of the bf16 case of the same shape and keys (gemm.h: every weight format takes the same
         decisions); the shapes the bf16 file does not have (ragged-*: K = 768, wide-F8192-*) carry literals worked out by
         hand in dense_reference.CASES_Q.  A quantized call that reports another form, or throws "a deferred-RMSNorm
         projection did not fit the decode kernels", fails here;
  W~     wt_o / wt_1 / wt_2 / wt_n — the device's codes and scales after finalize, read back through the tile path's
         dequantize kernel, W1 de-interleaved — equal the mirror bit for bit (check_wt names the first (matrix, row, k));
  stages dense_reference.check_stages with every derived bound unchanged: xn_raw bit for bit, the x^2 partials to
         (n + 1) 2^-24, rstd to 1e-6, the exact family's x1 / xn_raw / partials with np.array_equal, yn to F32_TOL, NaN
         pre-fill everywhere.  x2 is held to the exact family's fp32 dot product bound in BOTH families here: the device's
         own h and W~2 are both exact in bf16, so the emulation equals float64 and a ratio is undefined; for the same reason
         yn has no ratio behind a quantized wn (F32_TOL holds it).
  ratio  random family, per row and stage (x1, a normed operand, h, yn behind a bf16 wn): rms(dev - f64) <=
         DENSE_Q_RATIO_BOUND x rms(emulated - f64).
The exact families: {-1, 0, 1} weights survive fp8 and MXFP4 unchanged; INT4 takes integers (q - z) with q = 0 and q = 15 in
every group (dense_reference.exact_inputs_q), W~ == w asserted per matrix.

What the model-level tests (2-layer toys of H = 256 / 192 / 128, at most 4 decode rows, final logits at 1.5e-2) and
ops.matmul_*w (EPI_STORE only) cannot see and these can: a scale row of W1 that did not follow the interleave, a group word
or block scale fetched one group early by a wave whose K range starts inside a group (ragged-*), a dropped zero point, a K
slice one k-step short, rstd folded into the scale instead of the accumulator, the second 64-row group on another block's
scales, and every M = 16/17, 32/33, 64/65, 128/129 switch on the quantized instances.
tests/test_dense_reference_host.py shows on the CPU that each of those mutations fails the check aimed at it.

DENSE_Q_RATIO_BOUND = 1.25 x the largest ratio measured on the MI355X over all cases of this file
(profiles/dense_q_op_tests.txt, written by scripts/dense_op_figures.py q), never above 2 — the rule of DENSE_RATIO_BOUND.

What was found: nothing to fix.  All 398 (case, family, format) calls reported the bf16 literal of their shape, none threw,
W~ equalled the mirror everywhere, every derived bound held, and the ratios lie between 1.0000 and 1.0007 (W~ is exact in
bf16, so what is left beside the shared roundings is fp32 summation order)."""
import functools

import numpy as np
import pytest

import dense_reference as R
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu

DENSE_Q_RATIO_BOUND = 1.251      # 1.25 x the largest measured device / emulation rms ratio, 1.0007 (profiles/dense_q_op_tests.txt: x1 of gpt2-M17, fp8)


@functools.lru_cache(maxsize=4)
def inputs(name, fam, fmt, g):
    return R.quantized_inputs(name, fam, fmt, g)


def run(gpu, name, fam, fmt, g):
    inp = inputs(name, fam, fmt, g)
    pos, kw = R.op_args_q(inp)
    with Tuning(gpu, R.CASES_Q[name]["keys"]):
        out = gpu.ops.dense_stages(*pos, **kw)
    return inp, out


@pytest.mark.parametrize("name,fam,fmt,g", R.Q_PARAMS, ids=[f"{n}-{f}-{fmt}" + (f"-g{g}" if g else "") for n, f, fmt, g in R.Q_PARAMS])
def test_dense_stages_q(gpu, name, fam, fmt, g):
    inp, out = run(gpu, name, fam, fmt, g)
    print(name, fam, fmt, g, out["ran"])
    assert out["ran"] == R.CASES_Q[name]["ran"], (name, fmt, g, out["ran"], R.CASES_Q[name]["ran"])
    R.check_wt(out, inp)
    R.check_stages(inp, out, DENSE_Q_RATIO_BOUND, f"{name} {fam} {fmt} g{g}")


@pytest.mark.parametrize("fmt,g", R.Q_FORMATS)
def test_last_rows_form_completes_only_the_rows_it_reads_q(gpu, fmt, g):
    """llama-last-rows on quantized weights: the rows_idx norm adds the two pending FFN-down slices of the quantized
    projection into the three rows it normalises and into no other"""
    inp, out = run(gpu, "llama-last-rows", "exact", fmt, g)
    rows = np.asarray(inp["last_rows"])
    rest = np.setdiff1d(np.arange(inp["x"].shape[0]), rows)
    assert out["yn"].shape == (3, 1003) and out["op2"].shape == (3, 256)
    assert np.array_equal(out["x_end"][rows], out["x2"][rows])
    assert np.array_equal(out["x_end"][rest], out["x1"][rest])
    assert not np.array_equal(out["x2"][rest], out["x1"][rest])
