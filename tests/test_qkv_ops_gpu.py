"""The front of an attention layer stage by stage through nvl_op_qkv_stages (ops.qkv_stages: the forward pass's own embed()
and qkv_front() — attention norm, QKV projection + bias, RoPE, Q into the operand buffer, K / V into the paged cache — on a
batch as the paged front end lays it out) against the float64 statement of tests/qkv_reference.py.

Every stage is compared with the reference FED THE DEVICE'S OWN OUTPUT of the stage before.  Every case asserts what ran
(out["ran"]: the front form, the GEMM instance launch_gemm_bf16 launched, the norm kernel, the embedding kernel) against
literals worked out by hand in qkv_reference.CASES, so a dispatch change cannot silently uncover a kernel, and the op fills
every buffer with NaN and the pools with per-element sentinels first, so a row nobody wrote, a padded row that was written
and a K / V row that landed anywhere else all show.

Bounds: qkv_reference's docstring — all derived.  Only the operand's rms ratio against bf16(norm(x)) reuses the bound
test_dense_ops_gpu.py holds the same norm kernels to (DENSE_RATIO_BOUND).  tests/test_qkv_reference_host.py shows on the CPU
that each check fails under the mutation it is aimed at.  Figures: profiles/qkv_op_tests.txt (scripts/qkv_op_figures.py).

What the model-level suite (final logits at 1.5e-2 of the maximum, one sequence from position 0 in a slab cache, the
128x128 and the hd-128 4x2 instance only) could not see, and the cases that close each gap:
 1. the EPI_QKV epilogue in the 256x128, 256x256, ping-pong and hd-128 ping-pong kernels   -> epi-tile2 / tile3 / pingpong-*,
    epi-hd128-pingpong-32x8-M2041
 2. several sequences at different non-zero positions through a permuted block table inside one m-tile, a block boundary
    inside a tile, a ragged last tile of 3 rows, a ragged N tile whose last wave sub-tile is a lone V head -> every batch; *-3x1-*
 3. K / V one row off, another sequence's table row, heads swapped, a padded row stored      -> sentinels, exact family, NaN rows of q
 4. a bias shifted by a head, RoPE with the hd-64 partner distance in an hd-128 head          -> *-exact, epi-hd128-*, store-*-hd128-*
 5. rope_kv_kernel<bf16> behind the decode form and behind the 64-row groups, rope_kv_kernel<float>, rope_kv8_kernel
    (the 8-bit cache's only writer), a decode step that must leave the pools alone             -> store-*, f32-*, kv8-*, decode-step
 6. the embedding gather: first and last token id, a position at and past the learned table's end, multiplier 0 / 12 -> embed-*"""
import pytest

import qkv_reference as R
from test_dense_ops_gpu import DENSE_RATIO_BOUND
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu


def run(gpu, name):
    inp = R.make_inputs(name)
    with Tuning(gpu, R.CASES[name]["keys"]):
        out = gpu.ops.qkv_stages(**R.op_kwargs(inp))
    return inp, out


@pytest.mark.parametrize("name", list(R.CASES))
def test_qkv_stages(gpu, name):
    inp, out = run(gpu, name)
    print(name, out["ran"])
    assert out["ran"] == R.CASES[name]["ran"], (name, out["ran"], R.CASES[name]["ran"])
    fig = R.check(inp, out, DENSE_RATIO_BOUND, name)
    print(name, " ".join(f"{k}={v:.3g}" for k, v in fig.items()))


def test_tuning_keys_are_restored(gpu):
    """the cases force keys 0 and 18; afterwards both hold their defaults (nvl_set_tuning returns the old value)"""
    L = gpu.lib()
    for key, default in ((0, 0), (18, 256)):
        old = L.nvl_set_tuning(key, default)
        assert old == default, (key, old)
