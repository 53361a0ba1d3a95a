"""More than 64 experts, without a GPU: the expert-count rule — 1..64, or 80..256 in multiples of 16 with
at most 8 experts per token — is checked by nvl_create and by the MoE ops before the device probe, and the crafted inputs of
tests/test_moe_wide_gpu.py pass their own checks on the float64 reference."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import moe_reference as R
from test_moe_ops_gpu import MOE_RATIO_BOUND

# the tied pair of a crafted row, (lower, higher) expert: two slots of one lane (e, e + 64), a higher slot in a LOWER lane
# (the tie goes by expert index, not by lane), and both sides of a 16-expert tile edge
TIE_PAIRS = [(5, 66), (15, 16), (3, 67), (63, 64), (79, 130), (127, 128), (70, 129)]


def wide_routing_inputs(M, E, k, H=64, I=64):
    """moe_reference.crafted_routing_inputs for 64 < E <= 256 (that one draws its distinct logits from 65 values): x rows
    one-hot, router entries multiples of 1/8 in [-16, 16] — 257 values, exact in bf16 —, row r of kind ROW_KINDS[r % 4] with
    the tie of a boundary_tie / inner_tie row on the next pair of TIE_PAIRS"""
    assert M <= H and 64 < E <= 256
    inp = R.random_inputs(M, E, k, H, I)
    r = np.random.default_rng(7 * M + E)
    router = (r.integers(0, 257, (H, E)) - 128) / 8.0
    pairs = [p for p in TIE_PAIRS if p[1] < E]
    for row in range(M):
        vals = np.sort((r.permutation(257)[:E] - 128) / 8.0)[::-1]          # E distinct logits, descending
        kind = R.ROW_KINDS[row % 4]
        ranks = (k - 1, k) if kind == "boundary_tie" else (0, 1) if kind == "inner_tie" and k >= 2 else None
        v, order = np.empty(E), r.permutation(E)
        if ranks:
            a, b = pairs[(row // 4) % len(pairs)]
            v[[e for e in order if e not in (a, b)]] = np.delete(vals, ranks)
            v[a] = v[b] = vals[ranks[0]]
        else:
            v[order] = vals
        if kind == "all_equal":
            v[:] = vals[0]
        router[row] = v
    x = np.zeros((M, H), np.float32)
    x[np.arange(M), np.arange(M)] = 1.0
    inp.update(x=x, router=router.astype(np.float32))
    return inp


@pytest.mark.parametrize("E,k,code", [(72, 2, -1), (257, 2, -1), (272, 2, -1), (128, 9, -1), (128, 8, -8), (256, 1, -8)])
def test_expert_count_rule_before_the_device_probe(pkg, E, k, code):
    """NVL_ERR_INVALID (-1) outside the rule; inside it the call gets as far as the device probe — NVL_ERR_NO_DEVICE (-8)
    for a device that does not exist"""
    L, z = pkg._lib, lambda *s: np.zeros(s, np.float32)
    with pytest.raises(pkg.NvlError) as e:
        pkg.ops.moe_stages(z(2, 64), z(64, E), z(E, 128, 64), z(E, 64, 64), k, device=1 << 20)
    assert e.value.code == code
    cfgc = import_module("nano-vllm-go_amd.model")._cfg_struct(pkg.synth.tiny_config("granite_moe", num_experts=E, num_experts_per_tok=k))
    opts, h = L.RuntimeOptsC(device=1 << 20, precision=L.PRECISION["bf16"], tp_size=1, max_seqs=1), C.c_void_p()
    assert L.lib().nvl_create(C.byref(cfgc), C.byref(opts), C.byref(h)) == code and not h.value


@pytest.mark.parametrize("E", [128, 256])
def test_crafted_inputs_pass_on_the_reference(E):
    inp = wide_routing_inputs(17, E, 8)
    out = R.emulated_device(inp, "plan")
    R.check_routing_exact(inp, out)
    for a, b in TIE_PAIRS[:5 if E == 256 else 4]:           # rows 0, 4, .. (boundary ties): the lower expert of the pair is in, the higher out
        row = 4 * TIE_PAIRS.index((a, b))
        assert out["gate"][row, a] > 0 and out["gate"][row, b] == 0 and inp["router"][row, a] == inp["router"][row, b]
    rnd = R.random_inputs(17, E, 8, 64, 64)
    out = R.emulated_device(rnd, "plan")
    R.check_routing_random(rnd, out)
    R.check_experts(rnd, out, MOE_RATIO_BOUND)
