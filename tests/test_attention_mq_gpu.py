"""The multi-position decode attention of a verify pass (attn.h attn_decode_mq_bf16_kernel, through nvl_op_attention_mq):
S = 2..8 new positions per sequence on the decode kernel's 16-row MFMA query tile, row = (position, head-in-group).

* against oracle.gqa_core at the bf16 attention tolerance of tests/test_ops_gpu.py;
* a visibility census with teeth at weight 1/T: q = 0 gives every visible key the unnormalised weight exp(0) = 1 exactly,
  V marks one key per output dimension, so out[h][j][d] is exactly 0 when that key lies beyond the row's causal limit
  and 1 / (P + j + 1) otherwise — the sum and the division run in fp32, the only rounding is the bf16 store (2^-9)."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

BF16_TOL = 2e-2        # tests/test_ops_gpu.py

#         nH nKV S  T     hd
SHAPES = [(8, 2, 4, 66, 64),      # P = 62: the new keys straddle the first tile boundary (rows of one tile see 1 or 2 tiles)
          (8, 2, 4, 4, 64),       # no cache
          (8, 2, 2, 66, 64),      # half-empty tile
          (8, 2, 8, 71, 64),      # two query tiles
          (4, 4, 5, 69, 64),      # MHA
          (10, 2, 3, 130, 64),    # group 5: tiles straddle positions
          (71, 1, 2, 130, 64),    # MQA
          (8, 2, 4, 68, 128),     # hd 128
          (8, 2, 4, 2104, 64),    # several rounds per wave
          (4, 1, 3, 700, 128)]    # long context, hd 128
CASES = [(s, 0) for s in SHAPES] + [(s, nw) for s in SHAPES if s[3] in (66, 2104) for nw in (2, 4, 8)]

_REF = {}


def inputs(oracle, shape):
    """q, k, v and the oracle's output of a shape: computed once, shared, read-only"""
    if shape not in _REF:
        nH, nKV, S, T, hd = shape
        r = np.random.default_rng(list(shape))
        q = r.standard_normal((nH, S, hd), dtype=np.float32)
        k = r.standard_normal((nKV, T, hd), dtype=np.float32)
        v = r.standard_normal((nKV, T, hd), dtype=np.float32)
        want = oracle.gqa_core(q, k, v)
        for a in (q, k, v, want):
            a.setflags(write=False)
        _REF[shape] = (q, k, v, want)
    return _REF[shape]


@pytest.mark.parametrize("shape,nw", CASES)
def test_mq_against_oracle(gpu, oracle, shape, nw, request):
    q, k, v, want = inputs(oracle, shape)
    old = gpu.lib().nvl_set_tuning(15, nw)
    request.addfinalizer(lambda: gpu.lib().nvl_set_tuning(15, old))
    got = gpu.ops.attention_mq(q, k, v)
    err = rel_err(got, want)
    print(f"{shape} waves {nw or 'auto'}: rel err {err:.3e} (bound {BF16_TOL:.0e})")
    assert np.isfinite(got).all()
    assert err <= BF16_TOL


def test_mq_refusals(gpu):
    z = np.zeros((8, 1, 64), np.float32)
    kv = np.zeros((2, 16, 64), np.float32)
    with pytest.raises(gpu.NvlError):
        gpu.ops.attention_mq(z, kv, kv)                                   # S = 1
    with pytest.raises(gpu.NvlError):
        gpu.ops.attention_mq(np.zeros((8, 9, 64), np.float32), kv, kv)    # S = 9


def marked_keys(P, S, hd):
    """up to hd distinct keys < T: the tile edges, the last cached key, every new key, then an even spread"""
    T = P + S
    keys = [x for x in (0, 15, 16, 63, 64, P - 1) if 0 <= x < T] + list(range(P, T))
    keys = list(dict.fromkeys(keys))
    for x in np.linspace(0, T - 1, hd).astype(int).tolist():
        if len(keys) >= hd:
            break
        if x not in keys:
            keys.append(x)
    return keys


@pytest.mark.parametrize("P", [0, 61, 62, 63, 64, 200])
@pytest.mark.parametrize("nH,nKV,S,hd", [(8, 2, 4, 64), (8, 2, 4, 128), (10, 2, 3, 64)])
def test_mq_visibility_census(gpu, P, nH, nKV, S, hd):
    T = P + S
    keys = marked_keys(P, S, hd)
    key_d = np.asarray([keys[d % len(keys)] for d in range(hd)])
    for must in [x for x in (0, 15, 16, 63, 64, P - 1) if 0 <= x < T] + list(range(P, T)):
        assert must in key_d
    q = np.zeros((nH, S, hd), np.float32)
    k = np.random.default_rng(P).standard_normal((nKV, T, hd), dtype=np.float32)      # q = 0: K must not matter
    v = np.zeros((nKV, T, hd), np.float32)
    v[:, key_d, np.arange(hd)] = 1.0
    got = gpu.ops.attention_mq(q, k, v)
    worst = 0.0
    for j in range(S):
        visible = key_d <= P + j
        row = got[:, j, :]
        assert (row[:, ~visible] == 0.0).all(), (P, j, "a key beyond the causal limit was counted")
        want = 1.0 / (P + j + 1)
        if visible.any():
            worst = max(worst, float(np.abs(row[:, visible] / want - 1.0).max()))
    print(f"P {P} group {nH // nKV} S {S} hd {hd}: worst relative deviation from 1/(P+j+1): {worst:.3e} (bound 2^-8)")
    assert worst <= 2.0 ** -8
