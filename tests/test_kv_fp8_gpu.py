"""8-bit (OCP e4m3fn) KV cache on the device: the shared quantizer and read path against a numpy
restatement of the contract, exhaustively, and the 8-bit attention kernels (nvl_op_attention_kv8: prefill, decode, the
key-split decode) against attention over the numpy-dequantized cache."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

BF16_TOL = 2e-2        # the bf16 nvl_op_attention tolerance (test_ops_gpu.py): Q, P and V operands in bf16, fp32 accumulate


def _e4m3fn_values():
    """value of every code (NaN for 0x7f / 0xff): 1 sign, 4 exponent (bias 7), 3 mantissa bits, no infinities."""
    v = np.empty(256, np.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        mag = m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        v[c] = np.nan if (c & 0x7F) == 0x7F else (-mag if s else mag)
    return v


VALUES = _e4m3fn_values()
GRID = VALUES[:0x7F]                  # codes 0..126: the non-negative finite values, increasing


def ref_quant(x, s):
    """code = e4m3fn(x / s) in fp32: saturate finite (and infinite) values to +-448, round to nearest, ties to the even
    code, NaN -> NaN code."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.float32(x) / np.float32(s)
    y = np.where(y > 448, np.float32(448), np.where(y < -448, np.float32(-448), y)).astype(np.float32)
    a = np.abs(y.astype(np.float64))
    hi = np.clip(np.searchsorted(GRID, a, side="left"), 0, 126)
    lo = np.clip(hi - 1, 0, 126)
    dlo, dhi = a - GRID[lo], GRID[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a <= GRID[0], 0, code)
    code = code | np.where(np.signbit(y), 0x80, 0)
    return np.where(np.isnan(y), 0x7F | np.where(np.signbit(y), 0x80, 0), code).astype(np.uint8)


def dequant(codes, s):
    return (VALUES[codes].astype(np.float32) * np.float32(s)).astype(np.float32)


def crafted_inputs():
    """all 65 536 bf16 bit patterns, the e4m3 midpoints and their fp32 neighbours, subnormals, the +-448 boundary."""
    bf = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    mids = ((GRID[:-1] + GRID[1:]) / 2).astype(np.float32)
    near = [mids, np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
            GRID.astype(np.float32), np.float32([448, 464, 480, 481, 2 ** -9, 2 ** -10, 3 * 2 ** -11, 1e-30, 1e30])]
    x = np.concatenate(near)
    x = np.concatenate([x, -x])
    return bf, x


@pytest.mark.parametrize("scale", [1.0, 0.37, 2.0 ** -6])
def test_quantizer_contract_exhaustive(gpu, scale):
    bf, crafted = crafted_inputs()
    s = np.float32(scale)
    for x in (bf, crafted, crafted * s):          # crafted * s: the crafted points land on x / s (up to fp32 rounding)
        x = x.astype(np.float32)
        codes, back = gpu.ops.fp8_kv_roundtrip(x, float(s))
        want = ref_quant(x, s)
        nan_in = np.isnan(x)
        assert np.all((codes[nan_in] & 0x7F) == 0x7F), "NaN must give a NaN code"
        bad = np.flatnonzero((codes != want) & ~nan_in)
        assert bad.size == 0, [(float(x[i]), int(codes[i]), int(want[i])) for i in bad[:8]]
        wb = dequant(codes, s)
        fin = ~np.isnan(wb)
        assert np.array_equal(back[fin], wb[fin]) and np.all(np.isnan(back[~fin]))


def _attn_case(nH, nKV, S, T, hd, seed, k_scale, v_scale):
    r = np.random.default_rng(seed)
    q = r.standard_normal((nH, S, hd), dtype=np.float32)
    k = r.standard_normal((nKV, T, hd), dtype=np.float32)
    v = r.standard_normal((nKV, T, hd), dtype=np.float32)
    kd = dequant(ref_quant(k, k_scale), k_scale)
    vd = dequant(ref_quant(v, v_scale), v_scale)
    return q, k, v, kd, vd


@pytest.mark.parametrize("nH,nKV,S,T,hd", [
    (4, 2, 1, 1, 64), (8, 2, 1, 517, 64), (8, 2, 1, 4200, 64),          # decode (GQA); 4200 keys: the key split
    (4, 4, 1, 517, 64), (71, 1, 1, 517, 64), (71, 1, 1, 4200, 64),      # MHA; Falcon's MQA (71 heads, 16-head tiles)
    (8, 2, 1, 517, 128), (16, 1, 1, 4200, 128), (4, 4, 1, 1300, 128),   # hd 128
    (4, 2, 130, 130, 64), (8, 2, 300, 300, 128), (71, 1, 40, 40, 64),   # prefill S = T, causal
    (4, 4, 257, 257, 64), (2, 2, 520, 520, 128),
    (4, 2, 100, 700, 64)])                                              # chunked prefill against a longer cache
@pytest.mark.parametrize("k_scale,v_scale", [(1.0, 1.0), (0.37, 2.5)])
def test_attention_kv8_matches_dequantized_attention(gpu, oracle, nH, nKV, S, T, hd, k_scale, v_scale):
    q, k, v, kd, vd = _attn_case(nH, nKV, S, T, hd, nH * 1000 + T + hd, k_scale, v_scale)
    want = oracle.gqa_core(q, kd, vd)
    got = gpu.ops.attention_kv8(q, k, v, k_scale=k_scale, v_scale=v_scale)
    assert np.isfinite(got).all()
    assert rel_err(got, want) <= BF16_TOL


@pytest.mark.parametrize("nw", [2, 4, 8])
@pytest.mark.parametrize("nKV,T,hd", [(2, 70, 64), (2, 2100, 64), (1, 700, 128), (4, 1, 64)])
def test_decode_kv8_wave_counts(gpu, oracle, nw, nKV, T, hd):
    """every waves-per-workgroup instantiation (tuning key 15 forces one; it also turns the key split off)"""
    q, k, v, kd, vd = _attn_case(4 * nKV, nKV, 1, T, hd, T + nw, 0.5, 1.5)
    old = gpu.lib().nvl_set_tuning(15, nw)
    try:
        got = gpu.ops.attention_kv8(q, k, v, k_scale=0.5, v_scale=1.5)
    finally:
        gpu.lib().nvl_set_tuning(15, old)
    assert rel_err(got, oracle.gqa_core(q, kd, vd)) <= BF16_TOL


def test_attention_kv8_is_attention_over_the_dequantized_cache(gpu):
    """K/V already on the e4m3 grid (times the scale) quantize losslessly: the 8-bit op and the bf16 op then see the same
    cache, and agree to fp32 summation order plus one bf16 output rounding."""
    r = np.random.default_rng(11)
    for S, T in ((1, 900), (64, 64)):
        q = r.standard_normal((8, S, 64), dtype=np.float32)
        k = dequant(r.integers(0, 0x7E, (2, T, 64)).astype(np.uint8) | (r.integers(0, 2, (2, T, 64)) << 7).astype(np.uint8), 1.0) / 16
        v = dequant(r.integers(0, 0x7E, (2, T, 64)).astype(np.uint8), 1.0) / 64
        k, v = k.astype(np.float32), v.astype(np.float32)
        a = gpu.ops.attention_kv8(q, k, v, k_scale=1.0 / 16, v_scale=1.0 / 64)
        b = gpu.ops.attention(q, k, v, precision="bf16")
        assert rel_err(a, b) <= 1e-2
