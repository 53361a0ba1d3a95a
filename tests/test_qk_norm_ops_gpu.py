"""Per-head QK RMSNorm in the layer front through nvl_op_qkv_stages: qk_norm_rope_kv_kernel behind the
store forms (f32, bf16, 8-bit cache) and the EPI_QKV_NORM tile epilogue, against float64 numpy.  inputs(): q_norm_w != k_norm_w,
w[d] != w[d + hd/2]; row r scaled by 2^((r mod 7) - 3); rows 3, 5 and the last scaled down to their bias, mean(x^2) ~ 1.6e-5
against eps = 1e-5; V exactly what the un-normed path produces.  Bounds, derived (u = 2^-24, n the float64 normed head, v its
rotation, mag(e) = e1 |cos| + e2 |sin|): a sum of hd positive squares is within (hd + 1) u in any order; + eps, the square root
(which halves what came before) and the division add 3 u, the products x * r * w 2 u: |n_dev - n| <= (hd / 2 + 5) u |n|; the
rotation adds qkv_reference's 4 u mag(|n|), the store half a step of the output type.  Store forms (fed the device's fp32 qkv
rows): |dev - v| <= step(v) / 2 + (hd / 2 + 9) u mag(|n|).  Epilogue form (fed the float64 projection of the device's op rows,
accumulators within dx <= (K + 2) u S of it), first order through n = x w / rms, rms^2 = mean(x^2) + eps:
dn_d <= |w_d| / rms (dx_d + |x_d| sum_j |x_j| dx_j / (hd rms^2)); |dev - v| <= ulp_bf16(v) / 2 + mag(dn + (hd / 2 + 9) u |n|)."""
import numpy as np
import pytest

import qkv_reference as R
from qkv_reference import U24, bf16, kv8_dequantized
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu
EPS = 1e-5


def qk_norm64(t, w):      # HF Qwen3RMSNorm over the last axis, float64
    t = np.asarray(t, np.float64)
    return t / np.sqrt((t * t).mean(-1, keepdims=True) + EPS) * np.asarray(w, np.float64)


def inputs(seq_len, seq_pos, nH, nKV, hd, kv8, seed, K=128):
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s, dtype=np.float32)
    M, N = int(sum(seq_len)), (nH + 2 * nKV) * hd
    inp = dict(seq_len=seq_len, seq_pos=seq_pos, nH=nH, nKV=nKV, hd=hd, K=K, M=M, N=N, rope=10000.0, kv8=kv8)
    inp.update(R.make_batch(seq_len, seq_pos, nKV, hd, kv8 or (1.0, 1.0), rng))
    x = n(M, K) * (2.0 ** ((np.arange(M) % 7) - 3))[:, None].astype(np.float32)
    x[[3, 5, M - 1]] *= 1e-4
    ramp = np.linspace(-0.4, 0.4, hd, dtype=np.float32)                 # w[d] != w[d + hd/2]
    inp.update(x=x, w_qkv=0.1 * n(N, K), b_qkv=0.004 * n(N), q_norm_w=1.0 + ramp + 0.1 * n(hd), k_norm_w=1.3 - ramp + 0.1 * n(hd))
    return inp


def run(gpu, inp, precision, keys, **over):
    kw = dict(x=inp["x"], w_qkv=inp["w_qkv"], k_pool=inp["k_pool"], v_pool=inp["v_pool"], block_table=inp["table"], seq_len=inp["seq_len"],
              seq_pos=inp["seq_pos"], nH=inp["nH"], b_qkv=inp["b_qkv"], norm_eps=EPS, rope_base=inp["rope"], max_seq=inp["max_seq"],
              precision=precision, q_norm_w=inp["q_norm_w"], k_norm_w=inp["k_norm_w"])
    if inp["kv8"]:
        kw.update(kv8=True, k_scale=inp["kv8"][0], v_scale=inp["kv8"][1])
    kw.update(over)
    with Tuning(gpu, keys):
        return gpu.ops.qkv_stages(**kw)


B7, B70, B65, B300, B2041 = ((3, 1, 3), (5, 130, 61)), ((40, 1, 29), (5, 130, 50)), ((35, 1, 29), (5, 130, 50)), ((170, 1, 129), (5, 130, 50)), R.B2041
CASES = {}      # name -> (batch, (nH, nKV), hd, precision, kv8 scales, tuning keys, ran form, ran gemm)
for hd in (64, 128):
    for heads in ((3, 1), (4, 2)):
        t = f"hd{hd}-{heads[0]}x{heads[1]}"
        CASES[f"f32-{t}-M7"] = (B7, heads, hd, "f32", None, {0: 0}, "f32_store_rope", None)
        CASES[f"bf16-{t}-M7"] = (B7, heads, hd, "bf16", None, {0: 0}, "decode_store_rope", "decode")
        CASES[f"bf16-{t}-M70"] = (B70, heads, hd, "bf16", None, {0: 0, 18: 256}, "groups_store_rope", "groups")
    CASES[f"kv8-hd{hd}-3x1-M7"] = (B7, (3, 1), hd, "bf16", (0.25, 1.0), {0: 0}, "store_rope_kv8", "decode")
    CASES[f"kv8-hd{hd}-4x2-M70"] = (B70, (4, 2), hd, "bf16", (0.25, 1.0), {0: 0}, "store_rope_kv8", "groups")
# the epilogue form (key 18 = 0): 65 rows; 300 rows: a tile with 44 live rows beside lanes m >= M; the two ping-pong instances
CASES["epi-hd64-3x1-M65"] = (B65, (3, 1), 64, "bf16", None, {0: 0, 18: 0}, "epilogue", "tile1")
CASES["epi-hd64-4x2-M300"] = (B300, (4, 2), 64, "bf16", None, {0: 0, 18: 0}, "epilogue", "tile1")
CASES["epi-hd128-3x1-M300"] = (B300, (3, 1), 128, "bf16", None, {0: 0, 18: 0}, "epilogue", "hd128_4x2")
CASES["epi-hd64-pingpong-4x2-M259"] = (R.B259, (4, 2), 64, "bf16", None, {0: 5, 18: 0}, "epilogue", "pingpong")
CASES["epi-hd128-pingpong-32x8-M2041"] = (B2041, (32, 8), 128, "bf16", None, {0: 0, 18: 0}, "epilogue", "hd128_pingpong")


@pytest.mark.parametrize("name", list(CASES))
def test_qk_norm_front(gpu, name):
    batch, (nH, nKV), hd, precision, kv8, keys, form, gemm = CASES[name]
    # hidden 128; the hd-128 ping-pong instance needs K >= 160 (launch_gemm_bf16): 192 there, as in tests/qkv_reference.py
    K = 192 if gemm == "hd128_pingpong" else 128
    inp = dict(inputs(batch[0], batch[1], nH, nKV, hd, kv8, seed=len(name) * 131 + hd, K=K), precision=precision)
    out = run(gpu, inp, precision, keys)
    assert (out["ran"]["form"], out["ran"]["gemm"]) == (form, gemm), (name, out["ran"])
    M, wm = inp["M"], R.written_mask(inp)
    for pool in ("k_pool", "v_pool"):
        assert (R._bits(out[pool]) == R._bits(inp[pool]))[~wm].all(), f"{name}: {pool} changed outside the rows the batch names"
    assert np.isnan(out["q"][M:]).all(), f"{name}: a padded row m >= M of the q buffer was written"
    qd = out["q"][:M].reshape(M, nH, hd)
    kd, vd = R.gathered(inp, out["k_pool"]), R.gathered(inp, out["v_pool"])
    E = (hd / 2 + 9) * U24
    if form == "epilogue":
        p64, S = R.projection64(inp, out["op"])
        x3, dx3 = R.heads_of(inp, p64), R.heads_of(inp, (K + 2) * U24 * S)
    else:
        x3, dx3 = R.heads_of(inp, out["qkv"]), (0.0, 0.0, 0.0)
    small = (np.asarray(x3[0], np.float64)[[3, 5, M - 1]] ** 2).mean(-1)
    assert (small < 4 * EPS).all() and (small > EPS / 4).all(), small      # the eps rows are what they claim to be
    for what, dev, x, dx, w in (("Q", qd, x3[0], dx3[0], inp["q_norm_w"]), ("K", kd, x3[1], dx3[1], inp["k_norm_w"])):
        x = np.asarray(x, np.float64)
        n64 = qk_norm64(x, w)
        ms = (x * x).mean(-1, keepdims=True) + EPS
        dn = np.abs(w) / np.sqrt(ms) * (dx + np.abs(x) * (np.abs(x) * dx).sum(-1, keepdims=True) / (hd * ms))
        v, mag = R.rotate(inp, n64, dn + E * np.abs(n64))
        step = 2 * U24 * np.abs(v) if precision == "f32" else R.step_e4m3(v, kv8[0]) if kv8 and what == "K" else R.ulp_bf16(v)
        R._held(dev, v, 0.5 * step + mag + 1e-300, name, what)
    # V: exactly what the un-normed path produces
    if form == "epilogue":
        want = R.gathered(inp, run(gpu, inp, precision, keys, q_norm_w=None, k_norm_w=None)["v_pool"])
    else:
        v32 = R.heads_of(inp, out["qkv"])[2]
        want = v32 if precision == "f32" else kv8_dequantized(v32, kv8[1]) if kv8 else bf16(v32)
    assert np.array_equal(R._bits(vd), R._bits(want)), f"{name}: V is not the un-normed path's"


@pytest.mark.parametrize("batch,keys", [(B7, {0: 0}), (B300, {0: 0, 18: 0})])
def test_null_weights_in_the_longer_struct_change_no_bit(gpu, batch, keys):
    inp = inputs(batch[0], batch[1], 4, 2, 128, None, seed=3)
    old, new = (run(gpu, inp, "bf16", keys, q_norm_w=None, k_norm_w=None, qk_norm_struct=s) for s in (False, True))
    assert old["ran"] == new["ran"] and all(np.array_equal(R._bits(old[k]), R._bits(new[k])) for k in ("q", "k_pool", "v_pool", "qkv", "op"))
