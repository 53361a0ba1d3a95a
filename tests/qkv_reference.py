"""The front of an attention layer (generic_model.go:295-318: embedWithOffset, attention norm, the QKV projection with its
bias; rope.go:153-205 on Q and K; Q into the attention operand buffer, K / V into the paged cache) in float64, stage by
stage — numpy only, test infrastructure like tests/dense_reference.py — plus the batches, the case table and the
assertions tests/test_qkv_ops_gpu.py and tests/test_qkv_reference_host.py share.

Every stage's reference is FED THE DEVICE'S OWN OUTPUT of the stage before (out: what ops.qkv_stages returns): the operand
from the device's x, the fp32 projection from the device's operand, Q / K / V of a store form from the device's fp32
projection, Q / K / V of the epilogue form (which never stores the projection) from the device's operand.  No error is
charged twice and no row is excluded.

Pools.  Before the pass every element of both pools holds a finite sentinel that is bf16-exact — and e4m3-exact at the
case's k_scale / v_scale, so that the 8-bit cache returns it bit for bit — and differs from its neighbours; block ids are a
seeded permutation; every unused table entry names a poison block of its own.  After the pass every element outside the
rows (block, seq_pos + j) the batch names must be bit-equal to its sentinel, in every form, and every row of the q buffer
from `tokens` on must still be NaN.

Bounds, all derived (u = 2^-24; K = hidden):
  x (embedding)   bit-equal to numpy float32 (f32(T(emb[tok])) + f32(T(pos_emb[pos]))) * mult, T = bf16 rounding (the bf16
                  tables; identity in f32 mode): one fp32 add, one fp32 multiply; a position >= the table's rows adds nothing.
  op              norm path: per row rms(dev - f64) <= ratio bound x rms(bf16(f64) - f64), as dense_reference.check_operand
                  holds bf16(norm(x)); no norm: bit-equal to bf16(x).
  qkv             |dev - f64| <= (K + 2) u sum_k |a_k w_k| + 2 u |f64|, f64 = op_dev . bf16(W)^T + b: the worst case of an fp32
                  dot product in any order (Higham, Accuracy and Stability, eq. 3.5) plus the bias add.
  Q, K (store)    v = rope_f64(qkv_dev) on the fp32 tables: |dev - v| <= ulp_bf16(v) / 2 + 4 u (|x1 c| + |x2 s|) (two fp32
                  products and one add, each within u relative; the factor 4 also covers a fused multiply-add's different
                  rounding), and at most MISMATCH_CAP = 1e-3 of the elements may differ from bf16(v) at all: float32 against
                  float64 evaluation differs on ~2e-5 of them (test_qkv_reference_host.py recomputes that share and holds
                  it below 1e-4), so the cap is a condition with a 50-fold margin, not a measurement.
  V (store)       bit-equal to bf16(qkv_dev); 8-bit cache: bit-equal to kv8_dequantized(qkv_dev, v_scale), and K as Q / K
                  above with the e4m3 step of v / k_scale in place of the bf16 step, same cap.
  Q, K, V (epilogue, from op_dev)   |dev - v| <= ulp_bf16(v) / 2 + (K + 4) u (S1 |c| + S2 |s|), S = sum_k |a_k w_k| + |b| of
                  the element and of its partner (V: c = 1, s = 0).  No ulp distance here: near a cancellation fp32 and
                  float64 land several bf16 steps apart.
  f32 mode        F32_TOL (2e-5) of the row's largest value, per row, every stage.
  exact family    no norm, small-integer operands, weights that are a signed selection of operand columns, an integer bias,
                  every sum <= 128 in magnitude, no rotation (rope_base 0; a prefill batch has positions other than 0): Q, K, V and every untouched
                  element np.array_equal.  The values are random integers — asymmetric in row, head and column — so a value
                  that lands anywhere else cannot pass."""
import zlib

import numpy as np

import attention_reference as AR
import dense_reference as DR
from attention_reference import bf16, kv8_dequantized, rope_tables, rope_f64
from dense_reference import F32_TOL, U24, norm64

MISMATCH_CAP = 1e-3
BLOCK = 64


def _f64(a):
    return np.asarray(a, np.float64)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


# ---- the batch -----------------------------------------------------------------------------------------------------------
def token_rows(seq_len, seq_pos):
    """-> (sequence of every row, position of every row), rows back to back in sequence order (plan_rows)"""
    seq = np.concatenate([np.full(n, i) for i, n in enumerate(seq_len)])
    pos = np.concatenate([p + np.arange(n) for n, p in zip(seq_len, seq_pos)])
    return seq.astype(np.int64), pos.astype(np.int64)


def sentinel(shape, scale, salt):
    """finite, bf16-exact and e4m3-exact at `scale` (a power of two): scale x the e4m3 value of a code that runs through
    8 .. 119 with a period coprime to every pool dimension, the sign from another period"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    code = 8 + (i * 7 + salt) % 113 % 112
    sign = np.where((i // 3 + salt) % 5 < 2, -1.0, 1.0)
    v = sign * AR.E4M3[code] * scale
    assert np.array_equal(bf16(v), v) and np.array_equal(kv8_dequantized(v, scale), v)
    return v.astype(np.float32).reshape(shape)


def make_batch(seq_len, seq_pos, nKV, hd, scales, rng):
    """block table [n_seqs][stride] (one more column than any sequence needs), pools with sentinels, a poison block"""
    n_seqs = len(seq_len)
    need = [-(-(p + n) // BLOCK) for n, p in zip(seq_len, seq_pos)]
    stride = max(need) + 1
    n_blocks = sum(need) + 2                      # the used ones, the poison block, one nobody names
    ids = rng.permutation(n_blocks)
    poison, used = int(ids[0]), ids[1:1 + sum(need)]
    table = np.full((n_seqs, stride), poison, np.int32)
    at = 0
    for i, nb in enumerate(need):
        table[i, :nb] = used[at:at + nb]
        at += nb
    shape = (n_blocks, nKV, BLOCK, hd)
    return dict(table=table, n_blocks=n_blocks, poison=poison, max_seq=stride * BLOCK,
                k_pool=sentinel(shape, scales[0], 1), v_pool=sentinel(shape, scales[1], 40))


def locate(inp):
    """(block, row) of every token's K / V row (kv_locate)"""
    seq, pos = token_rows(inp["seq_len"], inp["seq_pos"])
    return inp["table"][seq, pos // BLOCK].astype(np.int64), pos % BLOCK


# ---- the case table --------------------------------------------------------------------------------------------------------
# name -> dict(the batch, the shape, the variant, keys of nvl_set_tuning, ran: literals worked out by hand from qkv_front(),
# launch_gemm_bf16 and launch_norm — a case whose ran differs from its literal is a finding about the dispatch: work the
# literal out again by hand before touching it, never copy it from a run)
B131 = ((70, 1, 60), (0, 130, 50))            # 131 rows: a block boundary inside an m-tile, a mid-block start, 3 rows in the last 128-row tile
B259 = ((70, 1, 188), (0, 130, 50))           # 259 rows: the same for the 256-row tiles
B37 = ((20, 1, 16), (0, 130, 50))             # 37 rows: the decode-form projection
B3 = ((1, 1, 1), (0, 130, 50))                # a decode step
B2041 = ((700, 1, 1340), (0, 130, 50))        # 2041 rows: 8 x 24 tiles of 256 x 256 at N = 6144
VARIANTS = (dict(norm="rms", bias=False, rope=10000.0), dict(norm="rms", bias=True, rope=500000.0),
            dict(norm="layer", bias=True, rope=0.0),                  # the GPT-2 shape: LayerNorm + bias + no RoPE
            dict(norm="rms", bias=True, rope=10000.0))
CASES = {}


def _ran(form, gemm, norm="row", embed=None):
    return dict(form=form, gemm=gemm, norm=norm, embed=embed)


def _add(name, batch, heads, hd, ran, keys=None, family="random", precision="bf16", kv8=None, K=192, **variant):
    v = dict(norm="rms", bias=True, rope=10000.0)
    v.update(variant)
    if family == "exact":
        v.update(norm=None)
        ran = dict(ran, norm=None)
    CASES[name] = dict(seq_len=batch[0], seq_pos=batch[1], nH=heads[0], nKV=heads[1], hd=hd, K=K, ran=ran, keys=keys or {},
                       family=family, precision=precision, kv8=kv8, **v)


# epilogue, hd 64: tiles 1, 2, 3 and the ping-pong kernel (5) forced by key 0 (which also switches the short-prefill form off);
# N = 512 and N = 320 (a ragged N tile whose last wave sub-tile is a lone V head); every tile sees all four variants
TILE_NAMES = {1: "tile1", 2: "tile2", 3: "tile3", 5: "pingpong"}
for tile, tname in TILE_NAMES.items():
    n = 0
    for heads in ((4, 2), (3, 1)):
        for bname, batch in (("131", B131), ("259", B259)):
            _add(f"epi-{tname}-{heads[0]}x{heads[1]}-M{bname}", batch, heads, 64, _ran("epilogue", tname), {0: tile}, **VARIANTS[n % 4])
            n += 1
        _add(f"epi-{tname}-{heads[0]}x{heads[1]}-M131-exact", B131, heads, 64, _ran("epilogue", tname), {0: tile}, "exact", rope=0.0)
# epilogue, hd 128: 259 rows are above the short-prefill bound, 2 x 4 (2 x 3) tiles of 256 x 256 -> the 4x2 instance
for n, heads in enumerate(((4, 2), (3, 1))):
    _add(f"epi-hd128-{heads[0]}x{heads[1]}-M259", B259, heads, 128, _ran("epilogue", "hd128_4x2"), {0: 0}, **VARIANTS[(n + 1) % 4])
    _add(f"epi-hd128-{heads[0]}x{heads[1]}-M259-exact", B259, heads, 128, _ran("epilogue", "hd128_4x2"), {0: 0}, "exact", rope=0.0)
# 8 x 24 = 192 tiles fill 3/4 of the CUs, K = 192 >= 160, key 0 = 0: the hd-128 ping-pong instance; 2041 rows take
# norm_tile16_kernel
_add("epi-hd128-pingpong-32x8-M2041", B2041, (32, 8), 128, _ran("epilogue", "hd128_pingpong", "tile16"), {0: 0})
# store forms
for heads in ((4, 2), (3, 1)):
    t = f"{heads[0]}x{heads[1]}"
    _add(f"store-decode-{t}-M37", B37, heads, 64, _ran("decode_store_rope", "decode"), {0: 0})
    _add(f"store-groups-{t}-M131", B131, heads, 64, _ran("groups_store_rope", "groups"), {0: 0, 18: 256}, rope=500000.0)
_add("store-decode-llama-M37", ((37,), (0,)), (4, 2), 64, _ran("decode_store_rope", "decode"), {0: 0}, bias=False)      # one prompt from position 0
_add("store-decode-hd128-M37", B37, (4, 2), 128, _ran("decode_store_rope", "decode"), {0: 0}, bias=False)
_add("store-groups-hd128-M131", B131, (4, 2), 128, _ran("groups_store_rope", "groups"), {0: 0, 18: 256})
_add("store-decode-M37-exact", B37, (4, 2), 64, _ran("decode_store_rope", "decode"), {0: 0}, "exact", rope=0.0)
_add("store-groups-M131-exact", B131, (3, 1), 64, _ran("groups_store_rope", "groups"), {0: 0, 18: 256}, "exact", rope=0.0)
_add("store-gpt2-M131", B131, (4, 2), 64, _ran("groups_store_rope", "groups"), {0: 0, 18: 256}, **VARIANTS[2])
_add("f32-M131", B131, (4, 2), 64, _ran("f32_store_rope", None), {0: 0}, precision="f32")
_add("f32-M131-3x1-gpt2", B131, (3, 1), 64, _ran("f32_store_rope", None), {0: 0}, precision="f32", **VARIANTS[2])
_add("f32-M131-exact", B131, (4, 2), 64, _ran("f32_store_rope", None), {0: 0}, "exact", precision="f32", rope=0.0)
_add("kv8-M37", B37, (4, 2), 64, _ran("store_rope_kv8", "decode"), {0: 0}, kv8=(1.0, 0.25))
_add("kv8-M131", B131, (4, 2), 64, _ran("store_rope_kv8", "groups"), {0: 0}, kv8=(1.0, 0.25))
_add("kv8-M131-hd128", B131, (3, 1), 128, _ran("store_rope_kv8", "groups"), {0: 0}, kv8=(0.25, 1.0), rope=500000.0)
_add("decode-step", B3, (4, 2), 64, _ran("store_only", "decode"), {0: 0})
# the embedding stage: V = 1003, learned positions [110][K] with one row at and one past the table's last row
for prec in ("bf16", "f32"):
    for mult in (0.0, 12.0):
        _add(f"embed-{prec}-mult{mult:g}", B37, (4, 2), 64,
             _ran("f32_store_rope" if prec == "f32" else "decode_store_rope", None if prec == "f32" else "decode", embed=prec), {0: 0},
             precision=prec, embed=dict(V=1003, P=110, mult=mult), **VARIANTS[2])

EPILOGUE_INSTANCES = ("tile1", "tile2", "tile3", "pingpong", "hd128_4x2", "hd128_pingpong")


def make_inputs(name):
    c = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = lambda *s: rng.standard_normal(s, dtype=np.float32)
    nH, nKV, hd, K = c["nH"], c["nKV"], c["hd"], c["K"]
    N = (nH + 2 * nKV) * hd
    M = int(sum(c["seq_len"]))
    inp = dict(c, name=name, N=N, M=M)
    inp.update(make_batch(c["seq_len"], c["seq_pos"], nKV, hd, c["kv8"] or (1.0, 1.0), rng))
    if c["family"] == "exact":
        # x in -8 .. 8; a weight row selects three operand columns with signs: |sum| <= 24, + a bias in -4 .. 4
        inp["x"] = rng.integers(-8, 9, (M, K)).astype(np.float32)
        w = np.zeros((N, K), np.float32)
        for r in range(N):
            w[r, rng.choice(K, 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
        inp["w_qkv"] = w
        inp["b_qkv"] = rng.integers(-4, 5, N).astype(np.float32) if c["bias"] else None
        inp["norm_w"] = inp["norm_b"] = None
        assert (np.abs(_f64(inp["x"])) @ np.abs(_f64(w)).T).max() + 4 <= 128
        assert not c["rope"]                     # (no rotation: a prefill batch has positions other than 0)
        return inp
    inp["x"] = n(M, K)
    inp["x"][3::7] *= 1e-3                       # rows whose mean(x^2) is of the order of eps
    inp["w_qkv"] = n(N, K) * 0.1
    inp["b_qkv"] = 0.5 * n(N) if c["bias"] else None
    inp["norm_w"] = 1.0 + 0.3 * n(K)
    inp["norm_b"] = 0.1 * n(K) if c["norm"] == "layer" else None
    e = c.get("embed")
    if e:
        inp["emb"], inp["pos_emb"] = n(e["V"], K), n(e["P"], K)
        tok = rng.integers(0, e["V"], M)
        tok[[0, 5, M - 1]] = (0, e["V"] - 1, e["V"] - 1)
        tp = rng.integers(0, e["P"], M)
        tp[[1, 7, M - 2]] = (e["P"] - 1, e["P"], 0)                 # at the table's last row, one past it, row 0
        inp.update(tokens=tok.astype(np.int32), tok_pos=tp.astype(np.int32), x=None)
    return inp


def op_kwargs(inp):
    """the arguments of ops.qkv_stages"""
    kw = dict(x=inp["x"], w_qkv=inp["w_qkv"], k_pool=inp["k_pool"], v_pool=inp["v_pool"], block_table=inp["table"],
              seq_len=inp["seq_len"], seq_pos=inp["seq_pos"], nH=inp["nH"], b_qkv=inp["b_qkv"], norm_w=inp["norm_w"],
              norm_b=inp["norm_b"], norm=inp["norm"] or "rms", rope_base=inp["rope"], max_seq=inp["max_seq"],
              precision=inp["precision"])
    if inp["kv8"]:
        kw.update(kv8=True, k_scale=inp["kv8"][0], v_scale=inp["kv8"][1])
    if inp.get("embed"):
        kw.update(tokens=inp["tokens"], tok_pos=inp["tok_pos"], emb=inp["emb"], pos_emb=inp["pos_emb"],
                  embedding_multiplier=inp["embed"]["mult"])
    return kw


# ---- the float64 statement ---------------------------------------------------------------------------------------------
def _T(inp):
    """what the upload does to a matrix operand"""
    return (lambda a: np.asarray(a, np.float32)) if inp["precision"] == "f32" else (lambda a: bf16(a).astype(np.float32))


def embed32(inp):
    """numpy float32: one add, one multiply"""
    T, e = _T(inp), inp["embed"]
    x = T(inp["emb"])[inp["tokens"]]
    inside = inp["tok_pos"] < e["P"]
    x[inside] = x[inside] + T(inp["pos_emb"])[inp["tok_pos"][inside]]
    if e["mult"] != 0.0:
        x = x * np.float32(e["mult"])
    assert x.dtype == np.float32
    return x


def operand64(inp, x):
    if inp["norm_w"] is None:
        return _f64(x)
    return norm64(x, inp["norm_w"], inp["norm_b"], 1e-5, "layer" if inp["norm"] == "layer" else "rms")


def projection64(inp, op):
    """-> (f64 [M][N], S = sum_k |a_k w_k| + |b|)"""
    w = _f64(_T(inp)(inp["w_qkv"]))
    b = 0.0 if inp["b_qkv"] is None else _f64(inp["b_qkv"])
    return _f64(op) @ w.T + b, np.abs(_f64(op)) @ np.abs(w).T + np.abs(b)


def heads_of(inp, y):
    """[M][N] -> q [M][nH][hd], k, v [M][nKV][hd]"""
    nH, nKV, hd = inp["nH"], inp["nKV"], inp["hd"]
    M = y.shape[0]
    return (y[:, :nH * hd].reshape(M, nH, hd), y[:, nH * hd:(nH + nKV) * hd].reshape(M, nKV, hd), y[:, (nH + nKV) * hd:].reshape(M, nKV, hd))


def rotate(inp, t, mag=None):
    """-> (rope_f64(t), |x1 c| + |x2 s|, with the magnitudes `mag` in place of |t| when given) for t [M][heads][hd]"""
    _, pos = token_rows(inp["seq_len"], inp["seq_pos"])
    a = np.abs(_f64(t)) if mag is None else _f64(mag)
    if not inp["rope"]:
        return _f64(t), a
    hd = t.shape[-1]
    cos, sin = rope_tables(inp["rope"], inp["max_seq"], hd)
    swap = np.concatenate([a[..., hd // 2:], a[..., :hd // 2]], -1)
    return rope_f64(t, pos[:, None], inp["rope"], inp["max_seq"]), a * np.abs(cos[pos])[:, None, :] + swap * np.abs(sin[pos])[:, None, :]


def ulp_bf16(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


def step_e4m3(v, s):
    """the spacing of the e4m3 grid around v / s, times s (subnormal codes: 2^-9; saturation is never reached here)"""
    y = np.abs(v) / s
    assert y.max() < 448.0
    return s * 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(y, 2.0 ** -30))), -6.0) - 3)


def gathered(inp, pool):
    """the K / V rows the batch names, out of a pool -> [M][nKV][hd]"""
    blk, row = locate(inp)
    return pool[blk, :, row, :]


def written_mask(inp):
    blk, row = locate(inp)
    m = np.zeros(inp["k_pool"].shape, bool)
    m[blk, :, row, :] = True
    return m


# ---- the assertions ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _row_tol(dev, want, name, what):
    """f32 mode: F32_TOL of the row's largest value, per row (rows = the leading axis)"""
    d, w = _f64(dev).reshape(len(dev), -1), _f64(want).reshape(len(want), -1)
    assert np.isfinite(d).all(), f"{name}: NaN in {what}"
    e = np.abs(d - w).max(1) / np.maximum(np.abs(w).max(1), 1e-30)
    assert (e <= F32_TOL).all(), f"{name}: {what} row {int(e.argmax())} off by {e.max():.2e} of its maximum"
    return float(e.max())


def _held(dev, v, tol, name, what):
    """-> the worst error as a share of its bound"""
    assert np.isfinite(dev).all(), f"{name}: NaN in {what}: a row no launch wrote"
    r = np.abs(_f64(dev) - v) / tol
    assert (r <= 1.0).all(), f"{name}: {what} beyond its bound at {np.unravel_index(int(r.argmax()), r.shape)}: {r.max():.3f} x"
    return float(r.max())


def _share(dev, want, name, what):
    s = float((_bits(dev) != _bits(want)).mean())
    assert s <= MISMATCH_CAP, f"{name}: {s:.2e} of {what} differ from the rounded float64 value (cap {MISMATCH_CAP:.0e})"
    return s


def check(inp, out, ratio_bound, name=""):
    """every stage of out against the reference fed the stage before -> {figure: worst value}"""
    name = name or inp["name"]
    fig, form, f32 = {}, out["ran"]["form"], inp["precision"] == "f32"
    nH, nKV, hd, M, K = inp["nH"], inp["nKV"], inp["hd"], inp["M"], inp["K"]
    exact = inp["family"] == "exact"
    # x
    x = inp["x"]
    if inp.get("embed"):
        x = out["x"]
        assert np.array_equal(_bits(x), _bits(embed32(inp))), f"{name}: x is not (f32(emb[tok]) + f32(pos_emb[pos])) * mult"
    # the operand
    op = out["op"]
    assert op.shape == (M, K) and np.isfinite(op).all(), f"{name}: NaN in the operand"
    o64 = operand64(inp, x)
    if inp["norm_w"] is None:
        assert np.array_equal(_bits(op), _bits(_T(inp)(x))), f"{name}: the operand is not the rounded x"
    elif f32:
        fig["op_f32"] = _row_tol(op, o64, name, "op")
    else:
        den = DR.row_rms(bf16(o64) - o64)
        assert (den > 0).all()
        r = DR.row_rms(_f64(op) - o64) / den
        fig["op_ratio"] = float(r.max())
        assert r.max() <= ratio_bound, f"{name}: operand row {int(r.argmax())}: {r.max():.4f} x the rounding error of bf16(norm(x))"
    p64, S = projection64(inp, op)
    # the fp32 projection (store forms)
    qkv = out["qkv"]
    if form == "epilogue":
        assert np.isnan(qkv).all(), f"{name}: the epilogue form stored an fp32 projection"
    elif f32:
        fig["qkv_f32"] = _row_tol(qkv, p64, name, "qkv")
    else:
        fig["qkv"] = _held(qkv, p64, (K + 2) * U24 * S + 2 * U24 * np.abs(p64) + 1e-300, name, "qkv")
    if exact and form != "epilogue":
        assert np.array_equal(_f64(qkv), p64), f"{name}: qkv is not exact"
    # Q, K, V
    qbuf = out["q"]
    assert qbuf.shape == (-(-M // 256) * 256, nH * hd)
    assert np.isnan(qbuf[M:]).all(), f"{name}: a padded row m >= M of the q buffer was written"
    same_k = _bits(out["k_pool"]) == _bits(inp["k_pool"])
    same_v = _bits(out["v_pool"]) == _bits(inp["v_pool"])
    if form == "store_only":
        assert np.isnan(qbuf).all(), f"{name}: a decode step's projection wrote the q buffer"
        assert same_k.all() and same_v.all(), f"{name}: a decode step's projection touched the pools"
        return fig
    wm = written_mask(inp)
    assert same_k[~wm].all(), f"{name}: K pool changed outside the rows the batch names ({int((~same_k & ~wm).sum())} elements)"
    assert same_v[~wm].all(), f"{name}: V pool changed outside the rows the batch names ({int((~same_v & ~wm).sum())} elements)"
    qd = qbuf[:M].reshape(M, nH, hd)
    kd, vd = gathered(inp, out["k_pool"]), gathered(inp, out["v_pool"])
    if form == "epilogue":
        (q64, k64, v64), (Sq, Sk, Sv) = heads_of(inp, p64), heads_of(inp, S)
        for what, dev, t, s in (("Q", qd, q64, Sq), ("K", kd, k64, Sk)):
            v, mag = rotate(inp, t, s)
            fig[f"{what}_epi"] = _held(dev, v, 0.5 * ulp_bf16(v) + (K + 4) * U24 * mag + 1e-300, name, what)
            if exact:
                assert np.array_equal(_f64(dev), v), f"{name}: {what} is not exact"
        fig["V_epi"] = _held(vd, v64, 0.5 * ulp_bf16(v64) + (K + 4) * U24 * Sv + 1e-300, name, "V")
        if exact:
            assert np.array_equal(_f64(vd), v64), f"{name}: V is not exact"
        return fig
    q32, k32, v32 = heads_of(inp, qkv)
    (qv, qmag), (kv, kmag) = rotate(inp, q32), rotate(inp, k32)
    if f32:
        fig["Q_f32"] = _row_tol(qd, qv, name, "Q")
        fig["K_f32"] = _row_tol(kd, kv, name, "K")
        assert np.array_equal(_bits(vd), _bits(v32)), f"{name}: V is not the fp32 projection"
    else:
        fig["Q"] = _held(qd, qv, 0.5 * ulp_bf16(qv) + 4 * U24 * qmag + 1e-300, name, "Q")
        fig["Q_share"] = _share(qd, bf16(qv), name, "Q")
        if inp["kv8"]:
            ks, vs = inp["kv8"]
            fig["K"] = _held(kd, kv, 0.5 * step_e4m3(kv, ks) + 4 * U24 * kmag + 1e-300, name, "K (e4m3)")
            fig["K_share"] = _share(kd, kv8_dequantized(_f32(kv), ks), name, "K (e4m3)")
            assert np.array_equal(_bits(vd), _bits(kv8_dequantized(v32, vs))), f"{name}: V is not kv8_dequantized(qkv, v_scale)"
        else:
            fig["K"] = _held(kd, kv, 0.5 * ulp_bf16(kv) + 4 * U24 * kmag + 1e-300, name, "K")
            fig["K_share"] = _share(kd, bf16(kv), name, "K")
            assert np.array_equal(_bits(vd), _bits(bf16(v32))), f"{name}: V is not bf16(qkv), rounded to nearest even"
    if exact:
        assert np.array_equal(_f64(qd), qv) and np.array_equal(_f64(kd), kv) and np.array_equal(_f64(vd), _f64(v32)), f"{name}: Q / K / V are not exact"
    return fig


# ---- a stand-in for ops.qkv_stages made of the reference alone (tests/test_qkv_reference_host.py) ---------------------
MUTATIONS = ("rope_position_minus_one", "rope_skipped_on_k", "rope_applied_to_v", "partner_at_32_in_hd128", "cos_sin_halves_swapped",
             "k_row_at_pos_plus_one", "other_sequences_table_row", "kv_heads_swapped", "bias_omitted", "bias_shifted_one_head",
             "last_ragged_tile_not_written", "padded_row_written", "q_hd64_row_stride_in_hd128", "v_truncated")


def _rope_mut(inp, t, mut, is_k):
    """the rotation as a kernel with the named defect would do it, float64"""
    t = _f64(t)
    if not inp["rope"] or (mut == "rope_skipped_on_k" and is_k):
        return t
    _, pos = token_rows(inp["seq_len"], inp["seq_pos"])
    if mut == "rope_position_minus_one":
        pos = np.maximum(pos - 1, 0)
    hd = t.shape[-1]
    cos, sin = rope_tables(inp["rope"], inp["max_seq"], hd)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    h = hd // 2
    if mut == "partner_at_32_in_hd128" and hd == 128:
        rot = np.concatenate([-t[..., 32:64], t[..., :32], -t[..., 96:], t[..., 64:96]], -1)
    elif mut == "cos_sin_halves_swapped":        # the second half's formula on the first half and the other way round
        rot = np.concatenate([t[..., h:], -t[..., :h]], -1)
    else:
        rot = np.concatenate([-t[..., h:], t[..., :h]], -1)
    return t * c + rot * s


def emulated_device(inp, ran, mut=None, tile_rows=128):
    """float64 with the kernels' roundings, stored as fp32, in the shape of ops.qkv_stages' result; mut: one of MUTATIONS,
    applied where a kernel would go wrong"""
    nH, nKV, hd, M = inp["nH"], inp["nKV"], inp["hd"], inp["M"]
    f32, form = inp["precision"] == "f32", ran["form"]
    T = _T(inp)
    out = dict(ran=ran)
    x = inp["x"]
    if inp.get("embed"):
        x = out["x"] = embed32(inp)
    op = T(_f32(operand64(inp, x)))
    w = _f64(T(inp["w_qkv"]))
    b = np.zeros(inp["N"]) if inp["b_qkv"] is None else _f64(inp["b_qkv"])
    if mut == "bias_omitted":
        b = np.zeros(inp["N"])
    if mut == "bias_shifted_one_head":
        b = np.roll(b, hd)
    y = _f64(op) @ w.T + b
    store = form != "epilogue"
    if store:
        y = _f32(y)
    out.update(op=op, qkv=y.astype(np.float32) if store else np.full((M, inp["N"]), np.nan, np.float32))
    q, k, v = heads_of(inp, _f64(y))
    q, k = _rope_mut(inp, q, mut, False), _rope_mut(inp, k, mut, True)
    if mut == "rope_applied_to_v":
        v = _rope_mut(inp, v, mut, False)
    if mut == "kv_heads_swapped":
        k, v = k[:, ::-1], v[:, ::-1]
    rnd = (lambda a: _f32(a)) if f32 else (lambda a: bf16(_f32(a)).astype(np.float32))
    if inp["kv8"]:
        kq, vq = kv8_dequantized(_f32(k), inp["kv8"][0]).astype(np.float32), kv8_dequantized(_f32(v), inp["kv8"][1]).astype(np.float32)
    else:
        kq, vq = rnd(k), rnd(v)
        if mut == "v_truncated" and not f32:
            vq = (_f32(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    qbuf = np.full((-(-M // 256) * 256, nH * hd), np.nan, np.float32)
    kp, vp = inp["k_pool"].copy(), inp["v_pool"].copy()
    if form == "store_only":
        out.update(q=qbuf, k_pool=kp, v_pool=vp)
        return out
    rows = np.arange(M)
    if mut == "last_ragged_tile_not_written":
        rows = rows[rows < (M - 1) // tile_rows * tile_rows]
    if mut == "q_hd64_row_stride_in_hd128" and hd == 128:
        flat = qbuf.reshape(-1)
        for t in rows:
            flat[t * nH * 64:t * nH * 64 + nH * hd] = rnd(q[t]).reshape(-1)
    else:
        qbuf[rows] = rnd(q).reshape(M, -1)[rows]
    if mut == "padded_row_written" and M % 256:
        qbuf[M] = qbuf[M - 1]
    seq, pos = token_rows(inp["seq_len"], inp["seq_pos"])
    kpos = np.minimum(pos + 1, inp["max_seq"] - 1) if mut == "k_row_at_pos_plus_one" else pos
    tseq = (seq + 1) % len(inp["seq_len"]) if mut == "other_sequences_table_row" else seq
    kp[inp["table"][tseq, kpos // BLOCK][rows], :, (kpos % BLOCK)[rows], :] = kq[rows]
    vp[inp["table"][tseq, pos // BLOCK][rows], :, (pos % BLOCK)[rows], :] = vq[rows]
    out.update(q=qbuf, k_pool=kp, v_pool=vp)
    return out
