"""The fused decode step of a QK-norm layer: attn_decode_bf16_kernel<128, .., QKNORM> and its WINDOW
instance through ops.attention_batch(form="fused", q_norm_w=, k_norm_w=) against tests/attention_reference.py's float64
attention, fed the Q rows and the new K row that float64 QK-norm + RoPE produce.  Contexts 1 / 63 / 130: an empty cache before
the new key, a tile edge, three tiles.  The inputs of test_qk_norm_ops_gpu.py: q_norm_w != k_norm_w, w[d] != w[d + hd/2], row r
scaled by 2^((r mod 7) - 3), row 1's Q and K scaled down to mean(x^2) ~ 1.6 eps.  Bounds: (a), (b) and the appended rows as
test_attention_ops_gpu.py / test_attention_window_gpu.py hold the fused form to them (the norm's fp32 terms, (hd / 2 + 5) 2^-24
relative, lie far below the 2^-9 rounding of Q and K); the draw rule of attention_reference.batch()."""
import numpy as np
import pytest

import attention_reference as R
from test_attention_window_gpu import check
from test_qk_norm_ops_gpu import EPS, qk_norm64

pytestmark = pytest.mark.gpu
HD, BS, POS, STRIDE = 128, 64, (0, 62, 129), 3
_B = {}


def batch(nH, nKV):
    if (nH, nKV) in _B:
        return _B[nH, nKV]
    ramp = np.linspace(-0.4, 0.4, HD)
    for attempt in range(16):
        r = np.random.default_rng([nH, nKV, attempt])
        wq, wk = (1.0 + ramp + 0.1 * r.standard_normal(HD)).astype(np.float32), (1.3 - ramp + 0.1 * r.standard_normal(HD)).astype(np.float32)
        ids = r.permutation(3 * STRIDE + 1)
        table = ids[1:].reshape(3, STRIDE).astype(np.int32)
        k_pool = R.bf16(r.uniform(-R.GARBAGE_K, R.GARBAGE_K, (len(ids), nKV, BS, HD)).astype(np.float32)).astype(np.float32)
        v_pool = np.full(k_pool.shape, R.GARBAGE_V, np.float32)
        b = dict(name=f"qkn{nH}x{nKV}", form="fused", nH=nH, nKV=nKV, hd=HD, block=BS, scale=HD ** -0.5, seq_len=[1, 1, 1], seq_pos=list(POS),
                 rope_base=R.ROPE_BASE, max_seq=STRIDE * BS, table=table, q_norm_w=wq, k_norm_w=wk, K=[], V=[], q_ref=[], new_rows=[], rows=[])
        for i, pos in enumerate(POS):
            K, V = R._exact(r, (nKV, pos + 1, HD)).astype(np.float64), R._exact(r, (nKV, pos + 1, HD)).astype(np.float64)
            s = np.sqrt(1.6 * EPS) if i == 1 else 2.0 ** ((i % 7) - 3)
            q, k = (s * r.standard_normal((nH, HD))).astype(np.float32),(s * r.standard_normal((nKV, HD))).astype(np.float32)
            b["rows"].append(np.concatenate([q.ravel(), k.ravel(), V[:, pos].ravel()]))
            b["q_ref"].append(R.bf16(R.rope_f64(qk_norm64(q, wq), pos, R.ROPE_BASE, b["max_seq"]))[None])
            K[:, pos] = R.bf16(R.rope_f64(qk_norm64(k, wk), pos, R.ROPE_BASE, b["max_seq"]))
            for t in range(pos):
                k_pool[table[i, t // BS], :, t % BS], v_pool[table[i, t // BS], :, t % BS] = K[:, t], V[:, t]
            b["new_rows"].append((int(table[i, pos // BS]), pos % BS))
            b["K"].append(K); b["V"].append(V)
        b.update(q=np.stack(b["rows"]).astype(np.float32), k_pool=k_pool, v_pool=v_pool, k_pool_after=k_pool.copy(), v_pool_after=v_pool.copy())
        for i, (blk, row) in enumerate(b["new_rows"]):
            b["k_pool_after"][blk, :, row], b["v_pool_after"][blk, :, row] = b["K"][i][:, POS[i]], b["V"][i][:, POS[i]]
        refs = [R.attend(b["q_ref"][i], b["K"][i], b["V"][i], POS[i], b["scale"]) for i in range(3)]
        if max(float((np.abs(f[e] - f["ref"]) / (1.05 * f["bound"] + 1e-6 * np.abs(f["ref"]).max())).max())
               for f in refs for e in ("emu_rounded", "emu_unrounded")) <= R.HEADROOM:
            break
    else:
        raise AssertionError("no draw within the element bound")
    return _B.setdefault((nH, nKV), b)


@pytest.mark.parametrize("window", [0, 64])
@pytest.mark.parametrize("nH,nKV", [(4, 2), (8, 1)])
def test_fused_decode_qk_norm(gpu, nH, nKV, window):
    b = batch(nH, nKV)
    small = (b["q"][1, :nH * HD].reshape(nH, HD).astype(np.float64) ** 2).mean(-1)
    assert (small < 4 * EPS).all() and (small > EPS / 4).all(), small
    res = gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], nH, form="fused", rope_base=b["rope_base"],
                                  max_seq=b["max_seq"], window=window, q_norm_w=b["q_norm_w"], k_norm_w=b["k_norm_w"], norm_eps=EPS)
    assert res["ran"] == "decode_fused", res["ran"]
    check(b, res, window or 1 << 30, f"{b['name']} W={window}")
    R.check_append(b, res)
