"""head_dim 256, the parts that need no GPU: what nvl_create and nvl_op_attention_batch accept and refuse,
decided before the device probe (NVL_ERR_INVALID -1; past it a machine without a GPU answers NVL_ERR_NO_DEVICE -8)."""
import ctypes as C

import numpy as np
import pytest

INVALID, PAST_VALIDATION = -1, (0, -8)


def create(pkg, head_dim, kv_cache_dtype=0):
    L = pkg._lib
    cfg = L.ModelConfigC()
    cfg.vocab_size, cfg.hidden, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads = 256, 512, 2, 2, 1
    cfg.head_dim, cfg.ffn_dim, cfg.max_seq_len = head_dim, 512, 128
    cfg.attention_type, cfg.norm_type, cfg.position_type = L.ATTN["gqa"], L.NORM["rmsnorm"], L.POS["rope"]
    cfg.activation_type, cfg.rope_base, cfg.norm_eps = L.ACT["swiglu"], 10000.0, 1e-5
    opts = L.RuntimeOptsC()
    opts.device, opts.precision, opts.max_seqs, opts.max_batch_tokens = 0, 0, 2, 64
    opts.kv_cache_dtype = kv_cache_dtype
    h = C.c_void_p()
    rc = L.lib().nvl_create(C.byref(cfg), C.byref(opts), C.byref(h))
    if rc == 0:
        L.lib().nvl_destroy(h)
    return rc, L.lib().nvl_last_error(None).decode()


@pytest.mark.parametrize("head_dim,kv_cache_dtype,want", [(256, 0, PAST_VALIDATION), (256, 1, (INVALID,)), (96, 0, (INVALID,))])
def test_create(pkg, head_dim, kv_cache_dtype, want):
    rc, msg = create(pkg, head_dim, kv_cache_dtype)
    assert rc in want, (rc, msg)
    if rc == INVALID:
        assert ("head_dim 256" if head_dim == 256 else "head_dim must be") in msg, msg


@pytest.mark.parametrize("form,want", [("plain", PAST_VALIDATION), ("mq", PAST_VALIDATION), ("fused", (INVALID,)), ("kv8", (INVALID,))])
def test_attention_batch_forms(pkg, form, want):
    nH, nKV, hd, bs = 8, 2, 256, 64
    pool = np.zeros((3, nKV, bs, hd), np.float32)
    fused, n = form == "fused", 1 if form != "mq" else 2
    q = np.zeros((2, (nH + 2 * nKV) * hd) if fused else (2 * n, nH, hd), np.float32)
    try:
        pkg.ops.attention_batch(q, pool, pool, [[0, 1], [2, 2]], [n, n], [70, 3], nH, form=form)
        rc = 0
    except pkg.NvlError as e:
        rc = e.code
    assert rc in want, (form, rc)
