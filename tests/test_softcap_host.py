"""Soft-capping without a GPU: the ABI additions, refusals before the device probe, the config key read alike by C and Python."""
import ctypes as C
import json

import numpy as np
import pytest

SYMBOLS = ("nvl_set_attn_softcap", "nvl_get_attn_softcap", "nvl_load_config_softcap", "nvl_op_attention_batch_softcap")
GEMMA2 = dict(model_type="llama", vocab_size=32000, hidden_size=512, num_hidden_layers=2, num_attention_heads=2, head_dim=256)


def test_abi_and_refusals_without_a_device(pkg):
    L = pkg.lib()
    assert all(s in pkg.declared_symbols() and hasattr(L, s) for s in SYMBOLS)
    assert L.nvl_set_attn_softcap(None, 50.0) == -1 == L.nvl_load_config_softcap(None, None) and L.nvl_get_attn_softcap(None) == 0.0
    # one decode row over one 64-key block: a legal batch, so only the cap can be what is refused
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pool, vpool, q, out = (np.zeros(shape, np.float32) for shape in ((1, 1, 64, 64), (1, 1, 64, 64), (1, 1, 64), (1, 1, 64)))
    one, zero, ran, cnt = np.ones(1, np.int32), np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(32, np.int32)
    args = (0, pkg._lib.PRECISION["bf16"], 0, 1, 1, 64, 0.0, 1, p(one), p(zero), p(pool), p(vpool), 1, 64, p(zero), 1, p(q), 0.0, 64,
            1.0, 1.0, p(out), p(ran), p(cnt), 0, None, None, 0.0)
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.nvl_op_attention_batch_softcap(*args, bad) == -1          # NVL_ERR_INVALID, with or without a device
    if L.nvl_device_count() < 1:
        assert L.nvl_op_attention_batch_softcap(*args, 0.0) == L.nvl_op_attention_batch_qknorm(*args) < 0


@pytest.mark.parametrize("value,want", [(50.0, 50.0), (None, 0.0), ("absent", 0.0), ("fifty", "refused")])
def test_config(pkg, tmp_path, value, want):
    raw = dict(GEMMA2) if value == "absent" else dict(GEMMA2, attn_logit_softcapping=value)
    path = tmp_path / "config.json"
    path.write_text(json.dumps(raw))
    cap = C.c_float(-1.0)
    rc = pkg.lib().nvl_load_config_softcap(str(path).encode(), C.byref(cap))
    if want == "refused":
        assert rc == -1
        with pytest.raises(ValueError):
            pkg.config.load_model_config(raw)
    else:
        assert rc == 0 and cap.value == want == pkg.config.load_model_config(raw).attn_logit_softcap
