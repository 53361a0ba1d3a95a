"""Sliding window without a GPU: the ABI additions, the refusals answered before a device is looked for, and
the config reading — model_type "mistral" / "MistralForCausalLM" selects the Llama template and "sliding_window" is read (null
or absent: 0) by nvl_load_config_json / nvl_load_config_window and by their Python mirror config.load_model_config alike."""
import ctypes as C
import json

import pytest

SYMBOLS = ("nvl_set_sliding_window", "nvl_get_sliding_window", "nvl_load_config_window", "nvl_op_attention_batch_window")
MISTRAL = dict(vocab_size=32000, hidden_size=4096, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8,
               intermediate_size=14336, rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False)


def test_abi_and_refusals_without_a_device(pkg):
    L = pkg.lib()
    assert all(s in pkg.declared_symbols() and hasattr(L, s) for s in SYMBOLS)
    assert L.nvl_set_sliding_window(None, 4096) == -1 == L.nvl_load_config_window(None, None) and L.nvl_get_sliding_window(None) == 0


@pytest.mark.parametrize("model_type", ["mistral", "MistralForCausalLM"])
@pytest.mark.parametrize("window,want", [(4096, 4096), (None, 0), ("absent", 0)])
def test_mistral_config(pkg, tmp_path, model_type, window, want):
    L = pkg._lib
    raw = dict(MISTRAL, model_type=model_type)
    if window != "absent":
        raw["sliding_window"] = window
    p = tmp_path / "config.json"
    p.write_text(json.dumps(raw))
    got, w = L.ModelConfigC(), C.c_int(-1)
    L.check(L.lib().nvl_load_config_json(str(p).encode(), C.byref(got)))
    L.check(L.lib().nvl_load_config_window(str(p).encode(), C.byref(w)))
    mirror = pkg.config.load_model_config(raw)
    assert w.value == want == mirror.sliding_window
    assert (got.attention_type, got.norm_type, got.position_type, got.activation_type) == (L.ATTN["gqa"], L.NORM["rmsnorm"], L.POS["rope"], L.ACT["swiglu"])
    assert (mirror.architecture, mirror.attention_type, mirror.activation_type) == ("llama", "gqa", "swiglu")
    assert (got.num_kv_heads, got.head_dim, got.ffn_dim, got.max_seq_len) == (8, 128, 14336, 4096) == \
        (mirror.num_kv_heads, mirror.head_dim, mirror.ffn_dim, mirror.max_seq_len)
    p.write_text('{"sliding_window": -3}')
    assert L.lib().nvl_load_config_window(str(p).encode(), C.byref(w)) == -1 == L.lib().nvl_load_config_window(b"/nonexistent.json", C.byref(w))
