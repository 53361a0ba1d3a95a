"""Per-head QK RMSNorm without a GPU: the two kinds sit directly before NVL_T_COUNT and move no older kind;
a tiny Qwen3 checkpoint (make_checkpoint.py's Llama layout + q_norm.weight / k_norm.weight per layer, model_type "qwen3", an
explicit head_dim) selects the Llama template in nvl_load_config_json and its Python mirror.  The loader reads tensors into a
device model only (as tests/test_loader_gpu.py does): test_qk_norm_model_gpu.py loads this checkpoint and reads both vectors back."""
import ctypes as C
import json
import re

import numpy as np


def qwen3_checkpoint(path, cfg, w):
    import make_checkpoint as mc
    import torch
    from safetensors.torch import save_file
    mc.write_checkpoint(path, cfg, w, "llama", dtype="f32")
    named = mc.to_hf_names(cfg, w, "llama")
    for l in range(cfg["num_layers"]):
        for n in "qk":
            named[f"model.layers.{l}.self_attn.{n}_norm.weight"] = w[(n + "_norm_w", l)]
    save_file({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in named.items()}, str(path / "model.safetensors"), metadata={"format": "pt"})
    (path / "config.json").write_text(json.dumps(dict(mc.HF_CONFIG["llama"](cfg), model_type="qwen3")))
    return path


def test_kinds_and_qwen3_config(pkg, tmp_path):
    L = pkg._lib
    text = re.sub(r"/\*.*?\*/", "", L.HEADER.read_text(), flags=re.S)
    kinds = re.findall(r"\b(NVL_T_[A-Z0-9_]+)\b", re.search(r"typedef enum nvl_tensor_kind \{(.*?)\} nvl_tensor_kind;", text, re.S).group(1))
    assert kinds[-3:] == ["NVL_T_Q_NORM_W", "NVL_T_K_NORM_W", "NVL_T_COUNT"] and [k[6:].lower() for k in kinds[:33]] == L.SLOTS
    assert (L.SLOT_ID["q_norm_w"], L.SLOT_ID["k_norm_w"], L.T_COUNT) == (33, 34, 35) and pkg.lib().nvl_abi_version() == 3
    cfg = pkg.synth.tiny_config("llama", hidden=128, ffn_dim=256, vocab_size=256, num_heads=4, num_kv_heads=2, head_dim=128, qk_norm=True)
    path = qwen3_checkpoint(tmp_path / "qwen3", cfg, pkg.synth.make_weights(cfg, seed=11, scale=0.05))
    raw = json.loads((path / "config.json").read_text())
    got, mirror = L.ModelConfigC(), pkg.config.load_model_config(raw)
    L.check(L.lib().nvl_load_config_json(str(path / "config.json").encode(), C.byref(got)))
    assert raw["model_type"] == "qwen3" and raw["head_dim"] == 128 and raw["hidden_size"] == 128
    assert (got.attention_type, got.activation_type, got.hidden, got.num_heads, got.head_dim) == (L.ATTN["gqa"], L.ACT["swiglu"], 128, 4, 128)
    assert (mirror.architecture, mirror.hidden, mirror.num_heads, mirror.head_dim) == ("llama", 128, 4, 128)
