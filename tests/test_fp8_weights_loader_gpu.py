"""FP8 checkpoints through nvl_load_safetensors: F8_E4M3 "<name>.weight" with a per-channel ([N] / [N,1])
or scalar "<name>.weight_scale" (F32 or BF16), "input_scale" ignored.  Loaded into an 8-bit-weight model the codes and
scales are taken as they are; into a bf16 model the weights become W~ = bf16(s * e4m3(q)).  Block-wise scales and NaN codes
are refused, as nvl_upload_tensor_fp8 refuses NaN codes."""
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from conftest import rel_err
from make_checkpoint import HF_CONFIG, to_hf_names
from test_fp8_weights_gpu import bf16_rne, ref_w8
from test_kv_fp8_gpu import VALUES, ref_quant

pytestmark = pytest.mark.gpu
PROJ = (".q_proj.weight", ".k_proj.weight", ".v_proj.weight", ".o_proj.weight", ".gate_proj.weight", ".up_proj.weight",
        ".down_proj.weight", "lm_head.weight")


def write_fp8(dirname, cfg, w, scale_form="row", poison=None):
    """Llama checkpoint whose projections are F8_E4M3 (quantized per row by the contract of DESIGN.md §3).
    -> {hf name: W~ [out, in]} of every 8-bit tensor.  scale_form: "row" ([N] F32 / [N,1] BF16 alternating), "scalar",
    "block" (a [N/16, K/16] scale: refused)."""
    os.makedirs(dirname, exist_ok=True)
    named = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in to_hf_names(cfg, w, "llama").items()}
    tilde, i = {}, 0
    for name in list(named):
        if not name.endswith(PROJ):
            continue
        a = named[name].numpy()                                   # [out, in]
        if scale_form == "scalar":
            s = np.float32(np.abs(a).max() / np.float32(448))
            codes, scales = ref_quant(a, s), np.full(a.shape[0], s, np.float32)
            st = torch.tensor(s, dtype=torch.float32)
        else:
            codes, scales, _ = ref_w8(a)
            st = torch.from_numpy(scales) if i % 2 == 0 else torch.from_numpy(scales[:, None]).to(torch.bfloat16)
            if i % 2:
                scales = st.float().numpy()[:, 0]
            if scale_form == "block":
                st = torch.ones(a.shape[0] // 16, a.shape[1] // 16)
        if poison == name:
            codes = codes.copy()
            codes[1, 2] = 0x7F
        named[name] = torch.from_numpy(codes).view(torch.float8_e4m3fn)
        named[name + "_scale"] = st
        named[name.replace(".weight", ".input_scale")] = torch.tensor(3.0)        # ignored
        tilde[name] = bf16_rne(VALUES[codes].astype(np.float32) * scales[:, None])
        i += 1
    with open(os.path.join(dirname, "config.json"), "w") as f:
        json.dump(HF_CONFIG["llama"](cfg), f)
    save_file({k: v.contiguous() for k, v in named.items()}, os.path.join(dirname, "model.safetensors"), metadata={"format": "pt"})
    return tilde


def read_back(gpu, hm, cfg, li):
    from test_fp8_weights_gpu import get_weight
    H, q, kv, F = cfg["hidden"], cfg["num_heads"] * cfg["head_dim"], cfg["num_kv_heads"] * cfg["head_dim"], cfg["ffn_dim"]
    return {f"model.layers.{li}.self_attn.o_proj.weight": get_weight(gpu, hm, "wo", li, q, H).T,
            f"model.layers.{li}.mlp.down_proj.weight": get_weight(gpu, hm, "w2", li, F, H).T}


@pytest.mark.parametrize("scale_form", ["row", "scalar"])
def test_fp8_checkpoint_into_fp8_and_bf16_models(gpu, tmp_path, scale_form):
    cfg = gpu.synth.tiny_config("llama", tied_embedding=False)     # untied: the embedding is bf16 in both models
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    tilde = write_fp8(str(tmp_path), cfg, w, scale_form)
    prompt = np.random.default_rng(0).integers(0, cfg["vocab_size"], 40).tolist()
    out = {}
    for wd in ("fp8_e4m3", "auto"):
        # read back before finalize (O / down stay separate kinds): exactly s * e4m3(code) rounded to bf16
        m = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, weight_dtype=wd)
        gpu._lib.check(m.lib.nvl_load_safetensors(m.h, str(tmp_path).encode()), m.h)
        for li in range(cfg["num_layers"]):
            for name, got in read_back(gpu, m, cfg, li).items():
                assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(tilde[name]).view(np.uint32)), (wd, name)
        m.close()
        hm = gpu.HipTransformerModel.from_pretrained(str(tmp_path), precision="bf16", max_seqs=2, max_batch_tokens=128,
                                                     weight_dtype=wd)
        out[wd] = hm.forward_with_cache(prompt, 0, 0, all_logits=True)
        hm.close()
    assert rel_err(out["fp8_e4m3"], out["auto"]) <= 1.5e-2


def test_block_scales_and_nan_codes_are_refused(gpu, tmp_path):
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    write_fp8(str(tmp_path / "block"), cfg, w, "block")
    write_fp8(str(tmp_path / "nan"), cfg, w, "row", poison="model.layers.0.self_attn.o_proj.weight")
    for sub, needle in (("block", "block-wise"), ("nan", "NaN")):
        for wd in ("fp8_e4m3", "auto"):
            with pytest.raises(gpu.NvlError) as e:
                gpu.HipTransformerModel.from_pretrained(str(tmp_path / sub), precision="bf16", max_seqs=2, max_batch_tokens=128,
                                                        weight_dtype=wd)
            assert e.value.code == -1 and needle in str(e.value), (sub, wd, str(e.value))


def test_upload_tensor_fp8(gpu):
    import ctypes as C
    from test_fp8_weights_gpu import get_weight
    cfg = gpu.synth.tiny_config("llama")
    H, q = cfg["hidden"], cfg["num_heads"] * cfg["head_dim"]
    rng = np.random.default_rng(2)
    codes = rng.integers(0, 256, (H, q)).astype(np.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x10
    scales = rng.uniform(0.01, 2.0, H).astype(np.float32)
    m = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3")
    kind = gpu._lib.SLOT_ID["wo"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert m.lib.nvl_upload_tensor_fp8(m.h, kind, 0, p(codes), p(scales), H, q, gpu._lib.LAYOUT_OUT_IN) == 0
    want = bf16_rne(VALUES[codes].astype(np.float32) * scales[:, None])
    assert np.array_equal(get_weight(gpu, m, "wo", 0, q, H).T.view(np.uint32), want.view(np.uint32))
    bad = codes.copy()
    bad[3, 3] = 0xFF
    assert m.lib.nvl_upload_tensor_fp8(m.h, kind, 0, p(bad), p(scales), H, q, gpu._lib.LAYOUT_OUT_IN) == -1
    assert m.lib.nvl_upload_tensor_fp8(m.h, gpu._lib.SLOT_ID["router"], 0, p(codes), p(scales), H, q, gpu._lib.LAYOUT_OUT_IN) == -1
    m.close()
    mb = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64)      # a bf16 model: refused
    assert mb.lib.nvl_upload_tensor_fp8(mb.h, kind, 0, p(codes), p(scales), H, q, gpu._lib.LAYOUT_OUT_IN) == -1
    mb.close()
