"""nvl_load_safetensors on AWQ- and GPTQ-layout checkpoints: synthetic Llama checkpoints whose projections
are .qweight / .qzeros / .scales packed here from the numpy mirror's (q, s, z); the loaded weights are W~ bit for bit, the
logits those of a model fed the same arrays through upload_int4, and the loader's refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from make_checkpoint import HF_CONFIG, to_hf_names
from test_int4_weights_gpu import QUANTIZED, get_weight, ref_gq
from test_int4_weights_host import pack_awq, pack_gptq

pytestmark = pytest.mark.gpu
G = 128
PROJ = (".q_proj", ".k_proj", ".v_proj", ".o_proj", ".gate_proj", ".up_proj", ".down_proj")


def unpack_codes(packed):
    q = np.empty((packed.shape[0], packed.shape[1] * 2), np.uint8)
    q[:, 0::2], q[:, 1::2] = packed & 15, packed >> 4
    return q


def write_int4_checkpoint(dirname, cfg, w, layout, g=G, act_order=False):
    """every Llama projection as qweight / qzeros / scales in `layout`; the rest bf16.  GPTQ cannot store z = 0 (it keeps
    z - 1): the weights of the test are shifted per group so that every zero point is at least 1 (see shifted())."""
    os.makedirs(dirname, exist_ok=True)
    named = {}
    for name, a in to_hf_names(cfg, w, "llama").items():
        base = name[:-len(".weight")] if name.endswith(".weight") else name
        if base.endswith(PROJ):                              # [out, in]
            codes, s, z, _ = ref_gq(a, g)
            qw, qz, sc = (pack_awq if layout == "awq" else pack_gptq)(unpack_codes(codes), z, s)
            named[base + ".qweight"] = torch.from_numpy(qw.view(np.int32).copy())
            named[base + ".qzeros"] = torch.from_numpy(qz.view(np.int32).copy())
            named[base + ".scales"] = torch.from_numpy(sc.copy())
            if layout == "gptq":
                idx = np.arange(a.shape[1], dtype=np.int32) // g
                if act_order:
                    idx[[1, a.shape[1] - 1]] = idx[[a.shape[1] - 1, 1]]
                named[base + ".g_idx"] = torch.from_numpy(idx)
        else:
            named[name] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).contiguous()
    with open(os.path.join(dirname, "config.json"), "w") as f:
        json.dump(HF_CONFIG["llama"](cfg), f)
    save_file(named, os.path.join(dirname, "model.safetensors"), metadata={"format": "pt"})
    return str(dirname)


def shifted(w, g=G):
    """the synthetic weights with every group of a projection holding a clearly negative value, so that no zero point is 0"""
    out = {}
    for (slot, li), a in w.items():
        a = np.array(a, np.float32)
        if slot in QUANTIZED:
            a[0::g, :] = -np.abs(a[0::g, :]) - 0.05          # [in, out]: the first input feature of every group
        out[(slot, li)] = a
    return out


@pytest.fixture(scope="module")
def model_weights(gpu):
    cfg = gpu.synth.tiny_config("llama")
    return cfg, shifted(gpu.synth.make_weights(cfg, seed=4, scale=0.05))


def new_model(gpu, cfg, **kw):
    return gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, **kw)


@pytest.mark.parametrize("layout", ["awq", "gptq"])
def test_load_int4_checkpoint(gpu, tmp_path, model_weights, layout):
    cfg, w = model_weights
    path = write_int4_checkpoint(tmp_path / layout, cfg, w, layout)
    a = new_model(gpu, cfg, gq_weight_dtype="uint4", gq_group_size=G)
    gpu._lib.check(a.lib.nvl_load_safetensors(a.h, path.encode()), a.h)
    b = new_model(gpu, cfg, gq_weight_dtype="uint4", gq_group_size=G)
    checked = 0
    for (slot, li), t in w.items():
        if slot in QUANTIZED:
            codes, s, z, wt = ref_gq(t.T, G)
            assert z.min() >= 1
            got = get_weight(gpu, a, slot, li, t.shape[0], t.shape[1])
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(wt.T).view(np.uint32)), (slot, li)
            b.upload_int4(slot, li, codes, s, z)
            checked += 1
        else:
            b.upload(slot, li, torch.from_numpy(np.ascontiguousarray(t)).to(torch.bfloat16))
    assert checked == 6 * cfg["num_layers"]
    a.finalize(); b.finalize()
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    prompt = np.random.default_rng(3).integers(0, cfg["vocab_size"], 40).tolist()
    assert np.array_equal(a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(3):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    a.close(); b.close()


def test_loader_refusals(gpu, tmp_path, model_weights):
    cfg, w = model_weights
    good = write_int4_checkpoint(tmp_path / "gptq", cfg, w, "gptq")
    act = write_int4_checkpoint(tmp_path / "act", cfg, w, "gptq", act_order=True)

    def refused(path, **kw):
        m = new_model(gpu, cfg, **kw)
        rc = m.lib.nvl_load_safetensors(m.h, path.encode())
        msg = m.lib.nvl_last_error(m.h).decode()
        m.close()
        assert rc < 0, path
        return msg
    assert "act-order" in refused(act, gq_weight_dtype="uint4", gq_group_size=G)
    assert "group size" in refused(good, gq_weight_dtype="uint4", gq_group_size=64)
    assert "nvl_set_gq_weight_dtype" in refused(good)
