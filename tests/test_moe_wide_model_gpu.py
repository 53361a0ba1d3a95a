"""A Llama-family MoE model with 128 experts, 8 per token, 2 layers through nvl_forward: f32 (the wide
route / hist / scan / scatter kernels) against the oracle at test_model_gpu.py's f32 tolerance; bf16 (moe_router_plan_kernel,
in eager passes and in replayed graphs) by its greedy ids; and a Qwen3-MoE checkpoint — per-expert gate / up / down tensors,
mlp.gate, q_norm / k_norm — through the loader.  The oracle has no per-head QK norm, so only the loader's model carries it."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import rel_err
from test_model_gpu import TOL
from test_moe_ops_gpu import Tuning

pytestmark = pytest.mark.gpu
WIDE = dict(use_moe=True, num_experts=128, num_experts_per_tok=8, ffn_dim=64, tied_embedding=False)


def build(gpu, oracle, precision, peaked=0.0):
    cfg = gpu.synth.tiny_config("llama", **WIDE)
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=peaked)
    return cfg, oracle.OracleModel(cfg, w), gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=4, max_batch_tokens=256)


def test_f32_prefill_and_decode_match_oracle(gpu, oracle):
    cfg, om, hm = build(gpu, oracle, "f32")
    r = np.random.default_rng(3)
    seqs = [r.integers(0, cfg["vocab_size"], 9).tolist() for _ in range(2)]
    forced = r.integers(0, cfg["vocab_size"], (3, 2)).tolist()
    kvs = [om.new_cache(), om.new_cache()]
    hm.seq_reset(0); hm.seq_reset(1)
    got = hm.forward_batch([0, 1], seqs, [0, 0], all_logits=True)[0]
    want = np.concatenate([om.forward_with_cache(s, kv, 0) for s, kv in zip(seqs, kvs)])
    assert rel_err(got, want) <= TOL["f32"], rel_err(got, want)
    for step, toks in enumerate(forced):
        got = hm.forward_batch([0, 1], [[t] for t in toks], [9 + step] * 2)[0]
        want = np.stack([om.forward_with_cache([t], kv, 9 + step)[-1] for t, kv in zip(toks, kvs)])
        assert rel_err(got, want) <= TOL["f32"], (step, rel_err(got, want))
    hm.close()


def test_bf16_greedy_ids_equal_f32(gpu, oracle):
    cfg, om, f32 = build(gpu, oracle, "f32", peaked=4.0)
    for seed in range(600):             # as test_greedy_token_ids_bit_exact: a prompt whose oracle margins exceed 2x the bf16 tolerance
        prompt = np.random.default_rng(100 + seed).integers(0, cfg["vocab_size"], 12).tolist()
        want, margins = om.greedy(prompt, 10, return_margins=True)
        if min(margins) > 2 * TOL["bf16"] and len(set(want)) > 3:
            break
    else:
        pytest.fail("no fixture prompt with safe margins")
    assert f32.greedy(prompt, 10) == want
    f32.close()
    for key31 in (2, 0):                # the one-launch decode route and the two-launch one
        with Tuning(gpu, {31: key31}):
            _, _, bf16 = build(gpu, oracle, "bf16", peaked=4.0)
            assert bf16.greedy(prompt, 10) == want, key31
            bf16.close()


def test_qwen3_moe_checkpoint_loads(gpu, tmp_path):
    import make_checkpoint as mc
    import torch
    from safetensors.torch import save_file
    L = gpu._lib
    cfg = gpu.synth.tiny_config("llama", hidden=128, vocab_size=256, num_heads=2, num_kv_heads=2, qk_norm=True, **WIDE)
    w = gpu.synth.make_weights(cfg, seed=11, scale=0.05)
    named, I = mc.to_hf_names(cfg, w, "llama"), cfg["ffn_dim"]
    for l in range(cfg["num_layers"]):
        p = f"model.layers.{l}."
        named[p + "mlp.gate.weight"] = named.pop(p + "block_sparse_moe.router.layer.weight")
        win, wout = named.pop(p + "block_sparse_moe.input_linear.weight"), named.pop(p + "block_sparse_moe.output_linear.weight")
        for e in range(cfg["num_experts"]):
            for name, a in (("gate_proj", win[e, :I]), ("up_proj", win[e, I:]), ("down_proj", wout[e])):
                named[f"{p}mlp.experts.{e}.{name}.weight"] = a
        for n in "qk":
            named[f"{p}self_attn.{n}_norm.weight"] = w[(n + "_norm_w", l)]
    tmp_path.mkdir(exist_ok=True)
    save_file({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in named.items()}, str(tmp_path / "model.safetensors"),
              metadata={"format": "pt"})
    hf = dict(mc.HF_CONFIG["llama"](cfg), model_type="qwen3_moe", num_experts=128, num_experts_per_tok=8, moe_intermediate_size=I,
              intermediate_size=4 * I, norm_topk_prob=True, decoder_sparse_step=1, mlp_only_layers=[])
    (tmp_path / "config.json").write_text(json.dumps(hf))
    got = L.ModelConfigC()
    L.check(L.lib().nvl_load_config_json(str(tmp_path / "config.json").encode(), C.byref(got)))
    assert (got.use_moe, got.num_experts, got.num_experts_per_tok, got.ffn_dim, got.hidden) == (1, 128, 8, I, 128)
    for bad in (dict(norm_topk_prob=False), dict(decoder_sparse_step=2), dict(mlp_only_layers=[0])):
        (tmp_path / "bad.json").write_text(json.dumps(dict(hf, **bad)))
        assert L.lib().nvl_load_config_json(str(tmp_path / "bad.json").encode(), C.byref(L.ModelConfigC())) == -1, bad
    toks = np.random.default_rng(5).integers(0, 256, 21).tolist()
    logits = []
    for weights in (w, None):
        hm = gpu.HipTransformerModel(cfg, weights, precision="bf16", max_seqs=1, max_batch_tokens=64)
        if weights is None:
            L.check(hm.lib.nvl_load_safetensors(hm.h, str(tmp_path).encode()), hm.h)
            hm.finalize()
        logits.append(hm.forward_with_cache(toks, seq_id=0, pos_offset=0))
        hm.close()
    assert np.isfinite(logits[0]).all() and np.array_equal(logits[0], logits[1])
