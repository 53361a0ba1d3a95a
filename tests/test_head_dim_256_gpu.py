"""A model with head_dim 256, after test_model_gpu.py::test_head_dim_128 and at its TOL: Gemma's head
geometry on a small Llama-path model (hidden 512, 2 heads over 1 kv head).  Prefill (the store form + rope_kv_kernel /
qk_norm_rope_kv_kernel + attn256_prefill_kernel), the KV contents, three decode steps (attn256_decode_kernel), in f32 and
bf16, with and without the per-head QK RMSNorm.  The reference is the oracle; with QK-norm, which the oracle does not have,
test_qk_norm_model_gpu.py's float64 model (logits only).  Then graph replay: decode_greedy against the same steps one by one."""
import numpy as np
import pytest

from conftest import rel_err
from test_model_gpu import TOL
from test_qk_norm_model_gpu import model64

pytestmark = pytest.mark.gpu


def config(gpu, **over):
    return gpu.synth.tiny_config("llama", head_dim=256, hidden=512, num_heads=2, num_kv_heads=1, ffn_dim=512, **over)


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("ntok", [29, 150])
def test_head_dim_256(gpu, oracle, precision, ntok, qk_norm):
    cfg = config(gpu, qk_norm=True) if qk_norm else config(gpu)
    w = gpu.synth.make_weights(cfg, seed=13, scale=0.05)
    hm = gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=2, max_batch_tokens=256)
    r = np.random.default_rng(8)
    toks = r.integers(0, cfg["vocab_size"], ntok).tolist()
    if qk_norm:
        forward = lambda new, pos: model64(cfg, w, toks[:pos] + new)[pos:]
    else:
        om = oracle.OracleModel(cfg, w)
        kv = om.new_cache()
        forward = lambda new, pos: om.forward_with_cache(new, kv, pos)
    want = forward(toks, 0)
    got = hm.forward_with_cache(toks, seq_id=1, pos_offset=0)
    assert rel_err(got, want) <= TOL[precision]
    if precision == "bf16":
        assert hm.attention_ran()[0] == "prefill_hd256", hm.attention_ran()
    for li in range(0 if qk_norm else cfg["num_layers"]):
        k_ref, v_ref = kv.layer(li, 1, 256)
        k_dev, v_dev = hm.get_kv(1, li)
        assert rel_err(k_dev, k_ref) <= TOL[precision] and rel_err(v_dev, v_ref) <= TOL[precision]
    for t in r.integers(0, cfg["vocab_size"], 3).tolist():
        want = forward([t], len(toks))[-1]
        got = hm.forward_with_cache([t], seq_id=1, pos_offset=len(toks), all_logits=False)[-1]
        assert rel_err(got, want) <= TOL[precision]
        toks.append(t)
    if precision == "bf16":
        assert hm.attention_ran()[0] == "decode_hd256", hm.attention_ran()
    hm.close()


def test_decode_greedy_equals_stepwise(gpu):
    """nvl_decode_greedy (graph replay) == the same four steps through forward_batch, bit for bit, on a ragged batch"""
    cfg = config(gpu)
    hm = gpu.HipTransformerModel(cfg, gpu.synth.make_weights(cfg, seed=13, scale=0.05), precision="bf16", max_seqs=2, max_batch_tokens=256)
    r = np.random.default_rng(11)
    prompts, ids, steps = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (70, 9)], [0, 1], 4
    want = []
    for stepwise in (True, False):
        for i in ids:
            hm.seq_reset(i)
        _, cur = hm.forward_batch(ids, prompts, [0, 0], want_logits=False)
        if not stepwise:
            assert (hm.decode_greedy(ids, cur, steps) == np.stack(want)).all()
            break
        for s in range(steps):
            _, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [len(p) + s for p in prompts], want_logits=False)
            want.append(cur.copy())
    hm.close()
