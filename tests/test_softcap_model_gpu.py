"""Attention logit soft-capping at model level: test_sliding_window_model_gpu.py's comparisons and constants
on its tiny Llama with attn_logit_softcap= on every route that ends in attention(); then the cap with sliding_window=100, a
head_dim 256 model, and a head_dim 128 QK-norm model, which must decode on the unfused form under a cap.
CAP: the largest of 4.0, 1.0, 0.25 at which the f32 capped and uncapped tiny Llama differ by more than 10 x TOL["f32"] = 1e-3.  Measured
rel_err, f32, last rows of the 150-token prompt: cap 4.0 4.5e-2, 1.0 3.8e-1, 0.25 7.1e-1 (hd 256 model 5.8e-1 at 4.0, QK-norm model 1.7e-1)."""
import numpy as np
import pytest

from block_manager_mirror import BlockManager
from conftest import rel_err
from test_sliding_window_model_gpu import BS, STEPS, TOL, stepwise

pytestmark = pytest.mark.gpu

CAP, PROMPT = 4.0, 150
MODELS = {"llama": dict(max_seq_len=256), "hd256": dict(head_dim=256, hidden=512, num_heads=2, num_kv_heads=1, ffn_dim=512),
          "qknorm": dict(hidden=128, ffn_dim=256, vocab_size=256, num_heads=4, num_kv_heads=2, head_dim=128, qk_norm=True)}
CASES = [("llama", "f32", {}, TOL["f32"]), ("llama", "bf16", {}, TOL["bf16"]), ("llama", "bf16", dict(kv_cache_dtype="fp8_e4m3"), 1e-1),      # (FP8_KV_TOL of test_kv_fp8_model_gpu.py)
         ("llama", "bf16", dict(sliding_window=100), TOL["bf16"]), ("hd256", "bf16", {}, TOL["bf16"]), ("qknorm", "bf16", {}, TOL["bf16"])]


def build(gpu, model, precision, cap, **kw):
    cfg = gpu.synth.tiny_config("llama", **MODELS[model])
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
    return cfg, gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=2, max_batch_tokens=256, attn_logit_softcap=cap, **kw)


@pytest.mark.parametrize("model,precision,kw,tol", CASES)
def test_routes_agree_under_a_cap(gpu, model, precision, kw, tol):
    cfg, hm = build(gpu, model, precision, CAP, **kw)
    prompt = np.random.default_rng(6).integers(0, cfg["vocab_size"], PROMPT).tolist()
    hm.seq_reset(0)
    rows, ids = stepwise(lambda t, p: hm.forward_batch([0], t, p), prompt)
    if model == "qknorm":       # no SOFTCAP x QKNORM kernel: norm + RoPE launch, then the plain capped decode kernel
        assert hm.attention_ran()[0] == "decode", hm.attention_ran()
    hm.seq_reset(1)
    whole = hm.forward_batch([1], [prompt + ids[:-1]], [0], all_logits=True)[0][PROMPT - 1:]
    assert rel_err(whole, rows) <= tol
    # the uncapped model answers something else (beyond what f32 rounding explains); the capped f32 model the same
    for other, cap, same in ((precision, 0.0, False), ("f32", CAP, True)):
        _, om = build(gpu, model, other, cap, **(kw if other == precision else {k: v for k, v in kw.items() if k == "sliding_window"}))
        om.seq_reset(1)
        err = rel_err(whole, om.forward_batch([1], [prompt + ids[:-1]], [0], all_logits=True)[0][PROMPT - 1:])
        assert err <= tol if same else err > TOL["f32"], (other, cap, err)
        om.close()
    hm.seq_reset(1)
    _, first = hm.forward_batch([1], [prompt], [0], want_logits=False)
    assert int(first[0]) == ids[0] and hm.decode_greedy([1], first, STEPS)[:, 0].tolist() == ids[1:]
    hm.seq_reset(1)
    hm.forward_batch([1], [prompt], [0], want_logits=False)
    acc, _ = hm.verify_greedy([1], [ids[:4]], 3)
    lp = hm.logprobs(ids[1:5])[0].astype(np.float64)
    x = rows[1:5].astype(np.float64) - rows[1:5].max(-1, keepdims=True)          # (row j of the pass = the step that fed ids[j])
    want = (x - np.log(np.exp(x).sum(-1, keepdims=True)))[np.arange(4), ids[1:5]]
    assert np.abs(lp - want).max() <= 2 * tol * np.abs(rows[1:5]).max() and hm.seq_len(1) == PROMPT + int(acc[0]) + 1
    _, paged = build(gpu, model, precision, CAP, kv_num_blocks=8, kv_block_size=BS, **kw)
    bm, seq = BlockManager(8, BS), gpu.Sequence(seq_id=0, token_ids=list(prompt), block_size=BS)
    bm.free = list(np.random.default_rng(7).permutation(8))
    bm.allocate(seq)
    def forward_paged(t, p):
        if p[0]:
            seq.append_token(t[0][0]); bm.may_append(seq)
        return paged.forward_paged(t, p, [seq.block_table])
    assert np.array_equal(stepwise(forward_paged, prompt)[0], rows)
    paged.close(); hm.close()


def test_setter(gpu):
    cfg = gpu.synth.tiny_config("llama")
    hm = gpu.HipTransformerModel(cfg, None)                      # (finalize deferred)
    put, get = hm.lib.nvl_set_attn_softcap, hm.lib.nvl_get_attn_softcap
    assert [put(hm.h, bad) for bad in (-1.0, float("nan"), float("inf"))] == [-1] * 3 and get(hm.h) == 0.0     # NVL_ERR_INVALID
    assert put(hm.h, 50.0) == 0 and get(hm.h) == 50.0
    for (slot, layer), arr in gpu.synth.make_weights(cfg, seed=7, scale=0.05).items():
        hm.upload(slot, layer, arr)
    hm.finalize()
    assert put(hm.h, 30.0) == -7 and get(hm.h) == 50.0       # NVL_ERR_STATE
    hm.close()
