"""Sliding-window attention at model level: test_model_gpu.py's tiny Llama with sliding_window= on every
route that ends in attention().  Context <= W: bit-equal to the unwindowed model.  Context > W (W = 100, 300-token prompt, 8
steps): the logits differ from the unwindowed model and the routes agree to the constants the same comparisons use without a
window — one call / prompt + steps within TOL (test_model_gpu.py; the 8-bit cache: FP8_KV_TOL), paged bit-equal to slab
(test_paged_kv_gpu.py), decode_greedy bit-equal to the stepwise loop, a verify pass's rows within 2 x TOL x max|logit| in
log-probability (test_spec_decode_gpu.py check_rows), bf16 against f32 within TOL["bf16"]."""
import numpy as np
import pytest

from block_manager_mirror import BlockManager
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "bf16": 1.5e-2}          # tests/test_model_gpu.py
W, PROMPT, STEPS, BS = 100, 300, 8, 64
MODES = [("f32", {}, TOL["f32"]), ("bf16", {}, TOL["bf16"]), ("bf16", dict(kv_cache_dtype="fp8_e4m3"), 1e-1)]   # (FP8_KV_TOL of test_kv_fp8_model_gpu.py)


def build(gpu, precision, window, **kw):
    cfg = gpu.synth.tiny_config("llama", max_seq_len=512)
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
    return cfg, gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=2, max_batch_tokens=512, sliding_window=window, **kw)


def stepwise(forward, prompt):       # prompt, then STEPS greedy steps -> (logits [1 + STEPS, V] of the choosing rows, the ids)
    lg, am = forward([prompt], [0])
    rows, ids = [lg[0]], [int(am[0])]
    for s in range(STEPS):
        lg, am = forward([[ids[-1]]], [len(prompt) + s])
        rows.append(lg[0]); ids.append(int(am[0]))
    return np.stack(rows), ids


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_context_within_the_window_changes_no_bit(gpu, precision):
    cfg, plain = build(gpu, precision, 0)
    _, win = build(gpu, precision, 128)
    prompt = np.random.default_rng(5).integers(0, cfg["vocab_size"], 70).tolist()
    outs = []
    for hm in (plain, win):
        hm.seq_reset(0); hm.seq_reset(1)
        outs.append(stepwise(lambda t, p: hm.forward_batch([0], t, p), prompt)[0])          # contexts 70 .. 78 <= 128
        outs.append(hm.forward_batch([1], [prompt], [0], all_logits=True)[0])
        hm.close()
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[3])


@pytest.mark.parametrize("precision,kw,tol", MODES)
def test_routes_agree_beyond_the_window(gpu, precision, kw, tol):
    cfg, hm = build(gpu, precision, W, **kw)
    prompt = np.random.default_rng(6).integers(0, cfg["vocab_size"], PROMPT).tolist()
    hm.seq_reset(0)
    rows, ids = stepwise(lambda t, p: hm.forward_batch([0], t, p), prompt)
    hm.seq_reset(1)
    whole = hm.forward_batch([1], [prompt + ids[:-1]], [0], all_logits=True)[0][PROMPT - 1:]
    assert rel_err(whole, rows) <= tol
    # the unwindowed model answers something else (beyond what f32 rounding explains); the windowed f32 model the same
    for other, window, same in ((precision, 0, False), ("f32", W, True)):
        _, om = build(gpu, other, window, **(kw if other == precision else {}))
        om.seq_reset(1)
        err = rel_err(whole, om.forward_batch([1], [prompt + ids[:-1]], [0], all_logits=True)[0][PROMPT - 1:])
        assert err <= tol if same else err > TOL["f32"], (other, window, err)
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
    _, paged = build(gpu, precision, W, kv_num_blocks=8, kv_block_size=BS, **kw)
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
    lib = hm.lib
    assert lib.nvl_set_sliding_window(hm.h, -1) == -1 and lib.nvl_get_sliding_window(hm.h) == 0      # NVL_ERR_INVALID
    assert lib.nvl_set_sliding_window(hm.h, 64) == 0 and lib.nvl_get_sliding_window(hm.h) == 64
    for (slot, layer), arr in gpu.synth.make_weights(cfg, seed=7, scale=0.05).items():
        hm.upload(slot, layer, arr)
    hm.finalize()
    assert lib.nvl_set_sliding_window(hm.h, 32) == -7 and lib.nvl_get_sliding_window(hm.h) == 64     # NVL_ERR_STATE
    hm.close()
