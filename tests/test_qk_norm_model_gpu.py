"""Per-head QK RMSNorm at model level: a synthetic 2-layer Qwen3-shaped model (hidden 128, nH, nKV = 4, 2,
head_dim 128 and 64).  model64(): the model in float64 numpy; a ragged 3-sequence prefill's all-rows logits against it at
test_model_gpu.py's TOL (f32: store form; bf16: the tile epilogue) and, with 8-bit QKV weights, on W~ at test_fp8_weights_gpu.py's
BF16_TOL / test_w8a8_gpu.py's w8a8_tol (the epilogue variant behind the dequantize step; W8A8: the store form).  Prefill, stepwise
decode and a verify_greedy pass agree (slab, bf16 8-bit cache; paged bit-equal to slab) at test_sliding_window_model_gpu.py's MODES
tolerances; hd 128 decodes on the fused kernel, hd 64 on the plain one.  The loader finds both vectors.  Refusals."""
import ctypes as C

import numpy as np
import pytest

import attention_reference as A
from block_manager_mirror import BlockManager
from conftest import rel_err
from test_fp8_weights_gpu import BF16_TOL, tilde
from test_moe_ops_gpu import Tuning
from test_qk_norm_host import qwen3_checkpoint
from test_qk_norm_ops_gpu import qk_norm64
from test_sliding_window_model_gpu import MODES, TOL
from test_w8a8_gpu import w8a8_tol

pytestmark = pytest.mark.gpu
PROMPT, STEPS = 70, 6
FP8 = dict(weight_dtype="fp8_e4m3")


def build(gpu, hd, precision=None, **kw):
    cfg = gpu.synth.tiny_config("llama", hidden=128, ffn_dim=256, vocab_size=256, num_heads=4, num_kv_heads=2, head_dim=hd,
                                 max_seq_len=256, norm_eps=1e-5, qk_norm=True)
    w = gpu.synth.make_weights(cfg, seed=11, scale=0.05)
    return cfg, w, gpu.HipTransformerModel(cfg, w if precision else None, precision=precision or "bf16", max_seqs=3, max_batch_tokens=256, **kw)


def model64(cfg, w, toks):       # one sequence from position 0 -> logits [len][V]
    f = lambda slot, l=0: np.asarray(w[(slot, l)], np.float64)
    rms = lambda x, g: x / np.sqrt((x * x).mean(-1, keepdims=True) + cfg["norm_eps"]) * g
    hd, F, T = cfg["head_dim"], cfg["ffn_dim"], len(toks)
    rope = lambda t: A.rope_f64(t, np.arange(T)[:, None], cfg["rope_base"], cfg["max_seq_len"])
    x = f("tok_emb")[toks]
    for l in range(cfg["num_layers"]):
        h = rms(x, f("attn_norm_w", l))
        q, k, v = ((h @ f(s, l)).reshape(T, -1, hd) for s in ("wq", "wk", "wv"))
        q, k = rope(qk_norm64(q, f("q_norm_w", l))), rope(qk_norm64(k, f("k_norm_w", l)))
        x = x + A.attention_f64(q, k.transpose(1, 0, 2), v.transpose(1, 0, 2), 0, hd ** -0.5).reshape(T, -1) @ f("wo", l)
        a = rms(x, f("ffn_norm_w", l)) @ f("w1", l)
        x = x + (a[:, :F] / (1.0 + np.exp(-a[:, :F])) * a[:, F:]) @ f("w2", l)
    return rms(x, f("final_norm_w")) @ f("tok_emb").T


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("precision,kw", [("f32", {}), ("bf16", {}), ("bf16", FP8), ("bf16", dict(FP8, act_dtype="fp8_e4m3"))])
def test_prefill_against_float64(gpu, hd, precision, kw):
    cfg, w, hm = build(gpu, hd, precision, **kw)
    seqs = [np.random.default_rng(s).integers(0, 256, n).tolist() for s, n in ((1, 70), (2, 3), (3, 29))]
    hm.seq_reset(0); hm.seq_reset(1); hm.seq_reset(2)
    with Tuning(gpu, {18: 0}):                      # (102 rows > 64: the bf16 modes take the epilogue form, W8A8 the store form)
        got = hm.forward_batch([0, 1, 2], seqs, [0, 0, 0], all_logits=True)[0]
    want = np.concatenate([model64(cfg, tilde(cfg, w) if kw else w, s) for s in seqs])
    tol = TOL["f32"] if precision == "f32" else w8a8_tol(cfg) if "act_dtype" in kw else BF16_TOL
    print(f"hd {hd} {precision} {kw}: rel err {rel_err(got, want):.3e} (bound {tol:.3e})")
    assert rel_err(got, want) <= tol, rel_err(got, want)
    hm.close()


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("precision,kw,tol", MODES)
def test_routes_agree(gpu, hd, precision, kw, tol):
    _, _, hm = build(gpu, hd, precision, **kw)
    prompt = np.random.default_rng(6).integers(0, 256, PROMPT).tolist()

    def stepwise(forward):
        lg, am = forward([prompt], [0])
        rows, ids = [lg[0]], [int(am[0])]
        for s in range(STEPS):
            lg, am = forward([[ids[-1]]], [PROMPT + s])
            rows.append(lg[0]); ids.append(int(am[0]))
        return np.stack(rows), ids
    hm.seq_reset(0); hm.seq_reset(1)
    rows, ids = stepwise(lambda t, p: hm.forward_batch([0], t, p))
    want = "decode_kv8" if kw else ("decode_fused" if hd == 128 else "decode")
    assert precision != "bf16" or hm.attention_ran()[0] == want, (hd, hm.attention_ran())
    whole = hm.forward_batch([1], [prompt + ids[:-1]], [0], all_logits=True)[0][PROMPT - 1:]
    assert rel_err(whole, rows) <= tol, rel_err(whole, rows)
    hm.seq_reset(1)
    hm.forward_batch([1], [prompt], [0], want_logits=False)
    acc, _ = hm.verify_greedy([1], [ids[:4]], 3)
    lp = hm.logprobs(ids[1:5])[0].astype(np.float64)
    x = rows[1:5].astype(np.float64) - rows[1:5].max(-1, keepdims=True)
    ref = (x - np.log(np.exp(x).sum(-1, keepdims=True)))[np.arange(4), ids[1:5]]
    assert np.abs(lp - ref).max() <= 2 * tol * np.abs(rows[1:5]).max() and hm.seq_len(1) == PROMPT + int(acc[0]) + 1
    hm.close()
    _, _, paged = build(gpu, hd, precision, kv_num_blocks=8, kv_block_size=64, **kw)          # bit-equal to slab (test_paged_kv_gpu.py)
    bm, seq = BlockManager(8, 64), gpu.Sequence(seq_id=0, token_ids=list(prompt), block_size=64)
    bm.free = list(np.random.default_rng(7).permutation(8))
    bm.allocate(seq)

    def forward_paged(t, p):
        if p[0]:
            seq.append_token(t[0][0]); bm.may_append(seq)
        return paged.forward_paged(t, p, [seq.block_table])
    assert np.array_equal(stepwise(forward_paged)[0], rows)
    paged.close()


def test_refusals_and_plumbing(gpu, tmp_path):
    cfg, w, hm = build(gpu, 128)
    assert not np.array_equal(w[("q_norm_w", 0)], w[("k_norm_w", 0)]) and np.ptp(w[("q_norm_w", 0)]) > 0.5
    gpu._lib.check(hm.lib.nvl_load_safetensors(hm.h, str(qwen3_checkpoint(tmp_path / "qwen3", cfg, w)).encode()), hm.h)
    out = np.zeros(128, np.float32)
    for slot, layer in ((s, l) for s in ("q_norm_w", "k_norm_w") for l in (0, 1)):       # the loader found both, in every layer
        gpu._lib.check(hm.lib.nvl_get_weight(hm.h, gpu._lib.SLOT_ID[slot], layer, out.ctypes.data_as(C.c_void_p), 128, 1), hm.h)
        assert np.array_equal(out, w[(slot, layer)]), (slot, layer)
    hm.close()
    _, _, hm = build(gpu, 128)
    with pytest.raises(gpu.NvlError) as e:                      # a wrong length is refused at upload
        hm.upload("q_norm_w", 0, np.ones(64, np.float32))
    assert e.value.code == -1
    for (slot, layer), arr in w.items():
        if (slot, layer) != ("k_norm_w", 1):
            hm.upload(slot, layer, arr)
    with pytest.raises(gpu.NvlError) as e:                      # layer 1 has only Q_NORM_W
        hm.finalize()
    assert e.value.code == -7
    hm.close()
