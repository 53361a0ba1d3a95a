"""8-bit (e4m3fn) projection weights (weight_dtype="fp8_e4m3", nvl_set_weight_dtype): the upload
quantizer against a numpy restatement of the contract, the GEMM dispatch of an 8-bit weight (decode kernels, 64-row groups,
dequantize + tile) against float64 products over W~, the model against the oracle run on W~, the identities that stay
bit-exact, and the setter's errors."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from test_kv_fp8_gpu import VALUES, ref_quant

pytestmark = pytest.mark.gpu
FAMILIES = ["llama", "gpt2", "falcon", "granite_moe", "granite_hybrid"]
BF16_TOL = 1.5e-2          # bf16 logits against the oracle (test_model_gpu.py TOL["bf16"])
FP8_KV_TOL = 1e-1          # ... with the 8-bit KV cache (test_kv_fp8_model_gpu.py FP8_TOL)
QUANTIZED = {"wq", "wk", "wv", "wkv", "wo", "w1", "w2", "lm_head"}


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def ref_w8(w_out_in):
    """rows = output channels: (codes, scales, W~) of DESIGN.md §3."""
    w = np.asarray(w_out_in, np.float32)
    amax = np.abs(w).max(axis=1)
    s = np.where(amax == 0, np.float32(1), (amax / np.float32(448)).astype(np.float32)).astype(np.float32)
    codes = ref_quant(w, s[:, None])
    wt = bf16_rne(VALUES[codes].astype(np.float32) * s[:, None])
    return codes, s, wt


def tilde(cfg, w):
    """the weights the fp8 model computes with, in the oracle's layout ([in, out] except the Mamba2 projections)"""
    out = {}
    for (slot, li), a in w.items():
        quant = slot in QUANTIZED or (slot == "tok_emb" and cfg.get("tied_embedding", False))
        if not quant:
            out[(slot, li)] = a
        elif slot == "tok_emb":
            out[(slot, li)] = ref_w8(a)[2]                      # [V][H]: rows are the output channels of the tied head
        else:
            out[(slot, li)] = np.ascontiguousarray(ref_w8(np.asarray(a).T)[2].T)
    return out


def build(gpu, family, wd="fp8_e4m3", paged=False, kv="auto", seed=7, **over):
    cfg = gpu.synth.tiny_config(family, **over)
    w = gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=512, weight_dtype=wd,
                                 kv_cache_dtype=kv, **kw)
    return cfg, w, hm


def get_weight(gpu, hm, slot, layer, n_in, n_out):
    out = np.empty((n_in, n_out), np.float32)
    gpu._lib.check(hm.lib.nvl_get_weight(hm.h, gpu._lib.SLOT_ID[slot], layer, out.ctypes.data_as(C.c_void_p), n_in, n_out), hm.h)
    return out


def crafted(rng, n_in, n_out):
    """[in, out] weights with an all-zero output channel, channels of exact midpoints between e4m3 values (ties to even),
    a channel whose maximum is one huge outlier, and random channels"""
    w = (rng.standard_normal((n_in, n_out)) * 0.05).astype(np.float32)
    w[:, 0] = 0
    mids = ((VALUES[1:0x7E] + VALUES[2:0x7F]) / 2).astype(np.float32)     # midpoints of consecutive codes (s = 1 below)
    col = np.resize(np.concatenate([mids, -mids]), n_in).astype(np.float32)
    col[0] = 448
    w[:, 1] = col
    w[:, 2] *= 1e-3
    w[5, 2] = 3.0
    return w


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_quantizer_read_back(gpu, dtype):
    """nvl_get_weight of every quantized kind, the tied embedding included, equals W~ of the numpy restatement bit for bit"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for family, tied in (("llama", True), ("falcon", False)):
        cfg = gpu.synth.tiny_config(family, tied_embedding=tied)
        w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
        rng = np.random.default_rng(0)
        hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3")
        sent = {}
        for (slot, li), a in w.items():
            a = np.asarray(a, np.float32)
            if a.ndim == 2 and slot in QUANTIZED:
                a = crafted(rng, *a.shape)
            t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
            sent[(slot, li)] = t.float().numpy()
            hm.upload(slot, li, t)
        checked = 0
        for (slot, li), a in sent.items():
            if slot in QUANTIZED:
                got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
                want = ref_w8(a.T)[2].T
            elif slot == "tok_emb" and tied:
                got = get_weight(gpu, hm, slot, li, a.shape[1], a.shape[0]).T
                want = ref_w8(a)[2]
                assert a.shape[0] % 256 != 0              # padded N: the vocabulary is not a whole number of row tiles
            elif slot == "tok_emb":                       # untied: stays bf16, the upload's plain RNE conversion
                got = get_weight(gpu, hm, slot, li, a.shape[1], a.shape[0]).T
                want = bf16_rne(a)
            else:
                continue
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (family, slot, li)
            checked += 1
        assert checked >= 6
        hm.close()


@pytest.mark.parametrize("K", [768, 2048, 4544])
def test_op_matmul_fp8w(gpu, K):
    """every dispatch form (decode narrow / wide, 64-row groups, dequantize + tile, chunked wide N) against bf16(A) @ W~"""
    rng = np.random.default_rng(K)
    for N in (200, 1000, 2600):
        w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        codes_ref, s_ref, wt = ref_w8(w.T)
        for M in (1, 5, 16, 17, 32, 33, 64, 65, 200, 1024):
            a = rng.standard_normal((M, K)).astype(np.float32)
            c, codes, s = gpu.ops.matmul_fp8w(a, w)
            assert np.array_equal(codes, codes_ref) and np.array_equal(s, s_ref)
            want = bf16_rne(a).astype(np.float64) @ wt.astype(np.float64).T
            assert rel_err(c, want) <= 2e-5, (M, N, K, rel_err(c, want))


@pytest.mark.parametrize("M", [1, 17, 33, 65, 300])
def test_op_matmul_fp8w_exact(gpu, M):
    """channels with amax = 448 (s = 1) and small integers: W~ = w and every fp32 sum is exact"""
    rng = np.random.default_rng(M)
    K, N = 2048, 1000
    w = rng.integers(-8, 9, (K, N)).astype(np.float32)
    w[0, :] = 448
    a = rng.integers(-4, 5, (M, K)).astype(np.float32)
    c, _, s = gpu.ops.matmul_fp8w(a, w)
    assert np.all(s == 1)
    assert np.array_equal(c, (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("family", FAMILIES)
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, family):
    cfg, w, hm = build(gpu, family)
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    prompt = np.random.default_rng(1).integers(0, cfg["vocab_size"], 60).tolist()
    kv = om.new_cache()
    want = om.forward_with_cache(prompt, kv, 0)
    got = hm.forward_with_cache(prompt, 0, 0, all_logits=True)
    errs = [rel_err(got, want)]
    tok = int(np.argmax(want[-1]))
    for step in range(12):
        pos = len(prompt) + step
        want = om.forward_with_cache([tok], kv, pos)[-1]
        got = hm.forward_with_cache([tok], 0, pos, all_logits=False)[-1]
        errs.append(rel_err(got, want))
        top = np.sort(want)[-2:]
        if top[1] - top[0] > 2 * BF16_TOL * np.abs(want).max():
            assert int(np.argmax(got)) == int(np.argmax(want)), step
        tok = int(np.argmax(want))
    print(f"{family}: max rel err vs oracle on W~ {max(errs):.3e}")
    assert max(errs) <= BF16_TOL
    hm.close()


@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_fp8_weights_with_fp8_kv_against_the_oracle(gpu, oracle, family):
    cfg, w, hm = build(gpu, family, kv="fp8_e4m3")
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    prompt = np.random.default_rng(2).integers(0, cfg["vocab_size"], 40).tolist()
    kv = om.new_cache()
    errs = [rel_err(hm.forward_with_cache(prompt, 0, 0, all_logits=False)[-1], om.forward_with_cache(prompt, kv, 0)[-1])]
    for step in range(8):
        tok = 1 + step
        errs.append(rel_err(hm.forward_with_cache([tok], 0, len(prompt) + step, all_logits=False)[-1],
                            om.forward_with_cache([tok], kv, len(prompt) + step)[-1]))
    assert max(errs) <= FP8_KV_TOL, errs
    hm.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, family):
    cfg, _, hm = build(gpu, family)
    r = np.random.default_rng(11)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (9, 33, 2)]
    ids, steps = [0, 1, 2], 10

    def stepwise(graphs):
        old = gpu.lib().nvl_set_tuning(21, int(graphs))
        try:
            for i in ids:
                hm.seq_reset(i)
            lg, cur = hm.forward_batch(ids, prompts, [0, 0, 0])
            out, toks, pos = [lg.copy()], [], [len(p) for p in prompts]
            first = cur.copy()
            for s in range(steps):
                lg, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [p + s for p in pos])
                out.append(lg.copy()); toks.append(cur.copy())
            return first, out, np.stack(toks)
        finally:
            gpu.lib().nvl_set_tuning(21, old)
    first, eager, toks = stepwise(False)
    _, graph, toks_g = stepwise(True)
    assert all(np.array_equal(a, b) for a, b in zip(eager, graph)) and np.array_equal(toks, toks_g)
    for i in ids:
        hm.seq_reset(i)
    _, first2 = hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
    assert np.array_equal(first, first2)
    assert np.array_equal(hm.decode_greedy(ids, first2, steps), toks)
    # the sampled decode loop runs on the same weights
    hist = [p + [int(t)] for p, t in zip(prompts, first2)]
    for i in ids:
        hm.seq_reset(i)
    hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
    u = np.random.default_rng(4).random((4, 3)).astype(np.float32)
    got = hm.decode_sampled(ids, first2, 4, hist, u)
    assert got.shape == (4, 3) and ((got >= 0) & (got < cfg["vocab_size"])).all()
    hm.close()


@pytest.mark.parametrize("family", ["llama", "gpt2", "granite_moe"])
def test_paged_equals_slab_and_prefix_hit(gpu, family):
    cfg, _, slab = build(gpu, family)
    _, _, paged = build(gpu, family, paged=True)
    r = np.random.default_rng(21)
    tables = [[5, 9], [1, 17, 3], [22]]
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (70, 130, 5)]
    for i in range(3):
        slab.seq_reset(i)
    lp, ap = paged.forward_paged(prompts, [0, 0, 0], tables)
    ls, as_ = slab.forward_batch([0, 1, 2], prompts, [0, 0, 0])
    assert np.array_equal(lp, ls) and np.array_equal(ap, as_)
    pos = [len(p) for p in prompts]
    for _ in range(8):
        lp, ap = paged.forward_paged([[int(t)] for t in ap], pos, tables)
        ls, as_ = slab.forward_batch([0, 1, 2], [[int(t)] for t in as_], pos)
        assert np.array_equal(lp, ls) and np.array_equal(ap, as_)
        pos = [p + 1 for p in pos]
    shared = r.integers(0, cfg["vocab_size"], 64).tolist()
    tail = r.integers(0, cfg["vocab_size"], 40).tolist()
    paged.forward_paged([shared], [0], [[10]])
    cold, _ = paged.forward_paged([tail], [64], [[10, 11]])
    paged.forward_paged([shared], [0], [[12]])
    hit, _ = paged.forward_paged([tail], [64], [[12, 13]])
    assert np.array_equal(cold, hit)
    slab.close(); paged.close()


def test_setter_errors_and_weight_bytes(gpu):
    L = gpu._lib
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64)
    assert hm.lib.nvl_set_weight_dtype(hm.h, 7) == -1
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_weight_dtype(hm.h, 0) == 0
    hm.upload("wq", 0, w[("wq", 0)])
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == -7
    hm.close()
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3")
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, tp_force_single=True,
                                weight_dtype="fp8_e4m3")
    assert e.value.code == -1
    # a non-finite weight is refused
    h8 = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3")
    bad = np.array(w[("wo", 0)], np.float32)
    bad[3, 4] = np.nan
    with pytest.raises(gpu.NvlError) as e:
        h8.upload("wo", 0, bad)
    assert e.value.code == -1
    h8.close()
    # resident weight bytes of a dense Llama-shaped model: codes + scales <= 0.55 x bf16
    big = dict(hidden=512, num_heads=8, num_kv_heads=2, head_dim=64, ffn_dim=2048, vocab_size=4096, num_layers=2)
    wb = {}
    for wd in ("auto", "fp8_e4m3"):
        c2, _, hm = build(gpu, "llama", wd, **big)
        wb[wd] = hm.stats()["weight_bytes"]
        hm.close()
    assert wb["fp8_e4m3"] <= 0.55 * wb["auto"], wb
