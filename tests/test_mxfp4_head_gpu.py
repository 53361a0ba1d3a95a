"""MXFP4 LM head and tied token embedding (mx_head_dtype="fp4_e2m1", nvl_set_mx_head_dtype): the
quantizer read-back of both kinds against the numpy mirror of the f-9 contract, the model against the oracle run on W~ (head
and tied table included), the embedding gather of both kernels, the dispatch forms the head uses, the chunked tile head, the
three decode loop forms, paged against slab, the pre-quantized upload, the setter's errors, the opt-out and the bytes."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from test_mxfp4_weights_gpu import BF16_TOL, FAMILIES, FP8_KV_TOL, QUANTIZED, bf16_rne, crafted, get_weight, ref_mx

pytestmark = pytest.mark.gpu


def tilde(cfg, w):
    """the weights the MX-head model computes with, in the oracle's layout: the seven projection slots ([in, out]), the LM
    head ([in, out]) and, when tied, the token embedding ([V][H]: rows are the output rows already)"""
    out = {}
    for (slot, li), a in w.items():
        if slot in QUANTIZED or slot == "lm_head":
            a = np.ascontiguousarray(ref_mx(np.asarray(a).T)[2].T)
        elif slot == "tok_emb" and cfg["tied_embedding"]:
            a = ref_mx(np.asarray(a))[2]
        out[(slot, li)] = a
    return out


def build(gpu, family, head="fp4_e2m1", paged=False, kv="auto", seed=7, weights=None, max_batch_tokens=512, **over):
    cfg = gpu.synth.tiny_config(family, **over)
    w = weights(cfg) if weights else gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=max_batch_tokens, mx_weight_dtype="fp4_e2m1",
                                 mx_head_dtype=head, kv_cache_dtype=kv, **kw)
    return cfg, w, hm


class tuning:
    """one nvl_set_tuning key for a block, restored afterwards"""
    def __init__(self, gpu, key, value):
        self.lib, self.key, self.value = gpu.lib(), key, value

    def __enter__(self):
        self.old = self.lib.nvl_set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        self.lib.nvl_set_tuning(self.key, self.old)


# ---- 1. quantizer read-back ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_quantizer_read_back(gpu, dtype):
    """nvl_get_weight of the head, and of the tied embedding, equals W~ of the mirror bit for bit (crafted tie, saturation and
    zero-block rows); falcon (untied): the head is quantized, the embedding reads back as the plain bf16 conversion"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for family in ("llama", "gpt2", "falcon"):
        cfg = gpu.synth.tiny_config(family)
        w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
        rng = np.random.default_rng(0)
        hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1",
                                     mx_head_dtype="fp4_e2m1")
        V, H = cfg["vocab_size"], cfg["hidden"]
        sent = {}
        for slot in ("tok_emb", "lm_head"):
            if (slot, 0) not in w:
                continue
            a = crafted(rng, H, V, extremes=dtype != "f16")      # [in, out]: the crafted blocks are the first 32 k of rows 0..6
            a = a if slot == "lm_head" else np.ascontiguousarray(a.T)
            t = torch.from_numpy(a).to(tdt)
            sent[slot] = t.float().numpy()
            hm.upload(slot, 0, t)
        emb = get_weight(gpu, hm, "tok_emb", 0, H, V).T
        if cfg["tied_embedding"]:
            assert "lm_head" not in sent
            assert np.array_equal(emb.view(np.uint32), ref_mx(sent["tok_emb"])[2].view(np.uint32)), family
        else:
            assert family == "falcon"
            assert np.array_equal(np.ascontiguousarray(emb).view(np.uint32), bf16_rne(sent["tok_emb"]).view(np.uint32))
            got = get_weight(gpu, hm, "lm_head", 0, H, V)
            want = np.ascontiguousarray(ref_mx(sent["lm_head"].T)[2].T)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        hm.close()


# ---- 2. logits against the oracle on W~ ----------------------------------------------------------------------------------
def oracle_run(gpu, oracle, family, kv="auto", **over):
    """prefill of 2 sequences (5 and 9 tokens) + 3 decode steps: the largest relative logit error against the oracle on W~"""
    cfg, w, hm = build(gpu, family, kv=kv, **over)
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    r = np.random.default_rng(1)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (5, 9)]
    caches = [om.new_cache() for _ in prompts]
    want = [om.forward_with_cache(p, c, 0) for p, c in zip(prompts, caches)]
    for i in (0, 1):
        hm.seq_reset(i)
    got, _ = hm.forward_batch([0, 1], prompts, [0, 0], all_logits=True)
    errs = [rel_err(got[:5], want[0]), rel_err(got[5:], want[1])]
    toks = [int(np.argmax(x[-1])) for x in want]
    for step in range(3):
        pos = [len(p) + step for p in prompts]
        want = [om.forward_with_cache([t], c, q)[-1] for t, c, q in zip(toks, caches, pos)]
        got, _ = hm.forward_batch([0, 1], [[t] for t in toks], pos)
        errs += [rel_err(got[i], want[i]) for i in range(2)]
        toks = [int(np.argmax(x)) for x in want]
    hm.close()
    print(f"{family} kv {kv}: max rel err vs oracle on W~ {max(errs):.3e}")
    return max(errs)


@pytest.mark.parametrize("family", FAMILIES)
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, family):
    assert oracle_run(gpu, oracle, family) <= BF16_TOL


@pytest.mark.parametrize("family", ["llama", "granite_moe"])
def test_with_fp8_kv_against_the_oracle(gpu, oracle, family):
    assert oracle_run(gpu, oracle, family, kv="fp8_e4m3") <= FP8_KV_TOL


def test_untied_model_without_a_head_runs_the_bf16_head(gpu):
    """tied_embedding=False and no LM head uploaded: the head falls back to the bf16 embedding — today's MXFP4 model, bit for bit"""
    def weights(cfg):
        w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
        del w[("lm_head", 0)]
        return w
    cfg, w, a = build(gpu, "llama", tied_embedding=False, weights=weights)
    _, _, b = build(gpu, "llama", head="none", tied_embedding=False, weights=weights)
    V, H = cfg["vocab_size"], cfg["hidden"]
    assert np.array_equal(get_weight(gpu, a, "tok_emb", 0, H, V).T, bf16_rne(w[("tok_emb", 0)]))
    prompt = np.random.default_rng(4).integers(0, V, 40).tolist()
    assert np.array_equal(a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(3):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    a.close(); b.close()


# ---- 3. embedding gather ---------------------------------------------------------------------------------------------
def gather_weights(gpu, pos_scale=0.01):
    """a one-layer model whose layer adds nothing (the output and FFN-down projections and every bias are zero, so layer 0's
    output is the embedding; Q, K and V stay random: the KV cache records the normed row) and whose norms are the identity
    scale; the tied table is random, the position rows small"""
    def weights(cfg):
        w = gpu.synth.make_weights(cfg, seed=13, scale=0.05)
        for (slot, li), a in list(w.items()):
            if slot in ("wo", "w2", "bq", "bk", "bv", "bo", "attn_norm_b", "ffn_norm_b", "final_norm_b"):
                w[(slot, li)] = np.zeros_like(a)
            elif slot.endswith("norm_w"):
                w[(slot, li)] = np.ones_like(a)
            elif slot == "pos_emb":
                w[(slot, li)] = gpu.synth.round_bf16(a * np.float32(pos_scale / 0.05))
        return w
    return weights


def embedding_rows(cfg, w, toks, pos):
    """what both gather kernels write: (W~[tok] + pos row) * multiplier in fp32, in that order"""
    x = ref_mx(np.asarray(w[("tok_emb", 0)]))[2][toks].astype(np.float32)
    if ("pos_emb", 0) in w:
        x = x + bf16_rne(w[("pos_emb", 0)])[pos]
    m = np.float32(cfg.get("embedding_multiplier", 0.0))
    return x * m if m != 0 else x


@pytest.mark.parametrize("family,over", [("llama", dict(embedding_multiplier=12.0)), ("gpt2", {})])
def test_embedding_gather(gpu, family, over):
    """prefill and single-token forward (embed_w4_kernel): layer 0's output equals the embedding row exactly.  The fused
    greedy loop (decode_seam_w4_kernel from its second step on): with a tied head and a layer that does nothing, the next
    token is argmax_v <W~[v], norm(row)>, which for these weights is the token itself by a wide margin — so the seam gathers
    tokens 0, 15, 16 and V-1 again and again; the K / V rows the loop caches from the seam's rows equal, bit for bit, those
    of stepwise forward calls, whose rows come from embed_w4_kernel and were compared exactly above"""
    cfg, w, hm = build(gpu, family, num_layers=1, weights=gather_weights(gpu), **over)
    V = cfg["vocab_size"]
    toks = [0, 15, 16, V - 1, 16]
    hm.set_debug(2)
    hm.seq_reset(0)
    hm.forward_batch([0], [toks], [0], want_logits=False)
    got = hm.get_hidden(len(toks))[0]
    want = embedding_rows(cfg, w, toks, np.arange(len(toks)))
    assert np.array_equal(got, want)                          # (as values: the layer's "+ 0" turns a -0 of W~ into +0)
    hm.forward_batch([0], [[V - 1]], [len(toks)], want_logits=False)          # the decode-shaped call
    got = hm.get_hidden(1)[0]
    want = embedding_rows(cfg, w, [V - 1], np.array([len(toks)]))
    assert np.array_equal(got, want)
    hm.set_debug(0)
    # the fused loop: the expected chain from W~ in float64 (final norm with unit scale, no bias)
    wt = ref_mx(np.asarray(w[("tok_emb", 0)]))[2].astype(np.float64)
    first, steps = [0, 15, 16, V - 1], 4
    for i in range(4):
        hm.seq_reset(i)
    _, am = hm.forward_batch([0, 1, 2, 3], [[t] for t in first], [0, 0, 0, 0], want_logits=False)
    chain = []
    cur = list(first)
    for s in range(steps + 1):
        x = embedding_rows(cfg, w, cur, np.full(4, s)).astype(np.float64)
        if cfg["norm_type"] == "layernorm":
            x = x - x.mean(axis=1, keepdims=True)
        xn = x / np.sqrt((x * x).mean(axis=1, keepdims=True) + cfg["norm_eps"])
        lg = xn @ wt.T
        top = np.sort(lg, axis=1)[:, -2:]
        assert ((top[:, 1] - top[:, 0]) > 2 * BF16_TOL * np.abs(lg).max(axis=1)).all(), "the test's weights leave no margin"
        cur = lg.argmax(axis=1).tolist()
        assert cur == first, "the test's weights do not map a token to itself"
        chain.append(cur)
    assert am.tolist() == chain[0]
    out = hm.decode_greedy([0, 1, 2, 3], am, steps)
    assert out.tolist() == chain[1:]
    kv_fused = [hm.get_kv(i, 0) for i in range(4)]
    for i in range(4):
        hm.seq_reset(i)
    for s in range(steps + 1):
        hm.forward_batch([0, 1, 2, 3], [[t] for t in first], [s] * 4, want_logits=False)
    for i in range(4):
        k, v = hm.get_kv(i, 0)
        assert k.shape[1] == steps + 1 and np.abs(k).max() > 0
        assert np.array_equal(k, kv_fused[i][0]) and np.array_equal(v, kv_fused[i][1]), i
    hm.close()


# ---- 4. head dispatch ------------------------------------------------------------------------------------------------
def test_head_dispatch_forms(gpu):
    """N = 1003 (not a multiple of 16), K = 128 at every row count at which the dispatch changes form"""
    rng = np.random.default_rng(1003)
    N, K = 1003, 128
    w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    codes_ref, s_ref, wt = ref_mx(w.T)
    for M in (1, 8, 16, 17, 32, 33, 64, 65, 200, 600):
        a = rng.standard_normal((M, K)).astype(np.float32)
        c, codes, s = gpu.ops.matmul_mxfp4w(a, w)
        assert np.array_equal(codes, codes_ref) and np.array_equal(s, s_ref)
        want = bf16_rne(a).astype(np.float64) @ wt.astype(np.float64).T
        print(f"M {M} N {N} K {K}: rel err {rel_err(c, want):.3e}")
        assert rel_err(c, want) <= 2e-5, (M, rel_err(c, want))


def test_head_dispatch_four_tiles_per_wave(gpu):
    """N >= 65536 at 17..32 rows: the wide form with 4 weight tiles per wave"""
    rng = np.random.default_rng(65552)
    N, K, M = 65552, 64, 20
    w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    wt = ref_mx(w.T)[2]
    a = rng.standard_normal((M, K)).astype(np.float32)
    c, _, _ = gpu.ops.matmul_mxfp4w(a, w)
    want = bf16_rne(a).astype(np.float64) @ wt.astype(np.float64).T
    print(f"M {M} N {N} K {K}: rel err {rel_err(c, want):.3e}")
    assert rel_err(c, want) <= 2e-5


# ---- 5. chunked tile head --------------------------------------------------------------------------------------------
def test_chunked_tile_head(gpu, oracle):
    """vocab 4099: Vpad * H exceeds the largest projection, so the tile-path head runs in several chunks with a ragged last
    one; every row of 3 x 200 tokens with all logits, and the same model's decode logits at B = 3"""
    cfg, w, hm = build(gpu, "llama", vocab_size=4099, max_batch_tokens=640)
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    r = np.random.default_rng(5)
    prompts = [r.integers(0, cfg["vocab_size"], 200).tolist() for _ in range(3)]
    caches = [om.new_cache() for _ in prompts]
    want = np.concatenate([om.forward_with_cache(p, c, 0) for p, c in zip(prompts, caches)])
    for i in range(3):
        hm.seq_reset(i)
    got, _ = hm.forward_batch([0, 1, 2], prompts, [0, 0, 0], all_logits=True)
    assert got.shape == want.shape == (600, 4099)
    err = max(rel_err(got[i], want[i]) for i in range(600))
    print(f"chunked head: max row rel err {err:.3e}")
    assert err <= BF16_TOL
    toks = [int(np.argmax(want[200 * i + 199])) for i in range(3)]
    wd = [om.forward_with_cache([t], c, 200)[-1] for t, c in zip(toks, caches)]
    gd, _ = hm.forward_batch([0, 1, 2], [[t] for t in toks], [200, 200, 200])
    err = max(rel_err(gd[i], wd[i]) for i in range(3))
    print(f"chunked head model, decode B=3: max rel err {err:.3e}")
    assert err <= BF16_TOL
    hm.close()


# ---- 6. loop forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["llama", "gpt2", "granite_moe"])
def test_loop_forms_agree(gpu, family):
    """nvl_decode_greedy, stepwise nvl_forward with graph replay, and the same without (key 21 = 0): identical token ids, and
    the forward call that follows each loop returns bit-identical logits; the fused loop of the MX-head model issues no more
    launches than that of the model with the bf16 head"""
    cfg, w, hm = build(gpu, family)
    r = np.random.default_rng(11)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (9, 33, 2)]
    ids, steps = [0, 1, 2], 12
    pos = [len(p) for p in prompts]

    def stepwise(graphs):
        with tuning(gpu, 21, int(graphs)):
            for i in ids:
                hm.seq_reset(i)
            _, cur = hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
            first, toks = cur.copy(), []
            for s in range(steps):
                _, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [p + s for p in pos], want_logits=False)
                toks.append(cur.copy())
            last, _ = hm.forward_batch(ids, [[int(t)] for t in cur], [p + steps for p in pos])
            return first, np.stack(toks), last

    def fused(m):
        for i in ids:
            m.seq_reset(i)
        _, first = m.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
        m.reset_stats()
        toks = m.decode_greedy(ids, first, steps)
        st = m.stats()
        last, _ = m.forward_batch(ids, [[int(t)] for t in toks[-1]], [p + steps for p in pos])
        return first, toks, last, st["gemm_launches"] + st["attn_launches"] + st["other_launches"]
    f0, t0, l0 = stepwise(False)
    f1, t1, l1 = stepwise(True)
    f2, t2, l2, n_mx = fused(hm)
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2)
    assert np.array_equal(t0, t1) and np.array_equal(t0, t2)
    assert np.array_equal(l0, l1) and np.array_equal(l0, l2)
    _, _, plain = build(gpu, family, head="none")
    n_plain = fused(plain)[3]
    print(f"{family}: launches of {steps} fused steps: MX head {n_mx}, bf16 head {n_plain}")
    assert n_mx <= n_plain
    hm.close(); plain.close()


# ---- 7. paged equals slab --------------------------------------------------------------------------------------------
def test_paged_equals_slab(gpu):
    cfg, _, slab = build(gpu, "llama")
    _, _, paged = build(gpu, "llama", paged=True)
    r = np.random.default_rng(21)
    tables = [[5, 9], [1, 17, 3], [22]]
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (70, 130, 5)]
    for i in range(3):
        slab.seq_reset(i)
    lp, ap = paged.forward_paged(prompts, [0, 0, 0], tables)
    ls, as_ = slab.forward_batch([0, 1, 2], prompts, [0, 0, 0])
    assert np.array_equal(lp, ls) and np.array_equal(ap, as_)
    pos = [len(p) for p in prompts]
    for _ in range(4):
        lp, ap = paged.forward_paged([[int(t)] for t in ap], pos, tables)
        ls, as_ = slab.forward_batch([0, 1, 2], [[int(t)] for t in as_], pos)
        assert np.array_equal(lp, ls) and np.array_equal(ap, as_)
        pos = [p + 1 for p in pos]
    slab.close(); paged.close()


# ---- 8. pre-quantized upload -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,slot", [("falcon", "lm_head"), ("llama", "tok_emb")])
def test_prequantized_upload(gpu, family, slot):
    """the mirror's codes and scales of the head / the tied table through nvl_upload_tensor_mxfp4: logits bit-identical to the
    model that quantized on upload; the refusals of the header"""
    L = gpu._lib
    cfg = gpu.synth.tiny_config(family)
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    mk = lambda: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, mx_weight_dtype="fp4_e2m1",
                                         mx_head_dtype="fp4_e2m1")
    rows_of = lambda t: np.asarray(t) if slot == "tok_emb" else np.asarray(t).T       # [V][H]
    codes, scales, _ = ref_mx(rows_of(w[(slot, 0)]))
    a, b = mk(), mk()
    for (s, li), t in w.items():
        a.upload(s, li, t)
        if s == slot:
            b.upload_mxfp4(s, li, codes, scales)
        else:
            b.upload(s, li, t)
    a.finalize(); b.finalize()
    prompt = np.random.default_rng(3).integers(0, cfg["vocab_size"], 70).tolist()
    assert np.array_equal(a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(3):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    a.close(); b.close()

    hm = mk()
    V, H = cfg["vocab_size"], cfg["hidden"]
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    up = lambda kind, c, s, rows, cols: hm.lib.nvl_upload_tensor_mxfp4(hm.h, L.SLOT_ID[kind], 0, p(c), p(s), rows, cols, L.LAYOUT_OUT_IN)
    assert up(slot, codes, scales, V, H) == 0
    assert up(slot, codes, scales, V - 1, H) == -1             # wrong shape
    assert up(slot, codes, scales, V, H - 32) == -1
    assert up(slot, codes, scales, H, V) == -1
    for byte in (0xFF, 6, 253, 0):
        s2 = scales.copy()
        s2[V - 1, 1] = byte
        assert up(slot, codes, s2, V, H) == -1, byte
    for byte in (7, 252):
        s2 = scales.copy()
        s2[V - 1, 1] = byte
        assert up(slot, codes, s2, V, H) == 0, byte
    if not cfg["tied_embedding"]:
        assert up("tok_emb", codes, scales, V, H) == -1        # the embedding of an untied model stays bf16
    hm.close()


# ---- 9. setter errors ------------------------------------------------------------------------------------------------
def test_setter_errors(gpu):
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    mk = lambda **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, **kw)
    lib = gpu.lib()
    assert lib.nvl_set_mx_head_dtype(None, 1) == -1
    hm = mk()
    assert lib.nvl_set_mx_head_dtype(hm.h, 1) == -1            # no MXFP4 projection weights
    assert lib.nvl_set_mx_head_dtype(hm.h, 0) == 0
    assert lib.nvl_set_weight_dtype(hm.h, 1) == 0 and lib.nvl_set_mx_head_dtype(hm.h, 1) == -1      # fp8 weights
    assert lib.nvl_set_weight_dtype(hm.h, 0) == 0 and lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0
    assert lib.nvl_set_mx_head_dtype(hm.h, 7) == -1 and lib.nvl_set_mx_head_dtype(hm.h, -1) == -1   # unknown values
    assert lib.nvl_set_mx_head_dtype(hm.h, 1) == 0
    assert lib.nvl_set_mx_weight_dtype(hm.h, 0) == -1          # NVL_MX_NONE is refused while the head dtype is set
    assert lib.nvl_set_mx_head_dtype(hm.h, 0) == 0 and lib.nvl_set_mx_weight_dtype(hm.h, 0) == 0
    assert lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0
    hm.upload("wq", 0, w[("wq", 0)])
    assert lib.nvl_set_mx_head_dtype(hm.h, 1) == -7            # after the first 2-D upload
    assert lib.nvl_set_mx_head_dtype(hm.h, 0) == -7
    hm.close()
    hm = gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64)
    assert lib.nvl_set_mx_head_dtype(hm.h, 1) == -1            # f32 precision
    hm.close()
    hm = mk(tp_force_single=True)
    assert lib.nvl_set_mx_weight_dtype(hm.h, 1) == -1 and lib.nvl_set_mx_head_dtype(hm.h, 1) == -1  # tensor parallelism
    hm.close()
    with pytest.raises(gpu.NvlError) as e:                     # through the constructor: after nvl_set_mx_weight_dtype
        gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1",
                                mx_head_dtype="fp4_e2m1")
    assert e.value.code == -1
    for slot in ("tok_emb", "lm_head"):                        # a non-finite head / embedding weight is refused
        h4 = mk(mx_weight_dtype="fp4_e2m1", mx_head_dtype="fp4_e2m1")
        bad = np.array(w[("tok_emb", 0)], np.float32)
        bad = bad if slot == "tok_emb" else np.ascontiguousarray(bad.T)
        bad[3, 4] = np.nan
        with pytest.raises(gpu.NvlError) as e:
            h4.upload(slot, 0, bad)
        assert e.value.code == -1
        h4.close()


# ---- 10. / 11. opt-out and bytes -------------------------------------------------------------------------------------
def f9_bytes(w, head):
    """weight_bytes of the f-9 accounting (test_mxfp4_weights_gpu.test_weight_bytes); head: the slots stored as MXFP4 too"""
    pad = lambda n: (n + 255) // 256 * 256
    q = lambda rows, k: pad(rows) * k / 2 + pad(rows) * k / 32
    want = 0.0
    for (slot, li), a in w.items():
        a = np.asarray(a)
        if a.ndim == 1:
            want += a.size * 4
        elif slot in QUANTIZED:                                # [in, out]
            want += q(a.shape[1], a.shape[0])
        elif slot in ("tok_emb", "pos_emb"):                   # [rows][H]
            want += q(*a.shape) if slot in head else pad(a.shape[0]) * a.shape[1] * 2
        else:                                                  # lm_head [in, out]
            want += q(a.shape[1], a.shape[0]) if slot in head else pad(a.shape[1]) * a.shape[0] * 2
    return want


@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_opt_out_is_exact_and_bytes(gpu, family):
    """mx_head_dtype="none" (the setter called with NVL_MXH_NONE, or not at all) beside an MX-head model in one process: the
    f-9 model, logits and weight_bytes; the MX-head model stores exactly Vpad*H*2 - (Vpad*H/2 + Vpad*H/32) bytes less, once
    (the tied table of llama, the untied head of falcon)"""
    cfg, w, mxh = build(gpu, family)
    _, _, a = build(gpu, family, head="none")
    b = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=4, max_batch_tokens=512, mx_weight_dtype="fp4_e2m1")
    assert b.lib.nvl_set_mx_head_dtype(b.h, 0) == 0
    for (slot, li), t in w.items():
        b.upload(slot, li, t)
    b.finalize()
    prompt = np.random.default_rng(9).integers(0, cfg["vocab_size"], 50).tolist()
    la = a.forward_with_cache(prompt, 0, 0, all_logits=True)
    assert np.array_equal(la, b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(3):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    assert not np.array_equal(la, mxh.forward_with_cache(prompt, 0, 0, all_logits=True))      # the MX-head model is another one
    plain, head = a.stats()["weight_bytes"], mxh.stats()["weight_bytes"]
    assert plain == b.stats()["weight_bytes"] == f9_bytes(w, ())
    V, H = cfg["vocab_size"], cfg["hidden"]
    vpad = (V + 255) // 256 * 256
    assert plain - head == vpad * H * 2 - (vpad * H / 2 + vpad * H / 32)
    assert head == f9_bytes(w, ("tok_emb",) if cfg["tied_embedding"] else ("lm_head",))
    a.close(); b.close(); mxh.close()
