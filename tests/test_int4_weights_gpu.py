"""INT4 group-quantized projection weights (gq_weight_dtype="uint4", nvl_set_gq_weight_dtype): the
upload quantizer against a numpy restatement of the contract (that mirror IS the contract), the GEMM dispatch of an INT4
weight (decode kernels, 64-row groups, dequantize + tile) against float64 products over W~, the model against the oracle run
on W~, the pre-quantized upload, the setter's errors and the byte accounting."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err

FAMILIES = ["llama", "gpt2", "falcon", "granite_moe", "granite_hybrid"]
BF16_TOL = 1.5e-2          # bf16 logits against the oracle (test_model_gpu.py TOL["bf16"])
FP8_KV_TOL = 1e-1          # ... with the 8-bit KV cache (test_kv_fp8_model_gpu.py FP8_TOL)
QUANTIZED = {"wq", "wk", "wv", "wkv", "wo", "w1", "w2"}
gpu_test = pytest.mark.gpu


def group_of(family):
    return 64 if family == "falcon" else 128      # Falcon's tiny hidden width is 192


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def ref_gq(w_out_in, g):
    """rows = output channels, groups of g consecutive k, everything in fp32 (IEEE division, round-half-even):
    -> (codes [N][K/2], scales [N][K/g] float16, zeros [N][K/g] uint8, W~ [N][K]) of DESIGN.md §3"""
    w = np.ascontiguousarray(w_out_in, np.float32)
    n, k = w.shape
    assert k % g == 0 and np.isfinite(w).all()
    b = w.reshape(n, k // g, g)
    lo = np.minimum(np.float32(0), b.min(axis=2))
    hi = np.maximum(np.float32(0), b.max(axis=2))
    r = (hi - lo).astype(np.float32)
    step = (r / np.float32(15)).astype(np.float32)
    assert (step <= 65504).all()
    s16 = step.astype(np.float16)                                       # RNE
    s16 = np.where(s16 == 0, np.float16(2.0 ** -24), s16).astype(np.float16)
    s16 = np.where(r == 0, np.float16(1), s16).astype(np.float16)
    s = s16.astype(np.float32)
    z = np.clip(np.rint((-lo / s).astype(np.float32)), 0, 15).astype(np.float32)
    q = np.clip(np.rint((b / s[:, :, None]).astype(np.float32)) + z[:, :, None], 0, 15).astype(np.float32)
    q = np.where(r[:, :, None] == 0, np.float32(0), q)
    z = np.where(r == 0, np.float32(0), z)
    wt = bf16_rne((s[:, :, None] * (q - z[:, :, None])).astype(np.float32)).reshape(n, k)
    code = q.astype(np.uint8).reshape(n, k)
    packed = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return packed, s16, z.astype(np.uint8), wt


def exact_weights(rng, n, k, g):
    """w = (q - z) * 2^e per group with q = 0 and q = 15 present: r = 15 * 2^e, s = 2^e, the round trip is exact"""
    q = rng.integers(0, 16, (n, k // g, g))
    q[:, :, 0], q[:, :, 1] = 0, 15
    z = rng.integers(0, 16, (n, k // g, 1))
    e = rng.integers(-6, 0, (n, k // g, 1))
    return ((q - z) * np.exp2(e)).astype(np.float32).reshape(n, k), e


def test_the_mirror_itself():
    """the relative error of the format on Gaussian weights at the three group sizes, and the exact round trip"""
    w = (np.random.default_rng(0).standard_normal((64, 1024)) * 0.05).astype(np.float32)
    for g, want in ((32, 0.081), (64, 0.091), (128, 0.101)):
        wt = ref_gq(w, g)[3]
        assert abs(np.linalg.norm(wt - w) / np.linalg.norm(w) - want) < 0.01, (g, np.linalg.norm(wt - w) / np.linalg.norm(w))
    rng = np.random.default_rng(1)
    for g in (32, 64, 128):
        w, e = exact_weights(rng, 16, 512, g)
        _, s, _, wt = ref_gq(w, g)
        assert np.array_equal(wt.view(np.uint32), w.view(np.uint32))
        assert np.array_equal(s.astype(np.float32), np.exp2(e[:, :, 0]).astype(np.float32))


def tilde(cfg, w, g):
    """the weights the INT4 model computes with, in the oracle's layout ([in, out]): the seven quantized slots only"""
    return {(slot, li): (np.ascontiguousarray(ref_gq(np.asarray(a).T, g)[3].T) if slot in QUANTIZED else a) for (slot, li), a in w.items()}


def build(gpu, family, gq="uint4", paged=False, kv="auto", seed=7, **over):
    cfg = gpu.synth.tiny_config(family, **over)
    w = gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=512, gq_weight_dtype=gq,
                                 gq_group_size=group_of(family), kv_cache_dtype=kv, **kw)
    return cfg, w, hm


def get_weight(gpu, hm, slot, layer, n_in, n_out):
    out = np.empty((n_in, n_out), np.float32)
    gpu._lib.check(hm.lib.nvl_get_weight(hm.h, gpu._lib.SLOT_ID[slot], layer, out.ctypes.data_as(C.c_void_p), n_in, n_out), hm.h)
    return out


def crafted(rng, n_in, n_out, g):
    """[in, out] weights whose first group of six output channels holds: zeros; only positive values; only negative values;
    r = 1.875 (s = 2^-3 exactly) with lo = -4.5 s and every other element an odd multiple of s / 2 (exact ties in -lo / s and
    in w / s); tiny values with one outlier; amax = 2^-30 (r / 15 rounds to the fp16 zero: the scale floor 2^-24)"""
    w = (rng.standard_normal((n_in, n_out)) * 0.05).astype(np.float32)
    w[:g, 0] = 0
    w[:g, 1] = rng.uniform(0.1, 1.0, g)
    w[:g, 2] = -rng.uniform(0.1, 1.0, g)
    w[:g, 3] = np.resize(np.arange(-9, 22, 2, dtype=np.float32) * 0.0625, g)      # -0.5625 .. 1.3125
    w[:g, 4] *= 1e-3
    w[5, 4] = 3.0
    w[:g, 5] = np.resize(np.array([2.0 ** -30, -2.0 ** -31, 0, 2.0 ** -32], np.float32), g)
    return w


@gpu_test
@pytest.mark.parametrize("dtype,g32", [("f32", False), ("bf16", False), ("f16", False), ("f32", True)])
def test_quantizer_read_back(gpu, dtype, g32):
    """nvl_get_weight of every quantized kind equals W~ of the numpy mirror bit for bit; the LM head and both embeddings read
    back as the plain bf16 conversion"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for family, over in (("llama", dict(tied_embedding=False)), ("falcon", {}), ("gpt2", {})):
        g = 32 if g32 else group_of(family)
        cfg = gpu.synth.tiny_config(family, **over)
        w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
        rng = np.random.default_rng(0)
        hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4", gq_group_size=g)
        sent = {}
        for (slot, li), a in w.items():
            a = np.asarray(a, np.float32)
            if a.ndim == 2 and slot in QUANTIZED:
                a = crafted(rng, *a.shape, g)
            t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
            sent[(slot, li)] = t.float().numpy()
            hm.upload(slot, li, t)
        checked, plain = 0, set()
        for (slot, li), a in sent.items():
            if slot in QUANTIZED:
                got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
                want = ref_gq(a.T, g)[3].T
                checked += 1
            elif slot in ("tok_emb", "pos_emb"):
                got = get_weight(gpu, hm, slot, li, a.shape[1], a.shape[0]).T
                want = bf16_rne(a)
                plain.add(slot)
            elif slot == "lm_head":
                got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
                want = bf16_rne(a)
                plain.add(slot)
            else:
                continue
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (family, slot, li)
        assert checked >= 8 and "tok_emb" in plain
        assert family != "llama" or "lm_head" in plain
        assert family != "gpt2" or "pos_emb" in plain
        hm.close()


@gpu_test
@pytest.mark.parametrize("K,g", [(768, 128), (2048, 128), (4544, 64), (768, 32)])
def test_op_matmul_int4w(gpu, K, g):
    """every dispatch form (decode narrow / wide, HALF, 64-row groups, dequantize + tile) against bf16(A) @ W~"""
    rng = np.random.default_rng(K + g)
    for N in (200, 1000, 2600):
        w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        codes_ref, s_ref, z_ref, wt = ref_gq(w.T, g)
        for M in (1, 5, 16, 17, 32, 33, 64, 65, 200, 1024):
            a = rng.standard_normal((M, K)).astype(np.float32)
            c, codes, s, z = gpu.ops.matmul_int4w(a, w, g)
            assert np.array_equal(codes, codes_ref) and np.array_equal(s.view(np.uint16), s_ref.view(np.uint16)) and np.array_equal(z, z_ref)
            want = bf16_rne(a).astype(np.float64) @ wt.astype(np.float64).T
            print(f"M {M} N {N} K {K} g {g}: rel err {rel_err(c, want):.3e}")
            assert rel_err(c, want) <= 2e-5, (M, N, K, g, rel_err(c, want))


@gpu_test
@pytest.mark.parametrize("M", [1, 17, 33, 65, 300])
def test_op_matmul_int4w_exact(gpu, M):
    """w = (q - z) * 2^e per group with q = 0 and q = 15 present, integer activations in [-4, 4]: W~ = w and every fp32 sum is
    exact, so the result equals the float64 product bit for bit"""
    rng = np.random.default_rng(M)
    K, N, g = 2048, 1000, 128
    w_oi, _ = exact_weights(rng, N, K, g)
    w = np.ascontiguousarray(w_oi.T)                              # [in, out]
    a = rng.integers(-4, 5, (M, K)).astype(np.float32)
    c, codes, s, z = gpu.ops.matmul_int4w(a, w, g)
    assert np.array_equal(ref_gq(w.T, g)[3], w.T)
    assert np.array_equal(c, (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32))


@gpu_test
@pytest.mark.parametrize("family", FAMILIES)
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, family):
    cfg, w, hm = build(gpu, family)
    om = oracle.OracleModel(cfg, tilde(cfg, w, group_of(family)))
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


@gpu_test
@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_int4_weights_with_fp8_kv_against_the_oracle(gpu, oracle, family):
    cfg, w, hm = build(gpu, family, kv="fp8_e4m3")
    om = oracle.OracleModel(cfg, tilde(cfg, w, group_of(family)))
    prompt = np.random.default_rng(2).integers(0, cfg["vocab_size"], 40).tolist()
    kv = om.new_cache()
    errs = [rel_err(hm.forward_with_cache(prompt, 0, 0, all_logits=False)[-1], om.forward_with_cache(prompt, kv, 0)[-1])]
    for step in range(8):
        tok = 1 + step
        errs.append(rel_err(hm.forward_with_cache([tok], 0, len(prompt) + step, all_logits=False)[-1],
                            om.forward_with_cache([tok], kv, len(prompt) + step)[-1]))
    print(f"{family}: max rel err with the 8-bit KV cache {max(errs):.3e}")
    assert max(errs) <= FP8_KV_TOL, errs
    hm.close()


@gpu_test
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, family):
    cfg, w, hm = build(gpu, family)
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
    hm.close()


@gpu_test
@pytest.mark.parametrize("family", ["llama", "gpt2", "granite_moe"])
def test_paged_equals_slab(gpu, family):
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
    slab.close(); paged.close()


@gpu_test
def test_prequantized_upload(gpu):
    """the mirror's codes, scales and zeros through nvl_upload_tensor_int4 give the logits of the float upload bit for bit;
    the refusals of the header"""
    L = gpu._lib
    g = 128
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    mk = lambda: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, gq_weight_dtype="uint4", gq_group_size=g)
    a, b = mk(), mk()
    for (slot, li), t in w.items():
        a.upload(slot, li, t)
        if slot in QUANTIZED:
            codes, scales, zeros, _ = ref_gq(np.asarray(t).T, g)
            b.upload_int4(slot, li, codes, scales, zeros)
        else:
            b.upload(slot, li, t)
    a.finalize(); b.finalize()
    prompt = np.random.default_rng(3).integers(0, cfg["vocab_size"], 70).tolist()
    la, lb = a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True)
    assert np.array_equal(la, lb)
    for step in range(4):
        la = a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False)
        lb = b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False)
        assert np.array_equal(la, lb)
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    a.close(); b.close()

    hm = mk()
    codes, scales, zeros, _ = ref_gq(np.asarray(w[("wo", 0)]).T, g)
    scales = scales.view(np.uint16)
    n, k = codes.shape[0], codes.shape[1] * 2
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    up = lambda kind, c, s, z, rows, cols, layout=L.LAYOUT_OUT_IN: hm.lib.nvl_upload_tensor_int4(hm.h, L.SLOT_ID[kind], 0, p(c), p(s), p(z), rows, cols, layout)
    assert up("wo", codes, scales, zeros, n, k) == 0
    assert up("lm_head", codes, scales, zeros, n, k) == -1     # a kind this model keeps in bf16
    assert up("tok_emb", codes, scales, zeros, n, k) == -1
    assert up("wo", codes, scales, zeros, n, k - 128) == -1    # shape mismatch
    assert up("wo", codes, scales, zeros, n - 16, k) == -1
    assert up("wo", codes, scales, zeros, n, k - 32) == -1     # cols % g != 0 (a shape mismatch as well: hidden % g == 0 here)
    assert up("wo", codes, scales, zeros, n, k, L.LAYOUT_IN_OUT) == -1
    z2 = zeros.copy()
    z2[3, 1] = 16
    assert up("wo", codes, scales, z2, n, k) == -1             # a zero point above 15
    for bits in (0x7E00, 0x7C00, 0xFC00, 0x0000, 0x8000, 0xBC00):     # NaN, +Inf, -Inf, +0, -0, -1
        s2 = scales.copy()
        s2[3, 1] = bits
        assert up("wo", codes, s2, zeros, n, k) == -1, hex(bits)
    for bits in (0x0001, 0x7BFF):                              # the smallest and the largest positive finite fp16
        s2 = scales.copy()
        s2[3, 1] = bits
        assert up("wo", codes, s2, zeros, n, k) == 0, hex(bits)
    hm.close()
    plain = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64)
    assert plain.lib.nvl_upload_tensor_int4(plain.h, L.SLOT_ID["wo"], 0, p(codes), p(scales), p(zeros), n, k, L.LAYOUT_OUT_IN) == -1
    plain.close()


@gpu_test
def test_setter_errors(gpu):
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    mk = lambda **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, **kw)
    hm = mk()
    gq = hm.lib.nvl_set_gq_weight_dtype
    assert gq(hm.h, 7, 128) == -1                              # unknown value
    for bad_g in (0, 16, 48, 256):
        assert gq(hm.h, 1, bad_g) == -1, bad_g
    assert gq(hm.h, 1, 128) == 0 and gq(hm.h, 0, 128) == 0 and gq(hm.h, 1, 32) == 0 and gq(hm.h, 1, 64) == 0
    hm.upload("wq", 0, w[("wq", 0)])
    assert gq(hm.h, 1, 64) == -7                               # state: after the first 2-D upload
    hm.close()
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4")
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:
        mk(tp_force_single=True, gq_weight_dtype="uint4")
    assert e.value.code == -1
    hm = mk()                                                  # fp8 first, then INT4
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == 0 and gq(hm.h, 1, 128) == -1
    assert hm.lib.nvl_set_weight_dtype(hm.h, 0) == 0 and gq(hm.h, 1, 128) == 0
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == -1          # INT4 first, then fp8
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == -1       # ... then MXFP4
    assert hm.lib.nvl_set_act_dtype(hm.h, 1) == -1 and hm.lib.nvl_set_mx_head_dtype(hm.h, 1) == -1
    hm.close()
    hm = mk()                                                  # MXFP4 first, then INT4
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0 and gq(hm.h, 1, 128) == -1
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 0) == 0 and gq(hm.h, 1, 128) == 0
    hm.close()
    h4 = mk(gq_weight_dtype="uint4")                           # a non-finite weight and an fp16-overflowing group are refused
    for val in (np.inf, np.nan, 1.0e6):                        # (1e6 / 15 > 65504)
        bad = np.array(w[("wo", 0)], np.float32)
        bad[3, 4] = val
        with pytest.raises(gpu.NvlError) as e:
            h4.upload("wo", 0, bad)
        assert e.value.code == -1
    h4.close()


@gpu_test
@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_a_model_without_the_call_is_the_bf16_model(gpu, family):
    """gq_weight_dtype="none" (the setter called with NVL_GQ_NONE, or not at all) leaves the bf16 model: logits bit-identical
    to a second model of the same process that never heard of it, prefill and decode"""
    cfg, w, a = build(gpu, family, gq="none")
    b = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=4, max_batch_tokens=512)
    assert b.lib.nvl_set_gq_weight_dtype(b.h, 0, 128) == 0
    for (slot, li), t in w.items():
        b.upload(slot, li, t)
    b.finalize()
    prompt = np.random.default_rng(9).integers(0, cfg["vocab_size"], 50).tolist()
    assert np.array_equal(a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(4):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    gqm = build(gpu, family)[2]                                # ... and the INT4 model is a different one
    assert not np.array_equal(gqm.forward_with_cache(prompt, 1, 0, all_logits=True), a.forward_with_cache(prompt, 1, 0, all_logits=True))
    a.close(); b.close(); gqm.close()


@gpu_test
@pytest.mark.parametrize("g", [32, 128])
def test_weight_bytes(gpu, g):
    """nvl_stats.weight_bytes = codes (in / 2 bytes per row) + one 4-byte word per group of the seven kinds (rows padded to
    256) + bf16 for the other 2-D tensors + fp32 for the 1-D ones"""
    big = dict(hidden=512, num_heads=8, num_kv_heads=2, head_dim=64, ffn_dim=2048, vocab_size=4096, num_layers=2,
               tied_embedding=False)
    cfg = gpu.synth.tiny_config("llama", **big)
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=512, gq_weight_dtype="uint4", gq_group_size=g)
    pad = lambda n: (n + 255) // 256 * 256
    want = 0.0
    for (slot, li), a in w.items():
        a = np.asarray(a)
        if a.ndim == 1:
            want += a.size * 4
        elif slot in QUANTIZED:                                # [in, out]
            want += pad(a.shape[1]) * a.shape[0] / 2 + pad(a.shape[1]) * (a.shape[0] // g) * 4
        elif slot == "tok_emb":                                # [V][H]
            want += pad(a.shape[0]) * a.shape[1] * 2
        else:                                                  # lm_head [in, out]
            want += pad(a.shape[1]) * a.shape[0] * 2
    got = hm.stats()["weight_bytes"]
    hm.close()
    assert got == want, (got, want)
