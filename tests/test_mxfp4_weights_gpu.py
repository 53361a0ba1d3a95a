"""MXFP4 projection weights (mx_weight_dtype="fp4_e2m1", nvl_set_mx_weight_dtype): the upload
quantizer against a numpy restatement of the contract (that mirror IS the contract), the GEMM dispatch of an MXFP4 weight
(decode kernels, 64-row groups, dequantize + tile) against float64 products over W~, the model against the oracle run on
W~, the pre-quantized upload, the setter's errors and the byte accounting."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
FAMILIES = ["llama", "gpt2", "falcon", "granite_moe", "granite_hybrid"]
BF16_TOL = 1.5e-2          # bf16 logits against the oracle (test_model_gpu.py TOL["bf16"])
FP8_KV_TOL = 1e-1          # ... with the 8-bit KV cache (test_kv_fp8_model_gpu.py FP8_TOL)
QUANTIZED = {"wq", "wk", "wv", "wkv", "wo", "w1", "w2"}
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def ref_mx(w_out_in):
    """rows = output channels, blocks of 32 consecutive k: (codes [N][K/2], scale bytes [N][K/32], W~ [N][K]) of DESIGN.md §3"""
    w = np.ascontiguousarray(w_out_in, np.float32)
    n, k = w.shape
    assert k % 32 == 0 and np.isfinite(w).all()
    b = w.reshape(n, k // 32, 32)
    amax = np.abs(b).max(axis=2)
    _, ex = np.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = np.where(amax == 0, 0, np.clip(ex.astype(np.int64) - 1 - 2, -120, 125)).astype(np.int32)
    v = np.ldexp(np.abs(b).astype(np.float64), -e[:, :, None])      # |w| / 2^e, exact
    d = np.abs(v[..., None] - GRID)                          # nearest grid point; above 6 that is 6 (saturation)
    q = d.argmin(axis=-1)                                    # (the first minimum: the lower code of a tie)
    nxt = np.minimum(q + 1, 7)
    tie = (np.take_along_axis(d, nxt[..., None], -1)[..., 0] == np.take_along_axis(d, q[..., None], -1)[..., 0]) & (nxt != q)
    q = np.where(tie & (q % 2 == 1), nxt, q)                 # ties go to the code with the even mantissa bit
    sign = np.signbit(b)
    val = np.ldexp(GRID[q], e[:, :, None]).astype(np.float32)
    wt = np.where(sign, -val, val).astype(np.float32).reshape(n, k)
    code = (q | (sign.astype(np.int64) << 3)).astype(np.uint8).reshape(n, k)
    packed = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return packed, (e + 127).astype(np.uint8), wt


def test_the_mirror_itself():
    """the tie rule and saturation of the issue, W~ exact in bf16, the relative error of the format on Gaussian weights"""
    row = np.zeros((1, 32), np.float32)
    row[0, :9] = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, 7, 6]
    _, s, wt = ref_mx(row)
    assert s[0, 0] == 127 + 0 and wt[0, :9].tolist() == [0, 1, 1, 2, 2, 4, 4, 6, 6]
    w = (np.random.default_rng(0).standard_normal((64, 1024)) * 0.05).astype(np.float32)
    wt = ref_mx(w)[2]
    assert np.array_equal(bf16_rne(wt).view(np.uint32), wt.view(np.uint32))
    assert abs(np.linalg.norm(wt - w) / np.linalg.norm(w) - 0.117) < 0.01


def tilde(cfg, w):
    """the weights the MX model computes with, in the oracle's layout ([in, out]): the seven quantized slots only"""
    return {(slot, li): (np.ascontiguousarray(ref_mx(np.asarray(a).T)[2].T) if slot in QUANTIZED else a) for (slot, li), a in w.items()}


def build(gpu, family, mx="fp4_e2m1", paged=False, kv="auto", seed=7, **over):
    cfg = gpu.synth.tiny_config(family, **over)
    w = gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=512, mx_weight_dtype=mx,
                                 kv_cache_dtype=kv, **kw)
    return cfg, w, hm


def get_weight(gpu, hm, slot, layer, n_in, n_out):
    out = np.empty((n_in, n_out), np.float32)
    gpu._lib.check(hm.lib.nvl_get_weight(hm.h, gpu._lib.SLOT_ID[slot], layer, out.ctypes.data_as(C.c_void_p), n_in, n_out), hm.h)
    return out


def crafted(rng, n_in, n_out, extremes):
    """[in, out] weights whose first 32-block of eight output channels holds: zeros; every tie below 4 with amax = 4 (both
    signs); every tie with amax = 5 (the tie at 5 cannot sit under amax = 4; e = 0 in both); values in (6, 8) that saturate;
    one huge outlier; and, when the upload type can hold them, amax = 2^-124 (the lower clamp, e = -120, all codes 0) and
    amax = 2^127 (e = 125)"""
    w = (rng.standard_normal((n_in, n_out)) * 0.05).astype(np.float32)
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5], np.float32)
    w[:32, 0] = 0
    w[:32, 1] = np.resize(np.concatenate([ties, -ties, [4, -0.0]]), 32)
    w[:32, 2] = np.resize(np.concatenate([ties, [5], -ties, [-5]]), 32)
    w[:32, 3] = np.resize(np.array([7, -6.5, 7.75, 6, 0.1, -3], np.float32), 32)
    w[:32, 4] *= 1e-3
    w[5, 4] = 3.0
    if extremes:
        w[:32, 5] = np.resize(np.array([2.0 ** -124, -2.0 ** -125, 2.0 ** -126, 0, -2.0 ** -124], np.float32), 32)
        w[:32, 6] = np.resize(np.array([2.0 ** 127, -1.5 * 2.0 ** 126, 2.0 ** 120, -2.0 ** 126, 1.25 * 2.0 ** 125, 1.0], np.float32), 32)
    return w


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_quantizer_read_back(gpu, dtype):
    """nvl_get_weight of every quantized kind equals W~ of the numpy mirror bit for bit; the LM head and both embeddings read
    back as the plain bf16 conversion"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for family, over in (("llama", dict(tied_embedding=False)), ("falcon", {}), ("gpt2", {})):
        cfg = gpu.synth.tiny_config(family, **over)
        w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
        rng = np.random.default_rng(0)
        hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1")
        sent = {}
        for (slot, li), a in w.items():
            a = np.asarray(a, np.float32)
            if a.ndim == 2 and slot in QUANTIZED:
                a = crafted(rng, *a.shape, extremes=dtype != "f16")
            t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
            sent[(slot, li)] = t.float().numpy()
            hm.upload(slot, li, t)
        checked, plain = 0, set()
        for (slot, li), a in sent.items():
            if slot in QUANTIZED:
                got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
                want = ref_mx(a.T)[2].T
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


@pytest.mark.parametrize("K", [768, 2048, 4544])
def test_op_matmul_mxfp4w(gpu, K):
    """every dispatch form (decode narrow / wide, HALF, 64-row groups, dequantize + tile) against bf16(A) @ W~"""
    rng = np.random.default_rng(K)
    for N in (200, 1000, 2600):
        w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        codes_ref, s_ref, wt = ref_mx(w.T)
        for M in (1, 5, 16, 17, 32, 33, 64, 65, 200, 1024):
            a = rng.standard_normal((M, K)).astype(np.float32)
            c, codes, s = gpu.ops.matmul_mxfp4w(a, w)
            assert np.array_equal(codes, codes_ref) and np.array_equal(s, s_ref)
            want = bf16_rne(a).astype(np.float64) @ wt.astype(np.float64).T
            print(f"M {M} N {N} K {K}: rel err {rel_err(c, want):.3e}")
            assert rel_err(c, want) <= 2e-5, (M, N, K, rel_err(c, want))


@pytest.mark.parametrize("M", [1, 17, 33, 65, 300])
def test_op_matmul_mxfp4w_exact(gpu, M):
    """weights on the e2m1 grid times a power of two per block, integer activations in [-4, 4]: W~ = w and every fp32 sum is
    exact, so the result equals the float64 product bit for bit"""
    rng = np.random.default_rng(M)
    K, N = 2048, 1000
    grid = np.concatenate([GRID, -GRID]).astype(np.float32)
    w = grid[rng.integers(0, 16, (N, K))]
    w[:, 0::32] = 6                                            # every block's amax is 6: e = 0 before the block's power of two
    w = (w.reshape(N, K // 32, 32) * np.exp2(rng.integers(-3, 3, (N, K // 32, 1))).astype(np.float32)).reshape(N, K)
    w = np.ascontiguousarray(w.T)                              # [in, out]
    a = rng.integers(-4, 5, (M, K)).astype(np.float32)
    c, codes, s = gpu.ops.matmul_mxfp4w(a, w)
    assert np.array_equal(ref_mx(w.T)[2], w.T)
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
def test_mxfp4_weights_with_fp8_kv_against_the_oracle(gpu, oracle, family):
    cfg, w, hm = build(gpu, family, kv="fp8_e4m3")
    om = oracle.OracleModel(cfg, tilde(cfg, w))
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


@pytest.mark.parametrize("family", FAMILIES)
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, oracle, family):
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
    # the fused greedy tokens against the oracle on W~, wherever its top-2 margin exceeds the bound
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    kv = om.new_cache()
    lg = om.forward_with_cache(prompts[1], kv, 0)[-1]
    for s in range(steps + 1):
        top = np.sort(lg)[-2:]
        mine = int(first[1]) if s == 0 else int(toks[s - 1][1])
        if top[1] - top[0] <= 2 * BF16_TOL * np.abs(lg).max():
            break                                              # (a near tie: the sequences may part from here on)
        assert mine == int(np.argmax(lg)), s
        lg = om.forward_with_cache([mine], kv, len(prompts[1]) + s)[-1]
    hm.close()


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


def test_prequantized_upload(gpu):
    """the mirror's codes and scales through nvl_upload_tensor_mxfp4 give the logits of the float upload bit for bit; the
    refusals of the header"""
    L = gpu._lib
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    mk = lambda: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, mx_weight_dtype="fp4_e2m1")
    a, b = mk(), mk()
    for (slot, li), t in w.items():
        a.upload(slot, li, t)
        if slot in QUANTIZED:
            codes, scales, _ = ref_mx(np.asarray(t).T)
            b.upload_mxfp4(slot, li, codes, scales)
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
    codes, scales, _ = ref_mx(np.asarray(w[("wo", 0)]).T)
    n, k = codes.shape[0], codes.shape[1] * 2
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    up = lambda kind, c, s, rows, cols, layout=L.LAYOUT_OUT_IN: hm.lib.nvl_upload_tensor_mxfp4(hm.h, L.SLOT_ID[kind], 0, p(c), p(s), rows, cols, layout)
    assert up("wo", codes, scales, n, k) == 0
    assert up("lm_head", codes, scales, n, k) == -1            # a kind this model keeps in bf16
    assert up("tok_emb", codes, scales, n, k) == -1
    assert up("wo", codes, scales, n, k - 32) == -1            # shape mismatch
    assert up("wo", codes, scales, n - 16, k) == -1
    assert up("wo", codes, scales, n, k - 16) == -1            # cols % 32 != 0 (nvl_create admits no such width: hidden and ffn_dim
                                                               # are multiples of 64, so this is a shape mismatch as well)
    assert up("wo", codes, scales, n, k, L.LAYOUT_IN_OUT) == -1
    for byte in (0xFF, 6, 253, 0):
        s2 = scales.copy()
        s2[3, 1] = byte
        assert up("wo", codes, s2, n, k) == -1, byte
    for byte in (7, 252):
        s2 = scales.copy()
        s2[3, 1] = byte
        assert up("wo", codes, s2, n, k) == 0, byte
    hm.close()
    plain = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64)
    assert plain.lib.nvl_upload_tensor_mxfp4(plain.h, L.SLOT_ID["wo"], 0, p(codes), p(scales), n, k, L.LAYOUT_OUT_IN) == -1
    plain.close()


def test_setter_errors(gpu):
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    mk = lambda **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, **kw)
    hm = mk()
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 7) == -1
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_mx_weight_dtype(hm.h, 0) == 0
    hm.upload("wq", 0, w[("wq", 0)])
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == -7
    hm.close()
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1")
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:
        mk(tp_force_single=True, mx_weight_dtype="fp4_e2m1")
    assert e.value.code == -1
    hm = mk()                                                  # fp8 first, then MX
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == -1
    assert hm.lib.nvl_set_weight_dtype(hm.h, 0) == 0 and hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0
    hm.close()
    hm = mk()                                                  # MX first, then fp8 — and what needs fp8 weights
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_weight_dtype(hm.h, 1) == -1
    assert hm.lib.nvl_set_weight_dtype(hm.h, 0) == 0
    assert hm.lib.nvl_set_act_dtype(hm.h, 1) == -1 and hm.lib.nvl_set_expert_dtype(hm.h, 1) == -1
    hm.close()
    moe = gpu.synth.tiny_config("granite_moe")
    hm = gpu.HipTransformerModel(moe, None, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1")
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == -1
    hm.close()
    h4 = mk(mx_weight_dtype="fp4_e2m1")                        # a non-finite weight is refused
    bad = np.array(w[("wo", 0)], np.float32)
    bad[3, 4] = np.inf
    with pytest.raises(gpu.NvlError) as e:
        h4.upload("wo", 0, bad)
    assert e.value.code == -1
    h4.close()


@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_a_model_without_the_call_is_the_bf16_model(gpu, family):
    """mx_weight_dtype="none" (the setter called with NVL_MX_NONE, or not at all) leaves the bf16 model: logits bit-identical
    to a second model of the same process that never heard of MX, prefill and decode"""
    cfg, w, a = build(gpu, family, mx="none")
    b = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=4, max_batch_tokens=512)
    assert b.lib.nvl_set_mx_weight_dtype(b.h, 0) == 0
    for (slot, li), t in w.items():
        b.upload(slot, li, t)
    b.finalize()
    prompt = np.random.default_rng(9).integers(0, cfg["vocab_size"], 50).tolist()
    assert np.array_equal(a.forward_with_cache(prompt, 0, 0, all_logits=True), b.forward_with_cache(prompt, 0, 0, all_logits=True))
    for step in range(4):
        assert np.array_equal(a.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False),
                              b.forward_with_cache([step + 1], 0, len(prompt) + step, all_logits=False))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    mxm = build(gpu, family)[2]                                # ... and the MX model is a different one
    assert not np.array_equal(mxm.forward_with_cache(prompt, 1, 0, all_logits=True), a.forward_with_cache(prompt, 1, 0, all_logits=True))
    a.close(); b.close(); mxm.close()


def test_weight_bytes(gpu):
    """nvl_stats.weight_bytes = codes + scales of the seven kinds (rows padded to 256) + bf16 for the other 2-D tensors + fp32
    for the 1-D ones"""
    big = dict(hidden=512, num_heads=8, num_kv_heads=2, head_dim=64, ffn_dim=2048, vocab_size=4096, num_layers=2,
               tied_embedding=False)
    cfg, w, hm = build(gpu, "llama", **big)
    pad = lambda n: (n + 255) // 256 * 256
    want = 0.0
    for (slot, li), a in w.items():
        a = np.asarray(a)
        if a.ndim == 1:
            want += a.size * 4
        elif slot in QUANTIZED:                                # [in, out]
            want += pad(a.shape[1]) * a.shape[0] / 2 + pad(a.shape[1]) * a.shape[0] / 32
        elif slot == "tok_emb":                                # [V][H]
            want += pad(a.shape[0]) * a.shape[1] * 2
        else:                                                  # lm_head [in, out]
            want += pad(a.shape[1]) * a.shape[0] * 2
    got = hm.stats()["weight_bytes"]
    hm.close()
    assert got == want, (got, want)
    _, _, ref = build(gpu, "llama", mx="none", **big)
    bf = ref.stats()["weight_bytes"]
    ref.close()
    print(f"weight bytes: MXFP4 {got:.0f}, bf16 {bf:.0f}, ratio {got / bf:.3f}")
