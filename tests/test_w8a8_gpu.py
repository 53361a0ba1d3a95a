"""8-bit activations on top of 8-bit weights (act_dtype="fp8_e4m3", nvl_set_act_dtype): the
activation quantizer against the numpy restatement bit for bit, the W8A8 tile GEMM exactly on integer data and against
float64 products of the dequantized operands, the decode form unchanged, the five families against the oracle on W~ within
the §3 bound, the identities that stay bit-exact in the mode, and the setter's errors."""
import math

import numpy as np
import pytest

from conftest import rel_err
from test_fp8_weights_gpu import BF16_TOL, FAMILIES, bf16_rne, build, ref_w8, tilde
from test_kv_fp8_gpu import VALUES, ref_quant

pytestmark = pytest.mark.gpu
E_P = 2.0 ** -4 / math.sqrt(3)      # RMS relative error of one W8A8 projection (uniform e4m3 rounding)


def w8a8_tol(cfg):
    """logits bound against the oracle on W~ — 3 sigma of sqrt(P) independent projection errors, P = 4 per
    layer + the LM head, on top of the bf16 tolerance"""
    return 3 * math.sqrt(4 * cfg["num_layers"] + 1) * E_P + BF16_TOL


def ref_act(a):
    """(codes, scales) of DESIGN.md §3 for the bf16-rounded rows of a"""
    b = bf16_rne(a)
    with np.errstate(invalid="ignore"):
        amax = np.nanmax(np.abs(b), axis=1)                    # (NaN elements do not enter the row maximum)
    s = np.where(amax == 0, np.float32(1), (amax / np.float32(448)).astype(np.float32)).astype(np.float32)
    return ref_quant(b, s[:, None]), s


class Tuning:
    """nvl_set_tuning keys for the test, restored afterwards"""

    def __init__(self, gpu, **keys):
        self.lib, self.keys, self.old = gpu.lib(), {int(k[1:]): v for k, v in keys.items()}, {}

    def __enter__(self):
        for k, v in self.keys.items():
            self.old[k] = self.lib.nvl_set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.nvl_set_tuning(k, v)


def tile_path(gpu, sk=1):
    """prefills of more than 64 tokens on the tile step: no 64-row decode groups (key 11 = 64), no short-prefill QKV
    groups (key 18 = 0); key 26 turns the K-split residual form on / off"""
    return Tuning(gpu, k11=64, k18=0, k26=sk)


def crafted_rows(rng, M, K):
    """random rows with, in turn (as far as M reaches), an all-zero row, a row of exact midpoints between codes at s = 1
    (ties to even), a row whose scale one outlier sets (the rest fall to subnormal codes) and a row of tiny values"""
    a = rng.standard_normal((M, K)).astype(np.float32)
    mids = ((VALUES[1:0x7E] + VALUES[2:0x7F]) / 2).astype(np.float32)
    row = np.resize(np.concatenate([mids, -mids]), K).astype(np.float32)
    row[3] = 448
    special = [np.zeros(K, np.float32), row, a[min(2, M - 1)] * 1e-3, a[min(3, M - 1)] * 1e-30]
    special[2][7] = 5e2
    special[3][:4] = [-448.0, 1e-9, -1e-9, 0.0]
    for i in range(min(M, len(special))):
        a[i] = special[i]
    return a


@pytest.mark.parametrize("M,K,lda", [(1, 64, 64), (17, 768, 768), (300, 2048, 2112), (65, 4544, 4672)])
def test_act_quantizer_bit_exact(gpu, M, K, lda):
    rng = np.random.default_rng(M + K)
    a = crafted_rows(rng, M, K)
    codes, s = gpu.ops.act_quant_fp8(a, lda=lda)
    want_c, want_s = ref_act(a)
    assert np.array_equal(s.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(codes, want_c)


def test_act_quantizer_nan_stays_nan(gpu):
    a = np.random.default_rng(5).standard_normal((20, 128)).astype(np.float32)
    a[4, 9] = np.nan
    codes, s = gpu.ops.act_quant_fp8(a)
    want_c, want_s = ref_act(a)
    assert (codes[4, 9] & 0x7F) == 0x7F and np.isfinite(s).all() and np.array_equal(s, want_s)
    codes[4, 9] = want_c[4, 9] = 0                             # (which of the two NaN codes is not part of the contract)
    assert np.array_equal(codes, want_c)


def exact_operands(rng, M, N, K):
    """rows / channels with amax = 448 (scales 1) and small integers: every product and fp32 sum is exact"""
    w = rng.integers(-8, 9, (K, N)).astype(np.float32)
    w[0, :] = 448
    a = rng.integers(-4, 5, (M, K)).astype(np.float32)
    a[:, 1] = -448
    return a, w


@pytest.mark.parametrize("M,N", [(4096, 3072), (65, 1000), (300, 1000)])
@pytest.mark.parametrize("K", [192, 2048, 4544])
def test_matmul_w8a8_exact(gpu, M, N, K):
    """both tile forms (256x256 at M = 4096, N = 3072: 192 tiles; the 128-row form below), K % 128 == 64 included"""
    rng = np.random.default_rng(M * 7 + K)
    a, w = exact_operands(rng, M, N, K)
    with tile_path(gpu):
        c, codes, s = gpu.ops.matmul_w8a8(a, w)
    assert np.all(s == 1) and np.array_equal(VALUES[codes].astype(np.float32), a)
    assert np.array_equal(c, (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("K", [768, 2048, 4544, 8192])
def test_matmul_w8a8_random(gpu, K):
    """ragged N, both forms: within 2e-5 of the float64 product of s_a * e4m3(q_a) and s_w * e4m3(q_w)"""
    rng = np.random.default_rng(K)
    for M, N in ((300, 1000), (1100, 2600)) + (((2048, 6200),) if K < 8192 else ()):
        w = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        a = rng.standard_normal((M, K)).astype(np.float32)
        a[5] *= 40
        wc, ws, _ = ref_w8(w.T)
        with tile_path(gpu):
            c, codes, s = gpu.ops.matmul_w8a8(a, w)
        ac, as_ = ref_act(a)
        assert np.array_equal(codes, ac) and np.array_equal(s, as_)
        want = (VALUES[ac] * as_[:, None].astype(np.float64)) @ (VALUES[wc] * ws[:, None].astype(np.float64)).T
        assert rel_err(c, want) <= 2e-5, (M, N, K, rel_err(c, want))


@pytest.mark.parametrize("M", [1, 17, 33, 64])
def test_decode_form_is_w8a16(gpu, M):
    """M <= 64: the decode kernels run, bit-identical to matmul_fp8w (bf16 activations)"""
    rng = np.random.default_rng(M)
    w = (rng.standard_normal((2048, 1000)) * 0.05).astype(np.float32)
    a = rng.standard_normal((M, 2048)).astype(np.float32)
    c8, codes, s = gpu.ops.matmul_w8a8(a, w)
    c16, _, _ = gpu.ops.matmul_fp8w(a, w)
    assert np.array_equal(c8, c16) and not codes.any() and np.all(s == 1)


def build8(gpu, family, act="fp8_e4m3", **kw):
    kw.setdefault("seed", 7)
    cfg = gpu.synth.tiny_config(family, **kw.pop("over", {}))
    w = gpu.synth.make_weights(cfg, seed=kw.pop("seed"), scale=0.05)
    mbt = kw.pop("max_batch_tokens", 512)
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=mbt, weight_dtype="fp8_e4m3",
                                 act_dtype=act, **kw)
    return cfg, w, hm


def oracle_errs(gpu, oracle, cfg, w, hm, n_prompt, steps=6):
    om = oracle.OracleModel(cfg, tilde(cfg, w))
    prompt = np.random.default_rng(1).integers(0, cfg["vocab_size"], n_prompt).tolist()
    kv = om.new_cache()
    want = om.forward_with_cache(prompt, kv, 0)
    got = hm.forward_with_cache(prompt, 0, 0, all_logits=True)
    errs = [rel_err(got, want)]
    tok = int(np.argmax(want[-1]))
    for step in range(steps):
        pos = n_prompt + step
        want = om.forward_with_cache([tok], kv, pos)[-1]
        got = hm.forward_with_cache([tok], 0, pos, all_logits=False)[-1]
        errs.append(rel_err(got, want))
        tok = int(np.argmax(want))
    return errs


@pytest.mark.parametrize("sk", [1, 0])
@pytest.mark.parametrize("family", FAMILIES + ["llama_hd128"])
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, family, sk):
    """a 150-token prefill (every projection W8A8, the LM head over all rows included), then decode steps (W8A16)"""
    over = dict(head_dim=128, num_heads=2, num_kv_heads=1) if family == "llama_hd128" else {}
    with tile_path(gpu, sk):
        cfg, w, hm = build8(gpu, family.replace("_hd128", ""), over=over)
        errs = oracle_errs(gpu, oracle, cfg, w, hm, 150)
        hm.close()
    tol = w8a8_tol(cfg)
    print(f"{family} key26={sk}: max rel err vs oracle on W~ {max(errs):.3e}, bound {tol:.3e}, ratio {max(errs) / tol:.3f}")
    assert max(errs) <= tol, errs


@pytest.mark.parametrize("sk", [1, 0])
def test_k_split_residual_form(gpu, oracle, sk):
    """a Llama shape whose residual projections take the K-split tile form at 512 rows (H = 1024: 4 x 8 tiles x 2 slices of
    K = 2048 for FFN-down) — with key 26 on and off"""
    over = dict(hidden=1024, num_heads=16, num_kv_heads=4, ffn_dim=2048, max_seq_len=640)
    with tile_path(gpu, sk):
        cfg, w, hm = build8(gpu, "llama", over=over, max_batch_tokens=512)
        errs = oracle_errs(gpu, oracle, cfg, w, hm, 512, steps=2)
        hm.close()
    tol = w8a8_tol(cfg)
    print(f"llama H=1024 key26={sk}: max rel err {max(errs):.3e}, bound {tol:.3e}, ratio {max(errs) / tol:.3f}")
    assert max(errs) <= tol, errs


@pytest.mark.parametrize("family", ["llama", "falcon"])
def test_with_fp8_kv_against_the_oracle(gpu, oracle, family):
    with tile_path(gpu):
        cfg, w, hm = build8(gpu, family, kv_cache_dtype="fp8_e4m3")
        errs = oracle_errs(gpu, oracle, cfg, w, hm, 120, steps=4)
        hm.close()
    tol = w8a8_tol(cfg) + 1e-1                  # + the 8-bit KV cache's own tolerance (test_kv_fp8_model_gpu.py)
    print(f"{family} + fp8 KV: max rel err {max(errs):.3e}, bound {tol:.3e}")
    assert max(errs) <= tol, errs


@pytest.mark.parametrize("family", FAMILIES)
def test_w8a8_differs_from_w8a16(gpu, family):
    """the same weights and prompt: the tile-step projections ran on 8-bit activations"""
    prompt = np.random.default_rng(3).integers(0, 1000, 130).tolist()
    with tile_path(gpu):
        out = {}
        for act in ("auto", "fp8_e4m3"):
            _, _, hm = build8(gpu, family, act=act)
            out[act] = hm.forward_with_cache(prompt, 0, 0, all_logits=True)
            hm.close()
    assert np.isfinite(out["fp8_e4m3"]).all()
    assert not np.array_equal(out["auto"], out["fp8_e4m3"])
    assert rel_err(out["fp8_e4m3"], out["auto"]) > 1e-4


@pytest.mark.parametrize("family", ["llama", "gpt2", "granite_moe"])
def test_paged_equals_slab(gpu, family):
    with tile_path(gpu):
        cfg, _, slab = build8(gpu, family)
        _, _, paged = build8(gpu, family, kv_num_blocks=24, kv_block_size=64)
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


@pytest.mark.parametrize("family", ["llama", "falcon", "granite_hybrid"])
def test_fused_greedy_equals_stepwise(gpu, family):
    with tile_path(gpu):
        cfg, _, hm = build8(gpu, family)
        r = np.random.default_rng(11)
        prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (90, 33, 70)]
        ids, steps = [0, 1, 2], 8
        for i in ids:
            hm.seq_reset(i)
        _, first = hm.forward_batch(ids, prompts, [0, 0, 0])
        toks, cur, pos = [], first.copy(), [len(p) for p in prompts]
        for s in range(steps):
            _, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [p + s for p in pos])
            toks.append(cur.copy())
        for i in ids:
            hm.seq_reset(i)
        _, first2 = hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
        assert np.array_equal(first, first2)
        assert np.array_equal(hm.decode_greedy(ids, first2, steps), np.stack(toks))
        hm.close()


def test_setter_errors(gpu):
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64)
    lib = hm.lib
    assert lib.nvl_set_act_dtype(hm.h, 1) == -1                # no 8-bit weights
    assert lib.nvl_set_act_dtype(hm.h, 0) == 0
    assert lib.nvl_set_weight_dtype(hm.h, 1) == 0
    assert lib.nvl_set_act_dtype(hm.h, 5) == -1                # unknown value
    assert lib.nvl_set_act_dtype(hm.h, 1) == 0 and lib.nvl_set_act_dtype(hm.h, 0) == 0 and lib.nvl_set_act_dtype(hm.h, 1) == 0
    for (slot, li), arr in w.items():
        hm.upload(slot, li, arr)
    hm.finalize()
    assert lib.nvl_set_act_dtype(hm.h, 0) == -7                # after nvl_finalize
    hm.close()
    with pytest.raises(ValueError):
        gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, act_dtype="fp8_e4m3")
    with pytest.raises(gpu.NvlError) as e:                     # f32 refuses the 8-bit weights the mode needs
        gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3",
                                act_dtype="fp8_e4m3")
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, tp_force_single=True,
                                weight_dtype="fp8_e4m3", act_dtype="fp8_e4m3")
    assert e.value.code == -1
