"""INT4 group-quantized MoE expert weights (gq_expert_dtype="uint4", nvl_set_gq_expert_dtype): the
upload quantizer against the numpy mirror of the INT4 contract (test_int4_weights_gpu.ref_gq: one {fp16 s, z} word per g input
features of an expert's output row), the model against the oracle run on W~ across the decode forms (narrow / wide up, K-split
down at MT 1 / 2 / 4), the grouped prefill paths and grouped decode on dequantized W~, the identities that stay bit-exact, the
pre-quantized upload, the default that stays today's INT4 model, the weight bytes and the setter's errors."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_int4_weights_gpu import BF16_TOL, FP8_KV_TOL, QUANTIZED, bf16_rne, crafted, get_weight, ref_gq

pytestmark = pytest.mark.gpu
EXPERTS = ("moe_in", "moe_out")
GRANITE_1B_LAYERS = dict(hidden=1024, num_heads=16, num_kv_heads=8, head_dim=64, ffn_dim=512, num_experts=32,
                         num_experts_per_tok=8, num_layers=2)


def rup(n, m=256):
    return (n + m - 1) // m * m


def tilde_e(w, g):
    """the weights an INT4-expert model computes with, in the oracle's layout: W~ of the seven projection kinds ([in, out]) and
    of every expert row ([E, out, in])"""
    out = {}
    for (slot, li), a in w.items():
        a = np.asarray(a, np.float32)
        if slot in EXPERTS:
            a = ref_gq(a.reshape(-1, a.shape[2]), g)[3].reshape(a.shape)
        elif slot in QUANTIZED:
            a = np.ascontiguousarray(ref_gq(a.T, g)[3].T)
        out[(slot, li)] = a
    return out


@functools.lru_cache(maxsize=None)
def case(seed, g, over):
    """(cfg, weights, W~) of one configuration: made once, shared by the tests that run it, never written to"""
    import importlib
    synth = importlib.import_module("nano-vllm-go_amd").synth
    cfg = synth.tiny_config("granite_moe", **dict(over))
    w = synth.make_weights(cfg, seed=seed, scale=0.05)
    return cfg, w, tilde_e(w, g)


def build(gpu, ge="uint4", g=64, seed=7, paged=False, kv="auto", mbt=512, max_seqs=4, **over):
    cfg, w, wt = case(seed, g, tuple(sorted(over.items())))
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=max_seqs, max_batch_tokens=mbt, gq_weight_dtype="uint4",
                                 gq_group_size=g, gq_expert_dtype=ge, kv_cache_dtype=kv, **kw)
    return cfg, w, wt, hm


def with_tuning(gpu, key, value):
    class _T:
        def __enter__(self):
            self.old = gpu.lib().nvl_set_tuning(key, value)

        def __exit__(self, *a):
            gpu.lib().nvl_set_tuning(key, self.old)
    return _T()


def against_oracle(oracle, cfg, wt, hm, prompt_len, steps=12, seed=1, tol=BF16_TOL):
    """teacher-forced: the oracle's argmax is fed to both, the logits are compared at every step"""
    om = oracle.OracleModel(cfg, wt)
    prompt = np.random.default_rng(seed).integers(0, cfg["vocab_size"], prompt_len).tolist()
    kv = om.new_cache()
    want = om.forward_with_cache(prompt, kv, 0)
    got = hm.forward_with_cache(prompt, 0, 0, all_logits=True)
    errs = [rel_err(got, want)]
    tok = int(np.argmax(want[-1]))
    for step in range(steps):
        pos = prompt_len + step
        want = om.forward_with_cache([tok], kv, pos)[-1]
        got = hm.forward_with_cache([tok], 0, pos, all_logits=False)[-1]
        errs.append(rel_err(got, want))
        tok = int(np.argmax(want))
    print(f"max rel err vs oracle on W~ {max(errs):.3e}")
    assert max(errs) <= tol, errs
    return max(errs)


def crafted_experts(rng, a, g):
    """[E, out, in] with, in every expert, the crafted groups of test_int4_weights_gpu.crafted in its first six output rows:
    all zero, one-signed (both signs), exact ties, an outlier among tiny values, and the 2^-24 scale floor"""
    return np.stack([crafted(rng, a.shape[2], a.shape[1], g).T for _ in range(a.shape[0])])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("g", [32, 64])
def test_expert_quantizer_read_back(gpu, dtype, g):
    """nvl_get_weight of moe_in / moe_out of every layer equals W~ of the numpy mirror bit for bit, crafted groups included
    (5 experts x 2*64 rows = 640 rows: the last row tile is padded); the dense projections still equal their W~; the router
    and the embedding read back as the plain bf16 conversion"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
    rng = np.random.default_rng(0)
    hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4",
                                 gq_group_size=g, gq_expert_dtype="uint4")
    sent = {}
    for (slot, li), a in w.items():
        a = np.asarray(a, np.float32)
        if slot in EXPERTS:
            a = crafted_experts(rng, a, g)
        elif slot in QUANTIZED:
            a = crafted(rng, *a.shape, g)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
        sent[(slot, li)] = t.float().numpy()
        hm.upload(slot, li, t)
    experts, dense, plain = 0, 0, set()
    for (slot, li), a in sent.items():
        if slot in EXPERTS:
            E, n_out, n_in = a.shape
            assert slot != "moe_in" or (E * n_out) % 256 != 0
            got = get_weight(gpu, hm, slot, li, n_in, E * n_out).T
            want = ref_gq(a.reshape(E * n_out, n_in), g)[3]
            experts += 1
        elif slot in QUANTIZED:
            got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
            want = ref_gq(a.T, g)[3].T
            dense += 1
        elif slot == "tok_emb":
            got = get_weight(gpu, hm, slot, li, a.shape[1], a.shape[0]).T
            want = bf16_rne(a)
            plain.add(slot)
        elif slot == "router":
            got = get_weight(gpu, hm, slot, li, a.shape[0], a.shape[1])
            want = bf16_rne(a)
            plain.add(slot)
        else:
            continue
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (slot, li)
    assert experts == 2 * cfg["num_layers"] and dense == 4 * cfg["num_layers"] and plain == {"tok_emb", "router"}
    hm.close()


@pytest.mark.parametrize("over,g,prompt_len", [
    ({}, 64, 60),                                  # tiny: decode down at MT = 4 at 60 rows
    ({}, 64, 100),                                 # tiny prefill beyond 64 rows: 128-row grouped GEMMs on dequantized W~
    ({"ffn_dim": 256}, 64, 20),                    # I = 256: down form at 20 rows (MT = 2, U = 4)
    ({"ffn_dim": 256}, 64, 40),                    # ... at 40 rows (MT = 4, M % 16 != 0)
    ({"ffn_dim": 256}, 64, 100),                   # H, 2I % 256 == 0, H, I >= 160: the ping-pong grouped prefill
    (GRANITE_1B_LAYERS, 128, 8),                   # Granite-1B layer shape: narrow up + K-split down at MT = 1
    (GRANITE_1B_LAYERS, 128, 30),                  # ... the wide up form (2 tiles per wave) and down at MT = 2
    ({}, 32, 20),                                  # g = 32: the group word changes with every k-step (twice per 64 inputs)
])
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, over, g, prompt_len):
    """prefill + 12 decode steps; prompts of <= 64 rows run the decode forms in the prefill as well"""
    cfg, _, wt, hm = build(gpu, g=g, **over)
    err = against_oracle(oracle, cfg, wt, hm, prompt_len)
    print(f"{over} g {g} {prompt_len}: max rel err vs oracle on W~ {err:.3e}")
    hm.close()


def test_grouped_decode_key_22(gpu, oracle):
    """key 22 = 0: decode through the planning launch and the grouped GEMMs on dequantized W~"""
    with with_tuning(gpu, 22, 0):
        cfg, _, wt, hm = build(gpu)
        against_oracle(oracle, cfg, wt, hm, 30)
        hm.close()


def test_deferred_down_conditions_with_key_33(gpu, oracle):
    """E = 16, I = 128 meets the deferred-norm producer's conditions; with key 33 = 1 the INT4 experts take the K-split form
    (there is no INT4 instance of the producer form: taking it would be refused by the dispatch)"""
    with with_tuning(gpu, 33, 1):
        cfg, _, wt, hm = build(gpu, num_experts=16, ffn_dim=128)
        against_oracle(oracle, cfg, wt, hm, 30)
        hm.close()


def test_down_block_mask_large_expert_width(gpu, oracle):
    """I = 8192: more blocks per expert than the decode down form's 32-bit live-block mask holds; such widths take the grouped
    form (on dequantized W~) and match the oracle"""
    over = dict(hidden=128, num_heads=2, num_kv_heads=2, num_experts=4, ffn_dim=8192)
    cfg, w, wt = case(9, 64, tuple(sorted(over.items())))
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4",
                                 gq_group_size=64, gq_expert_dtype="uint4")
    for n in (8, 48):
        hm.seq_reset(0)
        against_oracle(oracle, cfg, wt, hm, n, steps=2, seed=n)
    hm.close()


def test_with_fp8_kv_against_the_oracle(gpu, oracle):
    cfg, _, wt, hm = build(gpu, kv="fp8_e4m3")
    against_oracle(oracle, cfg, wt, hm, 40, steps=8, tol=FP8_KV_TOL)
    hm.close()


@pytest.mark.parametrize("kv", ["auto", "fp8_e4m3"])
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, kv):
    cfg, _, _, hm = build(gpu, kv=kv)
    r = np.random.default_rng(11)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (9, 80, 2)]
    ids, steps = [0, 1, 2], 10

    def stepwise(graphs):
        with with_tuning(gpu, 21, int(graphs)):
            for i in ids:
                hm.seq_reset(i)
            lg, cur = hm.forward_batch(ids, prompts, [0, 0, 0])
            out, toks, pos = [lg.copy()], [], [len(p) for p in prompts]
            first = cur.copy()
            for s in range(steps):
                lg, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [p + s for p in pos])
                out.append(lg.copy()); toks.append(cur.copy())
            return first, out, np.stack(toks)
    first, eager, toks = stepwise(False)
    _, graph, toks_g = stepwise(True)
    assert all(np.array_equal(a, b) for a, b in zip(eager, graph)) and np.array_equal(toks, toks_g)
    for i in ids:
        hm.seq_reset(i)
    _, first2 = hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
    assert np.array_equal(first, first2)
    assert np.array_equal(hm.decode_greedy(ids, first2, steps), toks)
    hm.close()


@pytest.mark.parametrize("kv", ["auto", "fp8_e4m3"])
def test_paged_equals_slab_and_prefix_hit(gpu, kv):
    cfg, _, _, slab = build(gpu, kv=kv)
    _, _, _, paged = build(gpu, kv=kv, paged=True)
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
    cold, ids_cold = paged.forward_paged([tail], [64], [[10, 11]])
    paged.forward_paged([shared], [0], [[12]])
    hit, ids_hit = paged.forward_paged([tail], [64], [[12, 13]])
    assert np.array_equal(cold, hit) and np.array_equal(ids_cold, ids_hit)
    slab.close(); paged.close()


def run_both(a, b, cfg, seed, n=70, steps=4, seq=0):
    """prefill + decode logits of two models, as two lists"""
    prompt = np.random.default_rng(seed).integers(0, cfg["vocab_size"], n).tolist()
    la, lb = [a.forward_with_cache(prompt, seq, 0, all_logits=True)], [b.forward_with_cache(prompt, seq, 0, all_logits=True)]
    for step in range(steps):
        la.append(a.forward_with_cache([step + 1], seq, n + step, all_logits=False))
        lb.append(b.forward_with_cache([step + 1], seq, n + step, all_logits=False))
    return la, lb


def test_prequantized_upload(gpu):
    """the mirror's codes, scales and zeros through nvl_upload_tensor_int4 — experts as [E * out][in / 2] and [E * out][in / g] —
    give the logits and the weight bytes of the float upload bit for bit, and the experts read back as W~; the refusals"""
    L = gpu._lib
    g = 64
    cfg, w, _ = case(5, g, ())
    mk = lambda **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, gq_weight_dtype="uint4",
                                              gq_group_size=g, **kw)
    a, b = mk(gq_expert_dtype="uint4"), mk(gq_expert_dtype="uint4")
    for (slot, li), t in w.items():
        a.upload(slot, li, t)
        t = np.asarray(t, np.float32)
        if slot in EXPERTS:
            codes, scales, zeros, want = ref_gq(t.reshape(-1, t.shape[2]), g)
            b.upload_int4(slot, li, codes, scales, zeros)
            back = get_weight(gpu, b, slot, li, t.shape[2], t.shape[0] * t.shape[1]).T
            assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), slot
        elif slot in QUANTIZED:                                # [in, out]
            codes, scales, zeros, _ = ref_gq(t.T, g)
            b.upload_int4(slot, li, codes, scales, zeros)
        else:
            b.upload(slot, li, t)
    a.finalize(); b.finalize()
    la, lb = run_both(a, b, cfg, 3)
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    a.close(); b.close()

    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    for slot in EXPERTS:
        t = np.asarray(w[(slot, 0)], np.float32)
        codes, scales, zeros, _ = ref_gq(t.reshape(-1, t.shape[2]), g)
        scales = scales.view(np.uint16)
        n, k = codes.shape[0], codes.shape[1] * 2
        hm = mk(gq_expert_dtype="uint4")
        up = lambda c, s, z, rows, cols, layout=L.LAYOUT_OUT_IN: hm.lib.nvl_upload_tensor_int4(hm.h, L.SLOT_ID[slot], 0, p(c), p(s), p(z), rows, cols, layout)
        z2 = zeros.copy()
        z2[3, 0] = 16
        assert up(codes, scales, z2, n, k) == -1, slot                     # a zero point above 15
        for bits in (0x7E00, 0x7C00, 0xFC00, 0x0000, 0x8000, 0xBC00):      # NaN, +Inf, -Inf, +0, -0, -1
            s2 = scales.copy()
            s2[3, 0] = bits
            assert up(codes, s2, zeros, n, k) == -1, (slot, hex(bits))
        assert up(codes, scales, zeros, n - 16, k) == -1 and up(codes, scales, zeros, n, k - g) == -1      # wrong shapes
        assert up(codes, scales, zeros, n // cfg["num_experts"], k) == -1  # one expert's rows
        assert up(codes, scales, zeros, n, k, L.LAYOUT_IN_OUT) == -1
        assert up(codes, scales, zeros, n, k) == 0
        hm.close()
        plain = mk()                                                       # INT4 projections without the expert mode
        assert plain.lib.nvl_upload_tensor_int4(plain.h, L.SLOT_ID[slot], 0, p(codes), p(scales), p(zeros), n, k, L.LAYOUT_OUT_IN) == -1
        plain.close()


def test_a_model_without_the_call_is_todays_int4_model(gpu):
    """gq_expert_dtype="none" leaves the INT4-projection model with bf16 experts: logits bit-identical to a second model of the
    same process that never calls the setter, prefill and 4 decode steps, the same weight bytes, and experts that read back as
    the plain bf16 conversion; the INT4-expert model is a different one"""
    g = 64
    cfg, w, _ = case(7, g, ())
    a = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=512, gq_weight_dtype="uint4", gq_group_size=g,
                                gq_expert_dtype="none")
    b = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=4, max_batch_tokens=512)
    assert b.lib.nvl_set_gq_weight_dtype(b.h, 1, g) == 0
    for (slot, li), t in w.items():
        b.upload(slot, li, t)
    c = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4", gq_group_size=g)
    assert c.lib.nvl_set_gq_expert_dtype(c.h, 1) == 0 and c.lib.nvl_set_gq_expert_dtype(c.h, 0) == 0      # set, then taken back
    for slot in EXPERTS:
        t = np.asarray(w[(slot, 0)], np.float32)
        for hm in (b, c):
            if hm is c:
                hm.upload(slot, 0, t)
            back = get_weight(gpu, hm, slot, 0, t.shape[2], t.shape[0] * t.shape[1]).T
            assert np.array_equal(back.view(np.uint32), bf16_rne(t.reshape(-1, t.shape[2])).view(np.uint32)), slot
    c.close()
    b.finalize()
    la, lb = run_both(a, b, cfg, 9, n=50)
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    e4 = build(gpu)[3]
    le, la = run_both(e4, a, cfg, 9, n=50, seq=1)
    assert not np.array_equal(le[0], la[0]) and not np.array_equal(le[-1], la[-1])
    a.close(); b.close(); e4.close()


@pytest.mark.parametrize("g", [32, 64])
def test_weight_bytes(gpu, g):
    """nvl_stats.weight_bytes = per INT4-stored tensor, padded rows x (in / 2 + 4 * in / g) — the experts as [E * out][in] —
    + bf16 for the other 2-D tensors + fp32 for the 1-D ones; below the bf16-expert figure by the experts' difference"""
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    wb = {}
    for ge in ("none", "uint4"):
        hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, gq_weight_dtype="uint4", gq_group_size=g,
                                     gq_expert_dtype=ge)
        wb[ge] = hm.stats()["weight_bytes"]
        hm.close()
    want, saved = 0, 0
    for (slot, li), a in w.items():
        a = np.asarray(a)
        if a.ndim == 1:
            want += a.size * 4
        elif slot in EXPERTS:                                  # [E, out, in]
            rows, k = rup(a.shape[0] * a.shape[1]), a.shape[2]
            want += rows * (k // 2 + 4 * (k // g))
            saved += rows * k * 2 - rows * (k // 2 + 4 * (k // g))
        elif slot in QUANTIZED:                                # [in, out]
            want += rup(a.shape[1]) * (a.shape[0] // 2 + 4 * (a.shape[0] // g))
        elif slot == "tok_emb":                                # [V][H]
            want += rup(a.shape[0]) * a.shape[1] * 2
        else:                                                  # router [in, out]
            want += rup(a.shape[1]) * a.shape[0] * 2
    assert wb["uint4"] == want, (wb, want)
    assert wb["none"] - wb["uint4"] == saved and saved > 0, (wb, saved)


def test_setter_errors(gpu):
    moe = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(moe, seed=1, scale=0.05)
    mk = lambda cfg=moe, **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, **kw)

    hm = mk()
    ge, gq = hm.lib.nvl_set_gq_expert_dtype, hm.lib.nvl_set_gq_weight_dtype
    assert ge(hm.h, 1) == -1                                              # wrong order: no INT4 projection weights yet
    assert gq(hm.h, 1, 128) == 0
    assert ge(hm.h, 1) == -1                                              # g = 128 on I = 64: a group would straddle two experts
    assert gq(hm.h, 1, 64) == 0
    assert ge(hm.h, 7) == -1                                              # unknown value
    assert ge(hm.h, 1) == 0 and ge(hm.h, 0) == 0
    assert gq(hm.h, 0, 64) == 0 and ge(hm.h, 1) == -1                     # INT4 weights taken back: none to follow
    assert gq(hm.h, 1, 64) == 0 and ge(hm.h, 1) == 0
    assert gq(hm.h, 0, 64) == -1                                          # NVL_GQ_NONE refused while INT4 experts are set
    assert gq(hm.h, 1, 32) == -1                                          # ... and another group size
    assert gq(hm.h, 1, 64) == 0
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == -1                     # the fp8 and MXFP4 expert forms stay refused on an INT4 model
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == -1
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == -1 and hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == -1
    hm.upload("moe_in", 0, w[("moe_in", 0)])
    assert ge(hm.h, 0) == -7                                              # after the first expert upload
    hm.close()

    hm = mk(gq_weight_dtype="uint4", gq_group_size=64)
    hm.upload("moe_out", 0, w[("moe_out", 0)])                            # a bf16 expert upload fixes the dtype too
    assert hm.lib.nvl_set_gq_expert_dtype(hm.h, 1) == -7
    hm.close()
    fin = build(gpu, ge="none")[3]                                        # after nvl_finalize
    assert fin.lib.nvl_set_gq_expert_dtype(fin.h, 1) == -7
    fin.close()
    with pytest.raises(gpu.NvlError) as e:                                # a model without MoE
        mk(gpu.synth.tiny_config("llama"), gq_weight_dtype="uint4", gq_group_size=64, gq_expert_dtype="uint4")
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:                                # g = 128 on I = 64 through the Python option
        mk(gq_weight_dtype="uint4", gq_group_size=128, gq_expert_dtype="uint4")
    assert e.value.code == -1
    h32 = gpu.HipTransformerModel(moe, None, precision="f32", max_seqs=2, max_batch_tokens=64)
    assert h32.lib.nvl_set_gq_expert_dtype(h32.h, 1) == -1                # f32 precision
    h32.close()
    h4 = mk(gq_weight_dtype="uint4", gq_group_size=64, gq_expert_dtype="uint4")
    for slot, bad_at, val in (("moe_out", (2, 3, 4), np.inf), ("moe_in", (1, 5, 6), np.nan), ("moe_in", (0, 7, 9), 1.0e6)):
        bad = np.array(w[(slot, 1)], np.float32)                          # a non-finite expert weight, and r / 15 > 65504
        bad[bad_at] = val
        with pytest.raises(gpu.NvlError) as e:
            h4.upload(slot, 1, bad)
        assert e.value.code == -1
    h4.close()
