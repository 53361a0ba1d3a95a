"""MXFP4 MoE expert weights (mx_expert_dtype="fp4_e2m1", nvl_set_mx_expert_dtype): the upload
quantizer against the numpy mirror of the MXFP4 contract (one e8m0 scale per 32 input features of an expert's output row),
the model against the oracle run on W~ across the decode forms (narrow / wide up, K-split down at U = 4 / 2), the grouped
prefill paths and grouped decode on dequantized W~, the identities that stay bit-exact, the pre-quantized upload, the
setter's errors and the weight bytes."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from test_mxfp4_weights_gpu import BF16_TOL, FP8_KV_TOL, bf16_rne, crafted, get_weight, ref_mx, tilde

pytestmark = pytest.mark.gpu
EXPERTS = ("moe_in", "moe_out")
GRANITE_1B_LAYERS = dict(hidden=1024, num_heads=16, num_kv_heads=8, head_dim=64, ffn_dim=512, num_experts=32,
                         num_experts_per_tok=8, num_layers=2)


def rup(n, m=256):
    return (n + m - 1) // m * m


def tilde_e4(cfg, w):
    """the weights an MXFP4-expert model computes with: tilde() of the projections plus W~ of every expert row"""
    out = tilde(cfg, w)
    for (slot, li), a in w.items():
        if slot in EXPERTS:
            a = np.asarray(a, np.float32)
            out[(slot, li)] = ref_mx(a.reshape(-1, a.shape[2]))[2].reshape(a.shape)
    return out


def build(gpu, me="fp4_e2m1", seed=7, paged=False, kv="auto", mbt=512, max_seqs=4, **over):
    cfg = gpu.synth.tiny_config("granite_moe", **over)
    w = gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=max_seqs, max_batch_tokens=mbt, mx_weight_dtype="fp4_e2m1",
                                 mx_expert_dtype=me, kv_cache_dtype=kv, **kw)
    return cfg, w, hm


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


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_expert_quantizer_read_back(gpu, dtype):
    """nvl_get_weight of moe_in / moe_out equals W~ of the numpy mirror bit for bit, per-expert crafted rows (zeros, ties,
    saturation, an outlier, both exponent clamps) included; 5 experts x 2*64 rows = 640 rows: the last row tile is padded"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
    rng = np.random.default_rng(0)
    hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1",
                                 mx_expert_dtype="fp4_e2m1")
    sent = {}
    for (slot, li), a in w.items():
        a = np.asarray(a, np.float32)
        if slot in EXPERTS:
            a = np.stack([crafted(rng, a.shape[2], a.shape[1], extremes=True).T for _ in range(a.shape[0])])     # [E, out, in]
        t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
        sent[(slot, li)] = t.float().numpy()
        hm.upload(slot, li, t)
    checked = 0
    for (slot, li), a in sent.items():
        if slot not in EXPERTS:
            continue
        E, n_out, n_in = a.shape
        assert slot != "moe_in" or (E * n_out) % 256 != 0
        got = get_weight(gpu, hm, slot, li, n_in, E * n_out).T
        want = ref_mx(a.reshape(E * n_out, n_in))[2]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (slot, li)
        checked += 1
    assert checked == 2 * cfg["num_layers"]
    hm.close()


@pytest.mark.parametrize("over,prompt_len", [
    ({}, 60),                                  # tiny: decode down MT = 4 (U = 2) at 60 rows, ragged tails only
    ({}, 100),                                 # tiny prefill beyond 64 rows: 128-row grouped GEMMs on W~
    ({"ffn_dim": 256}, 20),                    # I = 256: down form at 20 rows (MT = 2, U = 4)
    ({"ffn_dim": 256}, 40),                    # ... at 40 rows (U = 2, 4 blocks, M % 16 != 0)
    ({"ffn_dim": 256}, 100),                   # H, 2I % 256 == 0, H, I >= 160: the ping-pong grouped prefill
    (GRANITE_1B_LAYERS, 8),                    # Granite-1B layer shape: narrow up + K-split down at MT = 1
    (GRANITE_1B_LAYERS, 30),                   # ... the wide up form (2 tiles per wave) and down at MT = 2
])
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, over, prompt_len):
    """prefill + 12 decode steps; prompts of <= 64 rows run the decode forms in the prefill as well"""
    cfg, w, hm = build(gpu, **over)
    err = against_oracle(oracle, cfg, tilde_e4(cfg, w), hm, prompt_len)
    print(f"{over} {prompt_len}: max rel err vs oracle on W~ {err:.3e}")
    hm.close()


def test_grouped_decode_key_22(gpu, oracle):
    """key 22 = 0: decode through the planning launch and the grouped GEMMs on dequantized W~"""
    with with_tuning(gpu, 22, 0):
        cfg, w, hm = build(gpu)
        against_oracle(oracle, cfg, tilde_e4(cfg, w), hm, 30)
        hm.close()


def test_deferred_down_conditions_with_key_33(gpu, oracle):
    """E = 16, I = 128 meets the deferred-norm producer's conditions; with key 33 = 1 the MXFP4 experts take the K-split form"""
    with with_tuning(gpu, 33, 1):
        cfg, w, hm = build(gpu, num_experts=16, ffn_dim=128)
        against_oracle(oracle, cfg, tilde_e4(cfg, w), hm, 30)
        hm.close()


def test_down_block_mask_large_expert_width(gpu, oracle):
    """I = 8192: more blocks per expert than the decode down form's 32-bit live-block mask holds; such widths take the grouped
    form (on dequantized W~) and match the oracle"""
    cfg = gpu.synth.tiny_config("granite_moe", hidden=128, num_heads=2, num_kv_heads=2, num_experts=4, ffn_dim=8192)
    w = gpu.synth.make_weights(cfg, seed=9, scale=0.02)
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1",
                                 mx_expert_dtype="fp4_e2m1")
    wt = tilde_e4(cfg, w)
    for n in (8, 48):
        hm.seq_reset(0)
        against_oracle(oracle, cfg, wt, hm, n, steps=2, seed=n)
    hm.close()


def test_with_fp8_kv_against_the_oracle(gpu, oracle):
    cfg, w, hm = build(gpu, kv="fp8_e4m3")
    against_oracle(oracle, cfg, tilde_e4(cfg, w), hm, 40, steps=8, tol=FP8_KV_TOL)
    hm.close()


@pytest.mark.parametrize("kv", ["auto", "fp8_e4m3"])
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, kv):
    cfg, _, hm = build(gpu, kv=kv)
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
    cfg, _, slab = build(gpu, kv=kv)
    _, _, paged = build(gpu, kv=kv, paged=True)
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


def run_both(a, b, cfg, seed, n=70, steps=4, seq=0):
    """prefill + decode logits of two models, as two lists"""
    prompt = np.random.default_rng(seed).integers(0, cfg["vocab_size"], n).tolist()
    la, lb = [a.forward_with_cache(prompt, seq, 0, all_logits=True)], [b.forward_with_cache(prompt, seq, 0, all_logits=True)]
    for step in range(steps):
        la.append(a.forward_with_cache([step + 1], seq, n + step, all_logits=False))
        lb.append(b.forward_with_cache([step + 1], seq, n + step, all_logits=False))
    return la, lb


def test_prequantized_upload(gpu):
    """the mirror's codes and scales through nvl_upload_tensor_mxfp4 — experts as [E * out][in / 2] and [E * out][in / 32] — give
    the logits and the weight bytes of the float upload bit for bit, and the experts read back as W~"""
    cfg = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    mk = lambda: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, mx_weight_dtype="fp4_e2m1",
                                         mx_expert_dtype="fp4_e2m1")
    a, b = mk(), mk()
    for (slot, li), t in w.items():
        a.upload(slot, li, t)
        t = np.asarray(t, np.float32)
        if slot in EXPERTS:
            codes, scales, want = ref_mx(t.reshape(-1, t.shape[2]))
            b.upload_mxfp4(slot, li, codes, scales)
            back = get_weight(gpu, b, slot, li, t.shape[2], t.shape[0] * t.shape[1]).T
            assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), slot
        elif slot in ("wq", "wk", "wv", "wo"):                 # [in, out]
            codes, scales, _ = ref_mx(t.T)
            b.upload_mxfp4(slot, li, codes, scales)
        else:
            b.upload(slot, li, t)
    a.finalize(); b.finalize()
    la, lb = run_both(a, b, cfg, 3)
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    a.close(); b.close()


def test_a_model_without_the_call_is_todays_mxfp4_model(gpu):
    """mx_expert_dtype="none" leaves the MXFP4-projection model with bf16 experts: logits bit-identical to a second model of the
    same process that never calls the setter, prefill and decode, and the same weight bytes; the MXFP4-expert model differs"""
    cfg, w, a = build(gpu, me="none")
    b = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=4, max_batch_tokens=512)
    assert b.lib.nvl_set_mx_weight_dtype(b.h, 1) == 0
    for (slot, li), t in w.items():
        b.upload(slot, li, t)
    b.finalize()
    la, lb = run_both(a, b, cfg, 9, n=50)
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    assert a.stats()["weight_bytes"] == b.stats()["weight_bytes"]
    e4 = build(gpu)[2]
    le, la = run_both(e4, a, cfg, 9, n=50, seq=1)
    assert not np.array_equal(le[0], la[0]) and not np.array_equal(le[-1], la[-1])
    a.close(); b.close(); e4.close()


def test_weight_bytes(gpu):
    """the experts' codes + scales replace their bf16 bytes exactly (rows padded to 256 per uploaded tensor)"""
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    wb = {}
    for me in ("none", "fp4_e2m1"):
        hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, mx_weight_dtype="fp4_e2m1",
                                     mx_expert_dtype=me)
        wb[me] = hm.stats()["weight_bytes"]
        hm.close()
    E, H, I = cfg["num_experts"], cfg["hidden"], cfg["ffn_dim"]
    saved = 0
    for rows, k in ((E * 2 * I, H), (E * H, I)):
        saved += rup(rows) * k * 2 - (rup(rows) * k // 2 + rup(rows) * k // 32)
    assert wb["none"] - wb["fp4_e2m1"] == saved * cfg["num_layers"], wb


def test_setter_errors(gpu):
    L = gpu._lib
    moe = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(moe, seed=1, scale=0.05)
    mk = lambda cfg=moe, **kw: gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, **kw)
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    a = np.asarray(w[("moe_in", 0)], np.float32)
    codes, scales, _ = ref_mx(a.reshape(-1, a.shape[2]))
    n, k = codes.shape[0], codes.shape[1] * 2

    hm = mk()
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == -1                  # no MXFP4 projection weights
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 7) == -1                  # unknown value
    # without the mode the pre-quantized upload still refuses the expert kinds
    assert hm.lib.nvl_upload_tensor_mxfp4(hm.h, L.SLOT_ID["moe_in"], 0, p(codes), p(scales), n, k, L.LAYOUT_OUT_IN) == -1
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_mx_expert_dtype(hm.h, 0) == 0
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 0) == 0 and hm.lib.nvl_set_mx_weight_dtype(hm.h, 1) == 0
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == 0
    assert hm.lib.nvl_set_mx_weight_dtype(hm.h, 0) == -1                  # refused while MX experts are set
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == -1                     # the fp8 expert form stays refused on an MX model
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == -1
    # the pre-quantized upload's refusals, then a good one
    up = lambda c, s, rows, cols, layout=L.LAYOUT_OUT_IN: hm.lib.nvl_upload_tensor_mxfp4(hm.h, L.SLOT_ID["moe_in"], 0, p(c), p(s), rows, cols, layout)
    assert up(codes, scales, n - 16, k) == -1 and up(codes, scales, n, k - 32) == -1      # shape mismatch
    assert up(codes, scales, n, k - 16) == -1                             # cols % 32 != 0 (a shape mismatch as well)
    assert up(codes, scales, n, k, L.LAYOUT_IN_OUT) == -1
    for byte in (0xFF, 6, 253, 0):
        s2 = scales.copy()
        s2[3, 1] = byte
        assert up(codes, s2, n, k) == -1, byte
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 0) == 0 and hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == 0   # (no upload yet)
    assert up(codes, scales, n, k) == 0
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 0) == -7                  # after the first expert upload
    hm.close()

    hm = mk(mx_weight_dtype="fp4_e2m1")
    hm.upload("moe_out", 0, w[("moe_out", 0)])                            # a bf16 expert upload fixes the dtype too
    assert hm.lib.nvl_set_mx_expert_dtype(hm.h, 1) == -7
    hm.close()
    cfg, wf, fin = build(gpu, me="none")                                  # after nvl_finalize
    assert fin.lib.nvl_set_mx_expert_dtype(fin.h, 1) == -7
    fin.close()
    with pytest.raises(gpu.NvlError) as e:                                # a model without MoE
        mk(gpu.synth.tiny_config("llama"), mx_weight_dtype="fp4_e2m1", mx_expert_dtype="fp4_e2m1")
    assert e.value.code == -1
    h32 = gpu.HipTransformerModel(moe, None, precision="f32", max_seqs=2, max_batch_tokens=64)
    assert h32.lib.nvl_set_mx_expert_dtype(h32.h, 1) == -1                # f32 precision
    h32.close()
    h4 = mk(mx_weight_dtype="fp4_e2m1", mx_expert_dtype="fp4_e2m1")       # a non-finite expert weight is refused
    for slot, bad_at in (("moe_out", (2, 3, 4)), ("moe_in", (1, 5, 6))):
        bad = np.array(w[(slot, 1)], np.float32)
        bad[bad_at] = np.inf if slot == "moe_out" else np.nan
        with pytest.raises(gpu.NvlError) as e:
            h4.upload(slot, 1, bad)
        assert e.value.code == -1
    h4.close()
