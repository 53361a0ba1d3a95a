"""8-bit (e4m3fn) MoE expert weights (expert_dtype="fp8_e4m3", nvl_set_expert_dtype): the upload
quantizer against the numpy restatement of the contract (one scale per expert and output row), the model against the oracle
run on W~ across the decode forms (wide up, K-split down at U = 4 / 2), the grouped prefill paths (ping-pong, 128-row tiles)
and grouped decode, the identities that stay bit-exact, the weight bytes, the FP8 MoE checkpoint loader, and the decode
down form's 32-block mask (I = 8192 takes the grouped form, in bf16 and 8-bit mode)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import rel_err
from test_fp8_weights_gpu import BF16_TOL, FP8_KV_TOL, bf16_rne, crafted, get_weight, ref_w8, tilde
from test_kv_fp8_gpu import VALUES, ref_quant

pytestmark = pytest.mark.gpu
EXPERTS = ("moe_in", "moe_out")


def rup(n, m=256):
    return (n + m - 1) // m * m


def tilde_e8(cfg, w):
    """the weights an fp8-expert model computes with: tilde() of the projections plus W~ of every expert row"""
    out = tilde(cfg, w)
    for (slot, li), a in w.items():
        if slot in EXPERTS:
            a = np.asarray(a, np.float32)
            out[(slot, li)] = ref_w8(a.reshape(-1, a.shape[2]))[2].reshape(a.shape)
    return out


def build(gpu, ed="fp8_e4m3", seed=7, paged=False, kv="auto", act="auto", wd="fp8_e4m3", mbt=512, max_seqs=4, **over):
    cfg = gpu.synth.tiny_config("granite_moe", **over)
    w = gpu.synth.make_weights(cfg, seed=seed, scale=0.05)
    kw = dict(kv_num_blocks=24, kv_block_size=64) if paged else {}
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=max_seqs, max_batch_tokens=mbt, weight_dtype=wd,
                                 expert_dtype=ed, kv_cache_dtype=kv, act_dtype=act, **kw)
    return cfg, w, hm


def with_tuning(gpu, key, value):
    class _T:
        def __enter__(self):
            self.old = gpu.lib().nvl_set_tuning(key, value)

        def __exit__(self, *a):
            gpu.lib().nvl_set_tuning(key, self.old)
    return _T()


def against_oracle(oracle, cfg, wt, hm, prompt_len, steps=12, seed=1, tol=BF16_TOL):
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
    assert max(errs) <= tol, errs
    return max(errs)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_expert_quantizer_read_back(gpu, dtype):
    """nvl_get_weight of moe_in / moe_out equals W~ of the numpy restatement bit for bit, per-expert crafted rows (a zero
    row, exact midpoints, an outlier) included; 5 experts x 2*64 rows = 640 rows: the last row tile is padded"""
    import torch
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=3, scale=0.05)
    rng = np.random.default_rng(0)
    hm = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3",
                                 expert_dtype="fp8_e4m3")
    sent = {}
    for (slot, li), a in w.items():
        a = np.asarray(a, np.float32)
        if slot in EXPERTS:
            a = np.stack([crafted(rng, a.shape[2], a.shape[1]).T for _ in range(a.shape[0])])     # [E, out, in]
        t = torch.from_numpy(np.ascontiguousarray(a)).to(tdt)
        sent[(slot, li)] = t.float().numpy()
        hm.upload(slot, li, t)
    for (slot, li), a in sent.items():
        if slot not in EXPERTS:
            continue
        E, n_out, n_in = a.shape
        assert slot != "moe_in" or (E * n_out) % 256 != 0
        got = get_weight(gpu, hm, slot, li, n_in, E * n_out).T
        want = ref_w8(a.reshape(E * n_out, n_in))[2]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (slot, li)
    hm.close()


@pytest.mark.parametrize("over,prompt_len", [
    ({}, 60),                                  # tiny: decode down MT = 4 (U = 2) at 60 rows, ragged tails only
    ({}, 100),                                 # tiny prefill beyond 64 rows: 128-row grouped GEMMs on W~
    ({"ffn_dim": 256}, 40),                    # I = 256: down form at 40 rows (U = 2, 4 blocks, M % 16 != 0)
    ({"ffn_dim": 256}, 20),                    # ... at 20 rows (MT = 2, U = 4)
    ({"ffn_dim": 256}, 100),                   # H, 2I % 256 == 0, H, I >= 160: the ping-pong grouped prefill
])
def test_logits_against_the_oracle_on_w_tilde(gpu, oracle, over, prompt_len):
    cfg, w, hm = build(gpu, **over)
    err = against_oracle(oracle, cfg, tilde_e8(cfg, w), hm, prompt_len)
    print(f"{over} {prompt_len}: max rel err vs oracle on W~ {err:.3e}")
    hm.close()


def test_deferred_down_conditions_with_key_33(gpu, oracle):
    """E = 16, I = 128 meets the deferred-norm producer's conditions; with key 33 = 1 the 8-bit experts take the K-split form"""
    with with_tuning(gpu, 33, 1):
        cfg, w, hm = build(gpu, num_experts=16, ffn_dim=128)
        against_oracle(oracle, cfg, tilde_e8(cfg, w), hm, 30)
        hm.close()


def test_grouped_decode_key_22(gpu, oracle):
    """key 22 = 0: decode through the planning launch and the grouped GEMMs on W~"""
    with with_tuning(gpu, 22, 0):
        cfg, w, hm = build(gpu)
        against_oracle(oracle, cfg, tilde_e8(cfg, w), hm, 30)
        hm.close()


def test_with_fp8_kv_against_the_oracle(gpu, oracle):
    cfg, w, hm = build(gpu, kv="fp8_e4m3")
    against_oracle(oracle, cfg, tilde_e8(cfg, w), hm, 40, steps=8, tol=FP8_KV_TOL)
    hm.close()


@pytest.mark.parametrize("kv,act", [("auto", "auto"), ("fp8_e4m3", "auto"), ("auto", "fp8_e4m3")])
def test_decode_greedy_and_graph_replay_equal_stepwise(gpu, kv, act):
    cfg, _, hm = build(gpu, kv=kv, act=act)
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


@pytest.mark.parametrize("kv,act", [("auto", "auto"), ("fp8_e4m3", "auto"), ("auto", "fp8_e4m3")])
def test_paged_equals_slab_and_prefix_hit(gpu, kv, act):
    cfg, _, slab = build(gpu, kv=kv, act=act)
    _, _, paged = build(gpu, kv=kv, act=act, paged=True)
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


def test_weight_bytes(gpu):
    """the experts' codes + scales replace their bf16 bytes exactly (rows padded to 256 per uploaded tensor)"""
    cfg = gpu.synth.tiny_config("granite_moe", num_experts=5, ffn_dim=64)
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    wb = {}
    for ed in ("auto", "fp8_e4m3"):
        hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3",
                                     expert_dtype=ed)
        wb[ed] = hm.stats()["weight_bytes"]
        hm.close()
    E, H, I = cfg["num_experts"], cfg["hidden"], cfg["ffn_dim"]
    saved = 0
    for rows, k in ((E * 2 * I, H), (E * H, I)):
        saved += rup(rows) * k * 2 - (rup(rows) * k + 4 * rup(rows))
    assert wb["auto"] - wb["fp8_e4m3"] == saved * cfg["num_layers"], wb


def test_setter_errors(gpu):
    L = gpu._lib
    moe = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(moe, seed=1, scale=0.05)
    hm = gpu.HipTransformerModel(moe, None, precision="bf16", max_seqs=2, max_batch_tokens=64)
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == -1                     # no 8-bit projection weights
    assert hm.lib.nvl_set_weight_dtype(hm.h, 1) == 0
    assert hm.lib.nvl_set_expert_dtype(hm.h, 7) == -1                     # unknown value
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == 0 and hm.lib.nvl_set_expert_dtype(hm.h, 0) == 0
    assert hm.lib.nvl_set_expert_dtype(hm.h, 1) == 0
    hm.upload("moe_in", 0, w[("moe_in", 0)])
    assert hm.lib.nvl_set_expert_dtype(hm.h, 0) == -7                     # after the first expert upload
    hm.close()
    with pytest.raises(gpu.NvlError) as e:                                # a model without MoE
        gpu.HipTransformerModel(gpu.synth.tiny_config("llama"), None, weight_dtype="fp8_e4m3", expert_dtype="fp8_e4m3")
    assert e.value.code == -1
    h32 = gpu.HipTransformerModel(moe, None, precision="f32", max_seqs=2, max_batch_tokens=64)
    assert h32.lib.nvl_set_expert_dtype(h32.h, 1) == -1                   # f32 precision
    h32.close()
    # a non-finite expert weight is refused
    h8 = gpu.HipTransformerModel(moe, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3",
                                 expert_dtype="fp8_e4m3")
    bad = np.array(w[("moe_out", 1)], np.float32)
    bad[2, 3, 4] = np.inf
    with pytest.raises(gpu.NvlError) as e:
        h8.upload("moe_out", 1, bad)
    assert e.value.code == -1
    h8.close()


@pytest.mark.parametrize("ed", ["auto", "fp8_e4m3"])
def test_down_block_mask_large_expert_width(gpu, oracle, ed):
    """I = 8192: an expert is 256 k-steps, 64 blocks at U = 4 (8 rows) and 128 at U = 2 (48 rows) — more than the decode down
    form's 32-bit live-block mask holds; such widths take the grouped form and match the oracle"""
    cfg = gpu.synth.tiny_config("granite_moe", hidden=128, num_heads=2, num_kv_heads=2, num_experts=4, ffn_dim=8192)
    w = gpu.synth.make_weights(cfg, seed=9, scale=0.02)
    wd = "fp8_e4m3" if ed != "auto" else "auto"
    hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype=wd, expert_dtype=ed)
    wt = tilde_e8(cfg, w) if ed != "auto" else w
    for n in (8, 48):
        hm.seq_reset(0)
        against_oracle(oracle, cfg, wt, hm, n, steps=2, seed=n)
    hm.close()


# ---- FP8 MoE checkpoints ---------------------------------------------------------------------------------------------------
def write_fp8_moe(dirname, cfg, w, scale_form="row", poison=False):
    """Granite-MoE checkpoint whose expert weights are F8_E4M3 [E, out, in] with a weight_scale of `scale_form`:
    "row" ([E, out] F32), "row1" ([E, out, 1] BF16), "expert" ([E] F32), "expert11" ([E, 1, 1] BF16), "scalar", "block"
    ([E, out/16, in/16]: refused).  -> {(slot, layer): (codes [E*out][in], scales [E*out], W~ [E, out, in])}"""
    import torch
    from safetensors.torch import save_file
    from make_checkpoint import HF_CONFIG, to_hf_names
    os.makedirs(dirname, exist_ok=True)
    named = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in to_hf_names(cfg, w, "granite_moe").items()}
    out = {}
    for (slot, li), a in w.items():
        if slot not in EXPERTS:
            continue
        name = f"model.layers.{li}.block_sparse_moe." + ("input_linear.weight" if slot == "moe_in" else "output_linear.weight")
        a = np.asarray(a, np.float32)
        E, n_out, n_in = a.shape
        if scale_form in ("row", "row1", "block"):
            s = (np.abs(a).max(axis=2) / np.float32(448)).astype(np.float32)                          # [E, out]
            st = torch.from_numpy(s) if scale_form != "row1" else torch.from_numpy(s[:, :, None]).to(torch.bfloat16)
            if scale_form == "block":
                st = torch.ones(E, n_out // 16, n_in // 16)
        elif scale_form in ("expert", "expert11"):
            s = np.repeat((np.abs(a).max(axis=(1, 2)) / np.float32(448)).astype(np.float32)[:, None], n_out, axis=1)
            st = torch.from_numpy(s[:, 0].copy()) if scale_form == "expert" else torch.from_numpy(s[:, :1, None].copy()).to(torch.bfloat16)
        else:
            s = np.full((E, n_out), np.abs(a).max() / np.float32(448), np.float32)
            st = torch.tensor(float(s[0, 0]), dtype=torch.float32)
        if scale_form in ("row1", "expert11"):
            s = np.broadcast_to(st.float().numpy().reshape(E, -1), (E, n_out)).astype(np.float32)      # what the file holds
        codes = ref_quant(a, s[:, :, None])
        if poison and slot == "moe_out" and li == 0:
            codes = codes.copy()
            codes[1, 2, 3] = 0xFF
        named[name] = torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn)
        named[name + "_scale"] = st.contiguous()
        wt = bf16_rne(VALUES[codes].astype(np.float32) * s[:, :, None])
        out[(slot, li)] = (codes.reshape(E * n_out, n_in), s.reshape(-1), wt)
    with open(os.path.join(dirname, "config.json"), "w") as f:
        json.dump(HF_CONFIG["granite_moe"](cfg), f)
    save_file({k: v.contiguous() for k, v in named.items()}, os.path.join(dirname, "model.safetensors"), metadata={"format": "pt"})
    return out


@pytest.mark.parametrize("scale_form", ["row", "row1", "expert", "expert11", "scalar"])
def test_fp8_moe_checkpoint(gpu, oracle, tmp_path, scale_form):
    """into an fp8-expert model the codes and scales go in as they are (read back: W~); into a bf16 model and an fp8
    projections-only model the experts go in as W~; the fp8-expert model matches the oracle on W~"""
    cfg = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    got = write_fp8_moe(str(tmp_path), cfg, w, scale_form)
    for wd, ed in (("fp8_e4m3", "fp8_e4m3"), ("fp8_e4m3", "auto"), ("auto", "auto")):
        m = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=128, weight_dtype=wd,
                                    expert_dtype=ed)
        gpu._lib.check(m.lib.nvl_load_safetensors(m.h, str(tmp_path).encode()), m.h)
        for (slot, li), (codes, s, wt) in got.items():
            E, n_out, n_in = wt.shape
            back = get_weight(gpu, m, slot, li, n_in, E * n_out).T
            assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(wt.reshape(E * n_out, n_in)).view(np.uint32)), (wd, ed, slot)
        m.close()
    hm = gpu.HipTransformerModel.from_pretrained(str(tmp_path), precision="bf16", max_seqs=2, max_batch_tokens=128,
                                                 weight_dtype="fp8_e4m3", expert_dtype="fp8_e4m3")
    wt = tilde(cfg, w)
    for (slot, li), (_, _, t) in got.items():
        wt[(slot, li)] = t
    against_oracle(oracle, cfg, wt, hm, 30, steps=4)
    hm.close()


def test_fp8_moe_checkpoint_refusals(gpu, tmp_path):
    cfg = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(cfg, seed=5, scale=0.05)
    for name, kw, needle in (("block", dict(scale_form="block"), "block-wise"), ("nan", dict(poison=True), "NaN")):
        d = str(tmp_path / name)
        write_fp8_moe(d, cfg, w, **kw)
        for ed in ("fp8_e4m3", "auto"):
            with pytest.raises(gpu.NvlError) as e:
                gpu.HipTransformerModel.from_pretrained(d, precision="bf16", max_seqs=2, max_batch_tokens=128,
                                                        weight_dtype="fp8_e4m3", expert_dtype=ed)
            assert needle in str(e.value), str(e.value)


def test_upload_tensor_fp8_experts(gpu):
    """nvl_upload_tensor_fp8 takes MOE_IN / MOE_OUT as rows = E * out, cols = in, scales [E * out]"""
    cfg = gpu.synth.tiny_config("granite_moe")
    w = gpu.synth.make_weights(cfg, seed=2, scale=0.05)
    m = gpu.HipTransformerModel(cfg, None, precision="bf16", max_seqs=2, max_batch_tokens=64, weight_dtype="fp8_e4m3",
                                expert_dtype="fp8_e4m3")
    for slot in EXPERTS:
        a = np.asarray(w[(slot, 0)], np.float32)
        E, n_out, n_in = a.shape
        codes, s, want = ref_w8(a.reshape(E * n_out, n_in))
        codes = np.ascontiguousarray(codes, np.uint8)
        rc = m.lib.nvl_upload_tensor_fp8(m.h, gpu._lib.SLOT_ID[slot], 0, codes.ctypes.data_as(C.c_void_p),
                                         s.ctypes.data_as(C.c_void_p), E * n_out, n_in, gpu._lib.LAYOUT_OUT_IN)
        gpu._lib.check(rc, m.h)
        back = get_weight(gpu, m, slot, 0, n_in, E * n_out).T
        assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), slot
        bad = m.lib.nvl_upload_tensor_fp8(m.h, gpu._lib.SLOT_ID[slot], 0, codes.ctypes.data_as(C.c_void_p),
                                          s.ctypes.data_as(C.c_void_p), E * n_out - 1, n_in, gpu._lib.LAYOUT_OUT_IN)
        assert bad == -1
    m.close()
