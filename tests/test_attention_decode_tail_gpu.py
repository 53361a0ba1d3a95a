"""The tail of the fused decode attention (attn.h attn_decode_bf16_kernel<64, 8, true>) at the operating point the
benchmark runs it at: hd 64, a GQA group of 4, 8 waves per workgroup, 8-11 key tiles — where some waves hold two tiles
and the others one, the newest key's tile is a two-tile wave's second, and the last waves append the new row and combine.

Op level (nvl_op_attention_batch, helpers and ATTN_RATIO_BOUND of test_attention_ops_gpu.py, the float64 statement of
attention_reference.py): the newest key at 0, 62, 63, 64, 511, 512, 513, 575, 576, 639, 640 and 703 — one tile, the new
key first / last in its tile, exactly 8 tiles (no wave holds two), 9 and 10 tiles (waves 0 / 1 hold two), 11 tiles — two or
three sequences per launch, one launch with 2, 9 and 11 tiles side by side and 64-key blocks; with and without RoPE;
non-temporal K/V loads off and on (key 35 = 0 / 2).  Per launch: the form and launch shape that ran, both bf16 bounds,
the appended rows, and a second run bit-identical to the first.

The appended rows are the cache as the op reads it back after the launch.  V: bit-equal to bf16(v).  K without RoPE:
bit-equal to the row (it is bf16-exact).  K with RoPE: the kernel rotates in fp32, the reference in float64, so they may
round differently where the float64 value lies within the fp32 arithmetic's error of a bf16 rounding boundary.  That error
is at most three fp32 roundings of terms no larger than |a| + |b| (two products and a sum, or a product and a fused
multiply-add, plus the table entry's own rounding): below m = 2^-22 (|a| + |b|).  Every element with bf16(x - m) == bf16(x + m)
must therefore equal bf16(x) exactly — and these are more than 9 in 10 of the elements (m is 2^-14 of a bf16 step's
relative size) — and the others lie within one bf16 step (check_append).

Model level (a two-layer Llama with 8 query heads over 2 kv heads; contexts 64, 513 and 640 in one batch, 8 waves
forced): decode steps with every launch eager against hipGraph replay (key 21 = 0 / 1) give bit-identical logits, greedy
tokens and — read back with nvl_get_kv — bit-identical, finite appended K / V rows in every layer."""
import numpy as np
import pytest

import attention_reference as R
from test_attention_ops_gpu import ATTN_RATIO_BOUND, ran_as, run

pytestmark = pytest.mark.gpu

NW8 = {15: 8}
TAIL_CASES = {
    "T1": R._c(block=256, pos=(0, 62, 63), expect=(8, 1)),        # one tile: empty cache, the new key last but one / last in its tile
    "T2": R._c(block=256, pos=(64, 511, 512), expect=(8, 1)),     # first key of tile 1; exactly 8 tiles; 9 tiles, the new key first
    "T3": R._c(block=256, pos=(513, 575, 576), expect=(8, 1)),    # 9 tiles, the new key second / last; 10 tiles, the new key first
    "T4": R._c(block=256, pos=(639, 640, 703), expect=(8, 1)),    # 10 tiles, the new key last; 11 tiles, the new key first / last
    "T5": R._c(block=64, pos=(64, 513, 640), expect=(8, 1)),      # 2, 9 and 11 tiles in one launch; every tile its own block
}
R.ALL_CASES.update(TAIL_CASES)
FORMS = ["fused", "fused_norope"]


def appended_k_exact(b, res):
    """-> (elements compared exactly, elements of the appended K rows): see the module docstring"""
    nH, nKV, hd = b["nH"], b["nKV"], b["hd"]
    decided = total = 0
    for i, (blk, row) in enumerate(b["new_rows"]):
        pos = b["seq_pos"][i]
        raw = np.asarray(b["q"][i][nH * hd:(nH + nKV) * hd], np.float64).reshape(nKV, hd)
        dev = np.asarray(res["k_pool"][blk, :, row], np.float64)
        if not b["rope_base"]:
            assert np.array_equal(dev, raw), (b["name"], i, "appended K row (no RoPE)")
            decided += raw.size; total += raw.size
            continue
        x = R.rope_f64(raw, pos, b["rope_base"], b["max_seq"])
        m = 2.0 ** -22 * (np.abs(raw) + np.abs(np.concatenate([raw[:, hd // 2:], raw[:, :hd // 2]], -1)))
        sure = R.bf16(x - m) == R.bf16(x + m)
        assert np.array_equal(dev[sure], R.bf16(x)[sure]), (b["name"], i, "appended K row")
        decided += int(sure.sum()); total += raw.size
    return decided, total


@pytest.mark.parametrize("kv_nt", [0, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_tail_forms_against_float64(gpu, name, form, kv_nt):
    b = R.batch(name, form)
    keys = {**NW8, 35: kv_nt}
    res = run(gpu, b, keys=keys)
    ran_as(res, "decode_fused", (8, 1), (name, form, kv_nt))
    R.check_bf16(b, res, ATTN_RATIO_BOUND, f"8 waves, key 35 = {kv_nt}")
    R.check_append(b, res)
    decided, total = appended_k_exact(b, res)
    print(f"{name} {form}: appended K rows compared exactly on {decided} of {total} elements")
    assert decided >= 0.9 * total
    assert not res["part_cnt"].any()
    again = run(gpu, b, keys=keys)                      # the combine's order is a function of the wave index only
    for what in ("out", "k_pool", "v_pool"):
        assert np.array_equal(res[what], again[what]), (name, form, kv_nt, what, "second run differs")


@pytest.mark.parametrize("name", ["T3", "T5"])
def test_load_policy_changes_no_bit(gpu, name):
    for form in FORMS:
        b = R.batch(name, form)
        a, c = run(gpu, b, keys={**NW8, 35: 0}), run(gpu, b, keys={**NW8, 35: 2})
        for what in ("out", "k_pool", "v_pool"):
            assert np.array_equal(a[what], c[what]), (name, form, what)


def test_eager_and_graph_replay_agree_bit_for_bit(gpu):
    cfg = gpu.synth.tiny_config("llama", num_heads=8, num_kv_heads=2, hidden=512, ffn_dim=512, max_seq_len=704)
    w = gpu.synth.make_weights(cfg, seed=11, scale=0.05)
    r = np.random.default_rng(5)
    lens = (64, 513, 640)                                # the first decode step's newest key sits at these positions
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in lens]
    ids, steps = [0, 1, 2], 6
    lib = gpu.lib()

    def decode(keys):
        old = {k: lib.nvl_set_tuning(k, v) for k, v in keys.items()}
        hm = gpu.HipTransformerModel(cfg, w, precision="bf16", max_seqs=4, max_batch_tokens=2048)
        try:
            hm.reset_stats()
            for i in ids:
                hm.seq_reset(i)
            _, am = hm.forward_batch(ids, prompts, [0, 0, 0])
            logits, pos = [], list(lens)
            for _ in range(steps):
                lg, am = hm.forward_batch(ids, [[int(t)] for t in am], pos)
                logits.append(lg.copy()); pos = [p + 1 for p in pos]
            toks = hm.decode_greedy(ids, am, steps)      # the fused loop on top of the same caches
            rows = []
            for li in range(cfg["num_layers"]):
                for i, n in zip(ids, lens):
                    k, v = hm.get_kv(i, li)              # [nKV][keys][hd]
                    assert k.shape[1] >= n + steps
                    rows.append((k[:, n:].copy(), v[:, n:].copy()))
            return logits, toks, rows, hm.stats()["graph_replays"]
        finally:
            hm.close()
            for k, v in old.items():
                lib.nvl_set_tuning(k, v)

    eager = decode({15: 8, 21: 0})
    graph = decode({15: 8, 21: 1})
    assert eager[3] == 0 and graph[3] >= steps
    for a, c in zip(eager[0], graph[0]):
        assert np.array_equal(a, c)
    assert np.array_equal(eager[1], graph[1])
    for (ka, va), (kc, vc) in zip(eager[2], graph[2]):
        assert np.isfinite(ka).all() and np.isfinite(va).all()
        assert np.array_equal(ka, kc) and np.array_equal(va, vc)
