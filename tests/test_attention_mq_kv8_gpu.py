"""The multi-position decode attention of a verify pass over the 8-bit KV cache (kv8.h attn_decode_mq_kv8_kernel), through
ops.attention_batch(form="mq_kv8") against the float64 statement of tests/attention_reference.py on the dequantized cache,
and through a tiny model's verify_greedy.  Bounds (a) / (b) and the census are that file's; RATIO follows
test_attention_ops_gpu.py's rule: 1.25 x the largest device / emulation rms ratio measured on the MI355X over the cases of
this file where that exceeds ATTN_RATIO_BOUND = 1.550, never above 2 (profiles/attention_mq_kv8_tests.txt)."""
import numpy as np
import pytest

import attention_reference as R

pytestmark = pytest.mark.gpu

RATIO = 1.550                    # the largest measured ratio, 1.25 x it and the choice: profiles/attention_mq_kv8_tests.txt
FP8_KV_TOL = 1e-1                # tests/test_spec_decode_gpu.py: the 8-bit cache's stated logits tolerance

R.ALL_CASES.update(R.VERIFY_CASES)       # Q1 - Q3
CASES = ["M1", "M2", "Q1", "Q2", "Q3"]
TWO = {40: 2}                    # nvl_set_tuning key 40: two query tiles per workgroup whatever the grid size (Q1, Q3: these small
                                 # grids take one by default)


def run(gpu, b, keys=None, **over):
    a = dict(form="mq_kv8", k_scale=b["k_scale"], v_scale=b["v_scale"])
    a.update(over)
    with R.tuning(gpu, keys or {}):
        return gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"], **a)


def ran_as(res, shape, tag):
    assert (res["ran"], res["nw"], res["nsplit"]) == ("decode_mq_kv8",) + tuple(shape), (tag, res["ran"], res["nw"], res["nsplit"])
    assert np.isfinite(res["out"]).all(), tag


@pytest.mark.parametrize("name", CASES)
def test_verify_pass_kv8(gpu, name):
    b = R.batch(name, "kv8")
    res = run(gpu, b)
    ran_as(res, b["expect"], name)
    R.check_bf16(b, res, RATIO)
    if name in ("Q1", "Q3"):     # both tiles behind one stream: the same sums in the same order, so no bit changes
        two = run(gpu, b, keys=TWO)
        ran_as(two, b["expect"], (name, TWO))
        R.check_bf16(b, two, RATIO, "key 40 = 2")
        assert np.array_equal(two["out"], res["out"]), (name, "key 40")
    if name in ("M1", "Q2"):     # one tile per workgroup at the wave counts its context does not take: 4 at hd 64; 2 and 8 at hd 128
        for nw in {"M1": (4,), "Q2": (2, 8)}[name]:
            forced = run(gpu, b, keys={15: nw})
            ran_as(forced, (nw, 1), (name, "key 15", nw))
            R.check_bf16(b, forced, RATIO, f"key 15 = {nw}")


def test_wave_counts_and_load_policy(gpu):
    """two tiles per workgroup: nvl_set_tuning key 15 (2 / 4 / 8 waves per workgroup) under both bounds; key 35 (non-temporal
    K/V loads never / always) changes no bit"""
    b = R.batch("Q1", "kv8")
    for nw in (2, 4, 8):
        res = run(gpu, b, keys={15: nw, **TWO})
        ran_as(res, (nw, 1), nw)
        R.check_bf16(b, res, RATIO, f"key 15 = {nw}")
    base = run(gpu, b, keys=TWO)
    for nt in (0, 2):
        res = run(gpu, b, keys={35: nt, **TWO})
        ran_as(res, b["expect"], nt)
        assert np.array_equal(res["out"], base["out"]), ("key 35", nt)


@pytest.mark.parametrize("name", ["Q1", "Q3"])
def test_census(gpu, name):
    b = R.batch(name, "kv8", census=True)
    for keys in ({}, TWO):
        res = run(gpu, b, keys=keys)
        ran_as(res, b["expect"], (name, keys))
        R.check_census(b, res)


def accept_rule(tokens, greedy):
    """the longest-prefix rule of nvl_verify_greedy on one row -> (a, out_tokens)"""
    k = len(tokens) - 1
    a = 0
    while a < k and tokens[a + 1] == greedy[a]:
        a += 1
    return a, [int(greedy[j]) if j <= a else -1 for j in range(k + 1)]


def test_model_verify_takes_the_kernel(gpu):
    """verify_greedy of a tiny llama over an 8-bit cache runs the kernel (key 38 = 0: the prefill kernel); the rows' log-
    probabilities under the two routes agree within the mode's tolerance, and the accept rule holds on the reported ids"""
    cfg = gpu.synth.tiny_config("llama")
    hm = gpu.HipTransformerModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05), precision="bf16", kv_cache_dtype="fp8_e4m3",
                                 max_seqs=4, max_batch_tokens=256)
    r = np.random.default_rng(5)
    V = cfg["vocab_size"]
    prompts = [r.integers(0, V, n).tolist() for n in (62, 19)]
    for k in (3, 7):
        rows, targets = r.integers(0, V, (2, 1 + k)).astype(np.int32), r.integers(0, V, 2 * (1 + k)).astype(np.int32)
        lps = {}
        for key38, ran in ((1, "decode_mq_kv8"), (0, "prefill_kv8")):
            with R.tuning(gpu, {38: key38}):
                for i, p in enumerate(prompts):
                    hm.seq_reset(i)
                    hm.forward_batch([i], [p], [0], want_logits=False)
                acc, out = hm.verify_greedy([0, 1], rows, k)
            assert hm.attention_ran()[0] == ran, (k, key38, hm.attention_ran())
            lps[key38], am, _, _ = hm.logprobs(targets)
            for i in range(2):
                assert (int(acc[i]), out[i].tolist()) == accept_rule(rows[i].tolist(), am[i * (1 + k):(i + 1) * (1 + k)])
        for i in (2, 3):
            hm.seq_reset(i)
        logits, _ = hm.forward_batch([2, 3], [p + t.tolist() for p, t in zip(prompts, rows)], [0, 0], all_logits=True)
        err, bound = float(np.abs(lps[1].astype(np.float64) - lps[0]).max()), 2 * FP8_KV_TOL * float(np.abs(logits).max())
        print(f"k {k}: max |lp(key 38 = 1) - lp(key 38 = 0)| {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    hm.close()


def test_refusals(gpu):
    b = R.batch("M1", "kv8")
    for over in (dict(precision="f32"), dict(k_scale=0.0)):
        with pytest.raises(gpu.NvlError) as e:
            run(gpu, b, **over)
        assert e.value.code == -1, over
