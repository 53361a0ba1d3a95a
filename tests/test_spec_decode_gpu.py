"""Greedy speculative decoding at model level (nvl_verify_greedy[_paged], nvl_seq_truncate, nvl_decode_greedy_lookup) on the
tiny families of synth.tiny_config, as tests/test_model_gpu.py builds them.

Bounds, all taken from existing suites:
  rows   : |log-probability - oracle| <= 2 * TOL[precision] * max|oracle logit| (tests/test_logprobs_gpu.py: model-level rows
           against the oracle); over the 8-bit KV cache TOL is that mode's stated logits tolerance (FP8_KV_TOL there)
  cache  : K/V rows and the logits of a following step within TOL of tests/test_model_gpu.py
  ids    : f32 — identical to nvl_decode_greedy's; bf16 — identical to the oracle's on a prompt whose oracle top-2 margins
           all exceed 2 x TOL["bf16"] (the fixture search of test_greedy_token_ids_bit_exact)"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

FAMILIES = ["llama", "gpt2", "falcon", "granite_moe"]
TOL = {"f32": 1e-4, "bf16": 1.5e-2}          # tests/test_model_gpu.py
FP8_KV_TOL = 1e-1                            # tests/test_logprobs_gpu.py / test_kv_fp8_model_gpu.py
P0, P1 = 62, 19                              # cached lengths of the two sequences: 62 + drafts crosses a 64-key tile


def build(gpu, oracle, family, precision, peaked=0.0, cfg_over=None, **kw):
    cfg = gpu.synth.tiny_config(family, **(cfg_over or {}))
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=peaked)
    om = oracle.OracleModel(cfg, w) if oracle is not None else None
    kw.setdefault("max_seqs", 4)
    kw.setdefault("max_batch_tokens", 256)
    return cfg, om, gpu.HipTransformerModel(cfg, w, precision=precision, **kw)


class tuning:
    def __init__(self, gpu, key, value):
        self.lib, self.key, self.value = gpu.lib(), key, value

    def __enter__(self):
        self.old = self.lib.nvl_set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        self.lib.nvl_set_tuning(self.key, self.old)


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def prefill(hm, seq_id, prompt):
    hm.seq_reset(seq_id)
    _, am = hm.forward_batch([seq_id], [list(prompt)], [0], want_logits=False)
    return int(am[0])


def accept_rule(tokens, greedy):
    """the longest-prefix rule of nvl_verify_greedy on one row -> (a, out_tokens)"""
    k = len(tokens) - 1
    a = 0
    while a < k and tokens[a + 1] == greedy[a]:
        a += 1
    return a, [int(greedy[j]) if j <= a else -1 for j in range(k + 1)]


# ---- 1. rows ------------------------------------------------------------------------------------------------------
_ROWS = {}


def row_fixture(gpu, oracle, family, k):
    """prompts, verify rows, targets and the oracle's logits of the 2 x (1+k) rows: once per (family, k), read-only"""
    if (family, k) not in _ROWS:
        cfg, om, _hm = build(gpu, oracle, family, "f32")
        _hm.close()
        r = np.random.default_rng(11 + k)
        prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (P0, P1)]
        rows = r.integers(0, cfg["vocab_size"], (2, 1 + k)).astype(np.int32)
        targets = r.integers(0, cfg["vocab_size"], 2 * (1 + k)).astype(np.int32)
        want = []
        for p, t in zip(prompts, rows):
            kv = om.new_cache()
            om.forward_with_cache(p, kv, 0)
            want.append(om.forward_with_cache(t.tolist(), kv, len(p)))
        want = np.concatenate(want)
        want.setflags(write=False)
        _ROWS[(family, k)] = (prompts, rows, targets, want)
    return _ROWS[(family, k)]


def check_rows(hm, targets, want, tol):
    lp, am, _, _ = hm.logprobs(targets)
    want_lp = log_softmax(want)[np.arange(len(targets)), targets]
    err = float(np.abs(lp.astype(np.float64) - want_lp).max())
    b = 2 * tol * float(np.abs(want).max())
    print(f"rows {len(targets)}: max |lp - oracle lp| {err:.3e} (bound {b:.3e})")
    assert err <= b
    return am


ROW_MODES = [(f, "bf16", {}, TOL["bf16"]) for f in FAMILIES] + [("llama", "f32", {}, TOL["f32"]),
                                                               ("llama", "bf16", dict(kv_cache_dtype="fp8_e4m3"), FP8_KV_TOL)]


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("family,precision,kw,tol", ROW_MODES)
def test_rows_match_the_oracle(gpu, oracle, family, precision, kw, tol, k):
    prompts, rows, targets, want = row_fixture(gpu, oracle, family, k)
    _, _, hm = build(gpu, None, family, precision, **kw)
    for i, p in enumerate(prompts):
        prefill(hm, i, p)
    acc, out = hm.verify_greedy([0, 1], rows, k)
    am = check_rows(hm, targets, want, tol)
    # the accept rule on the very ids the device reports for these rows
    for i in range(2):
        a, o = accept_rule(rows[i].tolist(), am[i * (1 + k):(i + 1) * (1 + k)])
        assert (int(acc[i]), out[i].tolist()) == (a, o)
        assert hm.seq_len(i) == len(prompts[i]) + a + 1
    hm.close()


# ---- 2. accept rule, 3. rollback ------------------------------------------------------------------------------------
def greedy_ids(hm, seq_id, prompt, n):
    first = prefill(hm, seq_id, prompt)
    return first, [int(t) for t in hm.decode_greedy([seq_id], [first], n)[:, 0]]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_accept_rule_self_consistent(gpu, precision):
    """all-right drafts, drafts wrong at position 0 and wrong in the middle: n_accepted / out_tokens are the rule applied to
    the argmax logprobs() reports for the same rows; in f32 the drafts (nvl_decode_greedy's own ids) are accepted as built"""
    k = 4
    cfg, _, hm = build(gpu, None, "llama", precision)
    V = cfg["vocab_size"]
    prompt = np.random.default_rng(3).integers(0, V, 23).tolist()
    first, ids = greedy_ids(hm, 3, prompt, k)
    wrong0 = [(ids[0] + 1) % V] + ids[1:]
    wrong2 = ids[:2] + [(ids[2] + 1) % V] + ids[3:]
    for variants, expect in (((ids, wrong0), (k, 0)), ((wrong2, ids), (2, k))):
        for i in range(2):
            prefill(hm, i, prompt)
        rows = np.asarray([[first] + d for d in variants], np.int32)
        acc, out = hm.verify_greedy([0, 1], rows, k)
        _, am, _, _ = hm.logprobs(np.full(2 * (1 + k), -1, np.int32))
        for i in range(2):
            a, o = accept_rule(rows[i].tolist(), am[i * (1 + k):(i + 1) * (1 + k)])
            assert (int(acc[i]), out[i].tolist()) == (a, o)
            assert (out[i][a + 1:] == -1).all() and (out[i][:a + 1] >= 0).all()
            if precision == "f32":
                assert a == expect[i]
    hm.close()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rollback_leaves_the_accepted_cache(gpu, oracle, precision):
    k = 5
    cfg, om, hm = build(gpu, oracle, "llama", precision)
    V, tol = cfg["vocab_size"], TOL[precision]
    prompt = np.random.default_rng(4).integers(0, V, 20).tolist()
    P = len(prompt)
    first, ids = greedy_ids(hm, 3, prompt, k)
    draft = ids[:2] + [(ids[2] + 1) % V] + ids[3:]                 # wrong in the middle
    prefill(hm, 0, prompt)
    acc, out = hm.verify_greedy([0], [[first] + draft], k)
    a = int(acc[0])
    assert a < k and hm.seq_len(0) == P + a + 1
    kv = om.new_cache()
    om.forward_with_cache(prompt, kv, 0)
    om.forward_with_cache(([first] + draft)[:a + 1], kv, P)
    nkv = cfg["num_kv_heads"]
    for li in range(cfg["num_layers"]):
        k_ref, v_ref = kv.layer(li, nkv, cfg["head_dim"])
        k_dev, v_dev = hm.get_kv(0, li)
        assert k_dev.shape[1] == P + a + 1
        assert rel_err(k_dev, k_ref) <= tol and rel_err(v_dev, v_ref) <= tol
    nxt = int(out[0][a])
    want = om.forward_with_cache([nxt], kv, P + a + 1)[-1]
    got = hm.forward_with_cache([nxt], seq_id=0, pos_offset=P + a + 1, all_logits=False)[-1]
    assert rel_err(got, want) <= tol
    hm.close()


_SAFE = {}


def safe_prompt(gpu, oracle, family, precision, n_steps=10):
    """test_greedy_token_ids_bit_exact's fixture search: the first seeded prompt whose ORACLE margins all exceed 2 x TOL"""
    key = (family, precision, n_steps)
    if key not in _SAFE:
        cfg = gpu.synth.tiny_config(family, tied_embedding=False)
        om = oracle.OracleModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=4.0))
        for seed in range(600):
            prompt = np.random.default_rng(100 + seed).integers(0, cfg["vocab_size"], 12).tolist()
            want, margins = om.greedy(prompt, n_steps, return_margins=True)
            if min(margins) > 2 * TOL[precision] and len(set(want)) > 3:
                break
        else:
            pytest.fail("no fixture prompt with safe margins")
        _SAFE[key] = (prompt, want)
    return _SAFE[key]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_truncate_then_redecode(gpu, oracle, precision):
    """rolling back and decoding again gives the ids of never having gone further (margin-safe prompt)"""
    prompt, want = safe_prompt(gpu, oracle, "llama", precision)
    _, _, hm = build(gpu, None, "llama", precision, peaked=4.0, cfg_over=dict(tied_embedding=False))
    P = len(prompt)
    first, ids = greedy_ids(hm, 0, prompt, 9)
    assert [first] + ids == want
    assert hm.seq_len(0) == P + 9
    hm.seq_truncate(0, P + 3)                     # the cache keeps prompt, first, ids[0], ids[1]
    assert hm.seq_len(0) == P + 3
    again = [int(t) for t in hm.decode_greedy([0], [ids[2]], 6)[:, 0]]
    assert again == ids[3:]
    hm.close()


# ---- 4.-6. equivalence to greedy decoding in f32, the driver loop, passes_out -----------------------------------------
def periodic_prompt(cfg, seed, period=4, reps=5):
    pat = np.random.default_rng(seed).integers(0, cfg["vocab_size"], period).tolist()
    return pat * reps


@pytest.mark.parametrize("family", FAMILIES)
def test_lookup_equals_decode_greedy_f32(gpu, family):
    n_steps, k = 14, 3
    cfg, _, hm = build(gpu, None, family, "f32")
    prompts = [periodic_prompt(cfg, 30), np.random.default_rng(31).integers(0, cfg["vocab_size"], 9).tolist()]
    firsts = [prefill(hm, i, p) for i, p in enumerate(prompts)]
    want = hm.decode_greedy([0, 1], firsts, n_steps)
    firsts2 = [prefill(hm, i, p) for i, p in enumerate(prompts)]
    assert firsts2 == firsts
    got, passes = hm.greedy_lookup([0, 1], firsts, n_steps, k=k, ngram=3, histories=[p + [f] for p, f in zip(prompts, firsts)])
    assert np.array_equal(got, want)
    assert -(-n_steps // (k + 1)) <= passes <= n_steps
    assert [hm.seq_len(i) for i in range(2)] == [len(p) + n_steps for p in prompts]
    hm.close()


def drive(hm, seq_id, P, first, n_steps, k, draft_of):
    """a driver loop of direct verify_greedy calls with supplied drafts -> (ids, passes)"""
    out, cur, passes = [], first, 0
    while len(out) < n_steps:
        acc, toks = hm.verify_greedy([seq_id], [[cur] + draft_of(len(out))], k)
        out += toks[0][:int(acc[0]) + 1].tolist()
        cur = out[-1]
        passes += 1
    hm.seq_truncate(seq_id, P + n_steps)          # the overshoot of the last pass
    return out[:n_steps], passes


@pytest.mark.parametrize("k", [1, 3])
def test_driver_loop_with_supplied_drafts_f32(gpu, k):
    n_steps = 11
    cfg, _, hm = build(gpu, None, "llama", "f32")
    V = cfg["vocab_size"]
    prompt = np.random.default_rng(40).integers(0, V, 15).tolist()
    P = len(prompt)
    first, ids = greedy_ids(hm, 0, prompt, n_steps + k)
    perfect = lambda t: ids[t:t + k]
    wrong = lambda t: [(x + 1) % V for x in ids[t:t + k]]
    half = lambda t: perfect(t) if (t // (k + 1)) % 2 == 0 else wrong(t)
    for name, draft_of in (("perfect", perfect), ("wrong", wrong), ("half", half)):
        assert prefill(hm, 1, prompt) == first
        got, passes = drive(hm, 1, P, first, n_steps, k, draft_of)
        assert got == ids[:n_steps], name
        assert hm.seq_len(1) == P + n_steps
        if name == "perfect":
            assert passes == -(-n_steps // (k + 1))
        elif name == "wrong":
            assert passes == n_steps
        else:
            assert -(-n_steps // (k + 1)) < passes < n_steps
    hm.close()


def simulated_passes(pkg, history, ids, k, ngram):
    """the passes nvl_decode_greedy_lookup takes when the model's greedy ids are `ids`"""
    h, done, passes = list(history), 0, 0
    while done < len(ids):
        kp = min(k, len(ids) - done - 1)
        a = 0
        if kp > 0:
            draft, _ = pkg.ops.lookup_draft(h, kp, ngram)
            while a < kp and draft[a] == ids[done + a]:
                a += 1
        h += ids[done:done + a + 1]
        done += a + 1
        passes += 1
    return passes


def test_passes_out_f32(gpu, oracle):
    """a periodic prompt whose greedy continuation is periodic too (screened with the oracle on the CPU): fewer passes than steps"""
    n_steps, k, ngram = 16, 3, 3
    cfg = gpu.synth.tiny_config("llama", tied_embedding=False)
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=4.0)
    om = oracle.OracleModel(cfg, w)
    for seed in range(200):
        prompt = periodic_prompt(cfg, 500 + seed, period=3, reps=6)
        want, margins = om.greedy(prompt, n_steps + 1, return_margins=True)
        sim = simulated_passes(gpu, prompt + want[:1], want[1:], k, ngram)
        if min(margins) > 2 * TOL["f32"] and sim < n_steps:
            break
    else:
        pytest.fail("no periodic fixture prompt")
    hm = gpu.HipTransformerModel(cfg, w, precision="f32", max_seqs=2, max_batch_tokens=64)
    first = prefill(hm, 0, prompt)
    assert first == want[0]
    got, passes = hm.greedy_lookup([0], [first], n_steps, k=k, ngram=ngram, histories=[prompt + [first]])
    assert got[:, 0].tolist() == want[1:]
    print(f"passes {passes} of {n_steps} steps (simulated on the oracle's ids: {sim})")
    assert -(-n_steps // (k + 1)) <= passes < n_steps and passes == sim
    hm.close()


# ---- 7. equivalence to greedy decoding, bf16 ---------------------------------------------------------------------------
@pytest.mark.parametrize("mq", [1, 0])
@pytest.mark.parametrize("family", FAMILIES)
def test_lookup_equals_oracle_greedy_bf16(gpu, oracle, family, mq):
    prompt, want = safe_prompt(gpu, oracle, family, "bf16")
    _, _, hm = build(gpu, None, family, "bf16", peaked=4.0, cfg_over=dict(tied_embedding=False))
    with tuning(gpu, 38, mq):
        first = prefill(hm, 0, prompt)
        got, passes = hm.greedy_lookup([0], [first], len(want) - 1, k=3, ngram=2, histories=[prompt + [first]])
    assert [first] + got[:, 0].tolist() == want
    hm.close()


# ---- 8. graph replay ---------------------------------------------------------------------------------------------------
def test_third_identical_pass_is_replayed_bit_identically(gpu):
    k = 3
    cfg, _, hm = build(gpu, None, "llama", "bf16")
    _, _, eager = build(gpu, None, "llama", "bf16")
    r = np.random.default_rng(8)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (P0, P1)]
    rows = [r.integers(0, cfg["vocab_size"], (2, 1 + k)).astype(np.int32) for _ in range(3)]
    none = np.full(2 * (1 + k), -1, np.int32)

    def three(m):
        for i, p in enumerate(prompts):
            prefill(m, i, p)
        res = []
        for t in rows:
            before = m.stats()["graph_replays"]
            acc, out = m.verify_greedy([0, 1], t, k)
            lp = m.logprobs(none, top_k=4)
            res.append((acc, out, lp, m.stats()["graph_replays"] - before))
        return res

    got = three(hm)
    with tuning(gpu, 21, 0):
        want = three(eager)
    assert got[2][3] == 1 and [w[3] for w in want] == [0, 0, 0]
    for g, w in zip(got, want):
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes()
        for x, y in zip(g[2], w[2]):
            assert x.tobytes() == y.tobytes()
    hm.close(); eager.close()


# ---- 9. paged ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_paged_verify_equals_slab(gpu, oracle, precision):
    """block size 64, P = 62: the draft crosses into the second block"""
    k = 3
    prompts, rows, targets, want = row_fixture(gpu, oracle, "llama", k)
    _, _, slab = build(gpu, None, "llama", precision)
    _, _, paged = build(gpu, None, "llama", precision, kv_num_blocks=8, kv_block_size=64)
    tables = [[5, 2], [7]]
    paged.forward_paged(prompts, [0, 0], tables, want_logits=False)
    acc_p, out_p = paged.verify_greedy_paged(rows, k, [P0, P1], tables)
    check_rows(paged, targets, want, TOL[precision])
    for i, p in enumerate(prompts):
        prefill(slab, i, p)
    acc_s, out_s = slab.verify_greedy([0, 1], rows, k)
    assert np.array_equal(acc_p, acc_s) and np.array_equal(out_p, out_s)
    slab.close(); paged.close()


# ---- 10. errors --------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(Exception) as e:
        fn()
    return e.value.code


def test_error_codes_leave_the_lengths_alone(gpu):
    INVALID, POSITION, UNKNOWN_SEQ, STATE = -1, -2, -3, -7
    cfg, _, hm = build(gpu, None, "llama", "bf16", max_batch_tokens=16)
    prompt = np.random.default_rng(9).integers(0, cfg["vocab_size"], 12).tolist()
    t = prompt[0]
    prefill(hm, 0, prompt); prefill(hm, 1, prompt)
    assert code_of(lambda: hm.verify_greedy([0], [[t]], 0)) == INVALID
    assert code_of(lambda: hm.verify_greedy([0], [[t] * 9], 8)) == INVALID
    assert code_of(lambda: hm.verify_greedy([0, 1, 2], [[t] * 8] * 3, 7)) == INVALID           # 24 rows > max_batch_tokens
    assert code_of(lambda: hm.verify_greedy([0, 0], [[t] * 2] * 2, 1)) == INVALID             # duplicate
    assert code_of(lambda: hm.verify_greedy([0], [[t, cfg["vocab_size"]]], 1)) == INVALID      # token id
    assert code_of(lambda: hm.verify_greedy([9], [[t] * 2], 1)) == UNKNOWN_SEQ
    assert code_of(lambda: hm.greedy_lookup([9], [t], 4)) == UNKNOWN_SEQ
    assert code_of(lambda: hm.seq_truncate(0, 13)) == INVALID
    assert code_of(lambda: hm.seq_truncate(0, -1)) == INVALID
    assert code_of(lambda: hm.seq_truncate(9, 0)) == UNKNOWN_SEQ
    assert hm.seq_len(0) == 12 and hm.seq_len(1) == 12
    hm.close()
    _, _, hm = build(gpu, None, "llama", "bf16", cfg_over=dict(max_seq_len=64), max_batch_tokens=64)
    prefill(hm, 0, (prompt * 5)[:60])                                                          # 60 cached of 64
    assert code_of(lambda: hm.verify_greedy([0], [[t] * 6], 5)) == POSITION                    # 60 + 6 > 64
    assert code_of(lambda: hm.greedy_lookup([0], [t], 5)) == POSITION
    assert hm.seq_len(0) == 60
    acc, _ = hm.verify_greedy([0], [[t] * 4], 3)                                               # 60 + 4 fits exactly
    assert hm.seq_len(0) == 61 + int(acc[0])
    hm.close()
    # paged, hybrid (Mamba2 state cannot be rolled back) and tensor-parallel models are refused
    _, _, paged = build(gpu, None, "llama", "bf16", kv_num_blocks=4, kv_block_size=64)
    assert code_of(lambda: paged.verify_greedy([0], [[t] * 2], 1)) == STATE
    assert code_of(lambda: paged.seq_truncate(0, 0)) == STATE
    assert code_of(lambda: paged.greedy_lookup([0], [t], 4)) == STATE
    paged.close()
    _, _, slab = build(gpu, None, "llama", "bf16")
    assert code_of(lambda: slab.verify_greedy_paged([[t] * 2], 1, [0], [[0]])) == STATE
    slab.close()
    hcfg, _, hyb = build(gpu, None, "granite_hybrid", "bf16")
    prefill(hyb, 0, [1, 2, 3])
    assert code_of(lambda: hyb.verify_greedy([0], [[1, 2]], 1)) == STATE
    assert code_of(lambda: hyb.seq_truncate(0, 1)) == STATE
    assert hyb.seq_len(0) == 3
    hyb.close()
    _, _, tp1 = build(gpu, None, "llama", "bf16", tp_force_single=True)
    tp1.seq_reset(0) if tp1.seq_len(0) >= 0 else gpu._lib.check(tp1.lib.nvl_seq_open(tp1.h, 0), tp1.h)
    assert code_of(lambda: tp1.verify_greedy([0], [[t] * 2], 1)) == STATE
    assert code_of(lambda: tp1.greedy_lookup([0], [t], 4)) == STATE
    assert tp1.seq_len(0) == 0
    tp1.close()
