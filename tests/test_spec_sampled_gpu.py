"""Sampled speculative decoding (nvl_verify_sampled[_paged], nvl_decode_sampled_lookup,
nvl_op_sample_drafts): the verify pass of tests/test_spec_decode_gpu.py under tensor.SampleWithHistory
(sampling.go:33-102), the step every TensorModelRunner.Run ends in (tensor_model_runner.go:89-93).

A prompt-lookup draft is a point mass, so a row is sampled with its decode step's draw and the draft is accepted iff it
is the id drawn: given the same draws the calls emit what the sequential sampler emits, and everything here is tested by
equality.

Bounds, all taken from existing suites:
  sampler : ids and final distribution bit-identical to nvl_op_sample on the concatenated history; against the oracle the
            tolerances of tests/test_sampling_gpu.py's check_rows (1e-3 relative on the support, 1e-3 odd mass, 2e-3 of
            probability mass around the CDF interval)
  rows    : |log-probability - oracle| <= 2 * TOL[precision] * max|oracle logit| (tests/test_spec_decode_gpu.py), FP8_KV_TOL
            over the 8-bit cache
  cache   : K/V rows and the logits of a following step within TOL of tests/test_model_gpu.py
  ids     : f32 — the stepwise sampler's, on a fixture whose every draw lies more than 2e-3 of probability mass (the id
            tolerance of tests/test_sampling_gpu.py) inside its CDF interval: max|logit| < 5 there, so the
            2 * TOL["f32"] * max|logit| = 1e-3 by which the logits of a 1 + k row pass may differ from a one-row step's
            moves no CDF edge by more than 1e-3 of mass"""
import numpy as np
import pytest

from block_manager_mirror import BlockManager
from conftest import rel_err
from test_sampling_gpu import PARAMS
from test_sampling_gpu import check_rows as check_sampler_rows
from test_spec_decode_gpu import (FAMILIES, FP8_KV_TOL, P0, P1, TOL, accept_rule, build, check_rows, code_of, prefill,
                                  tuning)

pytestmark = pytest.mark.gpu

SAMPLING = dict(temperature=0.9, top_k=50, top_p=0.95, repetition_penalty=1.2)


def concat(hists, rows):
    """the explicit history of every row: row j of sequence i sees hists[i] ++ rows[i][1..j]"""
    return [list(h) + [int(t) for t in r[1:j + 1]] for h, r in zip(hists, rows) for j in range(len(r))]


def plant(rows, sampled, i, j, V, wrong=None):
    """make draft position j of sequence i (token j + 1 of its row) differ from the id sampled for row j"""
    s = int(sampled[i][j])
    rows[i][j + 1] = wrong if wrong is not None and wrong != s else (s + 1) % V


# ---- 1. the sampler with the history extension, op level ---------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("V", [1000, 50257])
@pytest.mark.parametrize("pi", [0, 4, 5])
def test_sampler_with_extension_equals_concatenated_history(gpu, oracle, V, k, pi):
    kw = PARAMS[pi]
    n, S = 4, 1 + k
    r = np.random.default_rng(1000 * pi + V + k)
    logits = (r.standard_normal((n * S, V)) * np.repeat([0.5, 2.0, 4.0, 1.0], S)[:, None]).astype(np.float32)
    base = [r.integers(0, V, m).tolist() for m in (1, 4, 9, 25)]      # |base| + j < 10, straddling, and a window past the base
    base[3][5] = V + 3                                                # ids >= V are ignored (sampling.go:57)
    u = r.random((n, S)).astype(np.float32)
    u[0, 0] = 0.0
    rows = r.integers(0, V, (n, S)).astype(np.int32)
    rows[:, 0] = [b[-1] for b in base]
    # drafts that are accepted: draft j + 1 = the id of row j, which depends on drafts 1..j only
    for j in range(k):
        sampled, _, _ = gpu.ops.sample_drafts(logits, rows, k, base, u, **kw)
        rows[:, j + 1] = sampled[:, j]
    sampled, acc, _ = gpu.ops.sample_drafts(logits, rows, k, base, u, **kw)
    assert acc.tolist() == [k] * n
    plant(rows, sampled, 0, 0, V)                                        # sequence 0 accepts nothing
    mid = k // 2                                                      # sequence 2 stops in the middle, at a token of its base
    plant(rows, sampled, 2, mid, V, wrong=base[2][0])                    # history: counted once, with the summed count
    sampled, acc, out, probs = gpu.ops.sample_drafts(logits, rows, k, base, u, return_probs=True, **kw)
    hists = concat(base, rows)
    want_tok, want_probs = gpu.ops.sample_with_history(logits, hists, u.reshape(-1), return_probs=True, **kw)
    assert sampled.reshape(-1).tobytes() == want_tok.tobytes()
    assert probs.tobytes() == want_probs.tobytes()
    for i in range(n):
        a, o = accept_rule(rows[i].tolist(), sampled[i])
        assert (int(acc[i]), out[i].tolist()) == (a, o)
    assert acc.tolist() == [0, k, mid, k]
    assert 0 in acc and k in acc and (k == 1 or any(0 < a < k for a in acc))
    check_sampler_rows(oracle, logits, hists, u.reshape(-1), sampled.reshape(-1), probs, kw)


# ---- 2. the pass, every mode ---------------------------------------------------------------------------------------------
PASS_MODES = ([("llama", "f32", {}, TOL["f32"], None)] +
              [(f, "bf16", {}, TOL["bf16"], mq) for f in FAMILIES for mq in (1, 0)] +
              [("llama", "bf16", dict(kv_cache_dtype="fp8_e4m3"), FP8_KV_TOL, None)])


def sampled_ids(hm, hists, rows, u, kw):
    """nvl_sample on the rows the pass left, with explicitly concatenated histories and the same draws -> [n, 1+k]"""
    return hm.sample(concat(hists, rows), np.asarray(u, np.float32).reshape(-1), **kw).reshape(len(rows), -1)


def self_consistent_pass(hm, ids, lens, rows, k, hists, u, kw):
    """one verify_sampled pass checked against the accept rule on hm.sample's ids; the lengths afterwards -> n_accepted"""
    acc, out = hm.verify_sampled(ids, rows, k, hists, u, **kw)
    s = sampled_ids(hm, hists, rows, u, kw)
    for i, sid in enumerate(ids):
        a, o = accept_rule(np.asarray(rows[i]).tolist(), s[i])
        assert (int(acc[i]), out[i].tolist()) == (a, o), (i, rows[i], s[i])
        assert hm.seq_len(sid) == lens[i] + a + 1
    return acc


_ORACLES = {}


def oracle_rows(gpu, oracle, family, prompts, rows):
    if family not in _ORACLES:
        cfg = gpu.synth.tiny_config(family)
        _ORACLES[family] = oracle.OracleModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05))
    om, want = _ORACLES[family], []
    for p, t in zip(prompts, rows):
        kv = om.new_cache()
        om.forward_with_cache(p, kv, 0)
        want.append(om.forward_with_cache([int(x) for x in t], kv, len(p)))
    return np.concatenate(want)


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("family,precision,kw,tol,mq", PASS_MODES)
def test_pass_is_self_consistent_and_matches_the_oracle(gpu, oracle, family, precision, kw, tol, mq, k):
    cfg, _, hm = build(gpu, None, family, precision, **kw)
    V, S = cfg["vocab_size"], 1 + k
    r = np.random.default_rng(21 + k)
    prompts = [r.integers(0, V, m).tolist() for m in (P0, P1)]
    u = r.random((2, S)).astype(np.float32)
    targets = r.integers(0, V, 2 * S).astype(np.int32)
    seen = set()
    with tuning(gpu, 38, 1 if mq is None else mq):
        firsts = [prefill(hm, i, p) for i, p in enumerate(prompts)]
        hists = [p + [f] for p, f in zip(prompts, firsts)]
        rows = r.integers(0, V, (2, S)).astype(np.int32)
        rows[:, 0] = firsts

        def rewind():
            for i, n in enumerate((P0, P1)):
                hm.seq_truncate(i, n)

        for j in range(k):                                            # drafts the model accepts, one position per pass
            hm.verify_sampled([0, 1], rows, k, hists, u, **SAMPLING)
            rows[:, j + 1] = sampled_ids(hm, hists, rows, u, SAMPLING)[:, j]
            rewind()
        full = rows.copy()
        # every draft right; then sequence 1 wrong in the middle (k > 1); then sequence 0 wrong at once
        acc = self_consistent_pass(hm, [0, 1], (P0, P1), full, k, hists, u, SAMPLING)
        s = sampled_ids(hm, hists, full, u, SAMPLING)
        assert acc.tolist() == [k, k], "drafts built from the pass's own ids are accepted"
        seen.update(int(a) for a in acc)
        check_rows(hm, targets, oracle_rows(gpu, oracle, family, prompts, full), tol)
        rewind()
        for i, j in ([(1, k // 2)] if k > 1 else []) + [(0, 0)]:
            rows = full.copy()
            plant(rows, s, i, j, V)
            acc = self_consistent_pass(hm, [0, 1], (P0, P1), rows, k, hists, u, SAMPLING)
            assert int(acc[i]) == j and int(acc[1 - i]) == k
            seen.update(int(a) for a in acc)
            check_rows(hm, targets, oracle_rows(gpu, oracle, family, prompts, rows), tol)
            rewind()
    assert 0 in seen and k in seen and (k == 1 or any(0 < a < k for a in seen))
    hm.close()


# ---- 3. the greedy anchor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_top_k_1_is_the_greedy_call(gpu, precision):
    """top_k = 1 without a penalty keeps the arg-max alone: the same pass, hence the same logits bit for bit, must give
    nvl_verify_greedy's answer, and the loop nvl_decode_greedy_lookup's ids and pass count (peaked head: no near-ties)"""
    k, n_steps = 4, 10
    greedy = dict(top_k=1, repetition_penalty=1.0)
    cfg, _, hm = build(gpu, None, "llama", precision, peaked=4.0, cfg_over=dict(tied_embedding=False))
    V = cfg["vocab_size"]
    r = np.random.default_rng(5)
    prompts = [r.integers(0, V, m).tolist() for m in (P0, P1)]
    firsts = [prefill(hm, i, p) for i, p in enumerate(prompts)]
    ids = hm.decode_greedy([0, 1], firsts, k).T                        # [2, k]: what greedy decoding goes on with
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    for wrong in (None, (0, 0), (1, 2)):
        rows = np.concatenate([np.asarray(firsts, np.int32)[:, None], ids.astype(np.int32)], axis=1)
        if wrong:
            rows[wrong[0], wrong[1] + 1] = (rows[wrong[0], wrong[1] + 1] + 1) % V
        for i, p in enumerate(prompts):
            prefill(hm, i, p)
        acc_g, out_g = hm.verify_greedy([0, 1], rows, k)
        for i, p in enumerate(prompts):
            prefill(hm, i, p)
        acc_s, out_s = hm.verify_sampled([0, 1], rows, k, hists, r.random((2, 1 + k)), **greedy)
        assert acc_s.tolist() == acc_g.tolist() and out_s.tolist() == out_g.tolist()
        assert [hm.seq_len(i) for i in range(2)] == [len(p) + int(a) + 1 for p, a in zip(prompts, acc_g)]
    pat = r.integers(0, V, 4).tolist() * 5                             # a periodic prompt: some drafts are accepted
    first = prefill(hm, 2, pat)
    want, passes_g = hm.greedy_lookup([2], [first], n_steps, k=3, ngram=2, histories=[pat + [first]])
    assert prefill(hm, 2, pat) == first
    got, passes_s = hm.sampled_lookup([2], [first], n_steps, [pat + [first]], r.random((n_steps, 1)), k=3, ngram=2, **greedy)
    assert got.tolist() == want.tolist() and passes_s == passes_g
    assert hm.seq_len(2) == len(pat) + n_steps
    hm.close()


# ---- 4. rollback -----------------------------------------------------------------------------------------------------------
def test_rollback_leaves_the_accepted_cache_f32(gpu):
    """after a partially accepted pass, the next step (forward_batch + sample) is the one taken from a fresh prefill of the
    accepted tokens"""
    k, tol = 5, TOL["f32"]
    cfg, _, hm = build(gpu, None, "llama", "f32")
    _, _, fresh = build(gpu, None, "llama", "f32")
    V = cfg["vocab_size"]
    r = np.random.default_rng(6)
    prompt = r.integers(0, V, 20).tolist()
    P = len(prompt)
    u = r.random((1, 1 + k)).astype(np.float32)
    first = prefill(hm, 0, prompt)
    hist = [prompt + [first]]
    rows = r.integers(0, V, (1, 1 + k)).astype(np.int32)
    rows[0, 0] = first
    for j in range(k):
        hm.verify_sampled([0], rows, k, hist, u, **SAMPLING)
        rows[:, j + 1] = sampled_ids(hm, hist, rows, u, SAMPLING)[:, j]
        hm.seq_truncate(0, P)
    plant(rows, rows[:, 1:], 0, 2, V)                                  # draft position 2 wrong
    acc, out = hm.verify_sampled([0], rows, k, hist, u, **SAMPLING)
    a = int(acc[0])
    assert a == 2 and hm.seq_len(0) == P + a + 1
    kept = prompt + rows[0, :a + 1].tolist()                           # what the cache holds
    assert prefill(fresh, 0, kept) is not None
    for li in range(cfg["num_layers"]):
        k_dev, v_dev = hm.get_kv(0, li)
        k_ref, v_ref = fresh.get_kv(0, li)
        assert k_dev.shape[1] == P + a + 1
        assert rel_err(k_dev, k_ref) <= tol and rel_err(v_dev, v_ref) <= tol
    nxt, u1 = int(out[0][a]), r.random(1).astype(np.float32)
    h1 = [kept + [nxt]]
    lg_a, _ = hm.forward_batch([0], [[nxt]], [P + a + 1])
    tok_a = hm.sample(h1, u1, **SAMPLING)
    lg_b, _ = fresh.forward_batch([0], [[nxt]], [P + a + 1])
    tok_b = fresh.sample(h1, u1, **SAMPLING)
    assert rel_err(lg_a, lg_b) <= tol
    assert tok_a.tolist() == tok_b.tolist()
    hm.close(); fresh.close()


# ---- 5. / 6. the loop and a driver loop equal the stepwise sampler, f32 ----------------------------------------------------
N_STEPS, K_LOOP, NGRAM = 12, 3, 3
GUARD = 2e-3                     # the id tolerance tests/test_sampling_gpu.py states, in probability mass
SEED = 757                       # the first seed whose stepwise reference alone passes the guard (smallest distance 2.2e-3)
_STEPWISE = {}


def edge_distance(probs, u, tok):
    """how far, in probability mass, the draw lies inside the CDF interval of the id it selected (an interval end that
    no other id borders — the start of the first, the end of the last supported id — is no edge)"""
    cum = np.cumsum(probs.astype(np.float64))
    r = float(u) * cum[-1]
    nz = np.flatnonzero(probs)
    lo = cum[tok - 1] if tok > 0 else 0.0
    d_lo = r - lo if tok != nz[0] else np.inf
    d_hi = cum[tok] - r if tok != nz[-1] else np.inf
    return min(d_lo, d_hi)


def stepwise(gpu, hm, seed=None, give_up=None):
    """the host loop of test_fused_sampled_decode_equals_stepwise (forward_batch + sample + append) in f32 ->
    prompts, first tokens, U [1 + 12, 3], ids [12, 3], the smallest edge distance, max|logit|; computed once for SEED and
    read-only.  (seed / give_up: the fixture search — another seed, uncached, stopping at the first draw that close to an edge)"""
    if seed is not None or not _STEPWISE:
        cfg = gpu.synth.tiny_config("llama")
        r = np.random.default_rng(31)
        prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (9, 33, 2)]
        ids = [0, 1, 2]
        U = np.random.default_rng(SEED if seed is None else seed).random((N_STEPS + 1, 3)).astype(np.float32)
        for i in ids:
            hm.seq_reset(i)
        hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)
        hist = [list(p) for p in prompts]
        first = hm.sample(hist, U[0], **SAMPLING)
        for h, t in zip(hist, first):
            h.append(int(t))
        want, dist, top = [], np.inf, 0.0
        for s in range(N_STEPS):
            lg, _ = hm.forward_batch(ids, [[h[-1]] for h in hist], [len(h) - 1 for h in hist])
            tok = hm.sample(hist, U[s + 1], **SAMPLING)
            ref, probs = gpu.ops.sample_with_history(lg, hist, U[s + 1], return_probs=True, **SAMPLING)
            assert ref.tolist() == tok.tolist()
            dist = min([dist] + [edge_distance(probs[i], U[s + 1][i], int(tok[i])) for i in range(3)])
            top = max(top, float(np.abs(lg).max()))
            want.append(tok.copy())
            for h, t in zip(hist, tok):
                h.append(int(t))
            if give_up is not None and dist <= give_up:
                break
        want = np.stack(want)
        want.setflags(write=False); U.setflags(write=False)
        ref = (prompts, [int(t) for t in first], U, want, float(dist), top)
        if seed is not None:
            return ref
        _STEPWISE["ref"] = ref
    return _STEPWISE["ref"]


def loop_model(gpu):
    return build(gpu, None, "llama", "f32")[2]


def restart(hm, prompts, firsts, U):
    for i in range(3):
        hm.seq_reset(i)
    hm.forward_batch([0, 1, 2], prompts, [0, 0, 0], want_logits=False)
    hist = [list(p) for p in prompts]
    assert hm.sample(hist, U[0], **SAMPLING).tolist() == firsts
    return [h + [f] for h, f in zip(hist, firsts)]


def simulated_passes(pkg, hists, ids, k, ngram):
    """the passes nvl_decode_sampled_lookup takes when the sampler's ids are `ids` [n_steps, n_seqs]"""
    n_steps, n = ids.shape
    h, done, passes = [list(x) for x in hists], [0] * n, 0
    while min(done) < n_steps:
        active = [i for i in range(n) if done[i] < n_steps]
        kp = min(k, max(n_steps - done[i] - 1 for i in active))
        for i in active:
            a = 0
            if kp > 0:
                draft, _ = pkg.ops.lookup_draft(h[i], kp, ngram)
                while a < kp and done[i] + a < n_steps and draft[a] == ids[done[i] + a, i]:
                    a += 1
            take = min(a + 1, n_steps - done[i])
            h[i] += ids[done[i]:done[i] + take, i].tolist()
            done[i] += take
        passes += 1
    return passes


def test_guard_every_draw_lies_inside_its_interval(gpu):
    hm = loop_model(gpu)
    _, _, _, _, dist, top = stepwise(gpu, hm)
    print(f"smallest edge distance {dist:.3e} (guard {GUARD:.0e}), max|logit| {top:.3f}")
    assert dist > GUARD and top < 5.0
    hm.close()


def test_loop_equals_the_stepwise_sampler_f32(gpu):
    hm = loop_model(gpu)
    prompts, firsts, U, want, dist, top = stepwise(gpu, hm)
    assert dist > GUARD and top < 5.0
    hists = restart(hm, prompts, firsts, U)
    got, passes = hm.sampled_lookup([0, 1, 2], firsts, N_STEPS, hists, U[1:], k=K_LOOP, ngram=NGRAM, **SAMPLING)
    assert got.tolist() == want.tolist()
    assert passes == simulated_passes(gpu, hists, want, K_LOOP, NGRAM)
    assert [hm.seq_len(i) for i in range(3)] == [len(p) + N_STEPS for p in prompts]
    hm.close()


def sampled_drive(hm, hists, firsts, U, want, k, V, wrong=None):
    """a driver loop of direct verify_sampled calls whose drafts are the reference's own continuation; `wrong` = (pass,
    sequence, draft position) of one planted wrong token.  Step t of a sequence always gets U[1 + t].
    -> (ids [n_steps, 3], per-pass n_accepted)"""
    n_steps, n = want.shape
    done, cur, out, accs = [0] * n, list(firsts), [[] for _ in range(n)], []
    h = [list(x) for x in hists]
    while min(done) < n_steps:
        act = [i for i in range(n) if done[i] < n_steps]
        rows = np.zeros((len(act), 1 + k), np.int32)
        u = np.full((len(act), 1 + k), 0.5, np.float32)
        for a, i in enumerate(act):
            rows[a, 0] = cur[i]
            for j in range(k + 1):
                t = done[i] + j
                if j < k and t < n_steps:
                    rows[a, j + 1] = want[t, i]
                if t < n_steps:
                    u[a, j] = U[1 + t, i]
            if wrong and wrong[0] == len(accs) and wrong[1] == i:
                rows[a, wrong[2] + 1] = (rows[a, wrong[2] + 1] + 1) % V
        acc, toks = hm.verify_sampled(act, rows, k, [h[i] for i in act], u, **SAMPLING)
        accs.append({i: int(acc[a]) for a, i in enumerate(act)})
        for a, i in enumerate(act):
            new = toks[a][:int(acc[a]) + 1].tolist()
            out[i] += new
            h[i] += new
            done[i] += len(new)
            cur[i] = out[i][-1]
    return np.asarray([o[:n_steps] for o in out]).T, accs


def test_driver_loop_with_supplied_drafts_f32(gpu):
    k = K_LOOP
    hm = loop_model(gpu)
    prompts, firsts, U, want, dist, top = stepwise(gpu, hm)
    assert dist > GUARD and top < 5.0
    V = gpu.synth.tiny_config("llama")["vocab_size"]
    hists = restart(hm, prompts, firsts, U)
    got, accs = sampled_drive(hm, hists, firsts, U, want, k, V)
    assert got.tolist() == want.tolist()
    assert len(accs) == -(-N_STEPS // (k + 1))
    seq = 1
    for j in (0, 1, k - 1):
        hists = restart(hm, prompts, firsts, U)
        got, accs = sampled_drive(hm, hists, firsts, U, want, k, V, wrong=(0, seq, j))
        assert accs[0][seq] == j and all(a == k for i, a in accs[0].items() if i != seq)
        assert got.tolist() == want.tolist()                           # each step t used U[1 + t], whatever the grouping
    hm.close()


# ---- 7. graph replay -------------------------------------------------------------------------------------------------------
def test_replayed_pass_reads_its_parameters_and_draws_afresh(gpu):
    k = 3
    cfg, _, hm = build(gpu, None, "llama", "bf16")
    V = cfg["vocab_size"]
    r = np.random.default_rng(8)
    prompts = [r.integers(0, V, m).tolist() for m in (P0, P1)]
    firsts = [prefill(hm, i, p) for i, p in enumerate(prompts)]
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    rows = r.integers(0, V, (2, 1 + k)).astype(np.int32)
    rows[:, 0] = firsts
    u = r.random((2, 1 + k)).astype(np.float32)
    res = []
    for _ in range(3):
        before = hm.stats()["graph_replays"]
        acc, out = hm.verify_sampled([0, 1], rows, k, hists, u, **SAMPLING)
        res.append((acc.tobytes(), out.tobytes(), hm.stats()["graph_replays"] - before))
        for i, n in enumerate((P0, P1)):
            hm.seq_truncate(i, n)
    assert res[0][2] == 0 and res[2][2] == 1
    assert res[0][:2] == res[1][:2] == res[2][:2]
    # the same shape with other parameters, other draws and other drafts: replayed, and it is THIS call's answer
    other = dict(temperature=0.7, top_k=5, top_p=0.8, repetition_penalty=1.5)
    rows2 = rows.copy()
    rows2[:, 1:] = r.integers(0, V, (2, k))
    u2 = r.random((2, 1 + k)).astype(np.float32)
    before = hm.stats()["graph_replays"]
    self_consistent_pass(hm, [0, 1], (P0, P1), rows2, k, hists, u2, other)
    assert hm.stats()["graph_replays"] - before == 1
    s_other = sampled_ids(hm, hists, rows2, u2, other)
    s_first = sampled_ids(hm, hists, rows2, u2, SAMPLING)
    assert s_other.tolist() != s_first.tolist(), "the fixture must tell the two parameter sets apart"
    hm.close()


# ---- 8. paged ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_paged_verify_equals_slab(gpu, precision):
    """block size 64, P = 62: the drafts cross into the second block"""
    k = 3
    cfg, _, slab = build(gpu, None, "llama", precision)
    _, _, paged = build(gpu, None, "llama", precision, kv_num_blocks=8, kv_block_size=64)
    V = cfg["vocab_size"]
    r = np.random.default_rng(9)
    bm = BlockManager(8, 64)
    bm.free = list(r.permutation(8))
    seqs = [gpu.Sequence(seq_id=i, token_ids=r.integers(0, V, m).tolist() + [0] * (1 + k), block_size=64)
            for i, m in enumerate((P0, P1))]                           # (tables that cover P + 1 + k tokens)
    for s in seqs:
        bm.allocate(s)
    tables = [[int(b) for b in s.block_table] for s in seqs]
    prompts = [s.token_ids[:m] for s, m in zip(seqs, (P0, P1))]
    _, am = paged.forward_paged(prompts, [0, 0], tables, want_logits=False)
    firsts = [prefill(slab, i, p) for i, p in enumerate(prompts)]
    assert am.tolist() == firsts
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    rows = r.integers(0, V, (2, 1 + k)).astype(np.int32)
    rows[:, 0] = firsts
    u = r.random((2, 1 + k)).astype(np.float32)
    for j in range(k + 1):                                             # the last round: every draft accepted
        acc_s, out_s = slab.verify_sampled([0, 1], rows, k, hists, u, **SAMPLING)
        s = sampled_ids(slab, hists, rows, u, SAMPLING)
        acc_p, out_p = paged.verify_sampled_paged(rows, k, [P0, P1], tables, hists, u, **SAMPLING)
        assert acc_p.tolist() == acc_s.tolist() and out_p.tolist() == out_s.tolist()
        for i, n in enumerate((P0, P1)):
            slab.seq_truncate(i, n)
        if j < k:
            rows[:, j + 1] = s[:, j]
    assert acc_s.tolist() == [k, k]
    slab.close(); paged.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_lengths_alone(gpu):
    INVALID, POSITION, UNKNOWN_SEQ, STATE = -1, -2, -3, -7
    cfg, _, hm = build(gpu, None, "llama", "bf16", max_batch_tokens=16)
    V = cfg["vocab_size"]
    prompt = np.random.default_rng(9).integers(0, V, 12).tolist()
    t = prompt[0]
    h = [prompt + [t]]
    u2, u8 = [[0.5] * 2], [[0.5] * 8]
    prefill(hm, 0, prompt); prefill(hm, 1, prompt)
    vs = hm.verify_sampled
    nan = float("nan")
    for bad in (lambda: vs([0, 1, 2], [[t] * 8] * 3, 7, h * 3, u8 * 3),                     # 24 rows > max_batch_tokens
                lambda: vs([0, 0], [[t] * 2] * 2, 1, h * 2, u2 * 2),                        # duplicate
                lambda: vs([0], [[t, V]], 1, h, u2),                                        # token id
                lambda: vs([0], [[t, t]], 1, [prompt + [t + 1]], u2),                       # history does not end with tokens[0][0]
                lambda: vs([0], [[t, t]], 1, [[-1, t]], u2),                                # negative history id
                lambda: vs([0], [[t, t]], 1, [([t] * cfg["max_seq_len"])], u2),             # history + k > max_seq_len
                lambda: vs([0], [[t, t]], 1, h, [[0.5, 1.5]]),                              # draw outside [0, 1]
                lambda: vs([0], [[t, t]], 1, h, [[nan, 0.5]]),
                lambda: vs([0], [[t, t]], 1, h, u2, repetition_penalty=0.0),
                lambda: vs([0], [[t, t]], 1, h, u2, temperature=nan),
                lambda: vs([0], [[t, t]], 1, h, u2, top_p=nan),
                lambda: hm.sampled_lookup([0], [t], 4, [prompt + [t + 1]], [[0.5]] * 4),
                lambda: hm.sampled_lookup([0], [t], 4, h, [[0.5]] * 3 + [[-0.1]]),
                lambda: hm.sampled_lookup([0], [t], 4, h, [[0.5]] * 4, repetition_penalty=0.0),
                lambda: hm.sampled_lookup([0], [t], 4, h, [[0.5]] * 4, ngram=0)):
        assert code_of(bad) == INVALID
    # (k = 0 and a missing history are refused by the library too, below the Python wrapper's own checks)
    import ctypes as C
    sp = gpu._lib.sampling_params()
    ids, toks, acc, out = np.zeros(1, np.int64), np.full(2, t, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int32)
    uu, lens, none = np.full(2, 0.5, np.float32), np.asarray([13], np.int32), (C.c_void_p * 1)(None)
    hist = np.asarray(h[0], np.int32)
    ptrs = (C.c_void_p * 1)(hist.ctypes.data)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda k, hp: hm.lib.nvl_verify_sampled(hm.h, 1, p(ids), p(toks), k, C.byref(sp), hp, p(lens), p(uu), p(acc), p(out))
    assert call(0, ptrs) == INVALID and call(8, ptrs) == INVALID and call(1, none) == INVALID
    assert code_of(lambda: vs([9], [[t, t]], 1, h, u2)) == UNKNOWN_SEQ
    assert code_of(lambda: hm.sampled_lookup([9], [t], 4, h, [[0.5]] * 4)) == UNKNOWN_SEQ
    assert hm.seq_len(0) == 12 and hm.seq_len(1) == 12
    assert call(1, ptrs) == 0 and hm.seq_len(0) == 13 + int(acc[0])                          # and the good call goes through
    hm.close()
    _, _, hm = build(gpu, None, "llama", "bf16", cfg_over=dict(max_seq_len=64), max_batch_tokens=64)
    long = (prompt * 5)[:60]
    prefill(hm, 0, long)                                                                     # 60 cached of 64
    h60 = [long + [t]]
    assert code_of(lambda: hm.verify_sampled([0], [[t] * 6], 5, h60, [[0.5] * 6])) == POSITION              # 60 + 6 > 64
    assert code_of(lambda: hm.verify_sampled([0], [[t] * 5], 4, [[t]], [[0.5] * 5])) == POSITION            # 60 + 5 > 64
    assert code_of(lambda: hm.sampled_lookup([0], [t], 5, [[t]], [[0.5]] * 5)) == POSITION
    assert hm.seq_len(0) == 60
    acc, _ = hm.verify_sampled([0], [[t] * 4], 3, h60, [[0.5] * 4])                          # 60 + 4 fits exactly
    assert hm.seq_len(0) == 61 + int(acc[0])
    hm.close()
    # paged, hybrid (a Mamba2 state cannot be rolled back) and tensor-parallel models are refused
    _, _, paged = build(gpu, None, "llama", "bf16", kv_num_blocks=4, kv_block_size=64)
    assert code_of(lambda: paged.verify_sampled([0], [[t] * 2], 1, h, u2)) == STATE
    assert code_of(lambda: paged.sampled_lookup([0], [t], 4, h, [[0.5]] * 4)) == STATE
    assert code_of(lambda: paged.verify_sampled_paged([[t] * 2], 1, [0], [[0]], [[-1, t]], u2)) == INVALID
    assert code_of(lambda: paged.verify_sampled_paged([[t] * 2], 1, [0], [[9]], h, u2)) == INVALID         # block id
    paged.close()
    _, _, slab = build(gpu, None, "llama", "bf16")
    assert code_of(lambda: slab.verify_sampled_paged([[t] * 2], 1, [0], [[0]], h, u2)) == STATE
    slab.close()
    _, _, hyb = build(gpu, None, "granite_hybrid", "bf16")
    prefill(hyb, 0, [1, 2, 3])
    assert code_of(lambda: hyb.verify_sampled([0], [[1, 2]], 1, [[3, 1]], u2)) == STATE
    assert code_of(lambda: hyb.sampled_lookup([0], [1], 4, [[3, 1]], [[0.5]] * 4)) == STATE
    assert hyb.seq_len(0) == 3
    hyb.close()
    _, _, tp1 = build(gpu, None, "llama", "bf16", tp_force_single=True)
    tp1.seq_reset(0) if tp1.seq_len(0) >= 0 else gpu._lib.check(tp1.lib.nvl_seq_open(tp1.h, 0), tp1.h)
    assert code_of(lambda: tp1.verify_sampled([0], [[t] * 2], 1, [[t]], u2)) == STATE
    assert code_of(lambda: tp1.sampled_lookup([0], [t], 4, [[t]], [[0.5]] * 4)) == STATE
    assert tp1.seq_len(0) == 0
    tp1.close()
    # the op-level tap
    lg = np.zeros((2, 16), np.float32)
    sd = gpu.ops.sample_drafts
    for bad in (lambda: sd(lg, [[3, 1]], 1, [[5, 4]], [0.5, 0.5]),                          # does not end with tokens[0][0]
                lambda: sd(lg, [[3, 1]], 1, [[-1, 3]], [0.5, 0.5]),
                lambda: sd(lg, [[3, 1]], 1, [[5, 3]], [0.5, 1.5]),
                lambda: sd(lg, [[3, 1]], 1, [[5, 3]], [0.5, 0.5], repetition_penalty=0.0)):
        assert code_of(bad) == INVALID
