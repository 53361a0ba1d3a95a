"""Speculative decoding with a draft MODEL (nvl_draft_sampled, nvl_verify_speculative,
nvl_decode_speculative, nvl_op_spec_reject) on the tiny families of synth.tiny_config.

Bounds, all stated before any device result:
  kernel   : on dyadic distributions (multiples of 2^-12: every sum is exact in any order) n_accepted, out_tokens and
             accept_prob_out equal tests/test_spec_draft_host.spec_reject_ref exactly; on general distributions the accept
             decisions are the fp32 compare on the returned pairs exactly, the pairs are the inputs' entries bit for bit, the
             emitted id of a rejected row owns the float64 CDF interval of the normalised residual around uf within 2e-3 of
             mass (the id tolerance of tests/test_sampling_gpu.py) and the bonus id of a fully accepted row is the sampler's
  greedy   : top_k = 1 without a penalty makes p and q point masses: the pass must give nvl_verify_greedy's answer on a twin
             target fed the same rows, and the loop nvl_decode_greedy's ids (margin-safe prompts of test_spec_decode_gpu)
  p_j(d_j) : against the oracle's sampler distribution on the oracle's rows, relative bound
             (1 + 1e-3) * e^(2 * TOL["f32"] * max|logit|) - 1: check_rows' 1e-3 of tests/test_sampling_gpu.py times what a
             log-probability error of 2 * TOL * max|logit| (tests/test_spec_decode_gpu.py) does to a probability
  cache    : the draft's next-step logits within TOL["bf16"] of a fresh draft prefilled with prompt + emitted ids"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import rel_err
from test_spec_decode_gpu import P0, P1, TOL, build, code_of, prefill, safe_prompt
from test_spec_draft_host import dyadic, spec_reject_ref
from test_spec_sampled_gpu import SAMPLING, concat, oracle_rows, sampled_ids

pytestmark = pytest.mark.gpu

GREEDY = dict(top_k=1, repetition_penalty=1.0)
PLAIN = dict(temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0)
BELOW_ONE = float(np.float32(1.0) - np.float32(2.0 ** -24))


def make(gpu, precision, weights=None, seed=7, peaked=0.0, family="llama", cfg_over=None, **kw):
    cfg = gpu.synth.tiny_config(family, **(cfg_over or {}))
    w = weights if weights is not None else gpu.synth.make_weights(cfg, seed=seed, scale=0.05, peaked_head=peaked)
    kw.setdefault("max_seqs", 4)
    kw.setdefault("max_batch_tokens", 256)
    return cfg, w, gpu.HipTransformerModel(cfg, w, precision=precision, **kw)


def perturbed(gpu, cfg, noise, peaked=0.0):
    """the seed-7 weights of tests/test_spec_decode_gpu.build with noise on every attention-output and FFN-down matrix: a
    model of DIFFERENT weights whose proposals the target still accepts now and then"""
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=peaked)
    r = np.random.default_rng(99)
    for key in sorted(w):
        if key[0] in ("w2", "wo"):
            w[key] = gpu.synth.round_bf16(w[key] + np.float32(noise * 0.05) * r.standard_normal(w[key].shape).astype(np.float32))
    return w


# ---- 4. the kernel against the restatement, exact ---------------------------------------------------------------------
def exact_case(r, V, k):
    """4 sequences accepting [0, k, k // 2, k] drafts; dyadic rows with <= 256 entries; every special draw of the rule"""
    n, S, s = 4, 1 + k, min(V - 2, 255)
    plan = [0, k, k // 2, k]
    p, q = np.zeros((n, S, V), np.float32), np.zeros((n, k, V), np.float32)
    toks = np.zeros((n, S), np.int32)
    ua = np.full((n, k), 2.0 ** -13, np.float32)                             # ua * q <= 2^-13 < 2^-12 <= any positive p
    uf = (r.integers(1, 1024, n) / 1024.0).astype(np.float32)
    for i in range(n):
        for j in range(S):
            ids = r.permutation(V)[: s + 1]
            sp, x, z = ids[:s], ids[0], ids[s]                               # p lives on sp; q on sp - {x} + {z}
            p[i, j] = dyadic(r, V, sp, 4096)
            if j == k:
                continue
            sq = np.concatenate([sp[1:], [z]])
            q[i, j] = dyadic(r, V, sq, 4096)
            if j < plan[i]:
                toks[i, j + 1] = sp[1]                                       # p > 0, q > 0, tiny draw: accepted
            elif j == plan[i]:
                toks[i, j + 1] = z                                           # p = 0 < q: rejected whatever the draw
            else:
                toks[i, j + 1] = sq[r.integers(0, len(sq))]                  # behind the rejection: never looked at
                ua[i, j] = r.random()
    ua[0, 0], uf[0] = 0.0, 0.0                                              # rejected even at ua = 0; uf = 0 emits id 0
    ua[1, 0], uf[1] = 0.0, BELOW_ONE                                        # accepted at ua = 0; the bonus scan's last step
    toks[3, 1], ua[3, 0] = np.flatnonzero((p[3, 0] > 0) & (q[3, 0] == 0))[0], 1.0      # q(d) = 0 < p(d): accepted at ua = 1
    m = plan[2]                                                             # p <= q everywhere (p == q), ua = 1: rejected, R == 0
    q[2, m] = p[2, m]
    toks[2, m + 1], ua[2, m] = np.flatnonzero(p[2, m])[0], 1.0
    return p, q, toks, ua, uf, plan


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("V", [7, 1000, 50257])
def test_kernel_equals_the_restatement_exactly(gpu, V, k):
    p, q, toks, ua, uf, plan = exact_case(np.random.default_rng(10 * V + k), V, k)
    want_acc, want_out, want_ap = spec_reject_ref(p, q, toks, ua, uf)
    assert want_acc.tolist() == plan
    assert ((np.maximum(p[2, plan[2]] - q[2, plan[2]], 0)).sum() == 0)        # the R == 0 fallback is exercised
    acc, out, ap = gpu.ops.spec_reject(p, q, toks, ua, uf)
    print(f"V {V} k {k}: n_accepted {acc.tolist()} out {out.tolist()}")
    assert acc.tolist() == want_acc.tolist()
    assert out.tolist() == want_out.tolist()
    assert ap.tobytes() == want_ap.astype(np.float32).tobytes()
    acc2, out2, ap2 = gpu.ops.spec_reject(p, q, toks, ua, uf)
    assert (acc2.tobytes(), out2.tobytes(), ap2.tobytes()) == (acc.tobytes(), out.tobytes(), ap.tobytes())


# ---- 5. the kernel on general distributions ----------------------------------------------------------------------------
def test_kernel_on_general_distributions(gpu):
    V, k, n = 50257, 3, 6
    S = 1 + k
    r = np.random.default_rng(17)
    temps = np.repeat([0.5, 1.0, 2.0], 2 * S)                               # three temperatures, two sequences each
    logits = (r.standard_normal((n * S, V)) * 2.0).astype(np.float32)
    # p: the device sampler's own final distribution of these logits (so the bonus id can be compared bit for bit)
    p = np.empty((n * S, V), np.float32)
    for t in (0.5, 1.0, 2.0):
        sel = np.flatnonzero(temps == t)
        _, p[sel] = gpu.ops.sample_with_history(logits[sel], None, np.full(len(sel), 0.5), return_probs=True,
                                                temperature=t, repetition_penalty=1.0)
    p = p.reshape(n, S, V)
    noisy = logits.reshape(n, S, V)[:, :k] / temps.reshape(n, S)[:, :k, None] + 0.7 * r.standard_normal((n, k, V))
    e = np.exp(noisy - noisy.max(axis=2, keepdims=True))
    q = (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
    q[0::2] = p[0::2, :k]                                                   # q = p: every draft of these sequences is accepted
    toks = np.zeros((n, S), np.int32)
    for i in range(n):
        for j in range(k):                                                  # d_j ~ q_j
            c = np.cumsum(q[i, j].astype(np.float64))
            toks[i, j + 1] = min(int(np.searchsorted(c, r.random() * c[-1])), V - 1)
    ua = r.random((n, k)).astype(np.float32)
    uf = r.random(n).astype(np.float32)
    acc, out, ap = gpu.ops.spec_reject(p, q, toks, ua, uf)
    rows = np.arange(n)
    for j in range(k):                                                      # the pairs are the inputs' entries, bit for bit
        assert ap[:, j, 0].tobytes() == p[rows, j, toks[:, j + 1]].tobytes()
        assert ap[:, j, 1].tobytes() == q[rows, j, toks[:, j + 1]].tobytes()
    ok = (np.float32(ua) * np.float32(ap[:, :, 1])).astype(np.float32) < np.float32(ap[:, :, 0])
    assert acc.tolist() == np.cumprod(ok, axis=1).sum(axis=1).tolist()
    assert (acc[0::2] == k).all() and (acc[1::2] < k).any()
    print("n_accepted", acc.tolist())
    for i in range(n):
        a = int(acc[i])
        assert out[i, :a].tolist() == toks[i, 1:a + 1].tolist() and (out[i, a + 1:] == -1).all()
        g = int(out[i, a])
        if a < k:
            res = np.maximum(p[i, a].astype(np.float64) - q[i, a].astype(np.float64), 0.0)
            c = np.cumsum(res / res.sum())
            x = float(uf[i])
            lo = c[g - 1] if g > 0 else 0.0
            assert lo - 2e-3 <= x <= c[g] + 2e-3, (i, a, g, lo, c[g], x)
            assert res[g] > 0 or g == 0
        else:
            t = float(temps[i * S + k])
            want = gpu.ops.sample_with_history(logits[i * S + k], None, [uf[i]], temperature=t, repetition_penalty=1.0)
            assert g == int(want[0])


# ---- 6. draft_sampled is decode_sampled --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7])
def test_draft_sampled_is_decode_sampled(gpu, k):
    cfg, _, a = build(gpu, None, "llama", "bf16")
    _, _, b = build(gpu, None, "llama", "bf16")
    r = np.random.default_rng(40 + k)
    prompts = [r.integers(0, cfg["vocab_size"], m).tolist() for m in (P0, P1)]
    firsts = [prefill(a, i, p) for i, p in enumerate(prompts)]
    assert [prefill(b, i, p) for i, p in enumerate(prompts)] == firsts
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    u = r.random((k, 2)).astype(np.float32)
    got = a.draft_sampled([0, 1], firsts, k, hists, u, **SAMPLING)
    want = b.decode_sampled([0, 1], firsts, k, hists, u, **SAMPLING)
    assert got.tobytes() == want.tobytes()
    assert [a.seq_len(i) for i in range(2)] == [b.seq_len(i) for i in range(2)] == [P0 + k, P1 + k]
    a.close(); b.close()


# ---- 7. the pass reduces to greedy verification ------------------------------------------------------------------------
def greedy_contexts(gpu, oracle, precision):
    """62 and 19 cached tokens ending in the margin-safe prompt and its continuation (62 + drafts crosses a 64-key tile)"""
    prompt, want = safe_prompt(gpu, oracle, "llama", precision)
    filler = np.random.default_rng(62).integers(0, 1000, P0 - len(prompt) - len(want)).tolist()
    return [filler + prompt + want, (prompt + want)[:P1]]


@pytest.mark.parametrize("precision,kw", [("f32", {}), ("bf16", {}), ("bf16", dict(kv_cache_dtype="fp8_e4m3"))])
def test_pass_reduces_to_greedy_verification(gpu, oracle, precision, kw):
    """top_k = 1: p_j and q_j are point masses, so row j is accepted iff the draft's id is the target's arg-max and the
    emitted id is the arg-max of the first rejected (or the bonus) row - nvl_verify_greedy, whatever the draws.  A sequence
    that read another sequence's or another step's row of p or q could not give this."""
    k = 4
    over = dict(tied_embedding=False)
    cfg, _, target = make(gpu, precision, peaked=4.0, cfg_over=over, **kw)
    _, _, twin = make(gpu, precision, peaked=4.0, cfg_over=over, **kw)
    _, _, draft = make(gpu, "bf16", weights=perturbed(gpu, cfg, 0.05, peaked=4.0), cfg_over=over)
    ctxs = greedy_contexts(gpu, oracle, precision)
    assert [len(c) for c in ctxs] == [P0, P1]
    r = np.random.default_rng(70)
    seen = []
    for rep in range(2):                                                    # the second pass starts from the first one's lengths
        if rep == 0:
            firsts = [prefill(target, i, c) for i, c in enumerate(ctxs)]
            assert [prefill(twin, i, c) for i, c in enumerate(ctxs)] == firsts
            for i, c in enumerate(ctxs):
                prefill(draft, i, c)
        lens = [target.seq_len(i) for i in range(2)]
        hists = [c + [f] for c, f in zip(ctxs, firsts)]
        d = draft.draft_sampled([0, 1], firsts, k, hists, r.random((k, 2)), **GREEDY)
        rows = np.concatenate([np.asarray(firsts, np.int32)[:, None], d.T.astype(np.int32)], axis=1)
        acc, out, ap = target.verify_speculative(draft, [0, 1], rows, k, hists, r.random((2, k)), r.random(2),
                                                 return_probs=True, **GREEDY)
        acc_g, out_g = twin.verify_greedy([0, 1], rows, k)
        print(f"{precision} {kw} pass {rep}: n_accepted {acc.tolist()}")
        assert acc.tolist() == acc_g.tolist() and out.tolist() == out_g.tolist()
        assert (ap[:, :, 1] == 1.0).all() and np.isin(ap[:, :, 0], (0.0, 1.0)).all()
        assert [target.seq_len(i) for i in range(2)] == [n + int(a) + 1 for n, a in zip(lens, acc)]
        assert [draft.seq_len(i) for i in range(2)] == [n + k for n in lens]          # untouched by the pass
        seen += acc.tolist()
        for i in range(2):                                                  # the caller's rollback, then go on from the emitted id
            draft.seq_truncate(i, min(target.seq_len(i), draft.seq_len(i)))
            target.seq_truncate(i, draft.seq_len(i)); twin.seq_truncate(i, draft.seq_len(i))
            a = int(acc[i])
            keep = draft.seq_len(i) - lens[i]                               # rows of this pass both caches keep (<= a + 1)
            ctxs[i] = ctxs[i] + rows[i, :keep].tolist()
            firsts[i] = int(out[i, keep - 1]) if keep == a + 1 else int(rows[i, keep])
    target.close(); twin.close(); draft.close()


# ---- 8. all accepted ------------------------------------------------------------------------------------------------------
def test_same_weights_accept_everything(gpu, oracle):
    """Target and draft of the SAME weights, both bf16, plain sampling (T = 1, no cuts, no penalty), accept draws <= 0.5.
    One-row (draft) and 1 + k-row (target) log-probabilities each lie within 2 * TOL["bf16"] * max|logit| of the oracle; with
    max|logit| < 5 (asserted on the oracle's rows) p / q >= e^(-4 * 0.015 * 5) = e^-0.3 ~ 0.74 > 0.5: every draft is accepted.
    The bonus id is the sampler's on row k (bit-identical: the same distribution, the same scan)."""
    k = 3
    cfg, _, target = build(gpu, None, "llama", "bf16")
    _, _, draft = build(gpu, None, "llama", "bf16")
    r = np.random.default_rng(80)
    prompts = [r.integers(0, cfg["vocab_size"], m).tolist() for m in (P0, P1)]
    firsts = [prefill(target, i, p) for i, p in enumerate(prompts)]
    for i, p in enumerate(prompts):
        prefill(draft, i, p)
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    d = draft.draft_sampled([0, 1], firsts, k, hists, r.random((k, 2)), **PLAIN)
    rows = np.concatenate([np.asarray(firsts, np.int32)[:, None], d.T.astype(np.int32)], axis=1)
    want = oracle_rows(gpu, oracle, "llama", prompts, rows)
    assert float(np.abs(want).max()) < 5.0
    ua, uf = (0.5 * r.random((2, k))).astype(np.float32), r.random(2).astype(np.float32)
    acc, out, ap = target.verify_speculative(draft, [0, 1], rows, k, hists, ua, uf, return_probs=True, **PLAIN)
    print("p/q", (ap[:, :, 0] / ap[:, :, 1]).tolist())
    assert acc.tolist() == [k, k]
    assert out[:, :k].tolist() == d.T.tolist()
    u_rows = np.zeros((2, 1 + k), np.float32)
    u_rows[:, k] = uf
    assert out[:, k].tolist() == sampled_ids(target, hists, rows, u_rows, PLAIN)[:, k].tolist()
    assert [target.seq_len(i) for i in range(2)] == [P0 + k + 1, P1 + k + 1]
    target.close(); draft.close()


# ---- 9. decisions replayable ----------------------------------------------------------------------------------------------
SEED9 = 109         # (a seed for which the oracle alone, drafting with its own sampler, excludes no case by cut_safe's rule)


def cut_safe(oracle, logits, hist, d, b, kw):
    """The margin rule of the p_j(d_j) comparison.  A case is compared unless a relative perturbation `b` of the oracle's
    pre-cut probabilities could change WHICH ids survive in a way that moves p(d) by more than b:
      top-k : d itself is the last id kept or the first dropped and the two are within b of each other (a flip among other
              ids exchanges two probabilities that differ by less than b: p(d) moves by less than b);
      top-p : the cumulative mass of the kept prefix lies within b of top_p on either side of the cut (one id more or
              fewer is kept and every survivor is rescaled by that id's share)."""
    _, pre = oracle.sample_with_history(logits, hist, 0.5, return_probs=True, **dict(kw, top_k=0, top_p=1.0))
    order = np.argsort(-pre.astype(np.float64), kind="stable")
    s = pre[order].astype(np.float64)
    K, top_p = kw["top_k"], kw["top_p"]
    if s[K - 1] * (1 - b) <= s[K] * (1 + b) and d in (int(order[K - 1]), int(order[K])):
        return False
    c = np.cumsum(s[:K] / s[:K].sum())
    n = int(np.searchsorted(c, top_p, side="left")) + 1                     # the shortest prefix whose mass reaches top_p
    lo = c[n - 2] if n >= 2 else 0.0
    return not (c[min(n, K) - 1] - top_p <= b or top_p - lo <= b)


def test_decisions_are_replayable_and_p_matches_the_oracle(gpu, oracle):
    k, S = 3, 4
    cfg, _, target = build(gpu, None, "llama", "f32")
    _, _, draft = make(gpu, "bf16", weights=perturbed(gpu, cfg, 0.2))
    r = np.random.default_rng(SEED9)
    prompts = [r.integers(0, cfg["vocab_size"], m).tolist() for m in (P0, P1)]
    firsts = [prefill(target, i, p) for i, p in enumerate(prompts)]
    for i, p in enumerate(prompts):
        prefill(draft, i, p)
    hists = [p + [f] for p, f in zip(prompts, firsts)]
    u_d, ua, uf = r.random((k, 2)).astype(np.float32), r.random((2, k)).astype(np.float32), r.random(2).astype(np.float32)
    d = draft.draft_sampled([0, 1], firsts, k, hists, u_d, **SAMPLING)
    rows = np.concatenate([np.asarray(firsts, np.int32)[:, None], d.T.astype(np.int32)], axis=1)
    acc, out, ap = target.verify_speculative(draft, [0, 1], rows, k, hists, ua, uf, return_probs=True, **SAMPLING)
    ok = (np.float32(ua) * np.float32(ap[:, :, 1])).astype(np.float32) < np.float32(ap[:, :, 0])
    assert acc.tolist() == np.cumprod(ok, axis=1).sum(axis=1).tolist()
    assert (ap[:, :, 1] > 0).all()                                          # the draft drew d from q: q(d) > 0
    want = oracle_rows(gpu, oracle, "llama", prompts, rows)
    big = float(np.abs(want).max())
    assert big < 5.0
    b = (1 + 1e-3) * math.exp(2 * TOL["f32"] * big) - 1                      # 1e-3 (sampler sums) x e^(log-probability bound)
    row_hists = concat(hists, rows)
    cases = excluded = 0
    for i in range(2):
        for j in range(k):
            cases += 1
            dj, row = int(rows[i, j + 1]), i * S + j
            if not cut_safe(oracle, want[row], row_hists[row], dj, b, SAMPLING):
                excluded += 1
                continue
            _, want_p = oracle.sample_with_history(want[row], row_hists[row], 0.5, return_probs=True, **SAMPLING)
            err = abs(float(ap[i, j, 0]) - float(want_p[dj]))
            print(f"seq {i} row {j}: p(d) {float(ap[i, j, 0]):.6e} oracle {float(want_p[dj]):.6e} (bound {b * float(want_p[dj]):.3e})")
            assert err <= b * float(want_p[dj]) + 1e-12, (i, j)
    assert excluded <= 0.05 * cases, (excluded, cases)
    target.close(); draft.close()


# ---- 10. the loop -----------------------------------------------------------------------------------------------------------
def loop_uniforms(r, n_steps, n, k, accept_max=1.0):
    u = r.random((n_steps, n, 2 * k + 1)).astype(np.float32)
    u[:, :, k:2 * k] *= np.float32(accept_max)
    return u


def check_draft_cache(gpu, draft, fresh, i, ctx, first, emitted):
    """the draft holds ctx + first + emitted[:-1]: its next step must be a fresh draft's after a prefill of exactly that"""
    n = len(ctx) + len(emitted)
    assert draft.seq_len(i) == n
    lg_a, _ = draft.forward_batch([i], [[int(emitted[-1])]], [n])
    prefill(fresh, i, list(ctx) + [first] + [int(t) for t in emitted[:-1]])
    lg_b, _ = fresh.forward_batch([i], [[int(emitted[-1])]], [n])
    err = rel_err(lg_a, lg_b)
    print(f"draft cache seq {i}: next-step logits rel err {err:.3e} (bound {TOL['bf16']:.1e})")
    assert err <= TOL["bf16"]


def test_loop_reduces_to_greedy_decoding(gpu, oracle):
    n_steps, k = 12, 3
    over = dict(tied_embedding=False)
    prompt, want = safe_prompt(gpu, oracle, "llama", "f32", n_steps=4 + n_steps + 1)
    ctxs = [prompt, prompt + want[:4]]
    cfg, _, target = make(gpu, "f32", peaked=4.0, cfg_over=over)
    _, _, twin = make(gpu, "f32", peaked=4.0, cfg_over=over)
    wd = perturbed(gpu, cfg, 0.1, peaked=4.0)      # (the oracle's copy of this draft is accepted 0, 3, 3, 0, 1 / 3, 0, 0, 1, 1, 1 times)
    _, _, draft = make(gpu, "bf16", weights=wd, cfg_over=over)
    _, _, fresh = make(gpu, "bf16", weights=wd, cfg_over=over)
    firsts = [prefill(target, i, c) for i, c in enumerate(ctxs)]
    assert [prefill(twin, i, c) for i, c in enumerate(ctxs)] == firsts == [want[0], want[4]]
    for i, c in enumerate(ctxs):
        prefill(draft, i, c)
    hists = [c + [f] for c, f in zip(ctxs, firsts)]
    u = loop_uniforms(np.random.default_rng(100), n_steps, 2, k)
    got, passes, accepted = target.decode_speculative(draft, [0, 1], firsts, n_steps, hists, u, k=k, **GREEDY)
    ref = twin.decode_greedy([0, 1], firsts, n_steps)
    print(f"passes {passes}, accepted {accepted.tolist()}")
    assert got.tolist() == ref.tolist()
    assert got[:, 0].tolist() == want[1:1 + n_steps] and got[:, 1].tolist() == want[5:5 + n_steps]
    assert [target.seq_len(i) for i in range(2)] == [draft.seq_len(i) for i in range(2)] == [len(c) + n_steps for c in ctxs]
    assert math.ceil(n_steps / (k + 1)) < passes <= n_steps and accepted.sum() > 0         # rejections and acceptances both happened
    assert (accepted >= 0).all() and (accepted <= n_steps).all()
    for i in range(2):
        check_draft_cache(gpu, draft, fresh, i, ctxs[i], firsts[i], got[:, i])
    for m in (target, twin, draft, fresh):
        m.close()


def test_loop_with_the_target_as_draft_takes_the_fewest_passes(gpu, oracle):
    """draft == target in weights (bf16), accept draws <= 0.5, top_k = 1 on a margin-safe prompt: every proposal is the
    target's own arg-max, every pass emits k + 1 ids, and each pass needs the cached row of its last proposal (the extra
    draft step): without it the draft's next proposals, and the cache check below, go wrong."""
    n_steps, k = 12, 3
    over = dict(tied_embedding=False)
    prompt, want = safe_prompt(gpu, oracle, "llama", "bf16", n_steps=n_steps + 1)
    cfg, _, target = make(gpu, "bf16", peaked=4.0, cfg_over=over)
    _, _, draft = make(gpu, "bf16", peaked=4.0, cfg_over=over)
    _, _, fresh = make(gpu, "bf16", peaked=4.0, cfg_over=over)
    first = prefill(target, 0, prompt)
    prefill(draft, 0, prompt)
    assert first == want[0]
    u = loop_uniforms(np.random.default_rng(101), n_steps, 1, k, accept_max=0.5)
    got, passes, accepted = target.decode_speculative(draft, [0], [first], n_steps, [prompt + [first]], u, k=k, **GREEDY)
    assert got[:, 0].tolist() == want[1:1 + n_steps]
    assert passes == math.ceil(n_steps / (k + 1)) and accepted.tolist() == [n_steps - passes]
    assert target.seq_len(0) == draft.seq_len(0) == len(prompt) + n_steps
    check_draft_cache(gpu, draft, fresh, 0, prompt, first, got[:, 0])
    for m in (target, draft, fresh):
        m.close()


def test_loop_up_to_the_last_position(gpu, oracle):
    """Two sequences, one of which ends at max_seq_len - 1 (the longest nvl_decode_sampled's history rule allows) and runs
    ahead of the other: the draft's extra step and its history must still fit, so k shrinks by the draft's needs too.  On the
    oracle's copies of these models the passes propose 3, 3, 3, 3, 1 (while the long sequence has one token left and room for
    one row only), 2, 1 drafts."""
    n_steps, k, T = 12, 3, 64
    over = dict(tied_embedding=False, max_seq_len=T)
    r = np.random.default_rng(0)
    ctxs = [r.integers(0, 1000, T - 1 - n_steps).tolist(), r.integers(0, 1000, 30).tolist()]
    cfg = gpu.synth.tiny_config("llama", **over)
    om = oracle.OracleModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05, peaked_head=4.0))
    for c in ctxs:                                                          # margin-safe, as safe_prompt demands of its prompts
        _, margins = om.greedy(c, n_steps + 1, return_margins=True)
        assert min(margins) > 2 * TOL["f32"]
    _, _, target = make(gpu, "f32", peaked=4.0, cfg_over=over)
    _, _, twin = make(gpu, "f32", peaked=4.0, cfg_over=over)
    wd = perturbed(gpu, cfg, 0.1, peaked=4.0)
    _, _, draft = make(gpu, "bf16", weights=wd, cfg_over=over)
    _, _, fresh = make(gpu, "bf16", weights=wd, cfg_over=over)
    firsts = [prefill(target, i, c) for i, c in enumerate(ctxs)]
    assert [prefill(twin, i, c) for i, c in enumerate(ctxs)] == firsts
    for i, c in enumerate(ctxs):
        prefill(draft, i, c)
    hists = [c + [f] for c, f in zip(ctxs, firsts)]
    u = loop_uniforms(np.random.default_rng(102), n_steps, 2, k)
    got, passes, accepted = target.decode_speculative(draft, [0, 1], firsts, n_steps, hists, u, k=k, **GREEDY)
    print(f"passes {passes}, accepted {accepted.tolist()}")
    assert got.tolist() == twin.decode_greedy([0, 1], firsts, n_steps).tolist()
    assert [target.seq_len(i) for i in range(2)] == [draft.seq_len(i) for i in range(2)] == [T - 1, 30 + n_steps]
    for i in range(2):
        check_draft_cache(gpu, draft, fresh, i, ctxs[i], firsts[i], got[:, i])
    # one step further does not fit the history: refused up front, nothing moves
    for i, c in enumerate(ctxs):
        prefill(target, i, c); prefill(draft, i, c)
    u13 = loop_uniforms(np.random.default_rng(103), n_steps + 1, 2, k)
    assert code_of(lambda: target.decode_speculative(draft, [0, 1], firsts, n_steps + 1, hists, u13, k=k, **GREEDY)) == -1
    assert [target.seq_len(i) for i in range(2)] == [draft.seq_len(i) for i in range(2)] == [len(c) for c in ctxs]
    for m in (target, twin, draft, fresh):
        m.close()


# ---- 11. error codes --------------------------------------------------------------------------------------------------------
def test_error_codes_leave_both_models_alone(gpu):
    INVALID, UNKNOWN_SEQ, STATE = -1, -3, -7
    k = 2
    cfg, _, target = build(gpu, None, "llama", "bf16")
    _, _, draft = make(gpu, "bf16", seed=8)
    V = cfg["vocab_size"]
    prompt = np.random.default_rng(9).integers(0, V, 12).tolist()
    first = prefill(target, 0, prompt)
    prefill(draft, 0, prompt)
    h = [prompt + [first]]
    ud, ua, uf = np.full((k, 1), 0.5, np.float32), np.full((1, k), 0.5, np.float32), [0.5]

    def propose():
        draft.seq_truncate(0, 12)
        d = draft.draft_sampled([0], [first], k, h, ud, **SAMPLING)
        return np.asarray([[first] + d[:, 0].tolist()], np.int32)

    vs = lambda rows, kk=k, ids=(0,), **kw: target.verify_speculative(kw.pop("draft", draft), list(ids), rows, kk, kw.pop("h", h),
                                                                      kw.pop("ua", ua), kw.pop("uf", uf), **SAMPLING)
    lens = lambda: (target.seq_len(0), draft.seq_len(0))
    assert code_of(lambda: vs(np.asarray([[first, 1, 2]], np.int32))) == STATE               # no proposals yet
    rows = propose()
    assert lens() == (12, 12 + k)
    draft.forward_batch([0], [[int(rows[0, k])]], [12 + k])                                    # a forward in between: stale
    assert code_of(lambda: vs(rows)) == STATE
    # ... also when that forward is a REPLAYED graph (third sight of its launch configuration on), which enqueues nothing anew
    replays = draft.stats()["graph_replays"]
    for _ in range(4):
        rows = propose()
        draft.forward_batch([0], [[int(rows[0, k])]], [12 + k])
        assert code_of(lambda: vs(rows)) == STATE
        assert lens() == (12, 12 + k + 1)
    assert draft.stats()["graph_replays"] > replays                                          # one of them was a replay
    rows = propose()
    wrong = rows.copy()
    wrong[0, 1] = (wrong[0, 1] + 1) % V
    assert code_of(lambda: vs(wrong)) == INVALID                                             # not the draft's id
    assert code_of(lambda: vs(rows[:, :2], kk=1, ua=ua[:, :1])) == INVALID                   # k is not the kept proposals'
    assert code_of(lambda: vs(rows, ids=(1,))) == INVALID                                    # nor the sequence
    assert code_of(lambda: vs(rows, ua=[[0.5, 1.5]])) == INVALID                             # a uniform outside [0, 1]
    assert code_of(lambda: vs(rows, uf=[-0.1])) == INVALID
    assert code_of(lambda: vs(rows, h=[prompt + [first + 1]])) == INVALID                    # nvl_verify_sampled's refusals apply
    # k = 0 and k = 8 (below the wrapper's own checks)
    sp = gpu._lib.sampling_params()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ids, acc, out = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(9, np.int32)
    toks9, u9, hist = np.full(9, first, np.int32), np.full(9, 0.5, np.float32), np.asarray(h[0], np.int32)
    ptrs, hl = (C.c_void_p * 1)(hist.ctypes.data), np.asarray([hist.size], np.int32)
    call = lambda t, d, kk: target.lib.nvl_verify_speculative(t, d, 1, p(ids), p(toks9), kk, C.byref(sp), ptrs, p(hl), p(u9), p(u9),
                                                              p(acc), p(out), None)
    assert call(target.h, draft.h, 0) == INVALID and call(target.h, draft.h, 8) == INVALID
    assert call(target.h, target.h, k) == INVALID                                            # draft == target
    assert draft.lib.nvl_draft_sampled(draft.h, 1, p(ids), p(toks9), 0, C.byref(sp), ptrs, p(hl), p(u9), p(out)) == INVALID
    assert draft.lib.nvl_draft_sampled(draft.h, 1, p(ids), p(toks9), 8, C.byref(sp), ptrs, p(hl), p(u9), p(out)) == INVALID
    # an unknown sequence on either model
    assert code_of(lambda: draft.draft_sampled([9], [first], k, h, ud, **SAMPLING)) == UNKNOWN_SEQ
    prefill(draft, 1, prompt)
    draft.seq_truncate(0, 12)
    d2 = draft.draft_sampled([0, 1], [first, first], k, h * 2, np.full((k, 2), 0.5, np.float32), **SAMPLING)
    rows2 = np.concatenate([np.full((2, 1), first, np.int32), d2.T.astype(np.int32)], axis=1)
    assert code_of(lambda: target.verify_speculative(draft, [0, 1], rows2, k, h * 2, np.full((2, k), 0.5), [0.5, 0.5], **SAMPLING)) == UNKNOWN_SEQ
    u_loop = np.full((4, 1, 2 * k + 1), 0.5, np.float32)
    assert code_of(lambda: target.decode_speculative(draft, [9], [first], 4, h, u_loop, k=k, **SAMPLING)) == UNKNOWN_SEQ
    assert code_of(lambda: target.decode_speculative(draft, [0], [first], 4, h, u_loop, k=k, **SAMPLING)) == INVALID   # 12 vs 12 + k cached
    assert lens() == (12, 12 + k) and draft.seq_len(1) == 12 + k
    # the good call still goes through on the kept proposals (the refusals above changed nothing on the draft)
    draft.seq_truncate(0, 12); draft.seq_truncate(1, 12)
    rows = propose()
    acc, _ = vs(rows)
    assert lens() == (13 + int(acc[0]), 12 + k)
    # vocabulary mismatch; paged target; paged draft; Mamba2 draft; f32 draft
    _, _, other = make(gpu, "bf16", seed=8, cfg_over=dict(vocab_size=1003))
    prefill(other, 0, prompt)
    d = other.draft_sampled([0], [first], k, h, ud, **SAMPLING)
    target.seq_truncate(0, 12)
    assert code_of(lambda: vs(np.asarray([[first] + d[:, 0].tolist()], np.int32), draft=other)) == INVALID
    assert code_of(lambda: target.decode_speculative(other, [0], [first], 4, h, u_loop, k=k, **SAMPLING)) == INVALID
    assert (target.seq_len(0), other.seq_len(0)) == (12, 12 + k)
    other.close()
    rows = propose()
    _, _, paged = build(gpu, None, "llama", "bf16", kv_num_blocks=4, kv_block_size=64)
    assert code_of(lambda: paged.verify_speculative(draft, [0], rows, k, h, ua, uf, **SAMPLING)) == STATE
    assert code_of(lambda: paged.draft_sampled([0], [first], k, h, ud, **SAMPLING)) == STATE
    assert code_of(lambda: target.decode_speculative(paged, [0], [first], 4, h, u_loop, k=k, **SAMPLING)) == STATE
    assert code_of(lambda: paged.decode_speculative(draft, [0], [first], 4, h, u_loop, k=k, **SAMPLING)) == STATE
    paged.close()
    _, _, hyb = build(gpu, None, "granite_hybrid", "bf16")
    prefill(hyb, 0, [1, 2, 3])
    assert code_of(lambda: hyb.draft_sampled([0], [1], k, [[3, 1]], ud, **SAMPLING)) == STATE
    assert hyb.seq_len(0) == 3
    hyb.close()
    _, _, f32 = build(gpu, None, "llama", "f32")
    prefill(f32, 0, prompt)
    assert code_of(lambda: f32.draft_sampled([0], [first], k, h, ud, **SAMPLING)) == STATE   # nvl_decode_sampled's rule
    assert f32.seq_len(0) == 12
    f32.close()
    assert lens() == (12, 12 + k)
    target.close(); draft.close()
