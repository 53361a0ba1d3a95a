"""the Mamba2 convolution window carried across calls (NVL_MAMBA_CONV_CARRIED,
HipTransformerModel(mamba_conv_state="carried")) — the general kernels (csrc/mamba.h MambaArgs::chain 3), the one-launch
decode form (mamba_conv_step_kernel, nvl_set_tuning key 39) and the model entry points.

What is mirrored and what is not.  The reference's Mamba2Layer.causalConv1d pads EVERY Forward call with zeros and never
uses its ConvCache (mamba2.go:27,181-254,356).  The DEFAULT ("per_call") still mirrors that — test_mamba_gpu.py pins it
against the oracle call by call, and the last test here pins that the default did not move.  "carried" deliberately does
NOT mirror it: the window reaches into the sequence's previous calls, so prefill(P) + decode(t) is the model's function
of the P + t tokens.  Its yardstick is therefore the oracle's ONE-SHOT Forward over the whole sequence (where the
reference's zero padding is the true padding before position 0), never the oracle fed call by call.  The SSM state is
per sequence and reset at position 0, as before.

Tolerances: the op stage against float64 F32_ELEM = 1e-5 (test_mamba_ops_gpu.py's bound for this stage); models fp32
parity mode 1e-4, bf16 1.5e-2 of the largest value (test_mamba_gpu.py TOL).  Kept rows are copies: compared bit for bit."""
import numpy as np
import pytest

import mamba_conv_state_reference as CR
import mamba_reference as R
from conftest import rel_err
from test_mamba_gpu import TOL, VARIANTS
from test_mamba_ops_gpu import F32_ELEM, Tuning, col_err, run

pytestmark = pytest.mark.gpu


# ---- the op ------------------------------------------------------------------------------------------------------------
def op_rounds(gpu, g, rounds, n_slots, seed):
    """rounds: [[(key, slot, n, pos), ...], ...], one batched chain-3 call per round on tail / state buffers that start
    as junk.  After every call: xbc / delta against the float64 contract, every touched slot's kept rows bit for bit,
    untouched slots unchanged.  -> the tails after every round."""
    rng = np.random.default_rng(seed)
    total = sum(n for rd in rounds for _, _, n, _ in rd)
    inp = R.make_inputs(g, (total,), rng)
    rows = inp["proj"]
    state = rng.standard_normal((n_slots, g.nh, g.hd, g.ss)).astype(np.float32)
    tail = rng.standard_normal((n_slots, g.K - 1, g.conv_dim)).astype(np.float32)
    ref = CR.Carried(g, inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    t0, tails = 0, []
    for ri, rd in enumerate(rounds):
        keys, slots, lens, pos = zip(*rd)
        M = sum(lens)
        part = dict(inp, proj=rows[t0:t0 + M])
        t0 += M
        out = run(gpu, g, part, lens, pos, slots, state, "f32", tail=tail, chain=3)
        want_x, want_d, want_t = ref.call(part["proj"], keys, lens, pos)
        e_x, e_d = rel_err(out["xbc"], want_x), col_err(out["delta"], want_d)
        print(f"K={g.K} round {ri} lens {lens} pos {pos}: xbc {e_x:.2e} delta {e_d:.2e}")
        assert np.isfinite(out["xbc"]).all() and np.isfinite(out["delta"]).all()
        assert e_x <= F32_ELEM and e_d <= F32_ELEM, (ri, e_x, e_d)
        for key, slot in zip(keys, slots):
            assert np.array_equal(out["tail"][slot], want_t[key].astype(np.float32)), f"round {ri}: kept rows of {key}"
        rest = [s for s in range(n_slots) if s not in slots]
        assert np.array_equal(out["tail"][rest], tail[rest]), f"round {ri}: an untouched slot changed"
        state, tail = out["state"], out["tail"]
        tails.append(tail)
    return tails


@pytest.mark.parametrize("K", [2, 4, 8])
def test_op_general_path(gpu, K):
    """Three sequences in permuted slots of four, fed raggedly in calls shorter than, equal to and longer than the
    window; "c" restarts at position 0 midway in its own slot (whose kept rows are then junk to it), and every first call
    lands on the random junk the buffers start with.  conv_dim 384 is no multiple of the 256 threads."""
    g = R.Geom(10, 32, 32, 1, K)
    calls = {"a": (2, [5, 1, 2, 1, 19]), "b": (0, [1, 1, 1, 7]), "c": (3, [2, 64, 1])}
    restart = {"c": [3, 1]}                                                 # after its three calls: from position 0 again
    rounds, pos = [], {k: 0 for k in calls}
    for ri in range(5):
        rd = []
        for key, (slot, lens) in calls.items():
            if ri < len(lens):
                n = lens[ri]
            elif key in restart and ri - len(lens) < len(restart[key]):
                j = ri - len(lens)
                n = restart[key][j]
                if j == 0:
                    pos[key] = 0
            else:
                continue
            rd.append((key, slot, n, pos[key]))
            pos[key] += n
        rounds.append(rd)
    assert [p for k, s, n, p in rounds[3] if k == "c"] == [0]               # the restart is in the batch of round 3
    op_rounds(gpu, g, rounds, 4, 20 + K)


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_op_step_kernel_against_the_two_launch_form(gpu, K, B):
    """Passes of one row per sequence (the decode form), several in a row, with key 39 = 1 (mamba_conv_step_kernel) and
    then 0 (conv kernel + tail kernel) on identical inputs: both within F32_ELEM of float64, kept rows bit-equal between
    the forms.  Sequences with an even index see their first ever call as a single row at position 0 on junk: zeros."""
    g = R.Geom(10, 32, 32, 1, K)
    slots = list(np.random.default_rng(B).permutation(B + 1)[:B])          # permuted, one slot never touched
    pre = [(i, int(slots[i]), i % 4 + 2, 0) for i in range(B) if i % 2]     # odd ones arrive with a short prefill
    pos = {i: (i % 4 + 2 if i % 2 else 0) for i in range(B)}
    rounds = [pre] if pre else []
    for _ in range(K + 1):
        rounds.append([(i, int(slots[i]), 1, pos[i]) for i in range(B)])
        for i in range(B):
            pos[i] += 1
    got = {}
    for key39 in (1, 0):
        with Tuning(gpu, 39, key39):
            got[key39] = op_rounds(gpu, g, rounds, B + 1, 40 + K)
    for a, b in zip(got[1], got[0]):
        assert np.array_equal(a, b)


# ---- models ------------------------------------------------------------------------------------------------------------
def build(gpu, precision, variant=0, mode="carried", max_seqs=4, max_batch_tokens=256, **kw):
    cfg = gpu.synth.tiny_config("granite_hybrid", **VARIANTS[variant])
    w = gpu.synth.make_weights(cfg, seed=17, scale=0.05, **kw)
    args = {} if mode is None else dict(mamba_conv_state=mode)
    return cfg, w, gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=max_seqs, max_batch_tokens=max_batch_tokens, **args)


def mamba_layers(cfg):
    return [li for li, kind in enumerate(cfg["hybrid_layers"]) if kind == "mamba"]


_ONE_SHOT = {}


def one_shot(gpu, oracle, variant, toks):
    """The oracle's one-shot Forward over toks from an empty cache: (logits of every row, SSM state per Mamba2 layer).
    Row n-1 is OracleModel.forward_with_cache(toks[:n], new_cache, 0)[-1]: the model is causal.  Shared by the tests."""
    key = (variant, tuple(toks))
    if key not in _ONE_SHOT:
        cfg = gpu.synth.tiny_config("granite_hybrid", **VARIANTS[variant])
        om = oracle.OracleModel(cfg, gpu.synth.make_weights(cfg, seed=17, scale=0.05))
        lg = np.array(om.forward_with_cache(list(toks), om.new_cache(), 0))
        _ONE_SHOT[key] = (lg, {li: np.array(om.mamba_state(li)) for li in mamba_layers(cfg)})
    return _ONE_SHOT[key]


def stepwise_errors(hm, toks, P, want, sid=3):
    """prefill toks[:P], then teacher-forced single-token nvl_forward calls: the error of every call's last-row logits
    against the one-shot rows"""
    errs = [rel_err(hm.forward_with_cache(toks[:P], seq_id=sid, pos_offset=0, all_logits=False)[-1], want[P - 1])]
    for n in range(P + 1, len(toks) + 1):
        errs.append(rel_err(hm.forward_with_cache([toks[n - 1]], seq_id=sid, pos_offset=n - 1, all_logits=False)[-1], want[n - 1]))
    return errs


@pytest.mark.parametrize("P", [1, 2, 23])                                     # the first two shorter than the window
@pytest.mark.parametrize("variant", range(len(VARIANTS)))                      # K = 4, 4, 3
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_model_parity_with_the_one_shot_forward(gpu, oracle, precision, variant, P):
    """prefill(P) + six decode steps through nvl_forward == the oracle's one-shot Forward over the same tokens, at every
    step; the SSM state and the kept rows afterwards are those of the whole sequence.  The same comparison on a per_call
    model must miss the bound (else this test could not tell the two apart)."""
    tol = TOL[precision]
    toks = np.random.default_rng(70 + variant).integers(0, 1000, P + 6).tolist()
    want, want_state = one_shot(gpu, oracle, variant, toks)
    cfg, w, hm = build(gpu, precision, variant)
    errs = stepwise_errors(hm, toks, P, want)
    print(f"{precision} variant {variant} P={P}: carried {max(errs):.2e}")
    assert max(errs) <= tol, errs
    for li in mamba_layers(cfg):
        assert rel_err(hm.get_mamba_state(3, li), want_state[li]) <= tol, li
    _, _, whole = build(gpu, precision, variant)
    whole.forward_with_cache(toks, seq_id=3, pos_offset=0, all_logits=False)
    for li in mamba_layers(cfg):
        kept, kept_whole = hm.get_mamba_conv_state(3, li), whole.get_mamba_conv_state(3, li)
        assert kept.shape == (cfg["mamba_conv_kernel"] - 1, cfg["mamba_expand"] * cfg["hidden"] + 2 * cfg["mamba_n_groups"] * cfg["mamba_state_size"])
        assert kept_whole.any() and rel_err(kept, kept_whole) <= tol, li
    whole.close()
    hm.close()
    _, _, ref = build(gpu, precision, variant, mode="per_call")
    errs_ref = stepwise_errors(ref, toks, P, want)
    print(f"{precision} variant {variant} P={P}: per_call {max(errs_ref):.2e}")
    assert max(errs_ref[1:]) > tol, errs_ref
    ref.close()


def test_split_invariance_of_prefill_and_scoring(gpu, oracle):
    """nvl_forward over 70 tokens as (33, 1, 36) == one call, every row; nvl_score over two calls == one call."""
    tol = TOL["f32"]
    toks = np.random.default_rng(81).integers(0, 1000, 70).tolist()
    cfg, w, hm = build(gpu, "f32")
    one = hm.forward_with_cache(toks, seq_id=1, pos_offset=0)
    parts, p = [], 0
    for n in (33, 1, 36):
        parts.append(hm.forward_with_cache(toks[p:p + n], seq_id=2, pos_offset=p))
        p += n
    e = rel_err(np.concatenate(parts), one)
    print(f"forward split: {e:.2e}")
    assert e <= tol
    hm.seq_reset(5)
    hm.seq_reset(6)
    lp_one, am_one, _, _ = hm.score([5], [toks], [0])
    a = hm.score([6], [toks[:40]], [0], targets=[toks[1:41]])
    b = hm.score([6], [toks[40:]], [40], targets=[toks[41:] + [-1]])
    lp_two = np.concatenate([a[0][0], b[0][0]])
    e = rel_err(lp_two, lp_one[0])
    print(f"score split: {e:.2e}")
    assert e <= tol
    assert np.array_equal(np.concatenate([a[1][0], b[1][0]]), am_one[0])
    hm.close()


def test_batch_and_slots(gpu, oracle):
    """Three sequences of different lengths prefilled together and decoded together (batch order changing) give, per
    sequence, the logits of the same sequence run alone; a new id that lands in a closed sequence's slot and prefills from
    position 0 equals that sequence on a fresh model (the slot's kept rows do not leak)."""
    tol = TOL["f32"]
    r = np.random.default_rng(91)
    lens, steps = (7, 31, 2), 8
    seqs = [r.integers(0, 1000, n + steps).tolist() for n in lens]
    cfg, w, hm = build(gpu, "f32", max_seqs=3)
    _, _, alone = build(gpu, "f32", max_seqs=3)
    want = [[alone.forward_with_cache(s[:n], seq_id=i, pos_offset=0, all_logits=False)[-1].copy()] +
            [alone.forward_with_cache([s[n + j]], seq_id=i, pos_offset=n + j, all_logits=False)[-1].copy() for j in range(steps)]
            for i, (s, n) in enumerate(zip(seqs, lens))]
    ids = [10, 11, 12]
    for i in ids:
        hm.seq_reset(i)
    lg, _ = hm.forward_batch(ids, [s[:n] for s, n in zip(seqs, lens)], [0, 0, 0])
    worst = max(rel_err(lg[i], want[i][0]) for i in range(3))
    for j in range(steps):
        order = [(j + q) % 3 for q in range(3)]
        lg, _ = hm.forward_batch([ids[i] for i in order], [[seqs[i][lens[i] + j]] for i in order], [lens[i] + j for i in order])
        worst = max([worst] + [rel_err(lg[row], want[i][j + 1]) for row, i in enumerate(order)])
    print(f"batched vs alone: {worst:.2e}")
    assert worst <= tol
    hm.seq_close(11)
    hm.seq_reset(20)                                                        # the only free slot is the one 11 left
    again, _ = hm.forward_batch([20], [seqs[0][:lens[0]]], [0])
    assert rel_err(again[0], want[0][0]) <= tol
    nxt, _ = hm.forward_batch([20], [[seqs[0][lens[0]]]], [lens[0]])
    assert rel_err(nxt[0], want[0][1]) <= tol
    alone.close()
    hm.close()


def test_fused_loops_equal_stepwise(gpu, oracle):
    """bf16, option on: nvl_decode_greedy (graph replay) returns the ids of step-by-step nvl_forward calls exactly, and
    nvl_decode_sampled those of nvl_forward + nvl_sample with the same draws."""
    cfg, w, hm = build(gpu, "bf16")
    r = np.random.default_rng(101)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (9, 33, 2)]
    ids, steps = [0, 1, 2], 10

    def prefill():
        for i in ids:
            hm.seq_reset(i)
        return hm.forward_batch(ids, prompts, [0, 0, 0], want_logits=False)[1]
    cur = first = prefill()
    want = []
    for s in range(steps):
        _, cur = hm.forward_batch(ids, [[int(t)] for t in cur], [len(p) + s for p in prompts], want_logits=False)
        want.append(cur.copy())
    assert np.array_equal(prefill(), first)
    hm.reset_stats()
    assert np.array_equal(hm.decode_greedy(ids, first, steps), np.stack(want))
    assert hm.stats()["graph_replays"] > 0
    # sampled
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, repetition_penalty=1.2)
    U = r.random((steps + 1, 3)).astype(np.float32)
    prefill()
    hist = [list(p) for p in prompts]
    first = hm.sample(hist, U[0], **kw)
    for h, t in zip(hist, first):
        h.append(int(t))
    want = []
    for s in range(steps):
        hm.forward_batch(ids, [[h[-1]] for h in hist], [len(h) - 1 for h in hist], want_logits=False)
        tok = hm.sample(hist, U[s + 1], **kw)
        want.append(tok.copy())
        for h, t in zip(hist, tok):
            h.append(int(t))
    prefill()
    hist2 = [list(p) for p in prompts]
    first2 = hm.sample(hist2, U[0], **kw)
    assert np.array_equal(first2, first)
    for h, t in zip(hist2, first2):
        h.append(int(t))
    assert np.array_equal(hm.decode_sampled(ids, first2, steps, hist2, U[1:], **kw), np.stack(want))
    hm.close()


def test_no_extra_launch_per_decode_step(gpu, oracle):
    """Per-site profile over N decode steps of two sequences: the mamba_conv site launches N x n_mamba_layers times with
    the option on (key 39 = 1), as with it off, and the step's total launch count is equal; with key 39 = 0 the tail
    kernel is a launch of its own per layer (so the key does switch the form)."""
    N = 5
    toks = np.random.default_rng(111).integers(0, 1000, 12 + N).tolist()

    def decode_counts(mode, key39):
        with Tuning(gpu, 39, key39):
            cfg, w, hm = build(gpu, "bf16", mode=mode)
            for i in (0, 1):
                hm.seq_reset(i)
            hm.forward_batch([0, 1], [toks[:12], toks[:5]], [0, 0], want_logits=False)
            hm.set_profile(True)
            hm.reset_stats()
            for j in range(N):
                hm.forward_batch([0, 1], [[toks[12 + j]], [toks[5 + j]]], [12 + j, 5 + j], want_logits=False)
            st = hm.stats()
            conv = sum(k["launches"] for k in hm.kernel_stats() if k["site"] == "mamba_conv" and k["phase"] == "decode")
            hm.close()
        return conv, st["gemm_launches"] + st["attn_launches"] + st["other_launches"], len(mamba_layers(cfg))
    off_conv, off_all, nm = decode_counts("per_call", 1)
    on_conv, on_all, _ = decode_counts("carried", 1)
    two_conv, two_all, _ = decode_counts("carried", 0)
    print(f"launches over {N} steps: off conv {off_conv} all {off_all}; on {on_conv} / {on_all}; key 39 = 0 {two_conv} / {two_all}")
    assert off_conv == N * nm and on_conv == N * nm
    assert on_all == off_all
    assert two_conv == 2 * N * nm and two_all == off_all + N * nm


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("variant", [0, 2])                                     # conv kernel 4 and 3
def test_runner_chunked_prefill_and_decode(gpu, oracle, precision, variant):
    """test_runner_chunked_prefill_of_a_long_history_matches_one_forward's setup: the runner's chunk seams were carried
    already, so the option on gives the option off's logits exactly; the runner's following decode steps then match the
    oracle's one-shot Forward."""
    tol = TOL[precision]
    steps = 3
    for ntok in (3 * 64 + 1, 2 * 64 + 37):
        toks = np.random.default_rng(40 + ntok).integers(0, 1000, ntok + steps).tolist()
        want, _ = one_shot(gpu, oracle, variant, toks)
        lg = {}
        for mode in ("per_call", "carried"):
            cfg, w, hm = build(gpu, precision, variant, mode=mode, max_seqs=2, max_batch_tokens=64)
            runner = gpu.HipModelRunner(hm)
            seq = gpu.Sequence(seq_id=5, token_ids=toks[:ntok])
            _, out = runner.run([seq], True, return_logits=True)
            assert hm.stats()["forward_calls"] == -(-ntok // 64)               # it really was chunked
            lg[mode] = out[0].copy()
            if mode == "carried":
                assert rel_err(lg[mode], want[ntok - 1]) <= tol
                for j in range(steps):
                    seq.append_token(toks[ntok + j])
                    _, out = runner.run([seq], False, return_logits=True)
                    assert rel_err(out[0], want[ntok + j]) <= tol, (ntok, j)
            hm.close()
        assert np.array_equal(lg["carried"], lg["per_call"]), ntok


def test_setter_refusals(gpu):
    """After nvl_finalize: NVL_ERR_STATE; an unknown mode and a model without Mamba2 layers: NVL_ERR_INVALID."""
    lib = gpu.lib()
    cfg, w, hm = build(gpu, "f32", mode=None)
    assert lib.nvl_set_mamba_conv_state(hm.h, 1) == -7
    hm.close()
    hm = gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2)       # created, not finalized
    assert lib.nvl_set_mamba_conv_state(hm.h, 2) == -1 and lib.nvl_set_mamba_conv_state(hm.h, -1) == -1
    assert lib.nvl_set_mamba_conv_state(hm.h, 1) == 0 and lib.nvl_set_mamba_conv_state(hm.h, 0) == 0
    hm.close()
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(gpu.synth.tiny_config("llama"), None, mamba_conv_state="carried")
    assert e.value.code == -1
    one = dict(cfg, mamba_conv_kernel=1)                                        # K == 1: accepted, nothing to carry
    hm = gpu.HipTransformerModel(one, gpu.synth.make_weights(one, seed=17, scale=0.05), precision="f32", max_seqs=2,
                                 mamba_conv_state="carried")
    a = hm.forward_with_cache([5, 6, 7], seq_id=1, pos_offset=0)
    b = np.concatenate([hm.forward_with_cache([t], seq_id=2, pos_offset=i) for i, t in enumerate([5, 6, 7])])
    assert rel_err(b, a) <= TOL["f32"]
    hm.close()


def test_default_untouched(gpu, oracle):
    """A per_call model's prefill and decode logits are bit-identical to those of a model constructed without the argument."""
    toks = np.random.default_rng(121).integers(0, 1000, 20).tolist()
    out = {}
    for mode in (None, "per_call"):
        cfg, w, hm = build(gpu, "bf16", mode=mode)
        lg = [hm.forward_with_cache(toks[:14], seq_id=1, pos_offset=0, all_logits=False)[-1].copy()]
        lg += [hm.forward_with_cache([toks[n]], seq_id=1, pos_offset=n, all_logits=False)[-1].copy() for n in range(14, 20)]
        out[mode] = np.stack(lg)
        hm.close()
    assert np.array_equal(out[None], out["per_call"])
