"""Speculative decoding on a hybrid model (nvl_set_mamba_rollback): csrc/mamba.h mamba_verify_kernel
and mamba_commit_kernel through nvl_op_mamba_verify against the float64 statements of tests/mamba_reference.py and
tests/mamba_conv_state_reference.py, then the model's verify calls and loops against the CPU oracle.

Bounds are the project's for these stages: F32_ELEM / F32_SCAN of test_mamba_ops_gpu.py for the op (each stage fed the
device's own output of the stage before), TOL of test_mamba_gpu.py for the model."""
import numpy as np
import pytest

import mamba_conv_state_reference as CR
import mamba_reference as R
from conftest import rel_err
from test_mamba_conv_state_gpu import mamba_layers
from test_mamba_gpu import TOL, VARIANTS
from test_mamba_ops_gpu import F32_ELEM, F32_SCAN, col_err

pytestmark = pytest.mark.gpu

STATE, INVALID = -7, -1
G_A, G_B, G_C = (32, 32, 10, 1), (64, 128, 4, 2), (4, 256, 16, 2)     # (hd, ss, nh, ng): PER 4 / 32 / 4, SG 8 / 4 / 64; conv_dim 384 = 1.5 x 256
OP_CASES = [(G_A, 2, 2, 0), (G_A, 4, 5, 3), (G_A, 8, 8, 3), (G_A, 4, 8, 0),   # (geometry, K, S, chain)
            (G_B, 2, 5, 3), (G_B, 4, 2, 3), (G_B, 8, 8, 0), (G_B, 4, 5, 0),
            (G_C, 2, 8, 3), (G_C, 4, 5, 3), (G_C, 8, 2, 3), (G_C, 8, 5, 0)]


@pytest.mark.parametrize("geom,K,S,chain", OP_CASES)
def test_op_verify_then_commit(gpu, geom, K, S, chain):
    """Three sequences in permuted slots of four at positions (0, 2, 37) — the second shorter than the window at K >= 4 —
    accepting (0, S - 1, S // 2) drafts: a kernel that commits all S rows, or none, or S // 2 for everyone misses one."""
    hd, ss, nh, ng = geom
    g = R.Geom(nh, hd, ss, ng, K)
    rng = np.random.default_rng(1000 * hd + 100 * K + 10 * S + chain)
    lens, pos, slots, n_acc = (S,) * 3, (0, 2, 37), (2, 0, 3), (0, S - 1, S // 2)
    inp = R.make_inputs(g, lens, rng)
    state = rng.standard_normal((4, nh, hd, ss)).astype(np.float32)
    tail = rng.standard_normal((4, K - 1, g.conv_dim)).astype(np.float32)          # junk where no history says otherwise
    ref = CR.Carried(g, inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    for i, p in enumerate(pos):
        if p:
            ref.history[i] = rng.standard_normal((p, g.conv_dim)).astype(np.float32)
            tail[slots[i]] = ref.tail(i)
    out = gpu.ops.mamba_verify(inp["proj"], lens, pos, slots, n_acc, state, nh, hd, ss, ng, K, inp["conv_w"], inp["conv_b"],
                               inp["a_log"], inp["D"], inp["dt_bias"], inp["norm_w"], tail=tail, chain=chain, precision="f32")
    # ---- after the verify launch: nothing committed ----
    assert np.array_equal(out["state"], state) and np.array_equal(out["tail"], tail)
    if chain == 3:
        xbc, delta, _ = ref.call(inp["proj"], range(3), lens, pos)
    else:                                                                           # every row a call of its own
        xbc, delta, _ = R.conv_softplus(g, inp["proj"], (1,) * (3 * S), None, None, inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    e_x, e_d = rel_err(out["xbc"], xbc), col_err(out["delta"], delta)
    y, _ = R.scan(g, out["xbc"], out["delta"], lens, pos, slots, state, inp["a_log"], inp["D"])
    e_y = R.head_errors(g, out["y"], y, lens).max()
    # ---- after the commit: 1 + n_acc rows of each sequence, no more ----
    rows = [i * S + j for i in range(3) for j in range(1 + n_acc[i])]
    _, st = R.scan(g, out["xbc"][rows], out["delta"][rows], [1 + a for a in n_acc], pos, slots, state, inp["a_log"], inp["D"])
    e_s = R.state_head_errors(out["state_commit"], st, slots).max()
    print(f"verify {geom} K={K} S={S} chain={chain}: xbc {e_x:.2e} delta {e_d:.2e} y {e_y:.2e} committed state {e_s:.2e}")
    assert e_x <= F32_ELEM and e_d <= F32_ELEM and e_y <= F32_SCAN and e_s <= F32_SCAN
    assert np.array_equal(out["state_commit"][1], state[1])
    want_tail = tail.copy()
    for i in range(3 if chain == 3 else 0):
        old = tail[slots[i]] if pos[i] else np.zeros((K - 1, g.conv_dim), np.float32)
        raw = inp["proj"][i * S:i * S + 1 + n_acc[i], g.EH:g.EH + g.conv_dim]
        want_tail[slots[i]] = np.concatenate([old, raw])[-(K - 1):]
    assert np.array_equal(out["tail_commit"], want_tail)


def build(gpu, precision, variant, mode, rollback="verify", peaked=0.0):
    cfg = gpu.synth.tiny_config("granite_hybrid", **dict(VARIANTS[variant], tied_embedding=False))      # (tied: greedy repeats its input)
    w = gpu.synth.make_weights(cfg, seed=17, scale=0.05, peaked_head=peaked)
    return cfg, w, gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=4, max_batch_tokens=256, mamba_conv_state=mode,
                                           mamba_rollback=rollback)


def prefill(hm, ids, prompts):
    for i in ids:
        hm.seq_reset(i)
    return hm.forward_batch(ids, prompts, [0] * len(ids), want_logits=False)[1]


@pytest.mark.parametrize("variant", [0, 2])                                     # K = 4 and 3
@pytest.mark.parametrize("mode", ["per_call", "carried"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_model_rollback_against_the_oracle(gpu, oracle, precision, mode, variant):
    """One verify_greedy pass of 1 + 5 rows over prompts of 2 and 23 tokens, drafts = the greedy continuation of twin
    sequences, the first with its middle draft wrong: lengths, every Mamba2 state and the next step's logits are those
    of prompt ++ accepted tokens — carried: the oracle's one-shot Forward; per_call: the oracle fed call by call."""
    cfg, w, hm = build(gpu, precision, variant, mode, peaked=4.0)
    tol, k = TOL[precision], 5
    r = np.random.default_rng(200 + variant)
    prompts = [r.integers(0, cfg["vocab_size"], n).tolist() for n in (2, 23)]
    first = prefill(hm, [0, 1, 2, 3], prompts + prompts)[:2]
    rows = np.concatenate([first[None], hm.decode_greedy([2, 3], first, k)]).T.copy()      # [2][1 + k]
    rows[0, 3] = (rows[0, 3] + 1) % cfg["vocab_size"]
    acc, out = hm.verify_greedy([0, 1], rows, k)
    assert acc.tolist() == [2, 5]
    for i, (p, a) in enumerate(zip(prompts, acc)):
        assert hm.seq_len(i) == len(p) + a + 1
        kept, nxt = rows[i, :a + 1].tolist(), int(out[i, a])
        om = oracle.OracleModel(cfg, w)
        kv = om.new_cache()
        if mode == "carried":
            om.forward_with_cache(p + kept, kv, 0)
            states = [np.array(om.mamba_state(li)) for li in mamba_layers(cfg)]
            want = om.forward_with_cache(p + kept + [nxt], om.new_cache(), 0)[-1]
        else:
            om.forward_with_cache(p, kv, 0)
            for j, t in enumerate(kept):
                om.forward_with_cache([t], kv, len(p) + j)
            states = [np.array(om.mamba_state(li)) for li in mamba_layers(cfg)]
            want = om.forward_with_cache([nxt], kv, len(p) + a + 1)[-1]
        for li, s in zip(mamba_layers(cfg), states):
            assert rel_err(hm.get_mamba_state(i, li), s) <= tol, (i, li)
        got = hm.forward_with_cache([nxt], seq_id=i, pos_offset=len(p) + a + 1, all_logits=False)[-1]
        assert rel_err(got, want) <= tol, i
    hm.close()


SAMPLING = dict(temperature=0.9, top_k=50, top_p=0.95, repetition_penalty=1.2)
LOOP_SEED, N_STEPS = 33, 14      # on the oracle's greedy ids: 3 of 66 drafts accepted per call, 1 of 69 carried (its one-shot greedy)


@pytest.mark.parametrize("mode", ["per_call", "carried"])
def test_loops_equal_plain_decoding_f32(gpu, mode):
    """greedy_lookup returns decode_greedy's ids and sampled_lookup those of step-by-step nvl_forward + nvl_sample with the
    same draws (nvl_decode_sampled's definition; the fused call is bf16 only), on prompts with repeats, drafts both
    accepted and rejected (LOOP_SEED was picked on the CPU oracle's greedy ids), and leave the plain loop's states."""
    cfg, w, hm = build(gpu, "f32", 0, mode, peaked=4.0)
    r = np.random.default_rng(LOOP_SEED)
    pat = r.integers(0, cfg["vocab_size"], 5).tolist()
    prompts = [pat * 3, r.integers(0, cfg["vocab_size"], 4).tolist() + pat[:3] * 2]
    ids, twins, k = [0, 1], [2, 3], 3
    first = prefill(hm, ids + twins, prompts + prompts)[:2]
    want = hm.decode_greedy(twins, first, N_STEPS)
    got, passes = hm.greedy_lookup(ids, first, N_STEPS, k=k, ngram=2, histories=[p + [int(f)] for p, f in zip(prompts, first)])
    assert got.tolist() == want.tolist()
    accepted = proposed = 0                                                  # the fixture: drafts are both accepted and rejected
    for i, p in enumerate(prompts):
        h, done = p + [int(first[i])], 0
        while done < N_STEPS:
            kp = min(k, N_STEPS - done - 1)
            d = gpu.ops.lookup_draft(h, kp, 2)[0] if kp else []
            a = next((j for j in range(kp) if d[j] != want[done + j, i]), kp)
            accepted, proposed, done = accepted + a, proposed + kp, done + a + 1
            h += want[done - a - 1:done, i].tolist()
    assert 0 < accepted < proposed and passes <= N_STEPS, (accepted, proposed, passes)
    for i, t in zip(ids, twins):
        assert hm.seq_len(i) == hm.seq_len(t) == len(prompts[i]) + N_STEPS
        for li in mamba_layers(cfg):
            assert rel_err(hm.get_mamba_state(i, li), hm.get_mamba_state(t, li)) <= TOL["f32"]
    # sampled
    U = r.random((N_STEPS + 1, 2)).astype(np.float32)
    prefill(hm, ids + twins, prompts + prompts)
    hist = [list(p) for p in prompts]
    first = hm.sample(hist + hist, np.concatenate([U[0], U[0]]), **SAMPLING)[:2]
    hist = [h + [int(t)] for h, t in zip(hist, first)]
    start = [list(h) for h in hist]
    want = []
    for s in range(N_STEPS):
        hm.forward_batch(twins, [[h[-1]] for h in hist], [len(h) - 1 for h in hist], want_logits=False)
        want.append(hm.sample(hist, U[s + 1], **SAMPLING).copy())
        hist = [h + [int(t)] for h, t in zip(hist, want[-1])]
    got, _ = hm.sampled_lookup(ids, first, N_STEPS, start, U[1:], k=k, ngram=2, **SAMPLING)
    assert got.tolist() == np.stack(want).tolist()
    assert [hm.seq_len(i) for i in ids] == [len(p) + N_STEPS for p in prompts]
    hm.close()


def test_verify_pass_replays_as_a_graph_bf16(gpu):
    """The third identical pass is a replay and gives the second's ids and states bit for bit."""
    cfg, w, hm = build(gpu, "bf16", 0, "carried", peaked=4.0)
    prompts = [np.random.default_rng(7).integers(0, cfg["vocab_size"], n).tolist() for n in (9, 3)]
    runs = []
    for _ in range(3):
        first = prefill(hm, [0, 1], prompts)
        rows = np.stack([first, first, (first + 1) % cfg["vocab_size"], first]).T.copy()
        replays = hm.stats()["graph_replays"]
        acc, out = hm.verify_greedy([0, 1], rows, 3)
        runs.append((acc, out, [hm.get_mamba_state(i, li) for i in (0, 1) for li in mamba_layers(cfg)],
                     [hm.get_mamba_conv_state(i, li) for i in (0, 1) for li in mamba_layers(cfg)]))
    assert hm.stats()["graph_replays"] > replays
    for a, b in zip(runs[1][:2] + tuple(runs[1][2] + runs[1][3]), runs[2][:2] + tuple(runs[2][2] + runs[2][3])):
        assert np.array_equal(a, b)
    hm.close()


def test_refusals(gpu):
    """With the option on, what cannot be rolled back stays refused and changes nothing; the setter's own rules."""
    lib = gpu.lib()
    cfg, w, hm = build(gpu, "bf16", 0, "per_call")
    prefill(hm, [0], [[5, 6, 7]])
    with pytest.raises(gpu.NvlError) as e:
        hm.seq_truncate(0, 2)
    assert e.value.code == STATE
    with pytest.raises(gpu.NvlError) as e:
        hm.draft_sampled([0], [8], 2, [[5, 6, 7, 8]], [[0.5], [0.5]])
    assert e.value.code == STATE and hm.seq_len(0) == 3
    assert lib.nvl_set_mamba_rollback(hm.h, 1) == STATE                      # after nvl_finalize
    hm.close()
    hm = gpu.HipTransformerModel(cfg, None, precision="f32", max_seqs=2)       # created, not finalized
    assert lib.nvl_set_mamba_rollback(hm.h, 2) == INVALID and lib.nvl_set_mamba_rollback(hm.h, 1) == 0
    hm.close()
    with pytest.raises(gpu.NvlError) as e:
        gpu.HipTransformerModel(gpu.synth.tiny_config("llama"), None, mamba_rollback="verify")
    assert e.value.code == INVALID
