"""One defect per call, every entry point that takes a batch: the error code, and that a refused call moved no cached length.

Tiny llama, two sequences per call, k = 2, n_steps = 4.  Slab models have max_seq_len 64: sequences 0 and 1 hold 12 tokens and sequence 2
holds 62 (two positions left: every call here needs at least three); the draft model holds the same.  The paged model has
max_seq_len 256 in blocks of 64.  Defects with more than one
cause in one call are not tested here: which of them is reported is the planner's business (csrc/nvllm.hip, "ORDER OF THE
CHECKS"), not the contract's."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, POSITION, UNKNOWN_SEQ = -1, -2, -3
T, K, N_STEPS, P, P_LATE = 64, 2, 4, 12, 62
T_PAGED = 256                                    # the paged model: blocks of 64 positions (the smallest), four per sequence
T0 = 5                                           # a valid token id
SAMPLING_PARAMS = None                           # the library binding's nvl_sampling_params (set with the paged model)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


@pytest.fixture(scope="module")
def slab(gpu):
    cfg = gpu.synth.tiny_config("llama", max_seq_len=T)
    models = []
    for seed in (7, 8):                           # target, draft
        m = gpu.HipTransformerModel(cfg, gpu.synth.make_weights(cfg, seed=seed, scale=0.05), precision="bf16", max_seqs=4,
                                    max_batch_tokens=64)
        for sid, n in ((0, P), (1, P), (2, P_LATE)):
            m.seq_reset(sid)
            m.forward_batch([sid], [[T0] * n], [0], want_logits=False)
        models.append(m)
    yield cfg, models[0], models[1]
    for m in models:
        m.close()


@pytest.fixture(scope="module")
def paged(gpu):
    global SAMPLING_PARAMS
    SAMPLING_PARAMS = gpu._lib.sampling_params
    cfg = gpu.synth.tiny_config("llama", max_seq_len=T_PAGED)
    m = gpu.HipTransformerModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05), precision="bf16", max_seqs=4,
                                max_batch_tokens=64, kv_num_blocks=8, kv_block_size=64)      # 4 blocks per sequence
    m.forward_paged([[T0] * P] * 2, [0, 0], [[0], [1]], want_logits=False)                   # what the served calls attend to
    yield cfg, m
    m.close()


def lengths(*models):
    return [m.seq_len(s) for m in models for s in (0, 1, 2)]


def code_of(fn):
    with pytest.raises(Exception) as e:
        fn()
    return e.value.code


# ---- slab ----------------------------------------------------------------------------------------------------------------
def slab_call(name, tgt, drf, ids, first, pos=None):
    """entry point `name` on sequences `ids` whose first (or only) token row starts with first[i]"""
    n = len(ids)
    cached = {0: P, 1: P, 2: P_LATE}
    pos = [cached.get(i, 0) for i in ids] if pos is None else pos
    rows = [[int(t), T0, T0] for t in first]                            # 1 + K rows per sequence
    hists = [[T0] * 3 + [int(t)] for t in first]
    u = lambda *shape: np.full(shape, 0.5, np.float32)
    if name == "nvl_forward":
        return tgt.forward_batch(ids, rows, pos, want_logits=False)
    if name == "nvl_score":
        return tgt.score(ids, rows, pos)
    if name == "nvl_decode_greedy":
        return tgt.decode_greedy(ids, first, N_STEPS)
    if name == "nvl_verify_greedy":
        return tgt.verify_greedy(ids, rows, K)
    if name == "nvl_verify_sampled":
        return tgt.verify_sampled(ids, rows, K, hists, u(n, 1 + K))
    if name == "nvl_decode_greedy_lookup":
        return tgt.greedy_lookup(ids, first, N_STEPS, k=K)
    if name == "nvl_decode_sampled_lookup":
        return tgt.sampled_lookup(ids, first, N_STEPS, hists, u(N_STEPS, n), k=K)
    if name == "nvl_decode_sampled":
        return tgt.decode_sampled(ids, first, N_STEPS, hists, u(N_STEPS, n))
    if name == "nvl_draft_sampled":
        return tgt.draft_sampled(ids, first, K, hists, u(K, n))
    if name == "nvl_decode_speculative":
        return tgt.decode_speculative(drf, ids, first, N_STEPS, hists, u(N_STEPS * n, 2 * K + 1), k=K)
    raise KeyError(name)


SLAB_ENTRIES = ["nvl_forward", "nvl_score", "nvl_decode_greedy", "nvl_verify_greedy", "nvl_verify_sampled", "nvl_decode_greedy_lookup",
                "nvl_decode_sampled_lookup", "nvl_decode_sampled", "nvl_draft_sampled", "nvl_decode_speculative"]
SLAB_DEFECTS = {                                  # -> (ids, first tokens, code); "V" stands for vocab_size
    "unknown sequence": ([0, 9], [T0, T0], UNKNOWN_SEQ),
    "duplicate sequence": ([1, 1], [T0, T0], INVALID),
    "token id < 0": ([0, 1], [T0, -1], INVALID),
    "token id >= V": ([0, 1], [T0, "V"], INVALID),
    "position beyond max_seq_len": ([0, 2], [T0, T0], POSITION),
}


# (nvl_draft_sampled's K = 2 steps fit behind 62 cached tokens: its position defect is nvl_decode_sampled's, the same function)
SLAB_CASES = [(e, d) for e in SLAB_ENTRIES for d in SLAB_DEFECTS if (e, d) != ("nvl_draft_sampled", "position beyond max_seq_len")]


@pytest.mark.parametrize("entry,defect", SLAB_CASES)
def test_slab_refusals(slab, entry, defect):
    cfg, tgt, drf = slab
    ids, first, code = SLAB_DEFECTS[defect]
    first = [cfg["vocab_size"] if t == "V" else t for t in first]
    assert code_of(lambda: slab_call(entry, tgt, drf, ids, first)) == code
    assert lengths(tgt, drf) == [P, P, P_LATE] * 2


@pytest.mark.parametrize("entry", ["nvl_forward", "nvl_score"])
@pytest.mark.parametrize("off", [-1, 1])
def test_forward_refuses_a_pos_offset_that_is_not_the_cached_length(slab, entry, off):
    _, tgt, drf = slab
    assert code_of(lambda: slab_call(entry, tgt, drf, [0, 1], [T0, T0], pos=[P, P + off])) == INVALID
    assert lengths(tgt, drf) == [P, P, P_LATE] * 2


@pytest.mark.parametrize("defect", ["unknown on the draft only", "cached lengths differ"])
def test_decode_speculative_refuses_a_draft_out_of_step(slab, defect):
    _, tgt, drf = slab
    if defect == "cached lengths differ":
        drf.seq_truncate(1, P - 1)
        want = INVALID
    else:
        drf.seq_close(1)
        want = UNKNOWN_SEQ
    try:
        assert code_of(lambda: slab_call("nvl_decode_speculative", tgt, drf, [0, 1], [T0, T0])) == want
        assert lengths(tgt) == [P, P, P_LATE] and drf.seq_len(0) == P and drf.seq_len(2) == P_LATE
    finally:                                      # the module's draft goes back to where the other cases expect it
        drf.seq_reset(1)
        drf.forward_batch([1], [[T0] * P], [0], want_logits=False)


@pytest.mark.parametrize("defect", ["token id >= V", "position beyond max_seq_len"])
def test_verify_speculative_refusals(slab, defect):
    """behind valid proposals of the draft (without them the call is refused before it looks at the batch)"""
    cfg, tgt, drf = slab
    ids = [0, 2] if defect.startswith("position") else [0, 1]          # 62 + K draft steps fit, 62 + 1 + K rows do not
    hists = [[T0] * 4] * 2
    d = drf.draft_sampled(ids, [T0, T0], K, hists, np.full((K, 2), 0.5, np.float32))
    rows = np.concatenate([[[T0], [T0]], d.T], axis=1).astype(np.int32)
    want = POSITION
    if defect.startswith("token"):
        rows[1, 0], want = cfg["vocab_size"], INVALID
    try:
        assert code_of(lambda: tgt.verify_speculative(drf, ids, rows, K, hists, np.full((2, K), 0.5, np.float32),
                                                      np.full(2, 0.5, np.float32))) == want
        assert lengths(tgt) == [P, P, P_LATE]
    finally:
        for s in ids:
            drf.seq_truncate(s, tgt.seq_len(s))
    assert lengths(drf) == [P, P, P_LATE]


# ---- paged -----------------------------------------------------------------------------------------------------------------
def paged_call(name, m, first, pos, tables, off=None):
    """the raw entry point (the wrappers of model.py build table_offsets themselves, and two defects live there)"""
    n = len(first)
    tbl = i32(np.concatenate([np.asarray(t, np.int64) for t in tables]))
    off = i32(np.concatenate([[0], np.cumsum([len(t) for t in tables])]) if off is None else off)
    pos, first = i32(pos), i32(first)
    rows = i32([[int(t), T0, T0] for t in first])
    lens, acc, out = i32([1 + K] * n), np.empty(n, np.int32), np.empty((max(N_STEPS, n), 1 + K), np.int32)
    h, lib = m.h, m.lib
    if name == "nvl_forward_paged":
        rc = lib.nvl_forward_paged(h, n, _ptr(rows), _ptr(lens), _ptr(pos), _ptr(tbl), _ptr(off), 0, None, _ptr(acc))
    elif name == "nvl_score_paged":
        targets, lp = i32([-1] * rows.size), np.empty(rows.size, np.float32)
        rc = lib.nvl_score_paged(h, n, _ptr(rows), _ptr(lens), _ptr(pos), _ptr(tbl), _ptr(off), _ptr(targets), 0, _ptr(lp), None,
                                 None, None)
    elif name == "nvl_decode_greedy_paged":
        rc = lib.nvl_decode_greedy_paged(h, n, _ptr(first), _ptr(pos), N_STEPS, _ptr(tbl), _ptr(off), _ptr(out))
    elif name == "nvl_verify_greedy_paged":
        rc = lib.nvl_verify_greedy_paged(h, n, _ptr(rows), K, _ptr(pos), _ptr(tbl), _ptr(off), _ptr(acc), _ptr(out))
    elif name == "nvl_verify_sampled_paged":
        hist = [i32([T0] * 3 + [int(t)]) for t in first]
        ptrs = (C.c_void_p * n)(*[a.ctypes.data_as(C.c_void_p).value for a in hist])
        sp = SAMPLING_PARAMS(1.0, 1.0, 0, 1.2)
        u = np.full((n, 1 + K), 0.5, np.float32)
        rc = lib.nvl_verify_sampled_paged(h, n, _ptr(rows), K, _ptr(pos), _ptr(tbl), _ptr(off), C.byref(sp), ptrs, _ptr(i32([4] * n)),
                                          _ptr(u), _ptr(acc), _ptr(out))
    else:
        raise KeyError(name)
    return rc


PAGED_ENTRIES = ["nvl_forward_paged", "nvl_score_paged", "nvl_decode_greedy_paged", "nvl_verify_greedy_paged", "nvl_verify_sampled_paged"]
FULL = [1, 2, 3, 4]
PAGED_DEFECTS = {                                 # -> (first tokens, positions, block tables, table_offsets or None, code)
    "negative position": ([T0, T0], [P, -1], [[0], [1]], None, INVALID),
    "negative table offset": ([T0, T0], [P, P], [[0], [1]], [-1, 0, 1], INVALID),
    "decreasing table offsets": ([T0, T0], [P, P], [[0], [1]], [0, 1, 0], INVALID),
    "table too short": ([T0, T0], [P, 100], [[0], [1]], None, INVALID),
    "table too long": ([T0, T0], [P, P], [[0], FULL + [5]], None, INVALID),
    "block id < 0": ([T0, T0], [P, P], [[0], [-1]], None, INVALID),
    "block id >= num_blocks": ([T0, T0], [P, P], [[0], [8]], None, INVALID),
    "token id < 0": ([T0, -1], [P, P], [[0], [1]], None, INVALID),
    "token id >= V": ([T0, "V"], [P, P], [[0], [1]], None, INVALID),
    "position beyond max_seq_len": ([T0, T0], [P, T_PAGED - 2], [[0], FULL], None, POSITION),
}


@pytest.mark.parametrize("defect", PAGED_DEFECTS)
@pytest.mark.parametrize("entry", PAGED_ENTRIES)
def test_paged_refusals(paged, entry, defect):
    cfg, m = paged
    first, pos, tables, off, code = PAGED_DEFECTS[defect]
    first = [cfg["vocab_size"] if t == "V" else t for t in first]
    assert paged_call(entry, m, first, pos, tables, off) == code
    # the defect was the only one: the same call without it is served
    assert paged_call(entry, m, [T0, T0], [P, P], [[0], [1]]) == 0
