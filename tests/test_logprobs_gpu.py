"""Token log-probabilities on the device (logprob.h): nvl_op_logprobs, nvl_logprobs, nvl_score and
nvl_score_paged.

Reference everywhere: numpy float64 on the very same fp32 logits, x64 = x / s, lp = x64[t] - logsumexp(x64); ids from a
stable sort of the fp32 values (value descending, index ascending) — selection is on input values, so ids are EXACT.

Bound for log-probabilities computed from identical logits (derived in DESIGN.md f-14, not tuned):
    |lp - lp64| <= 1e-5 + 2^-21 * max|x'|
(the roundings of x/s, x' - max and x'_t - lse: <= 2^-23 * 2 max|x'|; expf within 2 ulp + fixed tree sums of depth <= 25:
< 2e-6 relative on the sum; logf of a value <= log V ~ 11.8: < 2e-6; the whole doubled).
Where the LM head may run as another GEMM form than the reference's (chunked scoring against the oracle) the bound is
2 * TOL[precision] * max|oracle logit| with test_model_gpu.py's TOL, since |d lp_t| <= |d x_t| + max_j |d x_j|."""
import numpy as np
import pytest

from block_manager_mirror import BlockManager

pytestmark = pytest.mark.gpu

C = 4096                     # logprob.h LOGPROB_CHUNK: columns per workgroup of the partial pass
TOL = {"f32": 1e-4, "bf16": 1.5e-2}          # tests/test_model_gpu.py
FP8_KV_TOL = 1e-1                            # tests/test_kv_fp8_model_gpu.py FP8_TOL
LENS = (3, 64, 17, 1)                        # the ragged batch: 85 rows


def bound(xs):
    """1e-5 + 2^-21 max|x'| per row of the (scaled) logits"""
    return 1e-5 + 2.0 ** -21 * np.abs(np.asarray(xs, np.float64)).max(axis=1)


def reference(x, targets, top_k, s=0.0):
    """x [rows, V] fp32 -> (lp64 [rows], argmax [rows], ids [rows, top_k], their lp64 [rows, top_k], scaled fp32 rows)"""
    x = np.ascontiguousarray(x, np.float32)
    xs = x / np.float32(s) if s else x                    # what the ids are selected on
    x64 = x.astype(np.float64) / s if s else x.astype(np.float64)
    mx = x64.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(x64 - mx).sum(axis=1, keepdims=True)))[:, 0]
    rows, V = x.shape
    t = np.asarray(targets)
    lp = np.where(t >= 0, x64[np.arange(rows), np.maximum(t, 0)] - lse, 0.0)
    order = np.argsort(-xs, axis=1, kind="stable")        # value descending, index ascending among equals
    k = min(top_k, V)
    ids = np.full((rows, top_k), -1, np.int64)
    tlp = np.full((rows, top_k), -np.inf)
    ids[:, :k] = order[:, :k]
    tlp[:, :k] = np.take_along_axis(x64, order[:, :k], axis=1) - lse[:, None]
    return lp, order[:, 0], ids, tlp, xs


def check(got, x, targets, top_k, s=0.0, tol=None):
    lp, am, ti, tl = got
    want_lp, want_am, want_ids, want_tlp, xs = reference(x, targets, top_k, s)
    b = bound(xs) if tol is None else tol
    err = np.abs(lp.astype(np.float64) - want_lp)
    print(f"rows {x.shape[0]} V {x.shape[1]} top_k {top_k}: max |lp err| {err.max():.3e}, bound min {np.min(b):.3e}")
    assert (err <= b).all(), (err.max(), np.min(b))
    t = np.asarray(targets)
    assert (lp[t < 0] == 0).all() and not np.signbit(lp[t < 0]).any()          # "no target" is exactly +0.0
    assert np.array_equal(am, want_am)
    if top_k:
        assert np.array_equal(ti, want_ids)
        assert np.array_equal(ti[:, 0], am)
        fin = want_ids >= 0
        assert (np.abs(tl.astype(np.float64) - want_tlp)[fin] <= np.broadcast_to(np.reshape(b, (-1, 1)), fin.shape)[fin]).all()
        assert np.isneginf(tl[~fin]).all()
    else:
        assert ti is None and tl is None


def padded(x):
    """the [:, :V] view of a [rows, ld] buffer whose pad columns hold 3e38: a kernel that reads the pad fails"""
    rows, V = x.shape
    ld = (V + 63) // 64 * 64 + 64
    buf = np.full((rows, ld), 3e38, np.float32)
    buf[:, :V] = x
    return buf[:, :V], ld


def make_rows(V, n, seed):
    """n base rows of N(0, 4) logits and every special case of the issue stacked under them"""
    r = np.random.default_rng(seed)
    base = (2.0 * r.standard_normal((n, V))).astype(np.float32)
    tb = r.integers(0, V, n)
    rows, tg = [base, base + np.float32(90), base - np.float32(90)], [tb, tb, tb]
    d = int(r.integers(0, V))
    dom = base[:2].copy() if n >= 2 else np.repeat(base[:1], 2, axis=0)
    dom[:, d] = dom.max() + np.float32(100)                                   # one logit 100 above the rest
    rows.append(dom); tg.append(np.array([d, (d + 1) % V]))                   # dominant and non-dominant target
    edge = np.repeat(base[:1], 3, axis=0)
    rows.append(edge); tg.append(np.array([0, V - 1, -1]))                    # first / last column, no target
    ties = np.round(np.repeat(base[:1], 2, axis=0))                           # many equal values: top-k order under ties
    if V >= 2:
        i, j = sorted(r.choice(V, 2, replace=False).tolist())
        ties[1, i] = ties[1, j] = ties[1].max() + np.float32(1)               # duplicated maximum at i < j -> argmax i
    rows.append(ties); tg.append(np.array([V - 1, 0]))
    return np.concatenate(rows).astype(np.float32), np.concatenate(tg).astype(np.int32)


# ---- op level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n", [(1, 5), (63, 5), (64, 5), (65, 5), (1000, 5), (C - 1, 5), (C, 5), (C + 1, 5), (50257, 5),
                                 (128256, 3), (1000, 1), (1000, 65), (C + 1, 300)])
def test_op_logprobs(gpu, V, n):
    x, tg = make_rows(V, n, seed=V + n)
    xv, ld = padded(x)
    for top_k in (0, 1, 8):
        got = gpu.ops.logprobs(xv, tg, top_k=top_k, ld=ld)
        check(got, x, tg, top_k)
    again = gpu.ops.logprobs(xv, tg, top_k=8, ld=ld)                          # fixed summation order: the same bits
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    if V in (63, C + 1):                            # dense rows (ld = V, no 16-byte alignment): the scalar loads, same tree
        dense = gpu.ops.logprobs(x, tg, top_k=8)
        for a, b in zip(got, dense):
            assert a.tobytes() == b.tobytes()


def test_op_shifted_logits_agree(gpu):
    """+-90 shifts leave log-probabilities unchanged up to the bound (no plain exp(x))"""
    x, tg = make_rows(1000, 5, seed=3)
    lp = gpu.ops.logprobs(x, tg)[0]
    assert np.isfinite(lp).all()
    assert np.abs(lp[:5].astype(np.float64) - lp[5:10]).max() <= 2 * (1e-5 + 2.0 ** -21 * 100)


def test_op_logits_scaling(gpu):
    """s = 6 (Granite): the argmax is ops.argmax of the scaled row, log-probabilities are those of x / s"""
    for V in (1027, C + 1):
        x, tg = make_rows(V, 5, seed=11)
        x = x * np.float32(6)
        xv, ld = padded(x)
        got = gpu.ops.logprobs(xv, tg, top_k=8, logits_scaling=6.0, ld=ld)
        check(got, x, tg, 8, s=6.0)
        assert np.array_equal(got[1], gpu.ops.argmax(x / np.float32(6)))


def test_op_refusals(gpu):
    x = np.zeros((2, 10), np.float32)
    for kw, tg in ((dict(top_k=9), [0, 1]), (dict(top_k=-1), [0, 1]), (dict(), [0, 10]), (dict(), [-2, 0])):
        with pytest.raises(gpu.NvlError) as e:
            gpu.ops.logprobs(x, tg, **kw)
        assert e.value.code == -1


# ---- model level ------------------------------------------------------------------------------------------------------
FAMILIES = ["llama", "gpt2", "granite_moe", "granite_hybrid"]


def build(gpu, family, precision, **kw):
    cfg = gpu.synth.tiny_config(family)
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
    kw.setdefault("max_batch_tokens", 256)
    return cfg, w, gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=4, **kw)


def batch(cfg, seed=5, lens=LENS):
    r = np.random.default_rng(seed)
    return [r.integers(0, cfg["vocab_size"], n).tolist() for n in lens]


def targets_of(cfg, prompts, seed=6):
    """random targets (not the next tokens: every row gets one), one row without"""
    r = np.random.default_rng(seed)
    tg = [r.integers(0, cfg["vocab_size"], len(p)).tolist() for p in prompts]
    tg[1][5] = -1
    return tg


def open_seqs(hm, n):
    for i in range(n):
        hm.seq_reset(i)


class tuning:
    def __init__(self, gpu, key, value):
        self.lib, self.key, self.value = gpu.lib(), key, value

    def __enter__(self):
        self.old = self.lib.nvl_set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        self.lib.nvl_set_tuning(self.key, self.old)


_ORACLE = {}


def oracle_logits(oracle, gpu, family):
    """the oracle's logits of the ragged batch, computed once per family and shared (read-only)"""
    if family not in _ORACLE:
        cfg = gpu.synth.tiny_config(family)
        om = oracle.OracleModel(cfg, gpu.synth.make_weights(cfg, seed=7, scale=0.05))
        lg = np.concatenate([om.forward_with_cache(p, om.new_cache(), 0) for p in batch(cfg)])
        lg.setflags(write=False)
        _ORACLE[family] = lg
    return _ORACLE[family]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_score_unchunked_equals_all_logits(gpu, family, precision):
    """R >= the batch's rows: the LM head launch is the one an all-logits forward makes, so the derived bound applies"""
    cfg, w, hm = build(gpu, family, precision)
    _, _, ref = build(gpu, family, precision)
    prompts = batch(cfg)
    tg = targets_of(cfg, prompts)
    open_seqs(hm, 4); open_seqs(ref, 4)
    logits, _ = ref.forward_batch([0, 1, 2, 3], prompts, [0] * 4, all_logits=True)
    lp, am, ti, tl = hm.score([0, 1, 2, 3], prompts, [0] * 4, targets=tg, top_k=8)
    assert [len(a) for a in lp] == list(LENS) and ti[1].shape == (64, 8)
    check((np.concatenate(lp), np.concatenate(am), np.concatenate(ti), np.concatenate(tl)), logits, np.concatenate(tg), 8)
    # default targets: the next token of each list, none for its last row
    open_seqs(hm, 4)
    lp2, am2, ti2, tl2 = hm.score([0, 1, 2, 3], prompts, [0] * 4)
    assert ti2 is None and tl2 is None
    nxt = np.concatenate([p[1:] + [-1] for p in prompts])
    check((np.concatenate(lp2), np.concatenate(am2), None, None), logits, nxt, 0)
    hm.close(); ref.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("R", [16, 64])
def test_score_chunked_against_oracle(gpu, oracle, family, precision, R):
    want = oracle_logits(oracle, gpu, family)
    cfg, w, hm = build(gpu, family, precision)
    prompts = batch(cfg)
    tg = targets_of(cfg, prompts)
    open_seqs(hm, 4)
    hm.set_profile(True)
    hm.reset_stats()
    with tuning(gpu, 37, R):
        lp, am, _, _ = hm.score([0, 1, 2, 3], prompts, [0] * 4, targets=tg)
    sites = {k["site"]: k for k in hm.kernel_stats()}
    rows = sum(LENS)
    assert sites["logprobs"]["launches"] == -(-rows // R)
    assert sites["logprobs"]["bytes"] == rows * cfg["vocab_size"] * 4
    want_lp = reference(want, np.concatenate(tg), 0)[0]
    err = np.abs(np.concatenate(lp).astype(np.float64) - want_lp).max()
    b = 2 * TOL[precision] * np.abs(want).max()
    print(f"{family} {precision} R={R}: max |lp - oracle lp| {err:.3e} (bound {b:.3e})")
    assert err <= b
    hm.close()


@pytest.mark.parametrize("family", ["llama", "granite_hybrid"])
def test_score_appends_kv_like_a_prefill(gpu, family):
    """after score() the cache holds the tokens; greedy decode then gives the ids and bit-identical logits of the same
    model after a plain prefill"""
    cfg, w, hm = build(gpu, family, "bf16")
    _, _, ref = build(gpu, family, "bf16")
    prompts = batch(cfg)
    open_seqs(hm, 4); open_seqs(ref, 4)
    lp, am, _, _ = hm.score([0, 1, 2, 3], prompts, [0] * 4)
    assert [hm.seq_len(i) for i in range(4)] == list(LENS)
    _, am_ref = ref.forward_batch([0, 1, 2, 3], prompts, [0] * 4)
    tok = [int(a[-1]) for a in am]                     # the next token comes from argmax_out of the last row
    assert tok == am_ref.tolist()
    pos = list(LENS)
    for step in range(4):
        lg_a, am_a = hm.forward_batch([0, 1, 2, 3], [[t] for t in tok], pos)
        lg_b, am_b = ref.forward_batch([0, 1, 2, 3], [[t] for t in tok], pos)
        assert np.array_equal(am_a, am_b) and lg_a.tobytes() == lg_b.tobytes(), step
        tok = am_a.tolist()
        pos = [p + 1 for p in pos]
    hm.close(); ref.close()


def test_score_in_two_calls(gpu, oracle):
    """a 50-token sequence scored as 30 + 20 (pos_offsets) equals one call within the chunked bound"""
    cfg, w, hm = build(gpu, "llama", "bf16")
    toks = np.random.default_rng(4).integers(0, cfg["vocab_size"], 50).tolist()
    tg = np.random.default_rng(8).integers(0, cfg["vocab_size"], 50).tolist()
    om = oracle.OracleModel(cfg, w)
    b = 2 * TOL["bf16"] * np.abs(om.forward_with_cache(toks, om.new_cache(), 0)).max()
    hm.seq_reset(0); hm.seq_reset(1)
    one = hm.score([0], [toks], [0], targets=[tg], top_k=1)
    p1 = hm.score([1], [toks[:30]], [0], targets=[tg[:30]], top_k=1)
    p2 = hm.score([1], [toks[30:]], [30], targets=[tg[30:]], top_k=1)
    assert hm.seq_len(1) == 50
    two = np.concatenate([p1[0][0], p2[0][0]])
    err = np.abs(two.astype(np.float64) - one[0][0]).max()
    print(f"two-call vs one-call: max |d lp| {err:.3e} (bound {b:.3e})")
    assert err <= b
    hm.close()


@pytest.mark.parametrize("family", ["llama", "granite_moe"])
def test_logprobs_after_replayed_decode_step(gpu, family):
    """the third decode step of a batch is a replayed graph; logprobs() reads final (scaled) logits of that call"""
    cfg, w, hm = build(gpu, family, "bf16")
    prompts = batch(cfg)
    open_seqs(hm, 4)
    _, am = hm.forward_batch([0, 1, 2, 3], prompts, [0] * 4, want_logits=False)
    pos = list(LENS)
    for step in range(3):
        logits, am = hm.forward_batch([0, 1, 2, 3], [[int(t)] for t in am], pos)
        pos = [p + 1 for p in pos]
    assert hm.stats()["graph_replays"] >= 1
    tg = np.array([int(am[0]), 0, cfg["vocab_size"] - 1, -1], np.int32)
    check(hm.logprobs(tg, top_k=8), logits, tg, 8)
    assert np.array_equal(hm.logprobs(tg)[1], am)
    with pytest.raises(gpu.NvlError) as e:                # 5 rows asked, 4 left by the forward
        hm.logprobs([0, 0, 0, 0, 0])
    assert e.value.code == -1
    hm.close()


def test_logprobs_after_sampling_is_not_scaled_twice(gpu):
    """granite_moe (logits_scaling 6): the value is the same before and after sample(), and after a runner_run_sampled
    pass it is the log-softmax of that pass's logits"""
    cfg, w, hm = build(gpu, "granite_moe", "bf16")
    _, _, ref = build(gpu, "granite_moe", "bf16")
    prompts = batch(cfg)
    open_seqs(hm, 4); open_seqs(ref, 4)
    logits, am = hm.forward_batch([0, 1, 2, 3], prompts, [0] * 4)
    tg = np.array([5, 1026, 0, int(am[3])], np.int32)
    before = hm.logprobs(tg, top_k=8)
    check(before, logits, tg, 8)
    hm.sample(prompts, np.array([0.1, 0.5, 0.9, 0.3], np.float32))
    after = hm.logprobs(tg, top_k=8)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    runner = gpu.HipModelRunner(hm)
    seqs = [gpu.Sequence(seq_id=10 + i, token_ids=list(p)) for i, p in enumerate(prompts[:3])]
    runner.run_sampled(seqs, is_prefill=True, uniforms=[0.2, 0.4, 0.6])
    lg_ref, _ = ref.forward_batch([0, 1, 2], prompts[:3], [0] * 3)
    check(hm.logprobs(tg[:3], top_k=1), lg_ref, tg[:3], 1)
    hm.close(); ref.close()


def test_no_logits_rows_after_score(gpu):
    cfg, w, hm = build(gpu, "llama", "bf16")
    prompts = batch(cfg)
    open_seqs(hm, 4)
    hm.score([0, 1, 2, 3], prompts, [0] * 4)
    with pytest.raises(gpu.NvlError) as e:
        hm.sample(prompts, np.full(4, 0.5, np.float32))
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:
        hm.logprobs([0])
    assert e.value.code == -1
    with pytest.raises(gpu.NvlError) as e:                # a target outside [-1, V) is refused before the pass
        hm.score([0], [[1, 2]], [3], targets=[[0, cfg["vocab_size"]]])
    assert e.value.code == -1
    assert hm.seq_len(0) == 3
    _, am = hm.forward_batch([0], [[7]], [3])             # and a forward makes them available again
    assert hm.logprobs([1])[1][0] == am[0]
    hm.close()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_score_paged_equals_slab(gpu, precision):
    """score_paged over the block manager's tables after a prefix-cache hit (pos_offsets > 0) == slab score, bit for bit
    (the logits of the two modes are identical)"""
    BS = 64
    cfg = gpu.synth.tiny_config("llama")
    w = gpu.synth.make_weights(cfg, seed=7, scale=0.05)
    slab = gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=4, max_batch_tokens=512)
    paged = gpu.HipTransformerModel(cfg, w, precision=precision, max_seqs=4, max_batch_tokens=512, kv_num_blocks=24, kv_block_size=BS)
    r = np.random.default_rng(22)
    common = r.integers(0, cfg["vocab_size"], 128).tolist()
    a = gpu.Sequence(seq_id=0, token_ids=common + r.integers(0, cfg["vocab_size"], 40).tolist(), block_size=BS)
    b = gpu.Sequence(seq_id=1, token_ids=common + r.integers(0, cfg["vocab_size"], 75).tolist(), block_size=BS)
    bm = BlockManager(24, BS)
    bm.allocate(a)
    paged.forward_paged([a.token_ids], [0], [a.block_table], want_logits=False)
    bm.allocate(b)
    assert b.num_cached_tokens == 128
    with tuning(gpu, 37, 64):                              # 168 + 75 rows in chunks of 64
        got = paged.score_paged([a.token_ids, b.token_ids[128:]], [0, 128], [a.block_table, b.block_table], top_k=8)
        slab.seq_reset(0); slab.seq_reset(1)
        slab.forward_batch([1], [b.token_ids[:128]], [0], want_logits=False)
        want = slab.score([0, 1], [a.token_ids, b.token_ids[128:]], [0, 128], top_k=8)
    for g, h in zip(got, want):
        for x, y in zip(g, h):
            assert x.tobytes() == y.tobytes()
    assert np.isfinite(np.concatenate(got[0])).all()
    slab.close(); paged.close()


@pytest.mark.parametrize("mode,kw,tol", [
    ("kv_fp8", dict(kv_cache_dtype="fp8_e4m3"), FP8_KV_TOL),
    ("fp8_weights", dict(weight_dtype="fp8_e4m3"), TOL["bf16"]),
    ("mxfp4_weights_head", dict(mx_weight_dtype="fp4_e2m1", mx_head_dtype="fp4_e2m1"), TOL["bf16"])])
def test_score_in_quantized_modes(gpu, mode, kw, tol):
    """score with R = 64 against the same mode's own all-logits float64 log-softmax: both sides sit within the mode's
    logits tolerance of a common exact value, hence 4 * tol * max|logit|"""
    cfg, w, hm = build(gpu, "llama", "bf16", **kw)
    _, _, ref = build(gpu, "llama", "bf16", **kw)
    prompts = batch(cfg)
    tg = targets_of(cfg, prompts)
    open_seqs(hm, 4); open_seqs(ref, 4)
    logits, _ = ref.forward_batch([0, 1, 2, 3], prompts, [0] * 4, all_logits=True)
    with tuning(gpu, 37, 64):
        lp, am, _, _ = hm.score([0, 1, 2, 3], prompts, [0] * 4, targets=tg)
    want = reference(logits, np.concatenate(tg), 0)[0]
    err = np.abs(np.concatenate(lp).astype(np.float64) - want).max()
    b = 4 * tol * np.abs(logits).max()
    print(f"{mode}: max |lp - lp(all logits)| {err:.3e} (bound {b:.3e})")
    assert err <= b
    hm.close(); ref.close()
