"""Speculative decoding with a draft model, host side: a float64 / fp32 restatement of the rejection rule
(`spec_reject_ref`, shared with tests/test_spec_draft_gpu.py) whose emitted law is checked WITHOUT randomness, and the new
entry points: declared, exported, bound, and refusing NULL models and draft == target without touching a device.

The law.  With x ~ q, accept iff ua * q(x) < p(x), else emit y ~ max(p - q, 0) / R:
    P(emit y) = sum_d q(d) [alpha_d 1[y = d] + (1 - alpha_d) r(y) / R],  alpha_d = min(1, p(d) / q(d)),
              = min(p, q)(y) + (sum_d max(q - p, 0)(d)) r(y) / R = min(p, q)(y) + max(p - q, 0)(y) = p(y),
because sum max(q - p, 0) = sum max(p - q, 0) = R.  On midpoint grids of Na accept draws and Nf final draws the fraction of
accepted draws differs from alpha_d by at most one cell (1 / Na), and the fraction of final draws an id owns differs from
its share of the CDF by at most one cell (1 / Nf); both are weighted by q(d), which sums to 1.  So every emitted frequency
lies within 1 / Na + 1 / Nf of p."""
import ctypes as C
import re

import numpy as np
import pytest

NEW = ("nvl_draft_sampled", "nvl_verify_speculative", "nvl_decode_speculative", "nvl_op_spec_reject")


def spec_reject_ref(p, q, tokens, ua, uf):
    """The rule of nvl_verify_speculative restated: p [n, 1+k, V], q [n, k, V] float32, tokens [n, 1+k] (column j + 1 = the
    draft's id of step j), ua [n, k], uf [n].  The accept compare is the fp32 one; the sums run in float64 and the threshold
    uf * sum is the fp32 product the device forms.  -> (n_accepted [n], out_tokens [n, 1+k], accept_prob [n, k, 2])."""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    tokens = np.asarray(tokens, np.int64)
    n, k, V = q.shape
    ua, uf = np.asarray(ua, np.float32).reshape(n, k), np.asarray(uf, np.float32).reshape(n)
    rows = np.arange(n)
    d = tokens[:, 1:]
    pd = np.stack([p[rows, j, d[:, j]] for j in range(k)], axis=1)
    qd = np.stack([q[rows, j, d[:, j]] for j in range(k)], axis=1)
    ok = (ua * qd).astype(np.float32) < pd                                  # fp32 product, fp32 compare
    a = np.cumprod(ok, axis=1).sum(axis=1).astype(np.int64)
    pa = p[rows, a]
    qa = q[rows, np.minimum(a, k - 1)]
    r = np.where((a < k)[:, None], np.maximum(pa - qa, np.float32(0)), pa)
    R = r.astype(np.float64).sum(axis=1)
    r = np.where(((a < k) & (R == 0))[:, None], pa, r)                       # only rounding can leave the residual empty
    c = np.cumsum(r.astype(np.float64), axis=1)
    thr = (uf * c[:, -1].astype(np.float32)).astype(np.float32).astype(np.float64)
    hit = c >= thr[:, None]
    e = np.where(hit.any(axis=1), hit.argmax(axis=1), V - 1)
    out = np.full((n, 1 + k), -1, np.int32)
    for j in range(k):
        out[:, j] = np.where(j < a, d[:, j], out[:, j])
    out[rows, a] = e
    return a.astype(np.int32), out, np.stack([pd, qd], axis=2)


def dyadic(r, V, support, denom):
    """a distribution on V ids whose entries are multiples of 1 / denom, zero outside `support` (every id of it > 0)"""
    support = np.asarray(support)
    w = np.ones(len(support), np.int64) + r.multinomial(denom - len(support), np.full(len(support), 1.0 / len(support)))
    x = np.zeros(V, np.float32)
    x[support] = w / np.float32(denom)
    assert x.astype(np.float64).sum() == 1.0
    return x


def emitted_law(p, q, Na, Nf):
    """frequency of every FIRST emitted id (k = 1) when the draft id d carries weight q(d) and the draws run over grids"""
    V = p.size
    ua = np.repeat((np.arange(Na) + 0.5) / Na, Nf)
    uf = np.tile((np.arange(Nf) + 0.5) / Nf, Na)
    n = Na * Nf
    P = np.broadcast_to(np.stack([p, p])[None], (n, 2, V))                  # (the bonus row is not looked at)
    Q = np.broadcast_to(q[None, None], (n, 1, V))
    law = np.zeros(V)
    for d in np.flatnonzero(q):
        toks = np.stack([np.zeros(n, np.int64), np.full(n, d)], axis=1)
        acc, out, _ = spec_reject_ref(P, Q, toks, ua[:, None], uf)
        assert ((out[:, 0] == d) == (acc == 1)).all()
        law += float(q[d]) * np.bincount(out[:, 0], minlength=V) / n
    return law


@pytest.mark.parametrize("V", [8, 33])
def test_the_emitted_law_is_p(V):
    Na = Nf = 256
    bound = 1.0 / Na + 1.0 / Nf                                             # derived in the module docstring
    r = np.random.default_rng(V)
    ids = r.permutation(V)
    sp, sq = ids[: V - 2], ids[1: V - 1]                                    # zeros in each, and ids only one of them holds
    p, q = dyadic(r, V, sp, 64), dyadic(r, V, sq, 64)
    point = np.zeros(V, np.float32)
    point[sp[0]] = 1.0
    for name, qq in (("general", q), ("q = p", p), ("point mass", point)):
        law = emitted_law(p, qq, Na, Nf)
        err = float(np.abs(law - p.astype(np.float64)).max())
        print(f"V {V} {name}: max |law - p| {err:.3e} (bound {bound:.3e})")
        assert abs(law.sum() - 1.0) < 1e-12
        assert err <= bound, name
    # q = p: nothing is ever rejected; a point mass: accept iff ua < p(d) (f-16's sample-and-match in law), else p without d
    n = 64
    ua = ((np.arange(n) + 0.5) / n)[:, None]
    toks = np.stack([np.zeros(n, np.int64), np.full(n, sp[0])], axis=1)
    acc, _, _ = spec_reject_ref(np.broadcast_to(np.stack([p, p])[None], (n, 2, V)), np.broadcast_to(p[None, None], (n, 1, V)),
                                toks, ua, np.full(n, 0.5))
    assert (acc == 1).all()
    acc, out, _ = spec_reject_ref(np.broadcast_to(np.stack([p, p])[None], (n, 2, V)), np.broadcast_to(point[None, None], (n, 1, V)),
                                  toks, ua, np.full(n, 0.5))
    assert ((acc == 1) == (ua[:, 0] < p[sp[0]])).all() and (out[acc == 0, 0] != sp[0]).all()


def test_ref_edge_cases():
    """q(d) == 0 accepts iff p(d) > 0; uf = 0 emits id 0; an empty residual falls back to p; nothing reaches -> V - 1"""
    p = np.array([[[0, .5, .5, 0], [.25, .25, .25, .25]]], np.float32)
    q = np.array([[[.5, 0, .5, 0]]], np.float32)
    acc, out, ap = spec_reject_ref(p, q, [[0, 1]], [[1.0]], [1.0])          # q(1) = 0 < p(1): accepted even with ua = 1
    assert acc.tolist() == [1] and out.tolist() == [[1, 3]] and ap.tolist() == [[[.5, 0.]]]
    acc, out, _ = spec_reject_ref(p, q, [[0, 0]], [[0.0]], [0.0])           # p(0) = 0: rejected even with ua = 0; uf = 0 -> id 0
    assert acc.tolist() == [0] and out.tolist() == [[0, -1]]
    acc, out, _ = spec_reject_ref(p, q, [[0, 0]], [[0.5]], [0.75])          # residual (0, .5, 0, 0): id 1
    assert out.tolist() == [[1, -1]]
    acc, out, _ = spec_reject_ref(p, p[:, :1], [[0, 2]], [[1.0]], [0.75])   # p == q, ua = 1: rejected, residual empty -> scan p
    assert acc.tolist() == [0] and out.tolist() == [[2, -1]]


def test_prototypes_in_header_with_citations(pkg):
    text = pkg._lib.HEADER.read_text()
    declared = pkg.declared_symbols()
    for s in NEW:
        assert s in declared, s
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + s + r"\s*\(", text, flags=re.S)
        assert m, s
        assert "sampling.go:33-102" in m.group(1) and "tensor_model_runner.go:89-93" in m.group(1), s
    assert "#define NVL_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", text)


def test_exported_and_bound(pkg):
    L = pkg.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.nvl_draft_sampled.argtypes) == 10
    assert len(L.nvl_verify_speculative.argtypes) == 14
    assert len(L.nvl_decode_speculative.argtypes) == 14
    assert len(L.nvl_op_spec_reject.argtypes) == 12
    assert L.nvl_abi_version() == 3
    for name in ("draft_sampled", "verify_speculative", "decode_speculative"):
        assert callable(getattr(pkg.HipTransformerModel, name)), name
    assert callable(pkg.ops.spec_reject)


def test_null_and_self_draft_are_refused_without_a_device(pkg):
    L = pkg.lib()
    sp = pkg._lib.sampling_params()
    INVALID = -1
    dummy = C.create_string_buffer(64)                                      # never dereferenced: draft == target is refused first
    same = C.cast(dummy, C.c_void_p)
    for t, d in ((None, None), (same, None), (None, same), (same, same)):
        assert L.nvl_verify_speculative(t, d, 1, None, None, 1, C.byref(sp), None, None, None, None, None, None, None) == INVALID
        assert L.nvl_decode_speculative(t, d, 1, None, None, 4, 1, C.byref(sp), None, None, None, None, None, None) == INVALID
    assert L.nvl_draft_sampled(None, 1, None, None, 1, C.byref(sp), None, None, None, None) == INVALID
    assert L.nvl_op_spec_reject(0, None, None, None, 1, 1, 8, None, None, None, None, None) == INVALID
    with pytest.raises(ValueError):
        pkg.ops.spec_reject(np.zeros((1, 2, 8)), np.zeros((1, 2, 8)), [[0, 1]], [[0.5]], [0.5])      # q must have k = 1 rows
    with pytest.raises(ValueError):
        pkg.ops.spec_reject(np.zeros((1, 2, 8)), np.zeros((1, 1, 8)), [[0, 1]], [[0.5, 0.5]], [0.5])
    if L.nvl_device_count() > 0:
        return
    p = np.full((1, 2, 8), 0.125, np.float32)
    with pytest.raises(pkg.NvlError) as e:
        pkg.ops.spec_reject(p, p[:, :1], [[0, 1]], [[0.5]], [0.5])
    assert e.value.code == -8                                               # NVL_ERR_NO_DEVICE: no host path serves it
