"""Attention logit soft-capping: the SOFTCAP instantiations through ops.attention_batch(softcap=cap) against
float64 with s = cap * tanh(s / cap) BEFORE the visibility mask: the cases, pools (+-64 garbage K, 1024 V: a kernel that caps
after masking lets them in) and bounds (a) / (b) of tests/test_attention_ops_gpu.py.  cap 2.0 bends these scores (|s| up to 5);
50.0 is Gemma 2's, where 1 - 2 / (1 + e) cancels; boost 64 scales the scores so that exp2 of the cap's argument overflows.
Only cases whose float64 emulation alone stays within R.HEADROOM of bound (a) are listed (references asserts it).
Figures: profiles/attention_softcap_op_tests.txt (largest ratio (b) 1.13: ATTN_RATIO_BOUND holds with 1.25 x to spare)."""
import numpy as np
import pytest

import attention_reference as R
import test_attention_hd256_gpu  # noqa: F401  (registers the head_dim 256 cases G1 .. G9)
import test_attention_window_gpu as W
from test_attention_ops_gpu import ATTN_RATIO_BOUND

pytestmark = pytest.mark.gpu

_D = [(n, f) for n in ("D1", "D2", "D4", "D7") for f in ("plain", "fused", "kv8")]
_P = [(n, f) for n in ("P2", "P3") for f in ("plain", "kv8")] + [("Q2", "mq"), ("Q2", "mq_kv8")]
CASES = ([(n, f, cap, 0, 1) for cap in (2.0, 50.0) for n, f in _D + _P] + [("M1", "mq", 2.0, 0, 1), ("M1", "mq_kv8", 2.0, 0, 1)] +
         [(n, "plain", 2.0, 0, 1) for n in ("G1", "G2", "G6", "G8")] + [("G9", "mq", 2.0, 0, 1), ("G2", "plain", 50.0, 0, 1), ("G8", "plain", 50.0, 0, 1)] +
         [(n, f, 2.0, 100, 1) for n, f in (("D2", "fused"), ("D4", "plain"), ("P3", "plain"), ("P3", "kv8"), ("G8", "plain"))] +
         [("D1", f, 2.0, 0, 64) for f in ("plain", "fused", "kv8")] + [("P3", "plain", 2.0, 0, 64)])
assert W.WINDOW_RATIO_BOUND == ATTN_RATIO_BOUND       # (W.check asserts bound (b) against it)


def attend_capped(q, K, V, pos, scale, cap, visible):
    """R.attend with the scores capped before the mask: the same ref, bound, emu_rounded, emu_unrounded"""
    q, K, V = (np.asarray(a, np.float64) for a in (q, K, V))
    n, nH, hd = q.shape
    nKV, g = K.shape[0], nH // K.shape[0]
    qh = q.reshape(n, nKV, g, hd).transpose(1, 0, 2, 3).reshape(nKV, n * g, hd)
    s = cap * np.tanh(np.einsum("krd,ktd->krt", qh, K) * scale / cap)
    s = np.where(np.repeat(visible, g, axis=0)[None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    den = p.sum(-1, keepdims=True)
    ref = np.einsum("krt,ktd->krd", p, V) / den
    pr = R.bf16(p)
    num = np.einsum("krt,ktd->krd", pr, V)
    out = dict(ref=ref, bound=2.0 ** -9 * (np.einsum("krt,ktd->krd", p, np.abs(V)) / den + 2 * np.abs(ref)),
               emu_rounded=R.bf16(num / pr.sum(-1, keepdims=True)), emu_unrounded=R.bf16(num / den))
    return {k: R._unrows(v, n, nH) for k, v in out.items()}


def references(b, cap, window, boost, f32=False):
    """-> (the capped references, computed once, the key they have in W's reference cache: W.check(b, res, key, tag) finds them)"""
    key = ("softcap", cap, window, boost)
    if (b["name"], b["form"], key) not in W._REFS:
        refs = W._REFS[b["name"], b["form"], key] = []
        for i, (pos, n) in enumerate(zip(b["seq_pos"], b["seq_len"])):
            qi, kj = (pos + np.arange(n))[:, None], np.arange(pos + n)[None, :]
            vis = (kj <= qi) & ((kj > qi - window) if window else True)
            refs.append(attend_capped(b["q_ref"][i], b["K"][i], b["V"][i], pos, b["scale"] * boost, cap, vis))
    for r in W._REFS[b["name"], b["form"], key]:        # the listed cases only: the emulation alone leaves the device a tenth of bound (a)
        lim = 1.05 * r["bound"] + 1e-6 * np.abs(r["ref"]).max()
        assert f32 or max(float((np.abs(r[e] - r["ref"]) / lim).max()) for e in ("emu_rounded", "emu_unrounded")) <= R.HEADROOM, key
    return W._REFS[b["name"], b["form"], key], key


def run(gpu, name, form, cap, window=0, boost=1, precision="bf16"):      # (W.run's way of calling, with the cap)
    b = R.batch(name, {"mq": "plain", "mq_kv8": "kv8"}.get(form, form))
    return b, gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"], form=form,
                                      scale=b["scale"] * boost if boost != 1 else 0.0, rope_base=b["rope_base"], max_seq=b["max_seq"],
                                      k_scale=b.get("k_scale", 1.0), v_scale=b.get("v_scale", 1.0), precision=precision, window=window, softcap=cap)


@pytest.mark.parametrize("name,form,cap,window,boost", CASES)
def test_softcap(gpu, name, form, cap, window, boost):
    """bounds (a) and (b) as R.check_bf16 states them, by W.check's code, against the capped reference"""
    b, res = run(gpu, name, form, cap, window, boost)
    tag = f"{name} {form} cap={cap} W={window} x{boost}"
    want = "prefill_hd256" if name in ("G6", "G8", "G9") else "decode_hd256" if name[0] == "G" else {"plain": "prefill", "kv8": "prefill_kv8"}[form] if name[0] == "P" else W.RAN[form]
    assert res["ran"] == want, (tag, res["ran"])           # the name an uncapped launch reports
    W.check(b, res, references(b, cap, window, boost)[1], tag)          # finite; (a) <= 1; (b) <= ATTN_RATIO_BOUND
    if form == "fused":
        R.check_append(b, res)


@pytest.mark.parametrize("name", ["P3", "D7", "G8"])
def test_softcap_f32(gpu, name):          # check_f32's rule against the capped reference
    b, res = run(gpu, name, "plain", 2.0, precision="f32")
    assert res["ran"] == "f32" and np.isfinite(res["out"]).all()
    worst = max(float((np.abs(dev - ref["ref"]).max(-1) / np.abs(ref["ref"]).max(-1)).max())
                for ref, dev in zip(references(b, 2.0, 0, 1, f32=True)[0], R.split_rows(b, res["out"])))
    print(f"{name} f32 cap=2.0: worst row error {worst:.3e} of the row maximum (bound 5e-5)")
    assert worst <= 5e-5, (name, worst)


@pytest.mark.parametrize("name,form", [("D2", "plain"), ("D2", "fused"), ("D2", "kv8"), ("P1", "plain"), ("M1", "mq")])
def test_softcap_zero_changes_no_bit(gpu, name, form):          # softcap = 0 through the new entry point is the launch without it
    _, zero = run(gpu, name, form, 0.0)
    _, none = W.run(gpu, name, form, 0)          # (ops.attention_batch without the keyword)
    assert (zero["ran"], zero["nw"], zero["nsplit"]) == (none["ran"], none["nw"], none["nsplit"])
    assert np.array_equal(zero["out"], none["out"]), (name, form)
