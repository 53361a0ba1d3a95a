"""Sliding-window attention: the WINDOW instantiations of the kernels of attn.h / kv8.h through
ops.attention_batch(window=W) against tests/attention_reference.py's float64 statement under visible = (j <= i) & (j > i - W):
the cases, pools and bounds (a) / (b) of tests/test_attention_ops_gpu.py.  Windows: one key; an edge on a 64-key tile edge and
one past it; inside a tile; across a 192- / 256-key block edge.  P1's 70-row sequence at W = 64 / 65: rows of one wave whose
windows start in different tiles (the -inf guard of attn_prefill_tile<.., WINDOW>).  W = 1: exactly the own key's bf16 V row."""
import numpy as np
import pytest

import attention_reference as R

pytestmark = pytest.mark.gpu

WINDOW_RATIO_BOUND = 1.550       # the largest measured ratio is below 1.24: test_attention_ops_gpu.py's ATTN_RATIO_BOUND
CASES = ([(n, f) for n in ("D1", "D2", "D3", "D4", "D5", "D7") for f in ("plain", "fused", "kv8")] +
         [(n, f) for n in ("P1", "P2", "P3") for f in ("plain", "kv8")] + [(n, f) for n in ("M1", "M2") for f in ("mq", "mq_kv8")])
RAN = {"plain": "decode", "fused": "decode_fused", "kv8": "decode_kv8", "mq": "decode_mq", "mq_kv8": "decode_mq_kv8",
       "mq_kv8_two": "decode_mq_kv8"}
WINDOWS = [1, 64, 65, 100, 192]
# The launch shape follows the keys a workgroup reads, min(context, W + 63): the windows above are at most four tiles, which is
# two waves at head_dim 64 and two or four at 128.  The WINDOW instantiations they leave unreached, with the shape
# (waves, workgroups per (sequence, kv head)) decode_attn_cfg gives them: the one-position forms at 8 and 6 - 9 tiles; the
# verify forms at 6 tiles, at head_dim 128 (Q4) and with two query tiles per workgroup (Q1, form "mq_kv8_two": the 8-bit
# verify form under nvl_set_tuning key 40 = 2).
R.ALL_CASES.update(R.VERIFY_CASES)
SHAPES = {("D2", 500): (8, 1), ("D4", 500): (8, 1), ("D7", 500): (4, 1), ("M1", 300): (4, 1),
          ("Q4", 1): (2, 1), ("Q4", 100): (4, 1), ("Q4", 500): (8, 1), ("Q1", 100): (2, 1), ("Q1", 300): (4, 1), ("Q1", 500): (8, 1)}
MORE = ([(n, f, 500) for n in ("D2", "D4", "D7") for f in ("plain", "fused", "kv8")] + [("M1", f, 300) for f in ("mq", "mq_kv8")] +
        [("Q4", f, w) for f in ("mq", "mq_kv8") for w in (1, 100, 500)] + [("Q1", "mq_kv8_two", w) for w in (100, 300, 500)])
_REFS = {}


def run(gpu, name, form, window, precision="bf16"):      # (the verify forms: the plain / kv8 batch under the verify flag)
    b = R.batch(name, {"mq": "plain", "mq_kv8": "kv8", "mq_kv8_two": "kv8"}.get(form, form))
    with R.tuning(gpu, {40: 2} if form == "mq_kv8_two" else {}):
        return b, gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"],
                                          form=form.replace("_two", ""), rope_base=b["rope_base"], max_seq=b["max_seq"],
                                          k_scale=b.get("k_scale", 1.0), v_scale=b.get("v_scale", 1.0), precision=precision, window=window)


def references(b, window):
    key = (b["name"], b["form"], window)
    if key not in _REFS:
        _REFS[key] = []
        for i, (pos, n) in enumerate(zip(b["seq_pos"], b["seq_len"])):
            qi, kj = (pos + np.arange(n))[:, None], np.arange(pos + n)[None, :]
            _REFS[key].append(R.attend(b["q_ref"][i], b["K"][i], b["V"][i], pos, b["scale"], (kj <= qi) & (kj > qi - window)))
    return _REFS[key]


def check(b, res, window, tag):
    """bounds (a) and (b) as R.check_bf16 states them, against the windowed reference (pairs with emulation error 0 skip (b))"""
    assert np.isfinite(res["out"]).all(), (tag, "out is not finite")
    g, worst, top = b["nH"] // b["nKV"], 0.0, 0.0
    for i, (ref, dev) in enumerate(zip(references(b, window), R.split_rows(b, res["out"]))):
        if window == 1:
            own = np.stack([np.repeat(b["V"][i][:, b["seq_pos"][i] + j], g, axis=0) for j in range(b["seq_len"][i])])
            assert np.array_equal(dev, own), (tag, i, "W = 1: not the own key's V row")
        err = np.abs(dev - ref["ref"])
        worst = max(worst, float((err / (1.05 * ref["bound"] + 1e-6 * np.abs(ref["ref"]).max())).max()))
        emu = ref["emu_" + R.denominator(res["ran"])] - ref["ref"]
        for h in range(b["nKV"]):
            d, e = (float(np.sqrt((x[:, h * g:(h + 1) * g] ** 2).mean())) for x in (err, emu))
            if e > 0:
                top = max(top, d / e)
    print(f"{tag}: ran {res['ran']} nw {res['nw']} nsplit {res['nsplit']}  (a) {worst:.3f} of the bound  (b) largest ratio {top:.4f}")
    assert worst <= 1.0, (tag, "element bound", worst)
    assert top <= WINDOW_RATIO_BOUND, (tag, "rms ratio", top)


@pytest.mark.parametrize("name,form,window", [(n, f, w) for w in WINDOWS for n, f in CASES] + MORE)
def test_window(gpu, name, form, window):
    b, res = run(gpu, name, form, window)
    assert res["ran"] == (RAN[form] if name[0] != "P" else {"plain": "prefill", "kv8": "prefill_kv8"}[form]), (name, form, res["ran"])
    if (name, form, window) in MORE:
        assert (res["nw"], res["nsplit"]) == SHAPES[name, window], (name, form, window, res["nw"], res["nsplit"])
    check(b, res, window, f"{name} {form} W={window}")
    if form == "fused":
        R.check_append(b, res)


@pytest.mark.parametrize("name,form", [("D2", "plain"), ("D2", "fused"), ("D2", "kv8"), ("P1", "plain"), ("P1", "kv8"), ("M1", "mq"), ("M1", "mq_kv8")])
def test_window_beyond_every_context_changes_no_bit(gpu, name, form):
    _, wide = run(gpu, name, form, 4096)
    _, none = run(gpu, name, form, 0)
    assert (wide["ran"], wide["nw"], wide["nsplit"]) == (none["ran"], none["nw"], none["nsplit"])
    assert np.array_equal(wide["out"], none["out"]), (name, form)


@pytest.mark.parametrize("window", [65, 100])
@pytest.mark.parametrize("name", ["P1", "D7"])
def test_window_f32(gpu, name, window):          # check_f32's rule against the windowed reference
    b, res = run(gpu, name, "plain", window, precision="f32")
    assert res["ran"] == "f32" and np.isfinite(res["out"]).all()
    worst = max(float((np.abs(dev - ref["ref"]).max(-1) / np.abs(ref["ref"]).max(-1)).max())
                for ref, dev in zip(references(b, window), R.split_rows(b, res["out"])))
    print(f"{name} f32 W={window}: worst row error {worst:.3e} of the row maximum (bound 5e-5)")
    assert worst <= 5e-5, (name, window, worst)
