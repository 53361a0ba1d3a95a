"""The figures behind tests/test_attention_ops_gpu.py on this device, as the table profiles/attention_op_tests.txt keeps:
per (case, form) the kernel that ran and its launch shape, the largest |dev - f64| as a fraction of bound (a), and over the
(sequence, kv head) pools the largest and the median ratio rms(dev - f64) / rms(emulated - f64) of bound (b).
Usage: python scripts/attention_op_figures.py [output file, default profiles/attention_op_tests.txt]"""
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
T = importlib.import_module("test_attention_ops_gpu")
R = importlib.import_module("attention_reference")
gpu = importlib.import_module("nano-vllm-go_amd")
assert gpu.lib().nvl_device_count() >= 1, "needs the GPU"

lines = ["# tests/test_attention_ops_gpu.py on the MI355X (scripts/attention_op_figures.py)",
         "# (a): largest |dev - f64| / (1.05 x 2^-9 (A + 2 |f64|) + 1e-6 max|f64|) over the batch's elements",
         "# (b): per (sequence, kv head), pooled over its rows: rms(dev - f64) / rms(emulated - f64); pools whose emulation is exact are left out",
         "# case  form          keys        ran           nw nsplit  draw  (a)     (b) max  at (seq, kvh)  (b) median  pools  finite"]
worst = 0.0


def row(name, form, keys, res, b):
    global worst
    finite = bool(np.isfinite(res["out"]).all())
    a, pooled = R.figures(b, res["out"], res["ran"]) if finite else (float("nan"), [])
    ratios = [(d / e, i, h) for i, h, d, e in pooled if e > 0]
    top = max(ratios) if ratios else (float("nan"), -1, -1)
    med = float(np.median([x[0] for x in ratios])) if ratios else float("nan")
    lines.append(f"{name:5s} {form:13s} {str(keys):11s} {res['ran']:13s} {res['nw']:2d} {res['nsplit']:6d} {b['draw']:5d}  {a:6.3f}  {top[0]:7.4f}  "
                 f"({top[1]:2d}, {top[2]:2d})      {med:10.4f}  {len(ratios):5d}  {finite}")
    print(lines[-1], flush=True)
    if ratios:
        worst = max(worst, top[0])


for name in R.DECODE_CASES:
    for form in T.DECODE_FORMS:
        b = R.batch(name, form)
        row(name, form, {}, T.run(gpu, b), b)
        if name in ("D1", "D2"):
            for nw in (2, 4, 8):
                row(name, form, {15: nw}, T.run(gpu, b, keys={15: nw}), b)
for name in ("P1", "P2", "P3", "P4"):
    for form in ("plain", "kv8"):
        if (name, form) != ("P4", "plain"):
            b = R.batch(name, form)
            row(name, form, {}, T.run(gpu, b), b)
for name in R.MQ_CASES:
    b = R.batch(name, "plain")
    res = gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"], form="mq")
    row(name, "mq", {}, res, b)
lines.append(f"# largest ratio {worst:.4f}  ->  ATTN_RATIO_BOUND = min(2, 1.25 x {worst:.4f}) = {min(2.0, 1.25 * worst):.3f}")
print(lines[-1])
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "attention_op_tests.txt"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
