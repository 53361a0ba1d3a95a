"""The figures behind tests/test_moe_ops_gpu.py on this device, as the table profiles/moe_op_tests.txt keeps: per (case,
form, tuning keys) the largest per-row ratio rms(y_dev - y_f64) / rms(y_emulated - y_f64), the row it occurs in, the
median ratio, and whether y is finite under the NaN fill.
Usage: python scripts/moe_op_figures.py [output file, default profiles/moe_op_tests.txt]"""
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
T = importlib.import_module("test_moe_ops_gpu")
R = importlib.import_module("moe_reference")
gpu = importlib.import_module("nano-vllm-go_amd")
assert gpu.lib().nvl_device_count() >= 1, "needs the GPU"

lines = ["# tests/test_moe_ops_gpu.py on the MI355X (scripts/moe_op_figures.py)",
         "# per row m: rms(y_dev[m] - y_f64[m]) / rms(y_emulated[m] - y_f64[m]), both references fed the device's gate matrix",
         "# case                         form         keys                 rows  max_ratio  at_row  median  finite"]
worst = 0.0
cases = list(T.EXPERT_CASES) + [(f"skew-{s}", (lambda s=s: R.skew_inputs(s)), T.DENSE2) for s in R.SKEWS]
for name, make, forms in cases:
    inp = make()
    for form, keys in forms:
        with T.Tuning(gpu, keys):
            out = gpu.ops.moe_stages(inp["x"], inp["router"], inp["w_in"], inp["w_out"], inp["k"])
        finite = bool(np.isfinite(out["y"]).all())
        ratio = R.expert_ratio(inp, out) if finite else np.full(inp["x"].shape[0], np.nan)
        ran = out["form"] + ("" if out["form"] == form else f" (expected {form})")
        lines.append(f"{name:30s} {ran:12s} {str(keys):20s} {len(ratio):4d} {np.nanmax(ratio) if finite else float('nan'):10.4f} "
                     f"{int(np.nanargmax(ratio)) if finite else -1:7d} {float(np.median(ratio)):7.4f}  {finite}")
        print(lines[-1], flush=True)
        if finite:
            worst = max(worst, float(ratio.max()))
lines.append(f"# largest ratio {worst:.4f}  ->  MOE_RATIO_BOUND = min(2, 1.25 x {worst:.4f}) = {min(2.0, 1.25 * worst):.3f}")
print(lines[-1])
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "moe_op_tests.txt"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
