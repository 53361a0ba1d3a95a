"""The figures behind tests/test_mamba_ops_gpu.py on this device, as the table profiles/mamba_op_tests.txt keeps: per
(case, tuning key 30, head) the rms error of the MFMA (SSD) scan against the float64 reference divided by the rounding
emulation's own rms error on the same inputs (y and final state), the worst per-(sequence, head) errors beside them, and
the worst fp32 errors of the sequential scan.  Usage: python scripts/mamba_op_figures.py > profiles/mamba_op_tests.txt"""
import contextlib
import importlib
import io
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
T = importlib.import_module("test_mamba_ops_gpu")
gpu = importlib.import_module("nano-vllm-go_amd")
assert gpu.lib().nvl_device_count() >= 1, "needs the GPU"


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):       # (the stage checks print their own figures)
        return fn(*a, **k)



print("# tests/test_mamba_ops_gpu.py on the MI355X (scripts/mamba_op_figures.py)")
print("# bf16 SSD scan: device rms error / emulation rms error against the float64 scan of the device's xbc, delta;")
print("# per head over all tokens of the case.  key30 1 = chunk-parallel three-launch form, 2 = chunk after chunk.")
print("# case          key30 head regime  ratio_y ratio_state  max_err_y  max_err_state   (max over sequences, relative to the head's max)")
worst = 0.0
cases = [(f"({hd},{ss}) ng{ng}", T.ssd_inputs(hd, ss, ng), (T.SSD_LENS, T.SSD_POS, T.SSD_SLOTS, 8), hd + ss) for hd, ss, ng in T.SSD_CASES]
cases.append(("null (32,64)", T.null_inputs(), (T.NULL_LENS, T.NULL_POS, T.NULL_SLOTS, 4), 5))
for name, (g, inp), batch, seed in cases:
    for key30 in (1, 2):
        f = quiet(T.ssd_figures, gpu, g, inp, *batch, key30, seed=seed)
        for h in range(g.nh):
            print(f"{name:15s} {key30:5d} {h:4d} {inp['regimes'][h]:6s} {f['ry'][h]:8.4f} {f['rs'][h]:11.4f} {f['ey'][:, h].max():10.2e} {f['es'][:, h].max():14.2e}")
        worst = max(worst, float(f["ry"].max()), float(f["rs"].max()))
print(f"# largest ratio {worst:.4f}  ->  SSD_RATIO_BOUND = min(2, 1.25 x {worst:.4f}) = {min(2.0, 1.25 * worst):.3f}")
print("#")
print("# sequential scan (mamba_scan_kernel), worst per-(sequence, head) error against float64; bound 1e-4")
print("# (hd, ss)   nh precision  max_err_y  max_err_state")
w32 = 0.0
for hd, ss, nh, ng in T.SEQ_CASES:
    for precision in ("f32", "bf16"):
        g, inp = T.seq_inputs(hd, ss, nh, ng, precision)
        f = quiet(T.scan_figures, gpu, g, inp, T.SEQ_LENS[precision], T.SEQ_POS, T.SEQ_SLOTS, 5, precision, seed=hd + ss)
        print(f"({hd:3d},{ss:3d}) {nh:4d} {precision:9s} {f['ey'].max():10.2e} {f['es'].max():14.2e}")
        w32 = max(w32, float(f["ey"].max()), float(f["es"].max()))
for key30_case in [(hd, ss, ng) for hd, ss, ng in T.SSD_CASES]:
    g, inp = T.ssd_inputs(*key30_case)
    f = quiet(T.ssd_figures, gpu, g, inp, T.SSD_LENS, T.SSD_POS, T.SSD_SLOTS, 8, 0, seed=key30_case[0] + key30_case[1])
    print(f"({key30_case[0]:3d},{key30_case[1]:3d})    4 key30=0   {f['ey'].max():10.2e} {f['es'].max():14.2e}   (the 922-token ragged batch)")
    w32 = max(w32, float(f["ey"].max()), float(f["es"].max()))
print(f"# worst sequential-scan error {w32:.2e}")
