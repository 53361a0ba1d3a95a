"""The figures behind tests/test_moe_ops_gpu.py on this device, as the table profiles/moe_op_tests.txt keeps: per (case,
form, tuning keys) the largest per-row ratio rms(y_dev - y_f64) / rms(y_emulated - y_f64), the row it occurs in, the
median ratio, and whether y is finite under the NaN fill.  With --q: the figures behind tests/test_moe_q_ops_gpu.py
(quantized experts) instead, as profiles/moe_q_op_tests.txt keeps them: per (case, format, form, tuning keys) the largest
ratio of y per row and of h per picked (row, expert), whether W~ read back equals the mirror, and the largest fraction of
the fp32 summation bound that y takes against the down projection of the device's own h.
Usage: python scripts/moe_op_figures.py [--q] [output file, default profiles/moe_op_tests.txt / profiles/moe_q_op_tests.txt]"""
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


def q_figures(out_path):
    """every call of tests/test_moe_q_ops_gpu.py, measured instead of asserted (a HIP error ends the run)"""
    Q = importlib.import_module("test_moe_q_ops_gpu")
    D = importlib.import_module("dense_reference")
    lines = ["# tests/test_moe_q_ops_gpu.py on the MI355X (scripts/moe_op_figures.py --q)",
             "# y: per row m, rms(y_dev[m] - y_f64[m]) / rms(y_emulated[m] - y_f64[m]); h: the same per picked (row, expert), dense forms;",
             "# both references compute with W~ of the format's mirror and are fed the device's gate matrix.  wt: W~ read back == mirror.",
             "# down: the largest |y - down(h_dev)| as a fraction of the worst-case fp32 summation bound (moe_reference.down_error)",
             "# case                                   form         keys                 y_max  at_row   h_max  at (row, e)   wt    down   finite"]
    worst = 0.0

    def record(name, q, form, keys, call, gu=None, down_kw=None, y_ratio=None):
        nonlocal worst
        try:
            with T.Tuning(gpu, keys):
                out = call()
        except gpu.NvlError as e:
            lines.append(f"{name:40s} FAILED ({form} expected) {str(keys):20s} {e}")
            print(lines[-1], flush=True)
            if "HIP error" in str(e):
                out_path.write_text("\n".join(lines) + "\n")
                sys.exit(1)
            return
        finite = bool(np.isfinite(out["y"]).all())
        ran = out["form"] + ("" if out["form"] == form else f" (expected {form})")
        wt = all(np.array_equal(out["wt_" + k].view(np.uint32), q["w_" + k].view(np.uint32)) for k in ("in", "out"))
        y = (y_ratio(out) if y_ratio else R.expert_ratio(q, out)) if finite else np.full(1, np.nan)
        hmax, hat, down = float("nan"), "-", float("nan")
        if out["form"] in R.DENSE_FORMS:
            try:
                hr = R.h_ratio(q, out, gu(out) if gu else None)
                hat = max(hr, key=hr.get)
                hmax = hr[hat]
                err, bound = R.down_error(q, out, **(down_kw(out) if down_kw else {}))
                down = float((err / np.where(bound > 0, bound, 1.0)).max())
            except AssertionError as e:
                hat = f"h: {e}"
        lines.append(f"{name:40s} {ran:12s} {str(keys):20s} {np.nanmax(y) if finite else float('nan'):6.4f} {int(np.nanargmax(y)) if finite else -1:6d} "
                     f"{hmax:8.4f}  {str(hat):12s} {str(wt):5s} {down:6.3f}  {finite}")
        print(lines[-1], flush=True)
        worst = max([worst] + [v for v in (float(np.nanmax(y)) if finite else 0.0, hmax) if np.isfinite(v)])

    cases = list(Q.ALL_Q_CASES) + [(f"{fmt}-skew-{s}", fmt, None, 64, False, Q.DENSE2, s) for fmt in R.FORMATS for s in R.SKEWS]
    for case in cases:
        name, fmt, shape, g, crafted, forms = case[:6]
        q = Q.inputs(shape, fmt, g, crafted, *case[6:])
        for form, keys in forms:
            record(name, q, form, keys, lambda: gpu.ops.moe_stages(q["x"], q["router"], q["raw_in"], q["raw_out"], q["k"],
                                                                    expert_format=fmt, group_size=g))
    for (fmt, g, M, keys, form, ran, shape), cid in zip(D.MOE_Q_CASES, Q.CHAIN_IDS):
        q = D.moe_inputs_q(M, fmt, g, shape)
        a = float(np.float32(D.alphas(q)[0]))

        def y_ratio(out):
            f = [D._f64(out["x1"]) + a * D.moe_experts(out["op1"], out["rs1"], q, out["gate"], r) for r in (False, True)]
            return D._ratio(out["y"], f[0], f[1])
        record("chain-" + cid, q, form, keys,
               lambda: gpu.ops.dense_moe_stages(q["x"], q["attn_out"], q["wo"], q["norm_w"], q["router"], q["raw_in"], q["raw_out"],
                                                q["next_norm_w"], q["k"], norm_eps=q["norm_eps"], expert_format=fmt, group_size=g),
               gu=lambda out: Q.chain_gu(q, out), down_kw=lambda out: dict(base=out["x1"], alpha=a), y_ratio=y_ratio)
    lines.append(f"# largest ratio {worst:.4f}  ->  MOE_Q_RATIO_BOUND = min(2, 1.25 x {worst:.4f}) = {min(2.0, 1.25 * worst):.3f}")
    print(lines[-1])
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")


if "--q" in sys.argv[1:]:
    rest = [a for a in sys.argv[1:] if a != "--q"]
    q_figures(Path(rest[0]) if rest else ROOT / "profiles" / "moe_q_op_tests.txt")
    sys.exit(0)

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
