"""The figures behind tests/test_dense_ops_gpu.py on this device, as the table profiles/dense_op_tests.txt keeps: per (case,
family) whether what ran matches the case's literals, whether every check of dense_reference.check_stages held, and per
stage (x1, the FFN-up operand, h, x2, the next operand, yn) the largest per-row ratio rms(dev - f64) / rms(emulated - f64)
of the random family, each reference fed the device's output of the stage before.  Stops at the first error that is not
a failed assertion (a device error: nothing more is launched after one).
Usage: python scripts/dense_op_figures.py [output file, default profiles/dense_op_tests.txt]"""
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
T = importlib.import_module("test_dense_ops_gpu")
R = importlib.import_module("dense_reference")
gpu = importlib.import_module("nano-vllm-go_amd")
assert gpu.lib().nvl_device_count() >= 1, "needs the GPU"

STAGES = ("x1", "op1", "h", "x2", "op2", "yn")
lines = ["# tests/test_dense_ops_gpu.py on the MI355X (scripts/dense_op_figures.py)",
         "# per row m and stage: rms(dev[m] - f64[m]) / rms(emulated[m] - f64[m]), each reference fed the device's previous stage",
         "# (moe-chain rows: x1, and under x2 the block's output y; routing and logits have derived bounds)",
         "# ('-': the stage has a derived bound instead — exact family, or a deferred operand checked bit for bit)",
         f"# {'case':36s} {'family':6s} {'ran':4s} {'checks':6s} " + " ".join(f"{s:>7s}" for s in STAGES)]
worst, where = 0.0, ""
for name, fam in T.PARAMS:
    inp, out = T.run(gpu, name, fam)
    ran_ok = out["ran"] == R.CASES[name]["ran"]
    fig, held = {}, "ok"
    try:
        fig = R.check_stages(inp, out, 2.0, f"{name} {fam}")
    except AssertionError as e:
        held = "FAILED"
        print(f"{name} {fam}: {str(e)[:300]}", flush=True)
    if not ran_ok:
        print(f"{name} {fam}: ran {out['ran']}\n{'':12s}expected {R.CASES[name]['ran']}", flush=True)
    lines.append(f"{name:38s} {fam:6s} {'ok' if ran_ok else 'DIFF':4s} {held:6s} " +
                 " ".join(f"{fig[s].max():7.4f}" if s in fig else f"{'-':>7s}" for s in STAGES))
    print(lines[-1], flush=True)
    for s, r in fig.items():
        if r.max() > worst:
            worst, where = float(r.max()), f"{name} {s} row {int(r.argmax())}"
for M, keys, form, ran in R.MOE_CASES:      # the MoE chain (test_moe_chain): x1 and y
    inp = R.moe_inputs(M)
    with T.Tuning(gpu, keys):
        out = gpu.ops.dense_moe_stages(inp["x"], inp["attn_out"], inp["wo"], inp["norm_w"], inp["router"], inp["w_in"], inp["w_out"],
                                       inp["next_norm_w"], inp["k"], norm_eps=inp["norm_eps"])
    ran_ok = out["ran"] == ran and out["form"] == form
    fig, held = {}, "ok"
    try:
        fig = R.check_moe_chain(inp, out, 2.0, f"moe M={M} {form}")
    except AssertionError as e:
        held = "FAILED"
        print(f"moe M={M} {form}: {str(e)[:300]}", flush=True)
    if not ran_ok:
        print(f"moe M={M} {form}: ran {out['form']} {out['ran']}\n{'':12s}expected {form} {ran}", flush=True)
    cols = {"x1": fig.get("x1"), "x2": fig.get("y")}
    name = f"moe-chain-M{M}-{out['form']}"
    lines.append(f"{name:38s} {'random':6s} {'ok' if ran_ok else 'DIFF':4s} {held:6s} " +
                 " ".join(f"{cols[s].max():7.4f}" if cols.get(s) is not None else f"{'-':>7s}" for s in STAGES))
    print(lines[-1], flush=True)
    for s, r in fig.items():
        if r.max() > worst:
            worst, where = float(r.max()), f"{name} {s} row {int(r.argmax())}"
lines.append(f"# largest ratio {worst:.4f} ({where})  ->  DENSE_RATIO_BOUND = min(2, 1.25 x {worst:.4f}) = {min(2.0, 1.25 * worst):.3f}")
print(lines[-1])
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "dense_op_tests.txt"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
