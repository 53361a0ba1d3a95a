"""The figures behind tests/test_qkv_ops_gpu.py on this device, as the table profiles/qkv_op_tests.txt keeps: per case
whether what ran matches the case's literals, whether every check of qkv_reference.check held, and the worst figure per
bound — the operand's rms ratio, and for every derived bound the largest error as a share of the bound (1 = at the bound),
the share of Q / K elements that differ from the rounded float64 value, the f32 cases' error as a share of the row's
maximum —, then the worst per bound and case family, the kernels the cases name as having run, and the `--durations` of
the file beside those of tests/test_attention_ops_gpu.py (a child pytest process).  Stops at the first error that is not a
failed assertion (a device error: nothing more is launched after one).
Usage: python scripts/qkv_op_figures.py [output file, default profiles/qkv_op_tests.txt]"""
import importlib
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
T = importlib.import_module("test_qkv_ops_gpu")
R = importlib.import_module("qkv_reference")
gpu = importlib.import_module("nano-vllm-go_amd")
assert gpu.lib().nvl_device_count() >= 1, "needs the GPU"

COLS = ("op_ratio", "qkv", "Q", "K", "Q_share", "K_share", "Q_epi", "K_epi", "V_epi", "op_f32", "qkv_f32", "Q_f32", "K_f32")
KERNELS = {"epilogue": "EPI_QKV in {gemm}", "decode_store_rope": "rope_kv_kernel<bf16_t> behind the decode-form GEMM",
           "groups_store_rope": "rope_kv_kernel<bf16_t> behind the 64-row groups", "f32_store_rope": "rope_kv_kernel<float> behind gemm_f32_kernel",
           "store_rope_kv8": "rope_kv8_kernel behind the {gemm} GEMM", "store_only": "the decode-form GEMM alone (a decode step)"}
EMBED = {"bf16": "embed_kernel<bf16_t, true>", "f32": "embed_kernel<float, false>"}


def family(name):
    c = R.CASES[name]
    f = "embed" if c.get("embed") else c["ran"]["form"]
    return f + ("-hd128" if c["hd"] == 128 else "") + ("-exact" if c["family"] == "exact" else "")


lines = ["# tests/test_qkv_ops_gpu.py on the MI355X (scripts/qkv_op_figures.py)",
         "# op_ratio: per row rms(dev - f64) / rms(bf16(f64) - f64) of the normed operand; qkv, Q, K, *_epi: the largest error as a",
         "# share of its derived bound (1 = at the bound); *_share: elements that differ from the rounded float64 value (cap 1e-3);",
         "# *_f32: the largest error as a share of the row's maximum (bound 2e-5); '-': not part of this form (or bit for bit / exact)",
         f"# {'case':38s} {'ran':4s} {'checks':6s} " + " ".join(f"{c:>8s}" for c in COLS)]
worst, ran_names = {}, set()
for name in R.CASES:
    inp, out = T.run(gpu, name)
    ran_ok = out["ran"] == R.CASES[name]["ran"]
    fig, held = {}, "ok"
    try:
        fig = R.check(inp, out, 2.0, name)
    except AssertionError as e:
        held = "FAILED"
        print(f"{name}: {str(e)[:300]}", flush=True)
    if not ran_ok:
        print(f"{name}: ran {out['ran']}\n{'':12s}expected {R.CASES[name]['ran']}", flush=True)
    elif held == "ok":
        ran_names.add(KERNELS[out["ran"]["form"]].format(gemm=out["ran"]["gemm"]))
        if out["ran"]["embed"]:
            ran_names.add(EMBED[out["ran"]["embed"]])
        if out["ran"]["norm"]:
            ran_names.add(f"norm kernel: {out['ran']['norm']}")
    lines.append(f"{name:40s} {'ok' if ran_ok else 'DIFF':4s} {held:6s} " + " ".join(f"{fig[c]:8.2e}" if c in fig else f"{'-':>8s}" for c in COLS))
    print(lines[-1], flush=True)
    for k, v in fig.items():
        w = worst.setdefault((family(name), k), (0.0, ""))
        if v >= w[0]:
            worst[(family(name), k)] = (v, name)
lines.append("# worst per bound and case family")
for (fam, k), (v, name) in sorted(worst.items()):
    lines.append(f"# {fam:28s} {k:9s} {v:9.3e}  ({name})")
lines.append("# kernels named by cases whose ran literals and checks held:")
lines += [f"#   {k}" for k in sorted(ran_names)]
# the durations of the file, beside the attention op tests' in the same run
r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "--durations=0", "-p", "no:cacheprovider",
                    str(ROOT / "tests" / "test_qkv_ops_gpu.py"), str(ROOT / "tests" / "test_attention_ops_gpu.py")],
                   cwd=ROOT, capture_output=True, text=True, timeout=900)
dur = {"qkv": [], "attention": []}
for m in re.finditer(r"^([0-9.]+)s call\s+tests/test_(qkv|attention)_ops_gpu\.py::(\S+)", r.stdout, re.M):
    dur[m.group(2)].append((float(m.group(1)), m.group(3)))
tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else f"pytest exit {r.returncode}"
lines.append(f"# pytest --durations=0 of tests/test_qkv_ops_gpu.py + tests/test_attention_ops_gpu.py: {tail}")
if dur["qkv"] and dur["attention"]:
    slow_a = max(dur["attention"])
    lines.append(f"# slowest case of test_attention_ops_gpu.py: {slow_a[0]:.2f}s ({slow_a[1]}); test_qkv_ops_gpu.py: {sum(d for d, _ in dur['qkv']):.2f}s in all")
    for d, n in sorted(dur["qkv"], reverse=True)[:12]:
        lines.append(f"#   {d:6.2f}s {n}")
    over = [(d, n) for d, n in dur["qkv"] if d > 2 * slow_a[0]]
    lines.append("# cases longer than twice the slowest attention case: " + (", ".join(f"{n} ({d:.2f}s)" for d, n in over) if over else "none"))
else:
    lines.append("# (no durations parsed)")
    print(r.stdout[-3000:], r.stderr[-2000:])
print("\n".join(lines[-40:]))
out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "qkv_op_tests.txt"
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
