"""Prefill and decode throughput with bf16 weights, 8-bit weights (W8A16, weight_dtype="fp8_e4m3") and 8-bit weights plus
8-bit activations (W8A8, act_dtype="fp8_e4m3"): Llama-3.2-1B shapes at 32 x 512 and Llama-3-8B shapes at
16 x 512, each B x (512 prompt + G generated) with the fused greedy decode loop.  The three modes alternate in the same
process, each point repeated; the best of the repeats is reported.  Then one profiled prefill per mode gives the time and
FLOP rate of every projection site (nvl_get_kernel_stats; in W8A8 mode a site's time includes its activation quantize).
bench.py's seeded weights (gen_weights_on_device) are reused; bench.py itself is not changed or run.

    python scripts/w8a8_prefill.py [--points 1b:32,8b:16] [--reps 3] [--modes bf16,w8a16,w8a8]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SITES = ("qkv_proj", "o_proj", "ffn_up", "ffn_down", "lm_head")
MODES = {"bf16": ("auto", "auto"), "w8a16": ("fp8_e4m3", "auto"), "w8a8": ("fp8_e4m3", "fp8_e4m3")}
FP8_PEAK_TF = 5000.0        # MI355X dense FP8 MFMA (MI355X_MICROARCH.md), TFLOP/s


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def make(pkg, torch, bench, cfg, mode, B, S):
    wd, ad = MODES[mode]
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B,
                                    max_batch_tokens=min(B * S, 16384), weight_dtype=wd, act_dtype=ad)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    return model


def prefill(model, prompts):
    ids = list(range(len(prompts)))
    S = prompts.shape[1]
    for i in ids:
        model.seq_reset(i)
    step = max(1, 16384 // S)
    am = []
    for j in range(0, len(ids), step):
        chunk = ids[j:j + step]
        _, a = model.forward_batch(chunk, [prompts[i] for i in chunk], [0] * len(chunk), want_logits=False)
        am.append(a)
    return np.concatenate(am)


def once(model, torch, prompts, G):
    ids = list(range(len(prompts)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = prefill(model, prompts)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    toks = model.decode_greedy(ids, first, G)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return len(ids) * prompts.shape[1] / (t1 - t0), len(ids) * G / (t2 - t1), toks


def sites(model, prompts):
    model.set_profile(True)
    model.reset_stats()
    prefill(model, prompts)
    st = {k["site"]: k for k in model.kernel_stats() if k["phase"] == "prefill"}
    model.set_profile(False)
    return {s: (st[s]["ms"], st[s]["flops"]) for s in SITES if s in st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1b:32,8b:16")
    ap.add_argument("--modes", default="bf16,w8a16,w8a8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=64)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    names = {"1b": "llama-3.2-1b", "8b": "llama-3-8b"}
    modes = args.modes.split(",")
    S, G = args.prompt, args.gen
    for point in args.points.split(","):
        shape, B = point.split(":")
        B = int(B)
        cfg = dict(pkg.synth.FULL_CONFIGS[names[shape]])
        cfg["max_seq_len"] = max(cfg["max_seq_len"], S + G)
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
        models = {md: make(pkg, torch, bench, cfg, md, B, S) for md in modes}
        for m in models.values():
            once(m, torch, prompts, G)             # warm-up (graph capture)
        best = {md: [0.0, 0.0, None] for md in models}
        for _ in range(args.reps):                 # the modes alternate
            for md, m in models.items():
                p, d, toks = once(m, torch, prompts, G)
                b = best[md]
                b[0], b[1], b[2] = max(b[0], p), max(b[1], d), toks
        prof = {md: sites(m, prompts) for md, m in models.items()}
        for m in models.values():
            m.close()
        ref = modes[0]
        print(f"{names[shape]} B={B} prompt={S} gen={G}: " + " | ".join(
            f"{md} prefill tok/s {best[md][0]:9.1f} ({best[md][0] / best[ref][0]:.3f}x) decode tok/s {best[md][1]:8.1f} "
            f"({best[md][1] / best[ref][1]:.3f}x)" for md in modes), flush=True)
        if "w8a16" in best and "w8a8" in best:
            print(f"    greedy ids equal w8a8 vs w8a16: {float((best['w8a8'][2] == best['w8a16'][2]).mean()):.3f}", flush=True)
        for md in modes:
            tot_ms = sum(v[0] for v in prof[md].values())
            tot_fl = sum(v[1] for v in prof[md].values())
            line = "  ".join(f"{s} {v[0]:.2f}ms {v[1] / v[0] / 1e9:.0f}TF" for s, v in prof[md].items())
            print(f"    {md:6s} prefill projections {tot_ms:.2f} ms, {tot_fl / tot_ms / 1e9:.0f} TF/s "
                  f"({tot_fl / tot_ms / 1e9 / FP8_PEAK_TF * 100:.1f} % of the fp8 peak): {line}", flush=True)


if __name__ == "__main__":
    main()
