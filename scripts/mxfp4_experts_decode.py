"""Decode and prefill throughput of a MoE model in four weight modes: bf16; MXFP4 projections with bf16
experts (mx_weight_dtype="fp4_e2m1": the baseline of the ratios, what an MXFP4 MoE model was before nvl_set_mx_expert_dtype);
MXFP4 projections + MXFP4 experts (mx_expert_dtype="fp4_e2m1"); fp8 projections + fp8 experts (f-8).  Granite-3.0-1B-a400m
shapes at B = 1, 8, 32 and the Granite-3.0-3B-a800m shape of scripts/fp8_experts_decode.py (H 1536, 32 layers, 24 / 8 heads,
40 experts, top-8, I 512) at B = 8, each B x (512 prompt + 128 generated), the fused greedy decode loop.  The modes alternate
in the same process, each point repeated; the best of the repeats is reported.  Then one profiled decode pass per mode gives
the time per launch of the MoE sites (nvl_get_kernel_stats).  bench.py's seeded weights (gen_weights_on_device) are reused;
bench.py itself is not changed or run.

    python scripts/mxfp4_experts_decode.py [--points 1b:1,1b:8,1b:32,3b:8] [--reps 3]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SITES = ("moe_router", "moe_up", "moe_down", "qkv_proj", "o_proj", "lm_head")
# mode -> (weight_dtype, expert_dtype, mx_weight_dtype, mx_expert_dtype)
MODES = {"bf16": ("auto", "auto", "none", "none"), "mx4w": ("auto", "auto", "fp4_e2m1", "none"),
         "mx4w+e": ("auto", "auto", "fp4_e2m1", "fp4_e2m1"), "fp8w+e": ("fp8_e4m3", "fp8_e4m3", "none", "none")}
BASE = "mx4w"


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def config(pkg, shape):
    cfg = dict(pkg.synth.FULL_CONFIGS["granite-3.0-1b-a400m"])
    if shape == "3b":                              # Granite-3.0-3B-a800m's shapes
        cfg.update(hidden=1536, num_layers=32, num_heads=24, num_kv_heads=8, head_dim=64, num_experts=40,
                   num_experts_per_tok=8, ffn_dim=512)
    return cfg


def make(pkg, torch, bench, cfg, mode, B, S):
    wd, ed, mw, me = MODES[mode]
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B,
                                    max_batch_tokens=min(B * S, 16384), weight_dtype=wd, expert_dtype=ed,
                                    mx_weight_dtype=mw, mx_expert_dtype=me)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    return model


def once(model, torch, prompts, G):
    ids = list(range(len(prompts)))
    S = prompts.shape[1]
    for i in ids:
        model.seq_reset(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step = max(1, 16384 // S)
    am = []
    for j in range(0, len(ids), step):
        chunk = ids[j:j + step]
        _, a = model.forward_batch(chunk, [prompts[i] for i in chunk], [0] * len(chunk), want_logits=False)
        am.append(a)
    first = np.concatenate(am)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    toks = model.decode_greedy(ids, first, G)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return len(ids) * S / (t1 - t0), len(ids) * G / (t2 - t1), toks


def sites(model, prompts, G):
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    _, first = model.forward_batch(ids, list(prompts), [0] * len(ids), want_logits=False)
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(ids, first, G)
    st = {k["site"]: k for k in model.kernel_stats() if k["phase"] == "decode"}
    model.set_profile(False)
    return {s: 1e3 * st[s]["ms"] / max(1, st[s]["launches"]) for s in SITES if s in st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1b:1,1b:8,1b:32,3b:8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--no-sites", action="store_true", help="skip the profiled pass (for a run under rocprofv3)")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    S, G = args.prompt, args.gen
    for point in args.points.split(","):
        shape, B = point.split(":")
        B = int(B)
        cfg = config(pkg, shape)
        cfg["max_seq_len"] = max(cfg["max_seq_len"], S + G)
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
        models = {mode: make(pkg, torch, bench, cfg, mode, B, S) for mode in MODES}
        wb = {mode: m.stats()["weight_bytes"] / 1e9 for mode, m in models.items()}
        for m in models.values():
            once(m, torch, prompts, G)             # warm-up (graph capture)
        best = {mode: [0.0, 0.0, None] for mode in models}
        for _ in range(args.reps):                 # the modes alternate
            for mode, m in models.items():
                p, d, toks = once(m, torch, prompts, G)
                b = best[mode]
                b[0], b[1], b[2] = max(b[0], p), max(b[1], d), toks
        us = {} if args.no_sites else {mode: sites(m, prompts, G) for mode, m in models.items()}
        for m in models.values():
            m.close()
        base = best[BASE]
        print(f"granite-{shape} B={B} prompt={S} gen={G}: weights GB " + " ".join(f"{k} {v:.3f}" for k, v in wb.items()), flush=True)
        for mode, (p, d, toks) in best.items():
            print(f"    {mode:7s} decode tok/s {d:9.1f} (x{d / base[1]:.3f} of {BASE})  prefill tok/s {p:9.1f} (x{p / base[0]:.3f})  "
                  f"greedy ids equal to {BASE}: {float((toks == base[2]).mean()):.3f}", flush=True)
        if us:
            print("    decode us/launch " + "  ".join(f"{s} " + "->".join(f"{us[mode].get(s, 0):.2f}" for mode in MODES)
                                                     for s in SITES), flush=True)


if __name__ == "__main__":
    main()
