"""Decode and prefill throughput with INT4 group-quantized projection weights (gq_weight_dtype="uint4", g = 128, DESIGN.md §9
f-18) against the same build's bf16 and MXFP4 (mx_weight_dtype="fp4_e2m1") ones: Llama-3.2-1B and Llama-3-8B shapes with
random weights at B = 1, 8, 32, each B x (512 prompt + 64 generated), the fused greedy decode loop.  The three weight modes
alternate in the same process, each point repeated; the best of the repeats is reported as decode ms/step, with the
resident weight bytes; B = 32 also reports prefill tok/s (32 x 512 tokens through the dequantize + tile path).  Then one
profiled decode pass per mode gives, per projection site, the time per launch and the achieved bytes/s over the algorithmic
bytes of the launch (nvl_get_kernel_stats): the INT4 kernels against the MXFP4 kernels at the same shapes tells whether the
fragment conversion is the limiter.  bench.py's seeded weights (gen_weights_on_device) are reused; bench.py itself is not
changed or run.

    python scripts/int4_weights_decode.py [--points 1b:1,1b:8,1b:32,8b:1,8b:8,8b:32] [--reps 3]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SITES = ("qkv_proj", "o_proj", "ffn_up", "ffn_down")
MODES = {"bf16": {}, "mxfp4": dict(mx_weight_dtype="fp4_e2m1"), "int4": dict(gq_weight_dtype="uint4", gq_group_size=128)}


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def make(pkg, torch, bench, cfg, mode, B, S):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B,
                                    max_batch_tokens=min(B * S, 16384), **MODES[mode])
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
    _, first = model.forward_batch(ids, list(prompts), [0] * len(ids), want_logits=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.decode_greedy(ids, first, G)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return len(ids) * S / (t1 - t0), 1e3 * (t2 - t1) / G


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
    return {s: (1e3 * st[s]["ms"] / max(1, st[s]["launches"]), st[s]["bytes"] / max(st[s]["ms"], 1e-9) / 1e6) for s in SITES if s in st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1b:1,1b:8,1b:32,8b:1,8b:8,8b:32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=64)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    names = {"1b": "llama-3.2-1b", "8b": "llama-3-8b"}
    S, G = args.prompt, args.gen
    for point in args.points.split(","):
        shape, B = point.split(":")
        B = int(B)
        cfg = dict(pkg.synth.FULL_CONFIGS[names[shape]])
        cfg["max_seq_len"] = max(cfg["max_seq_len"], S + G)
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
        models = {md: make(pkg, torch, bench, cfg, md, B, S) for md in MODES}
        wb = {md: m.stats()["weight_bytes"] / 1e9 for md, m in models.items()}
        for m in models.values():
            once(m, torch, prompts, G)             # warm-up (graph capture)
        best = {md: [0.0, 1e30] for md in models}
        for _ in range(args.reps):                 # the modes alternate
            for md, m in models.items():
                p, d = once(m, torch, prompts, G)
                best[md] = [max(best[md][0], p), min(best[md][1], d)]
        us = {md: sites(m, prompts, G) for md, m in models.items()}
        for m in models.values():
            m.close()
        line = (f"{names[shape]} B={B} ctx={S} gen={G}: weights GB " + " ".join(f"{md} {wb[md]:.3f}" for md in MODES) + " | decode ms/step "
                + " ".join(f"{md} {best[md][1]:7.3f}" for md in MODES)
                + f" | int4/bf16 {best['int4'][1] / best['bf16'][1]:.3f} int4/mxfp4 {best['int4'][1] / best['mxfp4'][1]:.3f} (time ratios)")
        if B == 32:
            line += " | prefill tok/s " + " ".join(f"{md} {best[md][0]:9.1f}" for md in MODES)
        print(line, flush=True)
        print("    decode us/launch and GB/s (bf16 | mxfp4 | int4) " + "  ".join(
            f"{s} " + " | ".join(f"{us[md].get(s, (0, 0))[0]:.2f} us {us[md].get(s, (0, 0))[1]:.0f}" for md in MODES) for s in SITES), flush=True)


if __name__ == "__main__":
    main()
