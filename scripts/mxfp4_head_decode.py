"""Decode throughput with the MXFP4 LM head and tied embedding (mx_head_dtype="fp4_e2m1") against the same
build's MXFP4 projections with the bf16 head, its bf16 and its 8-bit (weight_dtype="fp8_e4m3") models: Llama-3.2-1B shapes
(tied) at B = 1, 8, 32 and Llama-3-8B shapes (untied) at B = 16, each B x (512 prompt + 128 generated), the fused greedy
decode loop.  The four modes alternate in the same process, each point repeated; the best of the repeats is reported, with
the resident weight bytes of every mode.  Then one profiled decode pass per mode gives the time per launch of the lm_head
and embed sites (nvl_get_kernel_stats; in the fused loop the gather is part of the seam launch, accounted under the site
that launch carries).  bench.py's seeded weights (gen_weights_on_device) are reused; bench.py itself is not changed or run.

    python scripts/mxfp4_head_decode.py [--points 1b:1,1b:8,1b:32,8b:16] [--reps 3]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SITES = ("lm_head", "embed", "norm")


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


MODES = {"bf16": {}, "mxfp4": dict(mx_weight_dtype="fp4_e2m1"),
         "mxfp4+head": dict(mx_weight_dtype="fp4_e2m1", mx_head_dtype="fp4_e2m1"), "fp8": dict(weight_dtype="fp8_e4m3")}


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


def sites(model, torch, prompts, G):
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
    ap.add_argument("--points", default="1b:1,1b:8,1b:32,8b:16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=128)
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
        best = {md: [0.0, 0.0, None] for md in models}
        for _ in range(args.reps):                 # the modes alternate
            for md, m in models.items():
                p, d, toks = once(m, torch, prompts, G)
                b = best[md]
                b[0], b[1], b[2] = max(b[0], p), max(b[1], d), toks
        us = {md: sites(m, torch, prompts, G) for md, m in models.items()}
        for m in models.values():
            m.close()
        print(f"{names[shape]} B={B} prompt={S} gen={G}: resident weights GB " + " ".join(f"{md} {wb[md]:.2f}" for md in MODES)
              + " | decode tok/s " + " ".join(f"{md} {best[md][1]:9.1f}" for md in MODES)
              + f" | mxfp4+head/mxfp4 {best['mxfp4+head'][1] / best['mxfp4'][1]:.3f} mxfp4+head/fp8 {best['mxfp4+head'][1] / best['fp8'][1]:.3f}"
              + f" mxfp4+head/bf16 {best['mxfp4+head'][1] / best['bf16'][1]:.3f}"
              + f" | greedy ids equal to mxfp4: {float((best['mxfp4'][2] == best['mxfp4+head'][2]).mean()):.3f}", flush=True)
        print("    decode us/launch (" + " / ".join(MODES) + ") " + "  ".join(
            f"{s} " + "/".join(f"{us[md].get(s, 0):.2f}" for md in MODES) for s in SITES), flush=True)


if __name__ == "__main__":
    main()
