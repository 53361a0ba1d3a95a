"""Decode time of a MoE model by expert storage: bf16 experts under bf16 projections; MXFP4 projections +
MXFP4 experts (f-10); INT4 g = 128 projections with bf16 experts (what an INT4 MoE model was before nvl_set_gq_expert_dtype);
INT4 g = 128 projections + INT4 experts.  Granite-3.0-1B-a400m shapes with bench.py's seeded random weights
(gen_weights_on_device; bench.py itself is not changed or run).  Per batch B = 1, 8, 32: B x (512 prompt, not timed + 128
generated tokens of the fused greedy decode loop), ms per step, the modes alternating in one process, the best of the repeats;
then one profiled decode pass per mode gives the algorithmic bytes per second of the MoE sites (nvl_get_kernel_stats).  Last, one
prefill figure: 32 x 512 tokens per mode.

    python scripts/int4_experts_decode.py [--batches 1,8,32] [--reps 2]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SITES = ("moe_up", "moe_down", "qkv_proj", "o_proj")
MODES = {"bf16": {}, "mx4w+e": dict(mx_weight_dtype="fp4_e2m1", mx_expert_dtype="fp4_e2m1"),
         "int4w": dict(gq_weight_dtype="uint4", gq_group_size=128),
         "int4w+e": dict(gq_weight_dtype="uint4", gq_group_size=128, gq_expert_dtype="uint4")}
BASE = "int4w"


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def make(pkg, torch, bench, cfg, mode, B, S):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B, max_batch_tokens=min(B * S, 16384), **MODES[mode])
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    return model


def prefill(model, torch, prompts):
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, first = model.forward_batch(ids, list(prompts), [0] * len(ids), want_logits=False)
    torch.cuda.synchronize()
    return first, time.perf_counter() - t0


def decode(model, torch, prompts, G):
    first, _ = prefill(model, torch, prompts)
    ids = list(range(len(prompts)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = model.decode_greedy(ids, first, G)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / G, toks


def sites(model, torch, prompts, G):
    first, _ = prefill(model, torch, prompts)
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(list(range(len(prompts))), first, G)
    st = {k["site"]: k for k in model.kernel_stats() if k["phase"] == "decode"}
    model.set_profile(False)
    return {s: st[s]["bytes"] / (1e6 * st[s]["ms"]) for s in SITES if s in st and st[s]["ms"] > 0}     # GB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=128)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    S, G = args.prompt, args.gen
    batches = [int(b) for b in args.batches.split(",")]
    cfg = dict(pkg.synth.FULL_CONFIGS["granite-3.0-1b-a400m"])
    cfg["max_seq_len"] = max(cfg["max_seq_len"], S + G)
    models = {mode: make(pkg, torch, bench, cfg, mode, max(batches + [32]), S) for mode in MODES}
    print("granite-3.0-1b-a400m shapes, random weights: weights GB " +
          " ".join(f"{k} {m.stats()['weight_bytes'] / 1e9:.3f}" for k, m in models.items()), flush=True)
    for B in batches:
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
        for m in models.values():
            decode(m, torch, prompts, G)               # warm-up (graph capture)
        best = {mode: [float("inf"), None] for mode in models}
        for _ in range(args.reps):                     # the modes alternate
            for mode, m in models.items():
                ms, toks = decode(m, torch, prompts, G)
                if ms < best[mode][0]:
                    best[mode] = [ms, toks]
        gbs = {mode: sites(m, torch, prompts, G) for mode, m in models.items()}
        print(f"B={B} prompt={S} gen={G}", flush=True)
        for mode, (ms, toks) in best.items():
            print(f"    {mode:8s} decode ms/step {ms:7.3f} (x{best[BASE][0] / ms:.3f} the speed of {BASE})  "
                  f"greedy ids equal to {BASE}: {float((toks == best[BASE][1]).mean()):.3f}  GB/s " +
                  "  ".join(f"{s} {gbs[mode].get(s, 0):7.1f}" for s in SITES), flush=True)
    prompts = np.random.default_rng(1).integers(0, cfg["vocab_size"], (32, S)).astype(np.int32)
    for m in models.values():
        prefill(m, torch, prompts)
    best = {mode: float("inf") for mode in models}
    for _ in range(args.reps):
        for mode, m in models.items():
            best[mode] = min(best[mode], prefill(m, torch, prompts)[1])
    print(f"prefill 32 x {S}: tok/s " + "  ".join(f"{mode} {32 * S / t:9.1f}" for mode, t in best.items()), flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
