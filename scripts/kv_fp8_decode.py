"""Decode throughput with a bf16 KV cache against an 8-bit (e4m3fn) one: bench.py's workload (Llama-3.2-1B shapes, 32 x
(512 prompt + 128 generated)) and a long-context point (8 x (4096 prompt + 128 generated)), both KV modes, the fused greedy
decode loop.  Prints decode tokens/s and the decode-attention time per launch (nvl_get_kernel_stats, one profiled pass).
bench.py's seeded weights (gen_weights_on_device) are reused; bench.py itself is not changed or run.

    python scripts/kv_fp8_decode.py [--points bench,long]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def run(pkg, torch, bench, cfg, kv, B, S, G, reps):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B,
                                    max_batch_tokens=min(B * S, 16384), kv_cache_dtype=kv)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
    ids = list(range(B))

    def prefill():
        for i in ids:
            model.seq_reset(i)
        step = max(1, 16384 // S)
        am = []
        for j in range(0, B, step):
            chunk = ids[j:j + step]
            _, a = model.forward_batch(chunk, [prompts[i] for i in chunk], [0] * len(chunk), want_logits=False)
            am.append(a)
        return np.concatenate(am)
    first = prefill()
    model.decode_greedy(ids, first, G)             # warm-up (graph capture)
    best, toks = 1e30, None
    for _ in range(reps):
        first = prefill()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.decode_greedy(ids, first, G)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    first = prefill()
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(ids, first, G)
    attn = [k for k in model.kernel_stats() if k["site"] == "attention" and k["phase"] == "decode"]
    model.set_profile(False)
    model.close()
    us = 1e3 * sum(k["ms"] for k in attn) / max(1, sum(k["launches"] for k in attn))
    return B * G / best, us, toks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="bench,long")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    cfg = dict(pkg.synth.FULL_CONFIGS["llama-3.2-1b"])
    points = {"bench": (32, 512, 128), "long": (8, 4096, 128)}
    for name in args.points.split(","):
        B, S, G = points[name]
        cfg["max_seq_len"] = max(cfg["max_seq_len"], S + G)
        res = {kv: run(pkg, torch, bench, cfg, kv, B, S, G, args.reps) for kv in ("auto", "fp8_e4m3")}
        (tb, ab, kb), (t8, a8, k8) = res["auto"], res["fp8_e4m3"]
        agree = float((kb == k8).mean())
        print(f"{name:5s} B={B} prompt={S} gen={G}: decode tok/s bf16-KV {tb:9.1f}  fp8-KV {t8:9.1f}  ratio {t8 / tb:.3f} | "
              f"decode attention us/launch bf16-KV {ab:7.2f}  fp8-KV {a8:7.2f}  ratio {a8 / ab:.3f} | "
              f"greedy ids equal: {agree:.3f}", flush=True)


if __name__ == "__main__":
    main()
