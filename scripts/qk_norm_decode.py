"""Decode and prefill cost of the per-head QK RMSNorm against the same build without it: Qwen3-0.6B and
Qwen3-8B shapes with random weights, QK-norm on against off in one process, alternating, best of --reps.  Prints decode
ms/step at B = 1 / 8 / 32 with context 512 and prefill tok/s at 32 x 512, and the launch counts of one profiled decode step
(nvl_stats: gemm + attention + other launches): equal with and without QK-norm at head_dim 128 (the norm lives in the fused
attention kernel's prologue), exactly one per attention layer higher at head_dim 64 (the norm + RoPE launch; a 0.6B-shaped
model with head_dim 64 is built for that check alone).  bench.py's seeded weights (gen_weights_on_device) are reused; the
two norm vectors per layer are drawn around 1.

    python scripts/qk_norm_decode.py [--models qwen3-0.6b,qwen3-8b] [--reps 5]"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from sliding_window_decode import load_bench  # noqa: E402

COMMON = dict(vocab_size=151936, num_kv_heads=8, head_dim=128, attention_type="gqa", norm_type="rmsnorm", position_type="rope",
              activation_type="swiglu", block_style="sequential", rope_base=1000000.0, norm_eps=1e-6)
SHAPES = {"qwen3-0.6b": dict(COMMON, hidden=1024, num_layers=28, num_heads=16, ffn_dim=3072, tied_embedding=True),
          "qwen3-8b": dict(COMMON, hidden=4096, num_layers=36, num_heads=32, ffn_dim=12288, tied_embedding=False)}
CTX, GEN = 512, 32


def make(pkg, torch, bench, cfg, qk_norm, B, tokens):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B, max_batch_tokens=tokens)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    rng = np.random.default_rng(3)
    for li in range(cfg["num_layers"] if qk_norm else 0):
        for slot in ("q_norm_w", "k_norm_w"):
            model.upload(slot, li, (1.0 + 0.25 * rng.standard_normal(cfg["head_dim"])).astype(np.float32))
    model.finalize()
    return model


def once(model, torch, prompts):
    """prefill of the whole batch in one call, then GEN fused decode steps -> (prefill tok/s, decode ms/step)"""
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, first = model.forward_batch(ids, list(prompts), [0] * len(ids), want_logits=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.decode_greedy(ids, first, GEN)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return prompts.size / (t1 - t0), 1e3 * (t2 - t1) / GEN


def launches_per_step(model, B):
    """one profiled decode step behind the timed ones"""
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(list(range(B)), np.zeros(B, np.int32), 1)
    s = model.stats()
    model.set_profile(False)
    return int(s["gemm_launches"] + s["attn_launches"] + s["other_launches"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    for name in args.models.split(","):
        for B in (1, 8, 32):
            cfg = dict(SHAPES[name], max_seq_len=CTX + GEN + 2)
            prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, CTX)).astype(np.int32)
            models = {on: make(pkg, torch, bench, cfg, on, B, B * CTX) for on in (True, False)}
            for m in models.values():
                once(m, torch, prompts)                # warm-up (graph capture)
            best = {on: [0.0, 1e30] for on in models}
            for _ in range(args.reps):                 # the two alternate
                for on, m in models.items():
                    p, d = once(m, torch, prompts)
                    best[on] = [max(best[on][0], p), min(best[on][1], d)]
            n = {on: launches_per_step(m, B) for on, m in models.items()}
            for m in models.values():
                m.close()
            line = (f"{name} B={B} ctx={CTX}: decode ms/step qk_norm {best[True][1]:7.3f} none {best[False][1]:7.3f} (ratio "
                    f"{best[True][1] / best[False][1]:.3f}) | launches/step qk_norm {n[True]} none {n[False]} ({'equal' if n[True] == n[False] else 'DIFFER'})")
            if B == 32:
                line += f" | prefill 32x{CTX} tok/s qk_norm {best[True][0]:9.1f} none {best[False][0]:9.1f}"
            print(line, flush=True)
    # head_dim 64: the norm is not fused into the decode kernel: one launch per attention layer more
    cfg = dict(SHAPES["qwen3-0.6b"], head_dim=64, max_seq_len=CTX + GEN + 2)
    prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (8, CTX)).astype(np.int32)
    n = {}
    for on in (True, False):
        m = make(pkg, torch, bench, cfg, on, 8, 8 * CTX)
        once(m, torch, prompts)
        n[on] = launches_per_step(m, 8)
        m.close()
    ok = n[True] - n[False] == cfg["num_layers"]
    print(f"qwen3-0.6b shapes at head_dim 64, B=8: launches/step qk_norm {n[True]} none {n[False]}: difference {n[True] - n[False]} "
          f"({'one per attention layer' if ok else 'NOT one per attention layer'}, {cfg['num_layers']} layers)", flush=True)


if __name__ == "__main__":
    main()
