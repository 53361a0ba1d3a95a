"""Decode and prefill at head_dim 256 beside the same model at head_dim 128: a Gemma-2-9B-like block
geometry on the Llama path with random weights (hidden 3584, 16 heads over 8 kv heads of 256, ffn 14336) against its twin with
32 heads over 16 kv heads of 128 — equal KV bytes, equal FLOPs, equal weights.  One process, the two alternating, best of
--reps.  Prints decode ms/step at B = 1 / 8 / 32 with contexts 512 and 4096, the attention site of one profiled decode step
(us per launch, and the K/V bytes of the batch over that time), and prefill tok/s at 8 x 512.  bench.py's seeded weights
(gen_weights_on_device) are reused.

    python scripts/hd256_decode.py [--layers 42] [--reps 5]"""
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

COMMON = dict(vocab_size=32000, hidden=3584, ffn_dim=14336, attention_type="gqa", norm_type="rmsnorm", position_type="rope",
              activation_type="swiglu", block_style="sequential", rope_base=10000.0, norm_eps=1e-6, tied_embedding=True)
TWINS = {256: dict(COMMON, num_heads=16, num_kv_heads=8, head_dim=256), 128: dict(COMMON, num_heads=32, num_kv_heads=16, head_dim=128)}
GEN = 16


def make(pkg, torch, bench, cfg, B, tokens):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B, max_batch_tokens=tokens)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    return model


def fill(model, prompts):
    """every sequence's context, one prefill call per sequence -> the first generated ids"""
    first = []
    for i, p in enumerate(prompts):
        model.seq_reset(i)
        first.append(model.forward_batch([i], [p], [0], want_logits=False)[1][0])
    return np.asarray(first, np.int32)


def decode(model, torch, prompts):
    ids, first = list(range(len(prompts))), fill(model, prompts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.decode_greedy(ids, first, GEN)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / GEN


def attention_site(model, cfg, B, ctx):
    """one profiled decode step behind the timed ones -> (us per attention launch, K/V bytes of the batch per second)"""
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(list(range(B)), np.zeros(B, np.int32), 1)
    s = model.stats()
    model.set_profile(False)
    us = 1e3 * s["attn_ms"] / max(int(s["attn_launches"]), 1)
    return us, B * (ctx + GEN) * 2.0 * cfg["num_kv_heads"] * cfg["head_dim"] * 2 / (us * 1e-6)


def prefill(model, torch, prompts):
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.forward_batch(ids, list(prompts), [0] * len(ids), want_logits=False)
    torch.cuda.synchronize()
    return prompts.size / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    print(f"hidden 3584, ffn 14336, {args.layers} layers, bf16; hd 256: 16 heads / 8 kv heads; hd 128: 32 / 16; best of {args.reps}", flush=True)
    for ctx in (512, 4096):
        for B in (1, 8, 32):
            cfgs = {hd: dict(c, num_layers=args.layers, max_seq_len=ctx + 2 * GEN + 2) for hd, c in TWINS.items()}
            prompts = np.random.default_rng(0).integers(0, 32000, (B, ctx)).astype(np.int32)
            models = {hd: make(pkg, torch, bench, cfgs[hd], B, ctx) for hd in cfgs}
            for m in models.values():
                decode(m, torch, prompts)              # warm-up (graph capture)
            best = {hd: 1e30 for hd in models}
            for _ in range(args.reps):                 # the two alternate
                for hd, m in models.items():
                    best[hd] = min(best[hd], decode(m, torch, prompts))
            site = {hd: attention_site(m, cfgs[hd], B, ctx) for hd, m in models.items()}
            ran = {hd: m.attention_ran() for hd, m in models.items()}
            for m in models.values():
                m.close()
            print(f"B={B:2d} ctx={ctx:4d}: decode ms/step hd256 {best[256]:7.3f} hd128 {best[128]:7.3f} (ratio {best[256] / best[128]:.3f}) | "
                  f"attention us/launch hd256 {site[256][0]:7.1f} ({site[256][1] / 1e9:6.1f} GB/s, {ran[256]}) "
                  f"hd128 {site[128][0]:7.1f} ({site[128][1] / 1e9:6.1f} GB/s, {ran[128]})", flush=True)
    cfgs = {hd: dict(c, num_layers=args.layers, max_seq_len=514) for hd, c in TWINS.items()}
    prompts = np.random.default_rng(0).integers(0, 32000, (8, 512)).astype(np.int32)
    models = {hd: make(pkg, torch, bench, cfgs[hd], 8, 8 * 512) for hd in cfgs}
    best = {hd: 0.0 for hd in models}
    for rep in range(args.reps + 1):                   # (the first round warms up)
        for hd, m in models.items():
            t = prefill(m, torch, prompts)
            best[hd] = max(best[hd], t) if rep else 0.0
    print(f"prefill 8 x 512 tok/s: hd256 {best[256]:9.1f} hd128 {best[128]:9.1f} (ratio {best[256] / best[128]:.3f})", flush=True)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
