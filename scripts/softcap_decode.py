"""Attention logit soft-capping on against off: a Gemma-2-9B-like block geometry on the Llama path with
random weights (hidden 3584, 16 heads over 8 kv heads of 256, ffn 14336: scripts/hd256_decode.py's) or its head_dim 128 twin,
cap 50 against none.  One process per invocation, the two models alternating, best of --reps.  Prints decode ms/step and the
attention site of one profiled decode step (us per launch) for every --batch at one --ctx, or with --prefill the prefill
tok/s at 8 x 512.  A whole measurement is one invocation per step, each under its own time limit, chained so that trouble
ends it:

    for hd in 256 128; do for ctx in 512 4096; do
      timeout -k 10 300 python scripts/softcap_decode.py --hd $hd --ctx $ctx || exit 1
    done; timeout -k 10 300 python scripts/softcap_decode.py --hd $hd --prefill || exit 1; done"""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from hd256_decode import TWINS, attention_site, decode, make, prefill  # noqa: E402
from sliding_window_decode import load_bench  # noqa: E402

CAPS = {"cap50": 50.0, "none": 0.0}


def models_of(pkg, torch, bench, cfg, B, tokens):
    out = {}
    for name, cap in CAPS.items():      # (the cap is set between create and finalize: make() finalizes, so through the config)
        out[name] = make(pkg, torch, bench, dict(cfg, attn_logit_softcap=cap), B, tokens)
        assert out[name].lib.nvl_get_attn_softcap(out[name].h) == cap
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hd", type=int, default=256, choices=sorted(TWINS))
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    base = dict(TWINS[args.hd], num_layers=args.layers)
    print(f"hidden 3584, ffn 14336, {args.layers} layers, bf16, head_dim {args.hd}; cap 50 against none; best of {args.reps}", flush=True)
    if args.prefill:
        prompts = np.random.default_rng(0).integers(0, 32000, (8, 512)).astype(np.int32)
        models = models_of(pkg, torch, bench, dict(base, max_seq_len=514), 8, 8 * 512)
        best = {k: 0.0 for k in models}
        for rep in range(args.reps + 1):                   # (the first round warms up)
            for k, m in models.items():
                t = prefill(m, torch, prompts)
                best[k] = max(best[k], t) if rep else 0.0
        print(f"hd {args.hd} prefill 8 x 512 tok/s: cap50 {best['cap50']:9.1f} none {best['none']:9.1f} (ratio {best['cap50'] / best['none']:.3f})", flush=True)
        for m in models.values():
            m.close()
        return
    ctx = args.ctx
    for B in args.batch:
        cfg = dict(base, max_seq_len=ctx + 2 * 16 + 2)
        prompts = np.random.default_rng(0).integers(0, 32000, (B, ctx)).astype(np.int32)
        models = models_of(pkg, torch, bench, cfg, B, ctx)
        for m in models.values():
            decode(m, torch, prompts)                      # warm-up (graph capture)
        best = {k: 1e30 for k in models}
        for _ in range(args.reps):                         # the two alternate
            for k, m in models.items():
                best[k] = min(best[k], decode(m, torch, prompts))
        site = {k: attention_site(m, cfg, B, ctx) for k, m in models.items()}
        ran = models["cap50"].attention_ran()
        for m in models.values():
            m.close()
        print(f"hd {args.hd} B={B:2d} ctx={ctx:4d}: decode ms/step cap50 {best['cap50']:7.3f} none {best['none']:7.3f} "
              f"(ratio {best['cap50'] / best['none']:.3f}) | attention us/launch cap50 {site['cap50'][0]:7.1f} none {site['none'][0]:7.1f} "
              f"(ratio {site['cap50'][0] / site['none'][0]:.3f}, {ran})", flush=True)


if __name__ == "__main__":
    main()
