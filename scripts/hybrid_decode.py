"""Decode time of a hybrid (Mamba2 + attention) model with the convolution window carried across calls
against the default, on the Granite-4-like geometry of scripts/hybrid_prefill.py (Mamba2 head_dim 64, state 128, conv_dim
2304; 7 of 8 layers Mamba2), seeded random weights.  Three modes: off (mamba_conv_state="per_call": the parent's path), on
with nvl_set_tuning key 39 = 1 (mamba_conv_step_kernel: one launch per layer) and on with key 39 = 0 (conv kernel + tail
kernel).  Per batch B = 1, 8, 32: B x (512 prompt tokens, not timed + 128 generated tokens of the fused greedy decode loop),
ms per step, the modes alternating in one process, best and worst of the repeats (the worst shows the run-to-run spread);
every change of the key starts a new tuning epoch, so each timed loop follows an untimed one that re-captures the graphs.
Then one profiled (eager) decode loop per mode gives the mamba_conv site's microseconds per launch and launches per step
(nvl_get_kernel_stats).

    python scripts/hybrid_decode.py [--batches 1,8,32] [--reps 5]"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
MODES = {"off": ("per_call", 1), "on, key 39 = 1": ("carried", 1), "on, key 39 = 0": ("carried", 0)}
BASE = "off"


def decode(pkg, model, key39, prompts, G):
    pkg.lib().nvl_set_tuning(39, key39)
    ids = list(range(len(prompts)))
    best = None
    for it in range(2):                               # (first pass untimed: graph capture in the new tuning epoch)
        for i in ids:
            model.seq_reset(i)
        _, first = model.forward_batch(ids, prompts, [0] * len(ids), want_logits=False)
        t0 = time.perf_counter()
        toks = model.decode_greedy(ids, first, G)     # (returns after the last step's ids are on the host)
        best = 1e3 * (time.perf_counter() - t0) / G
    return best, toks


def conv_site(pkg, model, key39, prompts, G):
    pkg.lib().nvl_set_tuning(39, key39)
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    _, first = model.forward_batch(ids, prompts, [0] * len(ids), want_logits=False)
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(ids, first, G)
    st = {k["site"]: k for k in model.kernel_stats() if k["phase"] == "decode"}
    model.set_profile(False)
    c = st["mamba_conv"]
    return 1e3 * c["ms"] / c["launches"], c["launches"] / G, 1e3 * c["ms"] / G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=128)
    args = ap.parse_args()
    pkg = importlib.import_module("nano-vllm-go_amd")
    S, G = args.prompt, args.gen
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches)
    cfg = pkg.synth.tiny_config("granite_hybrid", hidden=1024, ffn_dim=2048, num_heads=16, num_kv_heads=4, vocab_size=32000, num_layers=8,
                                max_seq_len=4096, mamba_expand=2, mamba_num_heads=32, mamba_head_dim=64, mamba_state_size=128, mamba_n_groups=1,
                                hybrid_layers=["mamba"] * 3 + ["attention"] + ["mamba"] * 4)
    w = pkg.synth.make_weights(cfg, seed=1, scale=0.02)
    models = {state: pkg.HipTransformerModel(cfg, w, precision="bf16", max_seqs=Bmax, max_batch_tokens=min(Bmax * S, 16384), mamba_conv_state=state)
              for state in ("per_call", "carried")}
    n_mamba = cfg["hybrid_layers"].count("mamba")
    print(f"hybrid decode: hidden 1024, 8 layers ({n_mamba} Mamba2: 32 heads x 64, state 128, K 4, conv_dim 2304), bf16, random weights", flush=True)
    for B in batches:
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).tolist()
        ms = {mode: [] for mode in MODES}
        toks = {}
        for _ in range(args.reps):                     # the modes alternate
            for mode, (state, key39) in MODES.items():
                t, toks[mode] = decode(pkg, models[state], key39, prompts, G)
                ms[mode].append(t)
        site = {mode: conv_site(pkg, models[state], key39, prompts, G) for mode, (state, key39) in MODES.items()}
        print(f"B={B} prompt={S} gen={G} reps={args.reps}", flush=True)
        for mode in MODES:
            us, per_step, us_step = site[mode]
            print(f"    {mode:15s} decode ms/step best {min(ms[mode]):7.4f} worst {max(ms[mode]):7.4f} (best / best of {BASE}: {min(ms[mode]) / min(ms[BASE]):.4f})"
                  f"  mamba_conv site, eager: {us:6.2f} us per launch, {per_step:4.1f} launches per step, {us_step:7.2f} us per step"
                  f"  greedy ids equal to 'on, key 39 = 1': {float((toks[mode] == toks['on, key 39 = 1']).mean()):.3f}", flush=True)
    pkg.lib().nvl_set_tuning(39, 1)
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
