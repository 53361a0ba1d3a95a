"""Time of a verify pass of a hybrid (Mamba2 + attention) model with nvl_set_mamba_rollback on against
a plain decode step of the same model, on the Granite-4-like geometry of scripts/hybrid_decode.py (Mamba2 head_dim 64,
state 128, conv_dim 2304; 7 of 8 layers Mamba2), seeded random weights, carried window, bf16.  Per batch B = 1, 8: B x (512
prompt tokens, not timed), then the two forms alternate, best of the repeats: `passes` verify_greedy passes of 1 + k rows
whose drafts repeat the input token (with random weights nearly all are rejected, so the context stays near 512; what is
accepted does not change the work of a pass), and a fused greedy decode loop of as many steps.  Both are graph replays
after an untimed first round.  Then one profiled (eager) round gives the launches per pass and per step and the two new
sites' microseconds (nvl_get_kernel_stats).  No acceptance rate is measured here: that needs a real checkpoint.

    python scripts/hybrid_verify.py [--batches 1,8] [--reps 5] [--k 3]"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def prefill(model, prompts):
    ids = list(range(len(prompts)))
    for i in ids:
        model.seq_reset(i)
    return ids, model.forward_batch(ids, prompts, [0] * len(ids), want_logits=False)[1]


def verify_ms(model, prompts, k, passes):
    ids, cur = prefill(model, prompts)
    t0 = time.perf_counter()
    for _ in range(passes):
        acc, out = model.verify_greedy(ids, np.repeat(cur[:, None], 1 + k, axis=1), k)
        cur = out[np.arange(len(ids)), acc]
    return 1e3 * (time.perf_counter() - t0) / passes


def step_ms(model, prompts, steps):
    ids, first = prefill(model, prompts)
    t0 = time.perf_counter()
    model.decode_greedy(ids, first, steps)
    return 1e3 * (time.perf_counter() - t0) / steps


def launches(model, prompts, k, n=8):
    """-> launches per verify pass, per decode step, and the new sites' microseconds per launch (one eager round each)"""
    out = []
    for verify in (True, False):
        ids, cur = prefill(model, prompts)
        model.set_profile(True)
        model.reset_stats()
        if verify:
            for _ in range(n):
                model.verify_greedy(ids, np.repeat(cur[:, None], 1 + k, axis=1), k)
            sites = {s["site"]: 1e3 * s["ms"] / s["launches"] for s in model.kernel_stats() if s["site"] in ("mamba_verify", "mamba_commit")}
        else:
            model.decode_greedy(ids, cur, n)
        st = model.stats()
        model.set_profile(False)
        out.append((st["gemm_launches"] + st["attn_launches"] + st["other_launches"]) / n)
    return out[0], out[1], sites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--passes", type=int, default=64)
    args = ap.parse_args()
    pkg = importlib.import_module("nano-vllm-go_amd")
    batches = [int(b) for b in args.batches.split(",")]
    cfg = pkg.synth.tiny_config("granite_hybrid", hidden=1024, ffn_dim=2048, num_heads=16, num_kv_heads=4, vocab_size=32000, num_layers=8,
                                max_seq_len=4096, mamba_expand=2, mamba_num_heads=32, mamba_head_dim=64, mamba_state_size=128, mamba_n_groups=1,
                                hybrid_layers=["mamba"] * 3 + ["attention"] + ["mamba"] * 4)
    w = pkg.synth.make_weights(cfg, seed=1, scale=0.02)
    model = pkg.HipTransformerModel(cfg, w, precision="bf16", max_seqs=max(batches), max_batch_tokens=max(batches) * args.prompt,
                                    mamba_conv_state="carried", mamba_rollback="verify")
    print(f"hybrid verify: hidden 1024, 8 layers (7 Mamba2: 32 heads x 64, state 128, K 4, conv_dim 2304), bf16, carried window, random weights, k = {args.k}", flush=True)
    for B in batches:
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, args.prompt)).tolist()
        v, s = [], []
        for rep in range(args.reps + 1):                  # the forms alternate; round 0 (capture) is not counted
            tv, ts = verify_ms(model, prompts, args.k, args.passes), step_ms(model, prompts, args.passes)
            if rep:
                v.append(tv); s.append(ts)
        lv, ls, sites = launches(model, prompts, args.k)
        print(f"B={B} context {args.prompt}: verify pass of {1 + args.k} rows best {min(v):.4f} ms worst {max(v):.4f}; decode step best {min(s):.4f} ms "
              f"worst {max(s):.4f}; pass / step {min(v) / min(s):.3f}; launches (eager): pass {lv:.1f} step {ls:.1f}; "
              + "; ".join(f"{k_} {us:.2f} us per launch" for k_, us in sorted(sites.items())), flush=True)
    model.close()


if __name__ == "__main__":
    main()
