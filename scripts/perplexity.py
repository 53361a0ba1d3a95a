"""Mean negative log-likelihood per token of one seeded synthetic Llama-3.2-1B-shaped model (bench.py's `synth` weights,
gen_weights_on_device) under every weight / KV mode, computed on the device by HipTransformerModel.score (nvl_score,
DESIGN.md §9 f-14), next to the route the library had before: forward_batch(all_logits=True) + a numpy log-softmax of the
[tokens, V] logits on the host.  The tokens are seeded random ids, each scored as the continuation of its prefix, so the
absolute figure is that of an untrained model (about log V); what the file records is the DIFFERENCE between the modes on
identical weights and tokens, and the time of the two routes for the same tokens.  bench.py itself is not changed or run.

    python scripts/perplexity.py [--batch 4] [--prompt 512] [--reps 3] [--out FILE]

Without --out the report goes to profiles/ under the next free rNN_ name."""
import argparse
import importlib
import importlib.util
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODES = {"bf16": {}, "fp8 weights": dict(weight_dtype="fp8_e4m3"), "fp8 KV": dict(kv_cache_dtype="fp8_e4m3"),
         "mxfp4 weights": dict(mx_weight_dtype="fp4_e2m1"),
         "mxfp4 weights + head": dict(mx_weight_dtype="fp4_e2m1", mx_head_dtype="fp4_e2m1")}


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def next_profile_name():
    n = max([int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)", p.name))] + [0])
    return ROOT / "profiles" / f"r{n + 1:02d}_perplexity.txt"


def host_nll(logits, tokens):
    """the all-logits route: per sequence, float32 log-softmax of [S, V] on the host, the next token's entry"""
    S = tokens.shape[1]
    nll = []
    for i in range(tokens.shape[0]):
        lg = logits[i * S:(i + 1) * S - 1]
        mx = lg.max(axis=1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(axis=1))
        nll.append(lse - lg[np.arange(S - 1), tokens[i, 1:]])
    return np.concatenate(nll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    B, S = args.batch, args.prompt
    cfg = dict(pkg.synth.FULL_CONFIGS["llama-3.2-1b"])
    tokens = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
    ids = list(range(B))
    lines = [f"llama-3.2-1b shapes, synthetic seeded weights, {B} x {S} seeded random tokens ({B * (S - 1)} scored), "
             f"V = {cfg['vocab_size']}, log V = {np.log(cfg['vocab_size']):.4f}; times: best of {args.reps}, whole call, host clock",
             f"{'mode':<22} {'mean NLL (score)':>17} {'mean NLL (all logits)':>22} {'|diff| max':>11} {'score ms':>9} {'all-logits ms':>14} "
             f"{'of it numpy':>12} {'speed-up':>9}"]
    for mode, kw in MODES.items():
        model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B, max_batch_tokens=B * S, **kw)
        bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
        model.finalize()
        t_score, t_all, t_np = [], [], []
        for rep in range(args.reps + 1):           # (first pass: warm-up, not timed)
            for i in ids:
                model.seq_reset(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp, _, _, _ = model.score(ids, list(tokens), [0] * B)
            t1 = time.perf_counter()
            for i in ids:
                model.seq_reset(i)
            t2 = time.perf_counter()
            logits, _ = model.forward_batch(ids, list(tokens), [0] * B, all_logits=True)
            t3 = time.perf_counter()
            nll_host = host_nll(logits, tokens)
            t4 = time.perf_counter()
            del logits
            if rep:
                t_score.append(t1 - t0); t_all.append(t4 - t2); t_np.append(t4 - t3)
        nll_dev = -np.concatenate([a[:-1] for a in lp]).astype(np.float64)
        model.close()
        lines.append(f"{mode:<22} {nll_dev.mean():17.5f} {nll_host.astype(np.float64).mean():22.5f} "
                     f"{np.abs(nll_dev - nll_host).max():11.2e} {1e3 * min(t_score):9.1f} {1e3 * min(t_all):14.1f} "
                     f"{1e3 * min(t_np):12.1f} {min(t_all) / min(t_score):8.1f}x")
        print(lines[-1], flush=True)
    out = Path(args.out) if args.out else next_profile_name()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
