"""Decode and prefill cost of sliding-window attention (sliding_window=W) against the same build without
a window: Mistral-7B shapes (32 heads, 8 kv heads, hd 128, hidden 4096, ffn 14336, 32 layers) with random weights at
B = 1, 8, 32 and contexts 4096, 8192, 16384, W = 4096 against W = 0 in one process.  The cache is filled by chunked
prefill, then the fused greedy decode loop runs --gen steps; the two models alternate, each point repeated, and the best of
the repeats is reported as decode ms/step; one profiled decode pass per model gives the attention site's time per launch
(nvl_get_kernel_stats).  The 8 x 8192 point also reports prefill tok/s.  The 16384 point is run at B = 1 and 8 only: at
B = 32 the two models' bf16 weights and caches come to about 170 GB, so that point is left out.
Expectations to hold the figures against: at context <= W the windowed model costs what the unwindowed one costs; beyond
it, decode attention time stops growing with the context.  bench.py's seeded weights (gen_weights_on_device) are reused;
bench.py itself is not changed or run.

    python scripts/sliding_window_decode.py [--points 1:4096,1:8192,1:16384,8:4096,8:8192,8:16384,32:4096,32:8192] [--reps 5]"""
import argparse
import importlib
import importlib.util
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
WINDOW = 4096
MISTRAL_7B = dict(vocab_size=32000, hidden=4096, num_layers=32, num_heads=32, num_kv_heads=8, head_dim=128, ffn_dim=14336,
                  attention_type="gqa", norm_type="rmsnorm", position_type="rope", activation_type="swiglu",
                  block_style="sequential", rope_base=10000.0, norm_eps=1e-5, tied_embedding=False)


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def make(pkg, torch, bench, cfg, window, B, chunk):
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=B, max_batch_tokens=B * chunk, sliding_window=window)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    return model


def once(model, torch, prompts, chunk, G):
    """chunked prefill of the whole context, then G fused decode steps -> (prefill tok/s, decode ms/step)"""
    ids = list(range(len(prompts)))
    S = prompts.shape[1]
    for i in ids:
        model.seq_reset(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(0, S, chunk):
        _, first = model.forward_batch(ids, list(prompts[:, p:p + chunk]), [p] * len(ids), want_logits=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    model.decode_greedy(ids, first, G)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return len(ids) * S / (t1 - t0), 1e3 * (t2 - t1) / G


def attention_us(model, G):
    """one more profiled decode pass from where the last one stopped: the attention site's us per launch"""
    ids = list(range(model.n_bench))
    model.set_profile(True)
    model.reset_stats()
    model.decode_greedy(ids, np.zeros(len(ids), np.int32), G)
    st = {k["site"]: k for k in model.kernel_stats() if k["phase"] == "decode"}
    model.set_profile(False)
    return 1e3 * st["attention"]["ms"] / max(1, st["attention"]["launches"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1:4096,1:8192,1:16384,8:4096,8:8192,8:16384,32:4096,32:8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gen", type=int, default=32)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    bench = load_bench()
    G = args.gen
    for point in args.points.split(","):
        B, S = (int(x) for x in point.split(":"))
        chunk = min(S, max(512, 16384 // B))
        cfg = dict(MISTRAL_7B, max_seq_len=S + 2 * G)         # (the timed steps and the profiled pass behind them)
        prompts = np.random.default_rng(0).integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
        models = {w: make(pkg, torch, bench, cfg, w, B, chunk) for w in (WINDOW, 0)}
        for m in models.values():
            m.n_bench = B
            once(m, torch, prompts, chunk, G)      # warm-up (graph capture)
        best = {w: [0.0, 1e30] for w in models}
        for _ in range(args.reps):                 # the modes alternate
            for w, m in models.items():
                p, d = once(m, torch, prompts, chunk, G)
                best[w] = [max(best[w][0], p), min(best[w][1], d)]
        us = {w: attention_us(m, G) for w, m in models.items()}
        for m in models.values():
            m.close()
        line = (f"mistral-7b B={B} ctx={S} gen={G}: decode ms/step W={WINDOW} {best[WINDOW][1]:7.3f} none {best[0][1]:7.3f}"
                f" (ratio {best[WINDOW][1] / best[0][1]:.3f}) | attention us/launch W={WINDOW} {us[WINDOW]:.1f} none {us[0]:.1f}")
        if (B, S) == (8, 8192):
            line += f" | prefill tok/s W={WINDOW} {best[WINDOW][0]:9.1f} none {best[0][0]:9.1f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
