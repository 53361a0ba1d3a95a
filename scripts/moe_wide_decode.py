"""Decode ms/step of a one-layer MoE model at Qwen3-30B-A3B block shapes (H 2048, I 768, E 128, k 8; random weights) with the
router and the expert plan as one launch (nvl_set_tuning key 31 = 2, gemm.h moe_router_plan_kernel) and as two (key 31 = 0):
same process, alternating, best of 5 windows of 200 steps after 20 warm-up steps, at B = 1 / 8 / 32.  Prints one JSON line
(profiles/moe_wide_decode.txt).  Run from the repository root on a machine with an MI355X."""
import importlib
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
pkg = importlib.import_module("nano-vllm-go_amd")
WARM, STEPS, FUSED, TWO = 20, 200, 2, 0

cfg = pkg.synth.tiny_config("llama", hidden=2048, ffn_dim=768, num_heads=16, num_kv_heads=4, head_dim=128, vocab_size=1024,
                            num_layers=1, max_seq_len=4096, use_moe=True, num_experts=128, num_experts_per_tok=8, tied_embedding=False)
hm = pkg.HipTransformerModel(cfg, pkg.synth.make_weights(cfg, seed=7, scale=0.05), precision="bf16", max_seqs=32, max_batch_tokens=256)
lib, res = pkg.lib(), {}
for B in (1, 8, 32):
    ids, r = list(range(B)), np.random.default_rng(B)
    for i in ids:
        hm.seq_reset(i)
    hm.forward_batch(ids, [r.integers(0, 1024, 4).tolist() for _ in ids], [0] * B, want_logits=False)
    pos, best = 4, {FUSED: 1e9, TWO: 1e9}
    for rep in range(5):
        for key in (FUSED, TWO):
            old = lib.nvl_set_tuning(31, key)
            toks = [[int(t)] for t in r.integers(0, 1024, B)]
            for phase in (WARM, STEPS):
                t = time.perf_counter()
                for _ in range(phase):
                    hm.forward_batch(ids, toks, [pos] * B)      # returns the logits: the step has finished
                    pos += 1
            lib.nvl_set_tuning(31, old)
            best[key] = min(best[key], (time.perf_counter() - t) / STEPS * 1e3)
    res[f"B={B}"] = dict(one_launch_ms=round(best[FUSED], 4), two_launch_ms=round(best[TWO], 4))
hm.close()
print(json.dumps(res))
