"""Decode attention over a bf16 cache against an 8-bit (e4m3fn) cache, one sequence, through the op entry points
(nvl_op_attention / nvl_op_attention_kv8) with the key split off in both: run it under
`rocprofv3 --kernel-trace --stats -- python scripts/kv8_attn_compare.py` and compare attn_decode_bf16_kernel with
attn_decode_kv8_kernel per shape (the op calls' own uploads are separate kernels)."""
import importlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("nano-vllm-go_amd")
L = pkg.lib()
old = L.nvl_set_tuning(25, 0)             # no key split (the bf16 op has no split scratch)
try:
    for nH, nKV, T, hd, reps in ((32, 8, 4096, 64, 10), (32, 8, 16384, 64, 5), (32, 8, 8192, 128, 5)):
        r = np.random.default_rng(T)
        q = r.standard_normal((nH, 1, hd), dtype=np.float32)
        k = r.standard_normal((nKV, T, hd), dtype=np.float32)
        v = r.standard_normal((nKV, T, hd), dtype=np.float32)
        for _ in range(reps):
            a = pkg.ops.attention(q, k, v, precision="bf16")
            b = pkg.ops.attention_kv8(q, k, v)
        print(f"nH={nH} nKV={nKV} T={T} hd={hd}: max |kv8 - bf16| / max |bf16| = {np.abs(a - b).max() / np.abs(a).max():.3e}")
finally:
    L.nvl_set_tuning(25, old)
