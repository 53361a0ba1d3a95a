"""One SHA-256 per case of a fixed-seed list of attention shapes: did a change to the attention kernels move any bit?

Run it with two builds of the library (NVLLM_LIB selects another build, one process per build) and diff the outputs:
identical digests for every case mean the outputs are byte-identical.  The cases reach every piece the bf16 and the 8-bit
-cache kernels share (attn.h): both head sizes, groups of 1, 4 and 71 query heads (71: five query tiles, the last one
partial), decode at tile-boundary context lengths with 2, 4 and 8 waves, the key split on and off, both K/V load policies,
prefill across a 256-row workgroup, the causal diagonal and whole tiles, a chunked prefill, and a short model decode
(slab and paged, bf16 and 8-bit cache) for the fused decode kernel and the key split of the bf16 kernel."""
import hashlib
import importlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("nano-vllm-go_amd")
L = pkg.lib()


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


class tuning:
    """nvl_set_tuning keys for the duration of a block"""

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: L.nvl_set_tuning(k, v) for k, v in self.kv.items()}

    def __exit__(self, *exc):
        for k, v in self.old.items():
            L.nvl_set_tuning(k, v)


def op_case(name, nH, nKV, S, T, hd):
    r = np.random.default_rng(nH * 100003 + nKV * 1009 + S * 131 + T * 7 + hd)
    q = r.standard_normal((nH, S, hd), dtype=np.float32)
    k = r.standard_normal((nKV, T, hd), dtype=np.float32)
    v = r.standard_normal((nKV, T, hd), dtype=np.float32)
    emit(f"{name} bf16", pkg.ops.attention(q, k, v, precision="bf16"))
    emit(f"{name} kv8", pkg.ops.attention_kv8(q, k, v, k_scale=0.37, v_scale=2.5))


GROUPS = ((2, 2), (8, 2), (71, 1))          # (query heads, kv heads): groups of 1, 4 and 71

for hd in (64, 128):
    for nH, nKV in GROUPS:
        g = f"hd{hd} g{nH // nKV}"
        for T, nw in ((1, 2), (64, 2), (65, 4), (200, 4), (200, 8), (600, 2), (600, 8)):      # decode, waves forced (key 15)
            with tuning(k15=nw):
                op_case(f"decode {g} T{T} nw{nw}", nH, nKV, 1, T, hd)
        for kv_nt in (0, 2):                                                                  # K/V load policy (key 35)
            with tuning(k35=kv_nt):
                op_case(f"decode {g} T600 kv_nt{kv_nt}", nH, nKV, 1, 600, hd)
        for split in (1, 0):                                  # >= 1024 keys, one sequence: the key split (key 25) on and off
            with tuning(k25=split):
                op_case(f"decode {g} T1100 split{split}", nH, nKV, 1, 1100, hd)
        for S, T in ((1, 1), (63, 63), (65, 65), (300, 300), (65, 165)):                     # prefill; (65, 165): chunked, pos0 = 100
            op_case(f"prefill {g} S{S} T{T}", nH, nKV, S, T, hd)

# a short model decode: the fused (RoPE + append) bf16 kernel, the 8-bit cache's writer + kernels, and with 1040 keys in
# one sequence the key split of both, slab and paged (256-key blocks)
for hd in (64, 128):
    over = dict(max_seq_len=1280) if hd == 64 else dict(max_seq_len=1280, head_dim=128, num_heads=2, num_kv_heads=1)
    cfg = pkg.synth.tiny_config("llama", **over)
    w = pkg.synth.make_weights(cfg, seed=5, scale=0.05)
    prompt = np.random.default_rng(hd).integers(0, cfg["vocab_size"], 1040).tolist()
    for kv in ("auto", "fp8_e4m3"):
        for paged in (False, True):
            for split in (1, 0):
                kw = dict(kv_num_blocks=8, kv_block_size=256) if paged else {}
                hm = pkg.HipTransformerModel(cfg, w, precision="bf16", max_seqs=2, max_batch_tokens=512, kv_cache_dtype=kv,
                                             kv_scales=(0.5, 1.5) if kv != "auto" else None, **kw)
                table = [[5, 2, 7, 0, 3]]
                if not paged:
                    hm.seq_reset(0)
                out = []
                with tuning(k25=split):
                    for pos in range(0, len(prompt), 512):                 # chunked prefill, then five decode steps
                        chunk = prompt[pos:pos + 512]
                        lg, am = (hm.forward_paged([chunk], [pos], table) if paged
                                  else hm.forward_batch([0], [chunk], [pos]))
                        out.append(lg.copy())
                    pos = len(prompt)
                    for _ in range(5):
                        tok = [[int(am[0])]]
                        lg, am = hm.forward_paged(tok, [pos], table) if paged else hm.forward_batch([0], tok, [pos])
                        out.append(lg.copy())
                        pos += 1
                hm.close()
                emit(f"model hd{hd} kv={kv} {'paged' if paged else 'slab'} split{split}", *out)
