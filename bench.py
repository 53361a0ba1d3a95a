#!/usr/bin/env python3
"""bench.py — prefill + decode tokens/s of the HIP forward path on synthetic fixed-seqlen/batch
prompts (BASELINE.json metric), with the kernel roofline and the CPU restatement beside it.

A "step" = one pass of the hot path over one batch: B sequences x S prompt tokens prefilled
(TransformerModel.ForwardWithCache at pos 0), then G greedy decode steps per sequence (the
cmd/ask generateResponse loop, argmax on the device, every step's token fed back).  `value` counts
every token the path processed (B*S + B*G) per second, summed over ranks (data parallel over
sequences: each rank owns its own sequences and KV slabs, no collective on the data path).

  python bench.py --gpus 1 --steps 3 --warmup 1
  python bench.py --gpus N ...            (starts its own N rank processes, one per GPU, before any GPU call)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (ranks given by the launcher)
  python bench.py ... --dump-outputs DIR  (also writes what the last timed step returned, as DIR/<name>.npy)

Inputs are resident in HBM before the timed region (weights uploaded, token ids are 4 bytes each).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0   # MI355X: ~2.5 PF dense bf16
HBM_PEAK_GBS = 8000.0            # 8.0 TB/s spec (6.29 TB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama-3.2-1b")
    ap.add_argument("--batch", type=int, default=32, help="sequences per GPU")
    ap.add_argument("--prompt", type=int, default=512, help="prompt tokens per sequence")
    ap.add_argument("--gen", type=int, default=128, help="decode steps per sequence")
    ap.add_argument("--decode", choices=["fused", "stepwise", "sampled"], default="fused",
                    help="fused: the G greedy steps in one nvl_decode_greedy call (token feedback on the device); "
                         "stepwise: one nvl_forward per step with the token round trip through the host; "
                         "sampled: nvl_decode_sampled — the reference runner's default SampleWithHistory(T 1, p 1, k 0, "
                         "repetition penalty 1.2) on the device each step instead of the argmax")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-prompt", type=int, default=24)
    ap.add_argument("--cpu-gen", type=int, default=8)
    ap.add_argument("--tp", action="store_true", help="all ranks form ONE tensor-parallel group (RCCL all-reduce) "
                    "and process the same batch: strong scaling, e.g. --model llama-3-8b --gpus 8 --tp")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="control-flow rehearsal of the multi-rank path on a box with ONE GPU: every rank uses device 0 and "
                         "the rendezvous/barrier/max-reduce run over gloo (the printed value is meaningless)")
    ap.add_argument("--tp-collective", choices=["p2p", "rccl"], default="p2p",
                    help="--tp: p2p = the hand-written all-reduce over peer-mapped buffers (csrc/tp_p2p.h; one-shot for decode, "
                         "reduce-scatter + all-gather for prefill, residual fused); rccl = ncclAllReduce, the comparison line")
    ap.add_argument("--tune", default="", help="nvl_set_tuning overrides, e.g. 1=2 (key=value, comma separated)")
    ap.add_argument("--launch-check", action="store_true",
                    help="no GPU work: every rank joins the rendezvous (gloo), passes the barrier / max-reduce and rank 0 "
                         "prints a line with n_gpus — the multi-rank control flow on a CPU-only machine")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(float64): prefill_next_token [B] (the argmax after each prompt) and decode_tokens [G, B] (the "
                         "token of every decode step).  Same arguments -> same weights, prompts and uniforms, so two "
                         "builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: Path, arrays: dict, suffix: str = ""):
    """Writes every array as float64 DIR/<name><suffix>.npy.  An array larger than its share of DUMP_LIMIT_BYTES is
    replaced by a fixed seeded sample of its flattened elements (<name>_sample_index.npy holds the sampled indices)."""
    out_dir.mkdir(parents=True, exist_ok=True)
    # the directory keeps itself out of version control wherever it is created (as .pytest_cache does)
    (out_dir / ".gitignore").write_text("*\n")
    share = DUMP_LIMIT_BYTES // (2 * max(1, len(arrays)))      # room for the index array of a sampled one
    for name, a in arrays.items():
        a = np.asarray(a, np.float64)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // 8, replace=False))
            np.save(out_dir / f"{name}_sample_index{suffix}.npy", idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(out_dir / f"{name}{suffix}.npy", a)


def gen_weights_on_device(pkg, cfg, model, torch, device, keep_host: bool):
    """Seeded N(0, 0.02^2) bf16 weights generated on the GPU in the checkpoint's [out,in] order and
    handed to nvl_upload_tensor by device pointer.  Returns {(slot, layer): fp32 ndarray in the
    reference's [in,out] layout} when keep_host (for the CPU baseline), else {}."""
    L = pkg._lib
    H, Lyr, V = cfg["hidden"], cfg["num_layers"], cfg["vocab_size"]
    nH, hd, F = cfg["num_heads"], cfg["head_dim"], cfg["ffn_dim"]
    at = cfg["attention_type"]
    nKV = nH if at == "mha" else (1 if at == "mqa" else cfg["num_kv_heads"])
    ln = cfg["norm_type"] == "layernorm"
    host = {}
    g = torch.Generator(device=device)

    def put(slot, layer, out_dim, in_dim=None, std=0.02, mean=0.0, seed=0):
        g.manual_seed(42 + layer * 1000 + seed)
        if in_dim is None:
            t = (torch.randn(out_dim, device=device, generator=g) * std + mean).to(torch.bfloat16).float()
            model.upload(slot, layer, t)
            if keep_host:
                host[(slot, layer)] = t.cpu().numpy()
            return
        shape = (out_dim, in_dim) if isinstance(out_dim, int) else (*out_dim, in_dim)
        t = (torch.randn(*shape, device=device, generator=g) * std).to(torch.bfloat16)
        if slot in ("tok_emb", "pos_emb", "moe_in", "moe_out"):
            model.upload(slot, layer, t)
            if keep_host:
                host[(slot, layer)] = t.float().cpu().numpy()
        else:
            model.upload(slot, layer, t, layout=L.LAYOUT_OUT_IN)
            if keep_host:
                host[(slot, layer)] = t.float().t().contiguous().cpu().numpy()
        del t

    put("tok_emb", 0, V, H, seed=1)
    if cfg["position_type"] == "learned":
        put("pos_emb", 0, cfg["max_seq_len"], H, seed=2)
    if not cfg.get("tied_embedding", False):
        put("lm_head", 0, V, H, seed=3)
    put("final_norm_w", 0, H, mean=1.0, seed=4)
    if ln:
        put("final_norm_b", 0, H, seed=5)
    for li in range(Lyr):
        put("attn_norm_w", li, H, mean=1.0, seed=10)
        if ln:
            put("attn_norm_b", li, H, seed=11)
        if cfg["block_style"] == "sequential":
            put("ffn_norm_w", li, H, mean=1.0, seed=12)
            if ln:
                put("ffn_norm_b", li, H, seed=13)
        put("wq", li, nH * hd, H, seed=20)
        if at == "mqa":
            put("wkv", li, 2 * hd, H, seed=21)
        else:
            put("wk", li, nKV * hd, H, seed=22)
            put("wv", li, nKV * hd, H, seed=23)
        put("wo", li, H, nH * hd, seed=24)
        if at == "mha":
            for b, n, s in (("bq", nH * hd, 30), ("bk", nKV * hd, 31), ("bv", nKV * hd, 32), ("bo", H, 33)):
                put(b, li, n, seed=s)
        if cfg.get("use_moe", False):
            E = cfg["num_experts"]
            put("router", li, E, H, std=0.5, seed=40)
            put("moe_in", li, (E, 2 * F), H, seed=41)
            put("moe_out", li, (E, H), F, seed=42)
        else:
            put("w1", li, 2 * F if cfg["activation_type"] == "swiglu" else F, H, seed=50)
            put("w2", li, H, F, seed=51)
    return host


def flops_per_token(cfg):
    """GEMM FLOPs per token for the layer stack, and for one LM-head row."""
    H, L, V = cfg["hidden"], cfg["num_layers"], cfg["vocab_size"]
    nH, hd, F = cfg["num_heads"], cfg["head_dim"], cfg["ffn_dim"]
    at = cfg["attention_type"]
    nKV = nH if at == "mha" else (1 if at == "mqa" else cfg["num_kv_heads"])
    if cfg.get("use_moe"):
        ffn = cfg["num_experts_per_tok"] * 3 * H * F + H * cfg["num_experts"]
    else:
        ffn = (3 if cfg["activation_type"] == "swiglu" else 2) * H * F
    p_layer = H * nH * hd + 2 * H * nKV * hd + nH * hd * H + ffn
    return 2.0 * L * p_layer, 2.0 * H * V


def main():
    args = parse()
    pkg = importlib.import_module("nano-vllm-go_amd")        # (ctypes declarations only: no HIP call yet)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plainly with --gpus N: become the launcher.  N fresh rank processes (one per GPU) are started BEFORE
        # this process makes any GPU call; it never turns into a rank and never execs.
        sys.exit(pkg.dist.launch_local_ranks([str(Path(__file__).resolve()), *sys.argv[1:]], args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch  # plumbing: device RNG for the synthetic weights, barrier/max-reduce across ranks
    import torch.distributed as dist

    if args.launch_check:
        if world > 1:
            pkg.dist.init("gloo")
            dist.barrier()
        t = pkg.dist.max_over_ranks([float(rank + 1)])
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "max_rank_plus_1": t[0]}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if args.rehearse_on_one_gpu:
        local_rank = 0
    assert pkg.lib().nvl_device_count() > local_rank, "bench.py needs a GPU: the HIP path has no CPU fallback"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        pkg.dist.init("gloo" if args.rehearse_on_one_gpu else "nccl", None if args.rehearse_on_one_gpu else device)

    for kv in filter(None, args.tune.split(",")):
        k, v = kv.split("=")
        pkg.lib().nvl_set_tuning(int(k), int(v))
    cfg = dict(pkg.synth.FULL_CONFIGS[args.model])
    B, S, G = args.batch, args.prompt, args.gen
    assert S + G <= cfg["max_seq_len"]
    max_batch_tokens = min(B * S, 16384)
    tp = args.tp
    model = pkg.HipTransformerModel(cfg, None, device=local_rank, precision=args.precision, max_seqs=B,
                                    max_batch_tokens=max_batch_tokens, tp_rank=rank if tp else 0,
                                    tp_size=world if tp else 1, tp_force_single=tp and world == 1)
    want_cpu = (rank == 0 and world == 1 and not args.no_cpu_baseline)
    t0 = time.time()
    host_w = gen_weights_on_device(pkg, cfg, model, torch, device, keep_host=want_cpu)
    model.finalize()
    if tp and (args.tp_collective == "rccl" or world == 1) and not args.rehearse_on_one_gpu:
        # rank 0 creates the RCCL unique id, every rank joins (collective)
        uid = [pkg.HipTransformerModel.tp_unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(uid, src=0)
        model.tp_init(uid[0])
    elif tp:
        # direct peer stores: every rank exports the IPC handle of its comm buffer, all ranks attach all of them
        # (on the one-GPU rehearsal both ranks live on device 0: RCCL refuses two ranks on one device, this path does not)
        handles = [None] * world
        dist.all_gather_object(handles, model.tp_p2p_export())
        model.tp_p2p_attach(handles)
    t_load = time.time() - t0

    # seed 1234 + cfg_idx; data parallel: +rank (own sequences); tensor parallel: same batch on all ranks
    rng = np.random.default_rng(1234 + 1 + (0 if tp else rank))
    prompts = rng.integers(0, cfg["vocab_size"], (B, S)).astype(np.int32)
    seq_ids = list(range(B))
    seqs_per_call = max(1, max_batch_tokens // S)
    sample_u = rng.random((G, B)).astype(np.float32)

    def one_step(profile_prefill: bool, profile_decode: bool = False):
        """prefill all B prompts, then G decode steps; returns (prefill_s, decode_s, {name: what the caller received})."""
        for sid in seq_ids:
            model.seq_reset(sid)
        torch.cuda.synchronize()
        t_a = time.perf_counter()
        model.set_profile(profile_prefill)
        nxt = np.empty(B, np.int32)
        for b0 in range(0, B, seqs_per_call):
            ids = seq_ids[b0:b0 + seqs_per_call]
            _, am = model.forward_batch(ids, [prompts[i] for i in ids], [0] * len(ids), want_logits=False)
            nxt[b0:b0 + len(ids)] = am
        prefill_tok = nxt.copy()
        model.set_profile(profile_decode)
        t_b = time.perf_counter()
        if args.decode == "fused":
            dec = model.decode_greedy(seq_ids, nxt, G)
        elif args.decode == "sampled":
            hist = [np.concatenate([prompts[i], nxt[i:i + 1]]) for i in range(B)]
            dec = model.decode_sampled(seq_ids, nxt, G, hist, sample_u)
        else:
            steps = []
            for g in range(G):
                _, am = model.forward_batch(seq_ids, [[int(t)] for t in nxt], [S + g] * B, want_logits=False)
                nxt = am
                steps.append(am)
        t_c = time.perf_counter()
        model.set_profile(False)
        if args.decode == "stepwise":
            dec = np.stack(steps) if steps else np.empty((0, B), np.int32)
        outputs = {"prefill_next_token": prefill_tok, "decode_tokens": dec}
        return t_b - t_a, t_c - t_b, outputs

    for _ in range(args.warmup):
        one_step(False)
    model.reset_stats()

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    sync_all()
    t_start = time.perf_counter()
    pre_s = dec_s = 0.0
    for _ in range(args.steps):
        p, d, last_outputs = one_step(True)
        pre_s += p
        dec_s += d
    sync_all()
    elapsed = time.perf_counter() - t_start
    elapsed, pre_s, dec_s = pkg.dist.max_over_ranks([elapsed, pre_s, dec_s],
                                                    device="cpu" if args.rehearse_on_one_gpu else device)
    st = model.stats()
    if args.dump_outputs and (rank == 0 or not tp):       # tensor parallel: every rank holds the same tokens
        dump_outputs(Path(args.dump_outputs), last_outputs, "" if rank == 0 else f"_rank{rank}")
    # Per-kernel view: ONE more step of the same workload AFTER the timed region with HIP events around every launch of
    # both phases (events in the decode loop would cost the timed value a few percent).  nvl_get_kernel_stats: per
    # launch site, launches, device time and algorithmic work.
    kernels = []
    if rank == 0 or tp:                  # (a tensor-parallel group steps together: every rank runs the extra step)
        model.reset_stats()
        one_step(True, True)
    if rank == 0:
        ks = model.kernel_stats()
        tot_ms = sum(k["ms"] for k in ks) or 1.0
        for k in sorted(ks, key=lambda k: -k["ms"]):
            if k["ms"] / tot_ms < 0.004:
                continue
            us = 1e3 * k["ms"] / k["launches"]
            tf = k["flops"] / (k["ms"] * 1e-3) / 1e12 if k["ms"] > 0 else 0.0
            gbs = k["bytes"] / (k["ms"] * 1e-3) / 1e9 if k["ms"] > 0 else 0.0
            mfma_bound = k["phase"] == "prefill" and k["site"] in ("qkv_proj", "o_proj", "ffn_up", "ffn_down", "attention",
                                                                   "moe_up", "moe_down", "lm_head") and tf / MFMA_BF16_PEAK_TFLOPS > gbs / HBM_PEAK_GBS
            e = {"site": k["site"], "phase": k["phase"], "launches": k["launches"], "avg_launch_us": round(us, 2),
                 "share_of_step": round(k["ms"] / tot_ms, 4), "bound": "mfma" if mfma_bound else "hbm",
                 "flops_per_launch": round(k["flops"] / k["launches"]), "bytes_per_launch": round(k["bytes"] / k["launches"]),
                 "achieved_tflops": round(tf, 1), "achieved_gbs": round(gbs, 1)}
            e["frac"] = round(tf / MFMA_BF16_PEAK_TFLOPS if mfma_bound else gbs / HBM_PEAK_GBS, 4)
            kernels.append(e)

    tokens_per_step = B * S + B * G
    nrep = 1 if tp else world          # tensor parallel: ONE batch for the whole group
    value = nrep * tokens_per_step * args.steps / elapsed
    body, head = flops_per_token(cfg)
    gemm_tflops = st["gemm_flops"] / (st["gemm_ms"] * 1e-3) / 1e12 if st["gemm_ms"] > 0 else 0.0
    # decode step: every weight byte is read once per step (algorithmic bytes), KV on top
    wbytes = (body / 2 + head / 2) * (2 if args.precision == "bf16" else 4)
    at = cfg["attention_type"]
    nKV = cfg["num_heads"] if at == "mha" else (1 if at == "mqa" else cfg["num_kv_heads"])
    kv_bytes = 2 * cfg["num_layers"] * nKV * cfg["head_dim"] * (S + G / 2) * 2 * B
    dec_gbs = (wbytes + kv_bytes) * G * args.steps / dec_s / 1e9

    # HBM-side traffic of the dominant kernel class comes from separate rocprofv3 --pmc passes (FETCH_SIZE x2 on
    # gfx950 + WRITE_SIZE; scripts/pmc_traffic.py), committed under profiles/ — it cannot be sampled from inside
    # this process.  null when the profile is absent or was taken on another workload.
    # The file is used only if it was taken on THIS kernel source (hash of csrc/*.h, *.hip recorded by
    # scripts/pmc_traffic_r02.py) and on this workload; otherwise traffic is null.
    traffic, traffic_note, site_traffic = None, "no PMC profile for this kernel source / workload", {}
    try:
        import hashlib
        h = hashlib.sha256()
        cdir = ROOT / "nano-vllm-go_amd" / "csrc"
        for fn in sorted(os.listdir(cdir)):
            if fn.endswith((".h", ".hip")):
                h.update(fn.encode()); h.update((cdir / fn).read_bytes())
        pmc_files = sorted((ROOT / "profiles").glob("r[0-9][0-9]_pmc_traffic.json"), reverse=True)     # newest round first
        pmc_name = f"profiles/{pmc_files[0].name}"
        pmc = json.load(open(pmc_files[0]))
        if pmc.get("kernel_src_sha16") != h.hexdigest()[:16]:
            traffic_note = f"{pmc_name} was taken on a different kernel source: refused"
        elif not (args.model == "llama-3.2-1b" and (B, S) == (32, 512) and args.precision == "bf16" and not tp):
            traffic_note = f"{pmc_name} is for llama-3.2-1b 32 x 512 bf16: refused for this workload"
        else:
            site_traffic = {k: round(v["hbm_bytes_per_launch"]) for k, v in pmc["sites"].items()}
            gs = [v for k, v in pmc["sites"].items() if k in ("prefill/qkv_proj", "prefill/o_proj", "prefill/ffn_up", "prefill/ffn_down")]
            traffic = round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in gs) / max(1, sum(v["launches"] for v in gs)))
            traffic_note = ("bytes/launch past L2 (Infinity-Cache hits included), prefill projection class, "
                            f"{pmc_name} (same kernel source hash)")
    except Exception as e:      # noqa: BLE001
        traffic, site_traffic = None, {}
        traffic_note = f"no usable PMC profile ({type(e).__name__})"
    for e in kernels:
        e["traffic"] = site_traffic.get(f"{e['phase']}/{e['site']}")

    out = {
        "metric": "prefill + decode tokens/sec, Llama-3.2-1B bf16, 1/2/4/8 MI355X",
        "value": round(value, 1), "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "strong" if tp else "weak",
        "vs_baseline": None, "dtype": args.precision, "data": "synthetic (seeded random weights at the model's "
        "shapes, uniform random token ids)",
        "config": {"workload": f"{args.model}: {B} seqs/GPU x {S} prompt tokens prefill + {G} greedy decode steps ({args.decode})",
                   "batch_per_gpu": B, "prompt_len": S, "gen_len": G, "parallelism": (f"tp{world} (column/row-parallel, " + ("RCCL all-reduce)" if (args.tp_collective == "rccl" or world == 1) and not args.rehearse_on_one_gpu
                                                                                     else "P2P all-reduce over peer-mapped buffers)") if tp else f"dp{world} over sequences")},
        "prefill_tokens_per_s": round(nrep * B * S * args.steps / pre_s, 1),
        "decode_tokens_per_s": round(nrep * B * G * args.steps / dec_s, 1),
        "roofline": {"bound": "mfma", "kernel": "gemm_bf16_pp_kernel (prefill QKV/O/FFN projections; gemm_bf16_kernel for the small LM-head GEMM)",
                     "achieved": round(gemm_tflops, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(gemm_tflops / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
                     "traffic_note": traffic_note,
                     "launches": int(st["gemm_launches"]),
                     "avg_launch_us": round(1e3 * st["gemm_ms"] / max(1, st["gemm_launches"]), 2)},
        "decode_roofline": {"bound": "hbm", "achieved": round(dec_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(dec_gbs / HBM_PEAK_GBS, 4),
                            "note": "algorithmic weight+KV bytes per decode step / wall time per step"},
        "kernels": kernels,
        "kernels_note": "per launch site, from ONE extra profiled step after the timed region (HIP events around every launch on the "
                        "library's stream; avg_launch_us is the event INTERVAL, which includes the bracket itself — about 2-3 us on this box, "
                        "so the entries of 5-20 us decode kernels understate their rates; rocprofv3's per-kernel durations of the same "
                        "command are in profiles/r03_bench_kernel_stats.csv / r03_phase_breakdown_b32.txt); work = algorithmic flops / bytes (weights once + operands + results; attention: every cached "
                        "K/V once); frac vs 2.5 PFLOP/s (mfma) or 8 TB/s (hbm)",
        "dominant_by_time": (max(kernels, key=lambda e: e["share_of_step"]) if kernels else None),
        "load_s": round(t_load, 1),
    }

    if want_cpu:
        from oracle import purego_oracle as O   # cpu_baseline leg only: the checker timed as the CPU reference
        om = O.OracleModel(cfg, host_w)
        cp, cg = args.cpu_prompt, args.cpu_gen
        t1 = time.perf_counter()
        kv = om.new_cache()
        toks = list(map(int, prompts[0, :cp]))
        lg = om.forward_with_cache(toks, kv, 0)
        nxt = O.argmax(lg[-1])
        first_cpu = nxt
        for i in range(cg):
            toks.append(nxt)
            lg = om.forward_with_cache([nxt], kv, len(toks) - 1)
            nxt = O.argmax(lg[-1])
        cpu_s = time.perf_counter() - t1
        # same prompt through the HIP path: first greedy token agrees (reported, not asserted here)
        model.seq_reset(0)
        _, am = model.forward_batch([0], [prompts[0, :cp]], [0], want_logits=False)
        out["cpu_baseline"] = {
            "value": round((cp + cg) / cpu_s, 3), "unit": "tokens/s", "cores": 1,
            "host_cores_available": os.cpu_count(), "kind": "port",
            "sample": f"C restatement of the purego path (not the Go binary), 1 thread: {args.model}, 1 sequence, "
                      f"{cp} prompt tokens prefill + {cg} decode steps, {cpu_s:.1f} s",
            "first_token_matches_gpu": bool(int(am[0]) == int(first_cpu)),
        }
    if rank == 0:
        print(json.dumps(out), flush=True)
    model.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
