"""Greedy speculative decoding on Llama-3.2-1B shapes (random weights, bench.py's generator), context 512, B in {1, 8},
k in {1, 3, 7}: milliseconds per verify pass of 1 + k rows per sequence for three routes, timed alternately in one process,
next to milliseconds per plain step of nvl_decode_greedy:
  (a) nvl_verify_greedy, nvl_set_tuning key 38 = 1 (the multi-position decode attention)
  (b) nvl_verify_greedy, key 38 = 0 (rope_kv + the prefill attention kernel)
  (c) nvl_forward with seq_lens = 1 + k and NVL_FWD_ALL_LOGITS, the accept rule on the host
Every pass runs at the same context: the sequences are rolled back (nvl_seq_truncate) after each.
Random weights have no real-text acceptance rate, so the generation rate is reported at its two bounds: drafts that are
always right (the ids of a plain greedy run) and drafts that are always wrong.  Acceptance on real checkpoints: not measured.
bench.py's seeded weights (gen_weights_on_device) are reused; bench.py itself is not changed or run.

    python scripts/spec_decode.py [--batches 1,8] [--ks 1,3,7] [--ctx 512] [--gen 64] [--passes 32] [--reps 5]

--sampled: the same shapes under tensor.SampleWithHistory, for the default sampling parameters and for
temperature 0.8 / top_k 40 / top_p 0.95, timed alternately in one process:
  (a) one nvl_verify_sampled pass (forward of 1 + k rows, sampler with the history extension, accept kernel; replayed graph)
  (c) the host route it replaces: nvl_forward of 1 + k rows, nvl_sample with the 1 + k hand-extended histories of every
      sequence, the compare on the host, nvl_seq_truncate
next to one step of nvl_decode_sampled.  Two figures per route: wall clock per pass with the device idle before and after
(what a host loop pays, synchronisations included), and the library's own HIP-event time of the forward passes
(nvl_stats; it covers (a) whole — its sampler and accept kernel lie inside the events — and of (c) only the nvl_forward).

    python scripts/spec_decode.py --sampled --ks 3

--draft: speculative decoding with a draft MODEL.  Target: the Llama-3.2-1B shapes; draft: the same width
with 4 layers; both random, so nothing is accepted beyond chance and only times are reported: per draft phase
(nvl_draft_sampled, k steps), per verify pass (nvl_verify_speculative: forward of 1 + k rows, sampler, rejection kernel;
launched eagerly), the rejection kernel's own time from the library's per-kernel events (nvl_set_profile, site
"spec_reject"; taken in a separate run of the same passes), one step of nvl_decode_sampled on the target, and the
accepted drafts per pass from which a pass pair pays:  (draft + verify) / plain step - 1.

    python scripts/spec_decode.py --draft --ks 3"""
import argparse
import importlib
import importlib.util
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_weights", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                   # (module level only defines; main() runs under __main__)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ks", default="1,3,7")
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--gen", type=int, default=64)
    ap.add_argument("--passes", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sampled", action="store_true")
    ap.add_argument("--draft", action="store_true")
    ap.add_argument("--draft-layers", type=int, default=4)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("nano-vllm-go_amd")
    assert pkg.lib().nvl_device_count() >= 1, "no GPU: nothing here can be measured without one"
    bench = load_bench()
    cfg = dict(pkg.synth.FULL_CONFIGS["llama-3.2-1b"])
    V, S, G = cfg["vocab_size"], args.ctx, args.gen
    batches = [int(b) for b in args.batches.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
    Bmax = max(batches)
    model = pkg.HipTransformerModel(cfg, None, device=0, precision="bf16", max_seqs=Bmax, max_batch_tokens=Bmax * S)
    bench.gen_weights_on_device(pkg, cfg, model, torch, torch.device("cuda", 0), keep_host=False)
    model.finalize()
    prompts = np.random.default_rng(0).integers(0, V, (Bmax, S)).astype(np.int32)
    tune = pkg.lib().nvl_set_tuning

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if args.draft:
        dcfg = dict(cfg, num_layers=args.draft_layers)
        draft = pkg.HipTransformerModel(dcfg, None, device=0, precision="bf16", max_seqs=Bmax, max_batch_tokens=Bmax * S)
        bench.gen_weights_on_device(pkg, dcfg, draft, torch, torch.device("cuda", 0), keep_host=False)
        draft.finalize()
        draft_mode(args, model, draft, prompts, batches, ks, clock)
        draft.close()
        model.close()
        return
    if args.sampled:
        sampled_mode(args, pkg, model, prompts, batches, ks, clock)
        model.close()
        return

    for B in batches:
        ids = list(range(B))

        def prefill():
            for i in ids:
                model.seq_reset(i)
            _, am = model.forward_batch(ids, [prompts[i] for i in ids], [0] * B, want_logits=False)
            return am.copy()

        def rewind():
            for i in ids:
                model.seq_truncate(i, S)

        first = prefill()
        ref = model.decode_greedy(ids, first, G + max(ks))             # [steps, B]: the plain greedy ids (also the warm-up)
        plain = []
        for _ in range(args.reps):
            rewind()
            plain.append(clock(lambda: model.decode_greedy(ids, first, G)) / G * 1e3)
        print(f"B={B} ctx={S}: plain nvl_decode_greedy {statistics.median(plain):.4f} ms/step "
              f"(min {min(plain):.4f}, max {max(plain):.4f}; {args.reps} x {G} steps)", flush=True)

        for k in ks:
            rows = np.concatenate([first[:, None], ref[:k].T], axis=1).astype(np.int32)       # [B, 1+k], drafts all right

            def verify():
                acc, _ = model.verify_greedy(ids, rows, k)
                return acc

            def forward_host():
                logits, _ = model.forward_batch(ids, list(rows), [S] * B, all_logits=True)
                g = logits.reshape(B, 1 + k, V).argmax(axis=2)
                acc = np.zeros(B, np.int32)
                for i in range(B):
                    while acc[i] < k and rows[i, acc[i] + 1] == g[i, acc[i]]:
                        acc[i] += 1
                return acc

            routes = {"a verify key38=1": (1, verify), "b verify key38=0": (0, verify), "c forward+host": (1, forward_host)}
            times = {name: [] for name in routes}
            accs = {}
            for rep in range(args.reps + 1):               # rep 0: warm-up of every route (first sight, graph capture)
                for name, (mq, fn) in routes.items():
                    old = tune(38, mq)

                    def many():
                        for _ in range(args.passes):
                            accs[name] = fn()
                            rewind()
                    rewind()
                    many() if rep == 0 else times[name].append(clock(many) / args.passes * 1e3)
                    tune(38, old)
            line = "  ".join(f"({name}) {statistics.median(t):.4f} [{min(t):.4f}..{max(t):.4f}]" for name, t in times.items())
            agree = {name: int((a == k).sum()) for name, a in accs.items()}
            ms_a = statistics.median(times["a verify key38=1"])
            print(f"B={B} k={k}: rate at full acceptance from (a): {B * (k + 1) / ms_a * 1e3:9.1f} tok/s; at none: "
                  f"{B / ms_a * 1e3:9.1f} tok/s", flush=True)
            print(f"B={B} k={k}: ms per pass, median [min..max] of {args.reps} x {args.passes}: {line} | "
                  f"sequences whose right drafts were all accepted: {agree}", flush=True)

            # the two bounds of the generation rate, key 38 = 1 then 0
            def generate(right):
                done, cur, passes = 0, first.copy(), 0
                while done < G:
                    d = ref[done:done + k].T if right else (ref[done:done + k].T + 1) % V
                    acc, toks = model.verify_greedy(ids, np.concatenate([cur[:, None], d], axis=1).astype(np.int32), k)
                    a = int(acc.min())                      # (all right: k everywhere; all wrong: 0 everywhere)
                    for i in ids:                           # keep the batch in step where bf16 margins made them differ
                        if acc[i] > a:
                            model.seq_truncate(i, model.seq_len(i) - int(acc[i] - a))
                    cur = toks[:, a].copy()
                    done += a + 1
                    passes += 1
                return passes

            for mq in (1, 0):
                old = tune(38, mq)
                res = []
                for right in (True, False):
                    rewind(); generate(right)              # warm-up
                    best, passes = 1e30, 0
                    for _ in range(3):
                        rewind()
                        t0 = time.perf_counter()
                        passes = generate(right)
                        best = min(best, time.perf_counter() - t0)
                    res.append((B * G / best, passes))
                tune(38, old)
                print(f"B={B} k={k} key38={mq}: >= {G} tokens per sequence: drafts always right {res[0][0]:9.1f} tok/s in "
                      f"{res[0][1]} passes, always wrong {res[1][0]:9.1f} tok/s in {res[1][1]} passes "
                      f"(plain greedy: {B / statistics.median(plain) * 1e3:9.1f} tok/s)", flush=True)
    model.close()


def sampled_mode(args, pkg, model, prompts, batches, ks, clock):
    V, S, G = model.cfg["vocab_size"], args.ctx, args.gen
    r = np.random.default_rng(1)

    def device_ms():
        st = model.stats()
        return st["decode_ms"] + st["prefill_ms"]

    for B in batches:
        ids = list(range(B))
        for i in ids:
            model.seq_reset(i)
        _, first = model.forward_batch(ids, [prompts[i] for i in ids], [0] * B, want_logits=False)
        first = first.copy()
        hists = [prompts[i].tolist() + [int(first[i])] for i in ids]

        def rewind():
            for i in ids:
                model.seq_truncate(i, S)

        for name, kw in (("default", {}), ("T0.8 k40 p0.95", dict(temperature=0.8, top_k=40, top_p=0.95))):
            U = r.random((G, B)).astype(np.float32)
            model.decode_sampled(ids, first, G, hists, U, **kw)          # warm-up
            plain, plain_dev = [], []
            for _ in range(args.reps):
                rewind()
                d0 = device_ms()
                plain.append(clock(lambda: model.decode_sampled(ids, first, G, hists, U, **kw)) / G * 1e3)
                plain_dev.append((device_ms() - d0) / G)
            print(f"B={B} ctx={S} [{name}]: plain nvl_decode_sampled {statistics.median(plain):.4f} ms/step wall "
                  f"[{min(plain):.4f}..{max(plain):.4f}], {statistics.median(plain_dev):.4f} ms/step device "
                  f"({args.reps} x {G} steps)", flush=True)
            for k in ks:
                rows = np.concatenate([first[:, None], r.integers(0, V, (B, k))], axis=1).astype(np.int32)
                u = r.random((B, 1 + k)).astype(np.float32)
                ext = [h + rows[i, 1:j + 1].tolist() for i, h in enumerate(hists) for j in range(1 + k)]
                got = {}

                def fused():
                    got["a"] = model.verify_sampled(ids, rows, k, hists, u, **kw)[0]

                def host():
                    model.forward_batch(ids, list(rows), [S] * B, all_logits=True, want_logits=False)
                    s = model.sample(ext, u.reshape(-1), **kw).reshape(B, 1 + k)
                    acc = np.zeros(B, np.int32)
                    for i in range(B):
                        while acc[i] < k and rows[i, acc[i] + 1] == s[i, acc[i]]:
                            acc[i] += 1
                        model.seq_truncate(i, S + int(acc[i]) + 1)
                    got["c"] = acc

                routes = {"a nvl_verify_sampled": fused, "c forward+sample+host": host}
                wall = {n: [] for n in routes}
                dev = {n: [] for n in routes}
                for rep_i in range(args.reps + 1):            # rep 0: warm-up of every route (first sight, graph capture)
                    for n, fn in routes.items():
                        def many():
                            for _ in range(args.passes):
                                fn()
                                rewind()
                        rewind()
                        d0 = device_ms()
                        t = clock(many) / args.passes * 1e3
                        if rep_i:
                            wall[n].append(t)
                            dev[n].append((device_ms() - d0) / args.passes)
                line = "  ".join(f"({n}) wall {statistics.median(wall[n]):.4f} [{min(wall[n]):.4f}..{max(wall[n]):.4f}] "
                                 f"device {statistics.median(dev[n]):.4f}" for n in routes)
                print(f"B={B} k={k} [{name}]: ms per pass, median [min..max] of {args.reps} x {args.passes}: {line} | "
                      f"accepted (random drafts): a {got['a'].tolist()} c {got['c'].tolist()}", flush=True)


def draft_mode(args, model, draft, prompts, batches, ks, clock):
    V, S, G = model.cfg["vocab_size"], args.ctx, args.gen
    r = np.random.default_rng(2)

    def device_ms(m):
        st = m.stats()
        return st["decode_ms"] + st["prefill_ms"]

    for B in batches:
        ids = list(range(B))
        for m in (model, draft):
            for i in ids:
                m.seq_reset(i)
        _, first = model.forward_batch(ids, [prompts[i] for i in ids], [0] * B, want_logits=False)
        draft.forward_batch(ids, [prompts[i] for i in ids], [0] * B, want_logits=False)
        first = first.copy()
        hists = [prompts[i].tolist() + [int(first[i])] for i in ids]

        def rewind():
            for i in ids:
                model.seq_truncate(i, S)
                draft.seq_truncate(i, S)

        for name, kw in (("default", {}), ("T0.8 k40 p0.95", dict(temperature=0.8, top_k=40, top_p=0.95))):
            U = r.random((G, B)).astype(np.float32)
            model.decode_sampled(ids, first, G, hists, U, **kw)          # warm-up
            plain = []
            for _ in range(args.reps):
                rewind()
                plain.append(clock(lambda: model.decode_sampled(ids, first, G, hists, U, **kw)) / G * 1e3)
            rewind()
            ms_plain = statistics.median(plain)
            print(f"B={B} ctx={S} [{name}]: plain nvl_decode_sampled (target) {ms_plain:.4f} ms/step wall "
                  f"[{min(plain):.4f}..{max(plain):.4f}] ({args.reps} x {G} steps)", flush=True)
            for k in ks:
                ud, ua, uf = r.random((k, B)).astype(np.float32), r.random((B, k)).astype(np.float32), r.random(B).astype(np.float32)
                got = {}

                def one_pass():
                    d = draft.draft_sampled(ids, first, k, hists, ud, **kw)
                    rows = np.concatenate([first[:, None], d.T], axis=1).astype(np.int32)
                    got["acc"] = model.verify_speculative(draft, ids, rows, k, hists, ua, uf, **kw)[0]

                t_draft, t_verify, d_draft, d_verify = [], [], [], []
                for rep_i in range(args.reps + 1):            # rep 0: warm-up (first sight of every launch configuration)
                    td = tv = 0.0
                    dd0, dv0 = device_ms(draft), device_ms(model)
                    for _ in range(args.passes):
                        rewind()
                        d = [None]
                        td += clock(lambda: d.__setitem__(0, draft.draft_sampled(ids, first, k, hists, ud, **kw)))
                        rows = np.concatenate([first[:, None], d[0].T], axis=1).astype(np.int32)
                        tv += clock(lambda: got.__setitem__("acc", model.verify_speculative(draft, ids, rows, k, hists, ua, uf, **kw)[0]))
                    if rep_i:
                        t_draft.append(td / args.passes * 1e3); t_verify.append(tv / args.passes * 1e3)
                        d_draft.append((device_ms(draft) - dd0) / args.passes); d_verify.append((device_ms(model) - dv0) / args.passes)
                # the rejection kernel alone: the library's per-kernel events, in a run of their own
                model.set_profile(True)
                model.reset_stats()
                for _ in range(args.passes):
                    rewind()
                    one_pass()
                rej = [s for s in model.kernel_stats() if s["site"] == "spec_reject"]
                model.set_profile(False)
                model.reset_stats()
                rewind()
                ms_rej = sum(s["ms"] for s in rej) / max(1, sum(s["launches"] for s in rej))
                md, mv = statistics.median(t_draft), statistics.median(t_verify)
                dv = statistics.median(d_verify)
                print(f"B={B} k={k} [{name}]: ms, median [min..max] of {args.reps} x {args.passes}: draft phase wall {md:.4f} "
                      f"[{min(t_draft):.4f}..{max(t_draft):.4f}] device {statistics.median(d_draft):.4f} | verify pass wall {mv:.4f} "
                      f"[{min(t_verify):.4f}..{max(t_verify):.4f}] device {dv:.4f} | spec_reject kernel {ms_rej:.4f} "
                      f"({100 * ms_rej / dv:.1f} % of the pass's device time) | break-even accepted drafts per pass "
                      f"{(md + mv) / ms_plain - 1:.2f} | accepted (random models): {got['acc'].tolist()}", flush=True)


if __name__ == "__main__":
    main()
