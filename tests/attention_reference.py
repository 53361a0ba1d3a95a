"""Float64 statement of one layer's attention on a paged batch, the bf16 emulation of the kernels' rounding points, the
bounds of tests/test_attention_ops_gpu.py and the batches it runs — test infrastructure, like tests/moe_reference.py.

The batch is what nvl_op_attention_batch (ops.attention_batch) takes: K / V pools [n_blocks][nKV][block][hd], a block
table [n_seqs][stride], sequence i = seq_len[i] new rows behind seq_pos[i] cached keys, row j seeing keys 0 .. seq_pos + j.

Pools.  Blocks a table names hold the sequence's rows; EVERY other row of both pools — rows past a sequence's last key,
the row a fused decode step is about to write, whole unnamed blocks, and one dedicated poison block that every unused
table entry names — holds finite garbage of large magnitude: K uniform in +-64, V the constant 1024, bf16-exact.  Block
ids are a seeded permutation.  The cache contract is "stale rows are finite" (nvl_create zeroes the pools, only the
kernels write them), so a masked garbage key contributes exp2(-inf) * 1024 = 0 exactly, and any wrong index in a kernel
— a wrong block, a wrong row, a key past the causal limit — yields wrong NUMBERS (about 1024 x the key's weight), never
an access outside the pool.  All real inputs are bf16-exact, so no input rounding enters; the 8-bit form's references run
on the dequantized cache scale * e4m3(code), garbage included (it goes through the same quantizer: never a NaN code).

Bounds (bf16 forms).
 (a) per element  |dev - f64| <= 1.05 * element_bound + 1e-6 * max|f64|,  element_bound = 2^-9 (A + 2 |f64|),
     A_d = sum_t p_t |v_td| / sum_t p_t: each P carries at most 2^-9 relative error into the numerator (-> 2^-9 A), the
     denominator at most 2^-9 relative (-> 2^-9 |f64|: it is exact in the decode forms, whose l_run sums the unrounded P),
     and the bf16 store at most 2^-9 |f64|.  The 5 % and the absolute term cover the exp2 approximation and fp32 sums.
 (b) per (sequence, kv head), pooled over its rows:  rms(dev - f64) <= ATTN_RATIO_BOUND * rms(emulated - f64).
attention_emulated is float64 with a bf16 rounding where the kernels round: P before P.V; the denominator the sum of the
ROUNDED P in the prefill forms (ones . P^T rides the MFMA pipe) and of the unrounded P in the decode, multi-position and
8-bit decode forms (l_run); the output.  It rounds P relative to the row's FINAL maximum; the device rounds relative to
the running maximum of its own tile order (and per split partial), so the two are different correct roundings of the
same thing — which is why the ratio of (b) is measured (profiles/attention_op_tests.txt) and not 1.
f32 precision: 5e-5 of the row's maximum, per row."""
import numpy as np

GARBAGE_K, GARBAGE_V = 64.0, 1024.0
LOG2E = 1.4426950408889634


def bf16(a):
    """round to nearest even bf16, returned as float64"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return (((u + r) >> 16) << 16).astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(bf16(a), a.astype(np.float64)), "not bf16-exact"
    return (a.view(np.uint32) >> 16).astype(np.int64)


def bf16_ulp_distance(a, b):
    """distance in bf16 steps between two bf16-exact arrays (sign-magnitude order)"""
    def key(x):
        u = bf16_bits(x)
        return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)
    return np.abs(key(a) - key(b))


# ---- the 8-bit cache: kv8.h's quantizer contract (tests/test_kv_fp8_gpu.py holds the device to it exhaustively) ----
def _e4m3_grid():
    c = np.arange(127)
    e, m = (c >> 3) & 15, c & 7
    return np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))


E4M3 = _e4m3_grid()


def kv8_dequantized(x, s):
    """scale * e4m3fn(x / scale): fp32 division, saturation to +-448, round to nearest, ties to the even code"""
    y = (np.asarray(x, np.float32) / np.float32(s)).astype(np.float32)
    a = np.minimum(np.abs(y.astype(np.float64)), 448.0)
    hi = np.clip(np.searchsorted(E4M3, a, side="left"), 0, 126)
    lo = np.clip(hi - 1, 0, 126)
    dlo, dhi = a - E4M3[lo], E4M3[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    return (np.copysign(E4M3[code], y).astype(np.float32) * np.float32(s)).astype(np.float64)


# ---- the float64 statement ----
def gather(pool, table_row, n_keys, block_size):
    """a sequence's first n_keys keys out of pool [n_blocks][nKV][block][hd] through its block-table row -> [nKV][n_keys][hd]"""
    nb = max(-(-n_keys // block_size), 1)
    rows = np.concatenate([pool[int(table_row[b])] for b in range(nb)], axis=1)
    return np.asarray(rows[:, :n_keys], np.float64)


def rope_tables(base, max_seq, hd):
    """the model's fp32 tables (rope.go:18-50): [max_seq][hd], both halves of a row the same hd/2 values"""
    inv = 1.0 / base ** (np.arange(hd // 2) * 2.0 / hd)
    ang = np.arange(max_seq)[:, None] * inv[None, :]
    cos = np.concatenate([np.cos(ang), np.cos(ang)], -1).astype(np.float32).astype(np.float64)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], -1).astype(np.float32).astype(np.float64)
    return cos, sin


def rope_f64(x, pos, base, max_seq):
    """rope_pair8's rotate-half convention on x [..., hd] at position pos: x * cos + rotate_half(x) * sin, rotate_half(x)
    = (-x[hd/2:], x[:hd/2]); base 0 = no rotation (the cos_t = NULL path)"""
    x = np.asarray(x, np.float64)
    if not base:
        return x
    hd = x.shape[-1]
    cos, sin = rope_tables(base, max_seq, hd)
    rot = np.concatenate([-x[..., hd // 2:], x[..., :hd // 2]], -1)
    return x * cos[pos] + rot * sin[pos]


def _softmax_rows(q, K, V, pos, scale, visible=None):
    """q [len][nH][hd], K / V [nKV][T][hd] -> p [nKV][len * group][T] unnormalised (exp(s - max), 0 where masked), rows
    position-major; visible [len][T] overrides the causal mask"""
    n, nH, hd = q.shape
    nKV, T, _ = K.shape
    g = nH // nKV
    if visible is None:
        visible = np.arange(T)[None, :] <= (pos + np.arange(n))[:, None]
    qh = q.reshape(n, nKV, g, hd).transpose(1, 0, 2, 3).reshape(nKV, n * g, hd)
    s = np.einsum("krd,ktd->krt", qh, K) * scale
    s = np.where(np.repeat(visible, g, axis=0)[None], s, -np.inf)
    return np.exp(s - s.max(-1, keepdims=True))


def _unrows(o, n, nH):
    nKV = o.shape[0]
    return o.reshape(nKV, n, nH // nKV, -1).transpose(1, 0, 2, 3).reshape(n, nH, -1)


def attend(q, K, V, pos, scale, visible=None):
    """-> dict of [len][nH][hd] float64 arrays: ref (attention_f64), bound (element_bound), emu_rounded / emu_unrounded
    (attention_emulated with the prefill / decode denominator)"""
    q, K, V = (np.asarray(a, np.float64) for a in (q, K, V))
    n, nH, _ = q.shape
    p = _softmax_rows(q, K, V, pos, scale, visible)
    den = p.sum(-1, keepdims=True)
    ref = np.einsum("krt,ktd->krd", p, V) / den
    A = np.einsum("krt,ktd->krd", p, np.abs(V)) / den
    pr = bf16(p)
    num = np.einsum("krt,ktd->krd", pr, V)
    out = dict(ref=ref, bound=2.0 ** -9 * (A + 2 * np.abs(ref)), emu_rounded=bf16(num / pr.sum(-1, keepdims=True)),
               emu_unrounded=bf16(num / den))
    return {k: _unrows(v, n, nH) for k, v in out.items()}


def attention_f64(q, K, V, pos, scale):
    """causal attention of one sequence: row j sees keys 0 .. pos + j"""
    return attend(q, K, V, pos, scale)["ref"]


def attention_emulated(q, K, V, pos, scale, denominator):
    """float64 with the kernels' bf16 roundings (module docstring); denominator "rounded" (prefill) or "unrounded" (decode)"""
    return attend(q, K, V, pos, scale)["emu_" + denominator]


def element_bound(q, K, V, pos, scale):
    return attend(q, K, V, pos, scale)["bound"]


# ---- cases ----
def _c(nH=8, nKV=2, hd=64, block=64, pos=(), lens=None, expect=None, stride=None):
    lens = tuple(lens) if lens else (1,) * len(pos)
    need = max(-(-(p + n) // block) for p, n in zip(pos, lens))
    return dict(nH=nH, nKV=nKV, hd=hd, block=block, pos=tuple(pos), lens=lens, expect=expect, stride=stride or need)


# expect = (waves per workgroup, workgroups per (sequence, kv head)) as decode_attn_cfg chooses them
DECODE_CASES = {
    "D1": _c(pos=(0, 63, 64), expect=(2, 1)),                      # empty cache, last key of a tile, first key of a new block
    "D2": _c(block=256, pos=(1023, 70), expect=(2, 4)),            # 16 tiles: nsplit 4; the short sequence: 3 of 4 workgroups idle
    "D3": _c(block=256, pos=(1024, 960), expect=(2, 5)),           # odd nsplit; the new key is row 0 of a fresh block
    "D4": _c(nH=4, nKV=1, hd=128, block=256, pos=(1000,), expect=(2, 8)),      # hd 128; automatic kv_nt (one sequence)
    "D5": _c(nH=71, nKV=1, block=256, pos=(1100, 5), expect=(2, 5)),           # MQA: 5 query tiles, the last with 7 heads
    "D6": _c(nKV=4, block=256, pos=(2047, 300, 64, 1500, 7), expect=(2, 6)),   # 20 pairs at 2048 keys: 128 / 20 = 6
    "D6p": _c(nKV=4, block=256, pos=(1099, 300, 64, 900, 7), expect=(8, 1)),   # 20 pairs below 32 tiles: unsplit
    "D7": _c(block=192, pos=(191, 192, 383, 500), expect=(4, 1)),  # the division path across block edges
    "D8": _c(nKV=4, block=256, pos=(1000,) * 9, expect=(8, 1)),    # 36 pairs: above ATTN_SPLIT_MAX_PAIRS
}
SPLIT_CASES = [n for n, c in DECODE_CASES.items() if c["expect"][1] > 1]
PREFILL_CASES = {
    "P1": _c(pos=(0, 60, 1000), lens=(5, 70, 1)),                  # ragged rows, a one-row sequence, more tiles than the ring
    "P2": _c(nH=71, nKV=1, pos=(30,), lens=(4,)),                  # 284 query rows: a ragged second query tile
    "P3": _c(hd=128, block=192, pos=(200,), lens=(40,)),
    "P4": _c(pos=(0, 70), lens=(5, 3), stride=129),                # more table entries than the bf16 prefill kernel's LDS copy
}
MQ_CASES = {
    "M1": _c(pos=(62, 0, 1030), lens=(4, 4, 4), expect=(8, 1)),
    "M2": _c(pos=(62, 0, 1030), lens=(4, 2, 4), expect=(8, 1)),
}
ALL_CASES = {**DECODE_CASES, **PREFILL_CASES, **MQ_CASES}
CENSUS_CASES = ["D1", "D3", "D7", "P1"]
KV8_SCALES = (2.0 ** -4, 2.0 ** -5)          # k_scale, v_scale of the random batches (+-28 / +-14 before saturation)
CENSUS_KV8_SCALES = (1.0, 4.0)               # marks (1 -> code 0.25) and the garbage (1024 -> code 256) stay exact
ROPE_BASE = 10000.0


def _exact(r, shape):
    return bf16(r.standard_normal(shape, dtype=np.float32))


def marked_keys(pos, n, block, hd):
    """up to hd distinct keys < pos + n, most telling first: tile and block edges, the last cached key, the first and
    last new key, key 0, the other new keys, then an even spread"""
    T = pos + n
    edges = [e + d for e in sorted({*range(64, T + 64, 64), *range(block, T + block, block)}) for d in (-1, 0)]
    keys = [k for k in [pos - 1, pos, T - 1, 0] + edges[::-1] + list(range(pos, T)) if 0 <= k < T]
    keys = list(dict.fromkeys(keys))[:hd]
    for k in np.linspace(0, T - 1, hd).astype(int).tolist():
        if len(keys) >= hd:
            break
        if k not in keys:
            keys.append(k)
    return keys


_BATCHES, _REFS = {}, {}
HEADROOM = 0.9


def batch(name, form="plain", census=False):
    """_build's batch of a case for a form, built once and shared read-only.
    bf16's unit roundoff is 2^-8: 2^-9 is half a step at the TOP of a binade, so element_bound is no theorem — a correct
    kernel can exceed it on an unlucky element of a short sequence (6 keys x 71 heads: 1.08 of the bound met in the
    emulation).  The bound stays as it is; the DRAWS are held to it instead: the first draw k = 0, 1, .. of a (case, form)
    on which both emulations stay within HEADROOM of bound (a) is the one every test uses, which leaves the device's
    different-but-correct roundings a tenth of the bound."""
    key = (name, form, census)
    if key not in _BATCHES:
        for attempt in range(16):
            b = _build(name, form, census, attempt)
            if census:
                break
            refs = [attend(b["q_ref"][i], b["K"][i], b["V"][i], b["seq_pos"][i], b["scale"]) for i in range(len(b["K"]))]
            lim = [1.05 * r["bound"] + 1e-6 * np.abs(r["ref"]).max() for r in refs]
            if max(float((np.abs(r[e] - r["ref"]) / l).max()) for r, l in zip(refs, lim) for e in ("emu_rounded", "emu_unrounded")) <= HEADROOM:
                _REFS[key] = refs
                break
        else:
            raise AssertionError(f"{key}: no draw within the element bound")
        b["draw"] = attempt
        _BATCHES[key] = b
    return _BATCHES[key]


def _build(name, form, census, attempt):
    """The batch of a case for a form ("plain", "fused", "fused_norope", "kv8", "mq"; prefill cases: "plain" / "kv8"),
    built once and shared read-only: the op's inputs, each sequence's keys as the reference must see them (K, V: float64
    lists, the 8-bit form's dequantized), the reference query rows q_ref, and for the fused forms the pools expected
    after the launch.  census: q = 0, V marks one key per output dimension (marked_keys), `want` the exact output."""
    c = ALL_CASES[name]
    nH, nKV, hd, bs, stride = c["nH"], c["nKV"], c["hd"], c["block"], c["stride"]
    fused = form.startswith("fused")
    base = ROPE_BASE if form == "fused" else 0.0
    n_seqs = len(c["pos"])
    r = np.random.default_rng([sum(map(ord, name)), int(census), attempt])
    need = [-(-(p + n) // bs) for p, n in zip(c["pos"], c["lens"])]
    n_blocks = sum(need) + 3                                           # + the poison block and two nobody names
    ids = r.permutation(n_blocks)
    poison, free = int(ids[0]), iter(ids[1:])
    k_pool = bf16(r.uniform(-GARBAGE_K, GARBAGE_K, (n_blocks, nKV, bs, hd)).astype(np.float32))
    v_pool = np.full((n_blocks, nKV, bs, hd), GARBAGE_V)
    table = np.full((n_seqs, stride), poison, np.int32)
    max_seq = stride * bs
    b = dict(name=name, form=form, census=census, nH=nH, nKV=nKV, hd=hd, block=bs, scale=1.0 / np.sqrt(hd), seq_len=list(c["lens"]),
             seq_pos=list(c["pos"]), poison=poison, rope_base=base, max_seq=max_seq, expect=c["expect"], K=[], V=[], q_ref=[],
             want=[], new_rows=[])
    q_rows, qkv_rows = [], []
    for i, (pos, n) in enumerate(zip(c["pos"], c["lens"])):
        T = pos + n
        K, V = _exact(r, (nKV, T, hd)), _exact(r, (nKV, T, hd))
        q = _exact(r, (n, nH, hd))
        if census:
            keys = marked_keys(pos, n, bs, hd)
            key_d = np.asarray([keys[d % len(keys)] for d in range(hd)])
            q = np.zeros_like(q)
            V = np.zeros_like(V)
            V[:, key_d, np.arange(hd)] = 1.0
            vis = key_d[None, :] <= (pos + np.arange(n))[:, None]
            b["want"].append(np.repeat((vis / (pos + np.arange(n) + 1.0)[:, None])[:, None, :], nH, axis=1))
        for j in range(need[i]):
            table[i, j] = next(free)
        q_ref = q
        if fused:       # the new row: raw q | k | v in the QKV row, rotated and rounded by the kernel; its pool row stays garbage
            qkv_rows.append(np.concatenate([q[0].ravel(), K[:, pos].ravel(), V[:, pos].ravel()]))
            q_ref = bf16(rope_f64(q, pos, base, max_seq))
            K = K.copy()
            K[:, pos] = bf16(rope_f64(K[:, pos], pos, base, max_seq))
        for t in range(T - 1 if fused else T):
            k_pool[table[i, t // bs], :, t % bs] = K[:, t]
            v_pool[table[i, t // bs], :, t % bs] = V[:, t]
        b["new_rows"].append((int(table[i, pos // bs]), pos % bs))
        q_rows.append(q)
        b["K"].append(K); b["V"].append(V); b["q_ref"].append(q_ref)
    if form == "kv8":
        ks, vs = CENSUS_KV8_SCALES if census else KV8_SCALES
        b.update(k_scale=ks, v_scale=vs)
        dk, dv = kv8_dequantized(k_pool, ks), kv8_dequantized(v_pool, vs)
        b["K"] = [gather(dk, table[i], p + n, bs) for i, (p, n) in enumerate(zip(c["pos"], c["lens"]))]
        b["V"] = [gather(dv, table[i], p + n, bs) for i, (p, n) in enumerate(zip(c["pos"], c["lens"]))]
    b.update(table=table, k_pool=k_pool.astype(np.float32), v_pool=v_pool.astype(np.float32),
             q=np.stack(qkv_rows).astype(np.float32) if fused else np.concatenate(q_rows).astype(np.float32))
    if fused:
        ek, ev = b["k_pool"].copy(), b["v_pool"].copy()
        for i, (blk, row) in enumerate(b["new_rows"]):
            ek[blk, :, row] = b["K"][i][:, c["pos"][i]]
            ev[blk, :, row] = b["V"][i][:, c["pos"][i]]
        b.update(k_pool_after=ek, v_pool_after=ev)
    for a in b.values():
        for x in (a if isinstance(a, list) else [a]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return b


def references(b):
    """per sequence attend() of a batch's own K / V / q_ref: computed once, shared"""
    key = (b["name"], b["form"], b["census"])
    if key not in _REFS:
        _REFS[key] = [attend(b["q_ref"][i], b["K"][i], b["V"][i], b["seq_pos"][i], b["scale"]) for i in range(len(b["K"]))]
    return _REFS[key]


def split_rows(b, out):
    return np.split(np.asarray(out, np.float64), np.cumsum(b["seq_len"])[:-1])


def denominator(ran):
    return "rounded" if ran.startswith("prefill") else "unrounded"


def figures(b, out, ran):
    """-> (worst |dev - f64| / (1.05 bound + 1e-6 max|f64|) over the batch, [(sequence, kv head, rms dev, rms emulated)])"""
    worst, pooled = 0.0, []
    g = b["nH"] // b["nKV"]
    for i, (ref, dev) in enumerate(zip(references(b), split_rows(b, out))):
        err = np.abs(dev - ref["ref"])
        worst = max(worst, float((err / (1.05 * ref["bound"] + 1e-6 * np.abs(ref["ref"]).max())).max()))
        emu = ref["emu_" + denominator(ran)] - ref["ref"]
        for h in range(b["nKV"]):
            hs = slice(h * g, (h + 1) * g)
            pooled.append((i, h, float(np.sqrt((err[:, hs] ** 2).mean())), float(np.sqrt((emu[:, hs] ** 2).mean()))))
    return worst, pooled


def check_bf16(b, res, ratio_bound, tag=""):
    """bounds (a) and (b) of a bf16 form's result (ops.attention_batch's dict) -> (worst of (a), largest ratio of (b))"""
    assert np.isfinite(res["out"]).all(), (b["name"], tag, "out is not finite")
    worst, pooled = figures(b, res["out"], res["ran"])
    ratios = [d / e for _, _, d, e in pooled if e > 0]
    top = max(ratios) if ratios else 0.0
    print(f"{b['name']} {b['form']} {tag}: ran {res['ran']} nw {res['nw']} nsplit {res['nsplit']}  (a) {worst:.3f} of the bound  "
          f"(b) largest ratio {top:.4f} (bound {ratio_bound})")
    assert worst <= 1.0, (b["name"], tag, "element bound", worst)
    for i, h, d, e in pooled:
        assert d <= ratio_bound * e, (b["name"], tag, "rms ratio", i, h, d, e)
    return worst, top


def check_f32(b, res):
    assert np.isfinite(res["out"]).all()
    worst = 0.0
    for ref, dev in zip(references(b), split_rows(b, res["out"])):
        worst = max(worst, float((np.abs(dev - ref["ref"]).max(-1) / np.abs(ref["ref"]).max(-1)).max()))
    print(f"{b['name']} f32: worst row error {worst:.3e} of the row maximum (bound 5e-5)")
    assert worst <= 5e-5, (b["name"], worst)


def check_census(b, res):
    """exactly 0 where the marked key is invisible, within 2^-8 relative of 1 / (pos + j + 1) where it is visible"""
    assert np.isfinite(res["out"]).all()
    worst = 0.0
    for i, (want, dev) in enumerate(zip(b["want"], split_rows(b, res["out"]))):
        assert (dev[want == 0] == 0.0).all(), (b["name"], b["form"], i, "a key beyond the causal limit (or a garbage row) was counted")
        if (want > 0).any():
            worst = max(worst, float(np.abs(dev[want > 0] / want[want > 0] - 1.0).max()))
    print(f"{b['name']} {b['form']} census: worst relative deviation from 1/(pos+j+1): {worst:.3e} (bound 2^-8)")
    assert worst <= 2.0 ** -8, (b["name"], b["form"], worst)


def check_append(b, res):
    """the fused form's pools: the appended K row within one bf16 step of bf16(rope_f64), the V row bit-equal to bf16(v),
    every other element of both pools unchanged"""
    assert np.array_equal(res["v_pool"], b["v_pool_after"]), (b["name"], "V pool")
    same = np.ones(b["k_pool"].shape, bool)
    for blk, row in b["new_rows"]:
        same[blk, :, row] = False
    assert np.array_equal(res["k_pool"][same], b["k_pool"][same]), (b["name"], "K pool outside the appended rows")
    assert np.isfinite(res["k_pool"]).all()
    assert bf16_ulp_distance(res["k_pool"][~same], b["k_pool_after"][~same]).max() <= 1, (b["name"], "appended K rows")


# ---- the stand-in for the device (CPU tests): the emulation, through the pools and the table, with the mutations the
# GPU tests are aimed at ----
MUTATIONS = ("drop_key", "extra_key", "swap_blocks", "poison_tile", "merge_scale_one", "next_position", "wrong_kv_head",
             "patch_skipped", "append_row_off", "append_block_off", "rope_position_minus_one")


def emulated_device(b, ran, nw=2, nsplit=1, mutation=None, seq=0):
    """What a device that rounds as attention_emulated would return for batch b (dict as ops.attention_batch), computed
    from the POOLS through the block table, the fused forms' patch and append included.  mutation: one of MUTATIONS,
    applied to sequence `seq`."""
    bs, n_seqs, kv8, fused = b["block"], len(b["seq_pos"]), b["form"] == "kv8", b["form"].startswith("fused")
    kp, vp = np.asarray(b["k_pool"], np.float64), np.asarray(b["v_pool"], np.float64)
    if kv8:
        kp, vp = kv8_dequantized(kp, b["k_scale"]), kv8_dequantized(vp, b["v_scale"])
    k_after, v_after = kp.astype(np.float32), vp.astype(np.float32)
    outs = []
    for i in range(n_seqs):
        pos, n = b["seq_pos"][i], b["seq_len"][i]
        hit = mutation is not None and i == seq
        if hit and mutation == "next_position":
            pos = b["seq_pos"][(i + 1) % n_seqs]
        T = pos + n
        row = np.array(b["table"][i])
        if hit and mutation == "swap_blocks":       # (first <-> last: two full, fully visible blocks may trade places unseen)
            last = (T - 1) // bs
            row[[0, last]] = row[[last, 0]]
        if hit and mutation == "poison_tile":
            row[(T - 1) // bs // 2] = b["poison"]
        nb = len(row)
        K = np.concatenate([kp[row[j]] for j in range(nb)], axis=1)[:, :max(T, 1)].copy()
        V = np.concatenate([vp[row[j]] for j in range(nb)], axis=1)[:, :max(T, 1)].copy()
        q = np.asarray(b["q"], np.float64)
        if fused:
            nH, nKV, hd = b["nH"], b["nKV"], b["hd"]
            raw = q[i]
            rp = pos - 1 if hit and mutation == "rope_position_minus_one" else pos
            qi = bf16(rope_f64(raw[:nH * hd].reshape(1, nH, hd), rp, b["rope_base"], b["max_seq"] + 1))
            kn = bf16(rope_f64(raw[nH * hd:(nH + nKV) * hd].reshape(nKV, hd), rp, b["rope_base"], b["max_seq"] + 1))
            vn = bf16(raw[(nH + nKV) * hd:].reshape(nKV, hd))
            if not (hit and mutation == "patch_skipped"):
                K[:, pos], V[:, pos] = kn, vn
            blk, r_ = int(b["table"][i][b["seq_pos"][i] // bs]), b["seq_pos"][i] % bs
            if hit and mutation == "append_row_off":
                r_ = (r_ + 1) % bs
            if hit and mutation == "append_block_off":
                blk = int(b["table"][i][(b["seq_pos"][i] // bs + 1) % nb])
            k_after[blk, :, r_], v_after[blk, :, r_] = kn, vn
        else:
            t0 = int(np.sum(b["seq_len"][:i]))
            qi = q[t0:t0 + n]
        if hit and mutation == "wrong_kv_head":
            K, V = np.roll(K, 1, axis=0), np.roll(V, 1, axis=0)
        visible = np.arange(T)[None, :] <= (pos + np.arange(n))[:, None]
        if hit and mutation == "drop_key":
            visible[-1, (pos + n - 1) // 2] = False
        if hit and mutation == "extra_key":       # (decode: the row after the last key, garbage; prefill: the next new key)
            K, V = (np.concatenate([a, (kp if a is K else vp)[row[min(T // bs, nb - 1)], :, T % bs][:, None]], axis=1) for a in (K, V))
            visible = np.concatenate([visible, np.zeros((n, 1), bool)], axis=1)
            visible[0, pos + 1] = True
        if nsplit > 1:
            outs.append(_split_merge(qi, K, V, visible, b["scale"], nw, nsplit, scale_one=hit and mutation == "merge_scale_one"))
        else:
            outs.append(attend(qi, K, V, pos, b["scale"], visible)["emu_" + denominator(ran)])
    res = dict(out=np.concatenate(outs).astype(np.float32), ran=ran, nw=nw, nsplit=nsplit, part_cnt=np.zeros(32, np.int32))
    if fused:
        res.update(k_pool=k_after, v_pool=v_after)
    return res


def _split_merge(q, K, V, visible, scale, nw, nsplit, scale_one=False):
    """the key-split decode form: 64-key tiles dealt round-robin over nw * nsplit virtual waves, workgroup z's partial
    {O, m, l} relative to its own maximum, merged with exp(m_z - m*) in z order (scale_one: one partial merged unscaled)"""
    n, nH, hd = q.shape
    T = K.shape[1]
    owner = (np.arange(T) // 64) % (nw * nsplit) // nw
    parts = []
    for z in range(nsplit):
        vis = visible & (owner == z)[None, :]
        if not vis.any():
            continue
        g = nH // K.shape[0]
        qh = q.reshape(n, K.shape[0], g, hd).transpose(1, 0, 2, 3).reshape(K.shape[0], n * g, hd)
        s = np.where(np.repeat(vis, g, axis=0)[None], np.einsum("krd,ktd->krt", qh, K) * scale, -np.inf)
        m = s.max(-1, keepdims=True)
        p = np.exp(s - m)
        parts.append((m, p.sum(-1, keepdims=True), np.einsum("krt,ktd->krd", bf16(p), V)))
    mstar = np.max([m for m, _, _ in parts], axis=0)
    victim = int(np.argmin([m.mean() for m, _, _ in parts]))        # (a partial that does not hold the maximum)
    L = sum(l * (1.0 if scale_one and z == victim else np.exp(m - mstar)) for z, (m, l, _) in enumerate(parts))
    O = sum(o * (1.0 if scale_one and z == victim else np.exp(m - mstar)) for z, (m, _, o) in enumerate(parts))
    return _unrows(bf16(O / L), n, nH)
