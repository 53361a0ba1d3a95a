"""The dense layer tail (generic_model.go:320-326,383-418: O projection, FFN norm, FFN-up, FFN-down, the next norm, the
next projection) in float64, stage by stage — numpy only, test infrastructure like tests/moe_reference.py — plus the
inputs, the case table and the assertions tests/test_dense_ops_gpu.py, tests/test_dense_q_ops_gpu.py (the same tail on
quantized weights: "quantized weights" below) and tests/test_dense_reference_host.py share.

Every stage's reference is FED THE DEVICE'S OWN OUTPUT of the stage before (out: what ops.dense_stages returns): x1 from
the inputs, the FFN-up operand from the device's x1, h from the device's operand and partials, x2 from the device's x1
and h, the next operand from the device's x2 (x_end on the last_rows form), yn from the device's operand and partials.
No error is charged twice and no row is excluded.

Where the device rounds to bf16 (the emulation mirrors exactly these points; sums are fp32 there, float64 here):
  attn_out, WO, W1, W2, Wn   on upload: the MFMA operands
  xn_raw = bf16(fp32(x) * fp32(w_norm))            deferred path (gemm.h EPI_RESID && rs_out): ONE fp32 multiply, ONE
                                                   rounding; the consumer scales its fp32 accumulators by rstd
  xn = bf16(norm(x))                               norm path (norm_row_kernel, norm_tile16_kernel)
  h = bf16(silu(g) * u) / bf16(gelu(a + b1))       epilogue_swiglu4 / epilogue4<EPI_GELU>
The residual stream x, the biases, alpha, the x^2 partials, rstd and yn are fp32 and never rounded.

Bounds that are derived, not measured:
  xn_raw            bit for bit against numpy float32 (both families).
  x^2 partials      n = 16 (8 on half tiles) non-negative fp32 terms: relative error <= (n + 1) 2^-24 against float64.
  rstd              formed by the test from the device's partials: 1e-6 relative to float64 1/sqrt(mean(x1^2) + eps).
  x1, xn_raw, partials, their row sums, exact family: np.array_equal (integers below 2^24: every order gives the same).
  x2, exact family  the device's h is bf16(silu(g) u) with g, u scaled by an irrational rstd — no integer — so the sum
                    h . W2 is not exact in fp32; the bound is the worst-case fp32 dot product error instead,
                    (K + 2) 2^-24 sum_k |h_k W2_k| + 2^-23 |x2|, whatever the order (Higham, Accuracy and Stability,
                    eq. 3.5).  The next operand is then again bit for bit from the device's own x2.
  h, exact family   half a bf16 ulp of the float64 value + H_F32_MARGIN x the error of a float32 evaluation of the stage.
Measured (random family): per row m and stage, rms(dev[m] - f64[m]) <= DENSE_RATIO_BOUND x rms(emulated[m] - f64[m])."""
import numpy as np

from bf16_emulator import round_bf16

F32_TOL = 2e-5          # tests/test_ops_gpu.py's file-wide bound on fp32 results of bf16-rounded operands, relative to max
U24 = 2.0 ** -24
# fp32 evaluation of rstd * acc -> silu(g) * u against float64, relative to |h|, exact family: the largest value over the
# exact cases it runs is 4.01e-7 (tests/test_dense_reference_host.py::test_h_f32_term recomputes it on the CPU and holds
# it below H_F32_REL); the device gets 4 x that
H_F32_REL, H_F32_MARGIN = 4.1e-7, 4.0


def _r64(a):
    return round_bf16(np.asarray(a, np.float32)).astype(np.float64)


def _f64(a):
    return np.asarray(a, np.float64)


def row_rms(a):
    return np.sqrt((_f64(a) ** 2).mean(1))


def silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def gelu(a):
    return 0.5 * a * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (a + 0.044715 * a ** 3)))


def norm64(x, w, b, eps, kind):
    x = _f64(x)
    if kind == "rms":
        return x / np.sqrt((x * x).mean(1, keepdims=True) + eps) * _f64(w)
    mu = x.mean(1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps) * _f64(w) + _f64(b)


def alphas(inp):
    """(O projection, FFN-down) multipliers as forward() picks them"""
    rm, am = inp.get("residual_multiplier", 0.0), inp.get("attention_multiplier", 0.0)
    if inp.get("block", "sequential") == "parallel":
        return (am, rm) if am != 0.0 and rm != 0.0 else (1.0, 1.0)
    a = rm if rm != 0.0 else 1.0
    return a, a


def resid(x, a, w, bias, alpha, rounded):
    """x + alpha (a . w^T + bias), float64; rounded: a and w through bf16 first"""
    cv = _r64 if rounded else _f64
    return _f64(x) + np.float64(np.float32(alpha)) * (cv(a) @ cv(w).T + (0.0 if bias is None else _f64(bias)))


def xn_raw32(x, w):
    """the deferred operand: one float32 multiply, one round to nearest even"""
    return round_bf16(np.asarray(x, np.float32) * np.asarray(w, np.float32)[None, :])


def partials64(x, tiles):
    x = _f64(x)
    return (x * x).reshape(x.shape[0], tiles, -1).sum(2)


def rstd_of(rs, H, eps):
    return 1.0 / np.sqrt(_f64(rs).sum(1) / H + eps)


def ffn_h(op, rs, inp, rounded, swap=False):
    """h from FFN-up's operand as the consumer reads it: op (bf16 values) and the partials (None: already normalised)"""
    cv = _r64 if rounded else _f64
    H = op.shape[1]
    a = _f64(op) @ cv(inp["w1"]).T
    if rs is not None:
        a = a * rstd_of(rs, H, inp["norm_eps"])[:, None]
    if inp.get("act", "swiglu") == "swiglu":
        F = a.shape[1] // 2
        g, u = (a[:, F:], a[:, :F]) if swap else (a[:, :F], a[:, F:])
        h = silu(g) * u
    else:
        h = gelu(a + (0.0 if inp.get("b1") is None else _f64(inp["b1"])))
    return _r64(h) if rounded else h


def next_y(op, rs, inp, rounded):
    y = _f64(op) @ (_r64 if rounded else _f64)(inp["wn"]).T
    return y if rs is None else y * rstd_of(rs, op.shape[1], inp["norm_eps"])[:, None]


# ---- inputs ------------------------------------------------------------------------------------------------------------
def random_inputs(M, H, qw, F, Nn, seed=0, **kw):
    """x, attn_out ~ N(0, 1) (every 7th row from row 3 scaled by 1e-3: mean(x^2) there is of the order of eps), weights x 0.05,
    a non-trivial norm weight; biases where the block has them"""
    r = np.random.default_rng(100003 * M + 17 * H + qw + F + Nn + seed)
    n = lambda *s: r.standard_normal(s, dtype=np.float32)
    swiglu = kw.get("act", "swiglu") == "swiglu"
    inp = dict(x=n(M, H), attn_out=n(M, qw), wo=n(H, qw) * 0.05, norm_w=1.0 + 0.3 * n(H), w1=n(2 * F if swiglu else F, H) * 0.05,
               w2=n(H, F) * 0.05, next_norm_w=1.0 + 0.3 * n(H), wn=n(Nn, H) * 0.05, norm_eps=1e-5, family="random")
    inp["x"][3::7] *= 1e-3
    inp["attn_out"][3::7] *= 1e-3
    if kw.get("norm", "rms") == "layer":
        inp.update(norm_b=0.1 * n(H), next_norm_b=0.1 * n(H))
    if kw.get("biases"):
        inp.update(bo=0.5 * n(H), b1=0.1 * n(F), b2=0.5 * n(H))
    inp.update(kw)
    return inp


def exact_inputs(M, H, qw, F, Nn, seed=0, **kw):
    """Small integers everywhere, alpha 1 or 0.5, norm weights powers of two: x1, xn_raw and the partials are exact in fp32
    in any summation order (checked here in float64: integers — half integers at alpha 0.5 — whose squares' row sums stay
    below 2^24).  Random integers: asymmetric in row and column, so a transposed or shifted tile cannot pass."""
    r = np.random.default_rng(7 * M + H + qw + F + Nn + seed)
    i = lambda lo, hi, *s: r.integers(lo, hi + 1, s).astype(np.float32)
    inp = dict(x=i(-4, 4, M, H), attn_out=i(-1, 1, M, qw), wo=i(-1, 1, H, qw), bo=i(-2, 2, H),
               norm_w=(2.0 ** i(-5, -3, H)), w1=i(-1, 1, 2 * F, H), w2=i(-1, 1, H, F), b2=i(-2, 2, H),
               next_norm_w=(2.0 ** i(-5, -3, H)), wn=i(-1, 1, Nn, H), norm_eps=1e-5, family="exact")
    inp.update(kw)
    a_o, _ = alphas(inp)
    assert a_o in (1.0, 0.5)
    x1 = resid(inp["x"], inp["attn_out"], inp["wo"], inp["bo"], a_o, False)
    q = 1.0 / a_o                                   # x1 is a multiple of 1/q, its square of 1/q^2
    assert np.array_equal(x1 * q, np.round(x1 * q)) and np.abs(x1 * q).max() < 2 ** 24
    assert (np.abs(_f64(inp["attn_out"])) @ np.abs(_f64(inp["wo"])).T).max() + 8 < 2 ** 24      # every partial sum
    assert ((x1 * q) ** 2).sum(1).max() < 2 ** 24, "the row sum of x1^2 is not exact in fp32"
    return inp


# ---- the case table (tests/test_dense_ops_gpu.py) -------------------------------------------------------------------
# name -> dict(shape (M, H, qw, F, Nn), kw of the builder / the op, keys of nvl_set_tuning, ran: the literals worked out by
# hand from resid_gemm, defer_half, launch_norm and the launchers of gemm.h, families)
def P(producer=0, half=0, form="decode", slices=0, consumer=None):
    return dict(producer=producer, half=half, form=form, slices=slices, consumer=consumer)


LL = (256, 256, 512)          # Llama-style H, qw, F: RMSNorm + SwiGLU, sequential


# The literals below are the guard, not an echo: the op reports rs1_tiles / rs2_tiles through the same defer_half() the
# consumers ask (that is how the key 3 = 2 / 3 mismatch showed), so an error inside defer_half() moves the op's stride
# with the consumers'.  A case whose "ran" differs from its literal is a finding about the code — work the literal out
# again by hand from resid_gemm / the launchers before touching it, and never copy it from a run.
def _ran(o, down, norms, t1, t2):
    return dict(o=o, down=down, norms=norms, rs1_tiles=t1, rs2_tiles=t2)


HALF = _ran(P(1, 1, "msplit"), P(1, 1, "msplit"), 0, 32, 32)            # M <= 16: H / 8 partials
MSPLIT = _ran(P(1, 0, "msplit"), P(1, 0, "msplit"), 0, 16, 16)          # 17..64 rows (or half tiles off)
GROUPS = _ran(P(1, 0, "groups"), P(1, 0, "groups"), 0, 16, 16)            # 65..128 decode rows: 64-row groups, one launch
SERIAL = _ran(P(1, 0, "groups_serial"), P(1, 0, "groups_serial"), 0, 16, 16)


def sk(o, d, co="row", cd="row", form="decode"):      # no deferral: O leaves o slices, FFN-down d; two norm launches
    return _ran(P(0, 0, form, o, co if o else None), P(0, 0, form, d, cd if d else None), 2, 0, 0)


CASES = {}


def _add(name, shape, ran, keys=None, families=("random", "exact"), **kw):
    CASES[name] = dict(shape=shape, ran=ran, keys=keys or {}, families=families, kw=kw)


for M in (1, 5, 16):                                                            # 1
    _add(f"llama-M{M}", (M, *LL, 384), HALF)
for M in (17, 32, 33, 48, 64):                                                  # 2
    _add(f"llama-M{M}", (M, *LL, 384), MSPLIT)
for M in (65, 100, 128):                                                        # 3
    _add(f"llama-M{M}", (M, *LL, 384), GROUPS)
    _add(f"llama-M{M}-serial", (M, *LL, 384), SERIAL, {13: 0}, ("random",))
# 129 rows: no deferral; K = 256 / 512 give the tile split one slice, so both projections add in the launch, as 64-row
# groups (4 tiles of 128 x 128 are fewer than g_chunk_min_tiles)
_add("llama-M129", (129, *LL, 384), sk(0, 0, form="groups"))
_add("llama-M5-nohalf", (5, *LL, 384), MSPLIT, {27: 0})                         # 4
for M in (5, 40):
    # key 3 = 2: producers without m_split (the plain decode form carries the norm); 3: only the O projection defers,
    # FFN-down (K = 512: two slices) is left to the next norm
    _add(f"llama-M{M}-key3=2", (M, *LL, 384), _ran(P(1, 0, "decode"), P(1, 0, "decode"), 0, 16, 16), {3: 2})
    _add(f"llama-M{M}-key3=3", (M, *LL, 384), _ran(P(1, 0, "decode"), P(0, 0, "decode", 2, "row"), 1, 16, 0), {3: 3}, ("random",))
    for ks in (1, 2):
        _add(f"llama-M{M}-key6={ks}", (M, *LL, 384), HALF if M <= 16 else MSPLIT, {6: ks})
for M in (1, 17, 64):
    # key 3 = 0: K = 256 gives the O projection one slice (8 k-steps: fewer than 8 per half), FFN-down two
    _add(f"llama-M{M}-key3=0", (M, *LL, 384), sk(0, 2), {3: 0})
    for s in (1, 2, 4):
        _add(f"llama-M{M}-key3=0-key1={s}", (M, *LL, 384), sk(s if s > 1 else 0, s if s > 1 else 0), {3: 0, 1: s})
_add("wide-H4096-M8", (8, 4096, 256, 256, 384), _ran(P(1, 0, "msplit"), P(1, 0, "msplit"), 0, 256, 256))     # 5
# H = 2048 at 8 rows: half tiles, 256 partials of 8 columns per row (a lost one is 0.4 % of the sum)
_add("h2048-M8", (8, 2048, 256, 256, 384), _ran(P(1, 1, "msplit"), P(1, 1, "msplit"), 0, 256, 256), None, ("random",))
for M in (5, 40):                                                                                              # 6
    _add(f"llama-M{M}-alpha0.22", (M, *LL, 384), HALF if M <= 16 else MSPLIT, None, ("random",), residual_multiplier=0.22)
    _add(f"llama-M{M}-alpha0.22-key3=0", (M, *LL, 384), sk(0, 2), {3: 0}, ("random",), residual_multiplier=0.22)
    _add(f"llama-M{M}-alpha0.5", (M, *LL, 384), HALF if M <= 16 else MSPLIT, None, ("exact",), residual_multiplier=0.5)
    _add(f"llama-M{M}-alpha0.5-key3=0-key1=2", (M, *LL, 384), sk(2, 2), {3: 0, 1: 2}, ("exact",), residual_multiplier=0.5)
for M in (5, 40):                                                                                              # 7
    _add(f"llama-last-M{M}", (M, *LL, 1003), HALF if M <= 16 else MSPLIT, has_next=False)
# 40 prefill rows of three sequences: M <= 64, so the O projection still carries the FFN norm; the last layer's FFN-down
# may not carry the final norm (M != n_seqs), leaves two slices, and the rows_idx form of norm_row_kernel sums them into
# the three rows it reads
_add("llama-last-rows", (40, *LL, 1003), _ran(P(1, 0, "msplit"), P(0, 0, "decode", 2, "row_idx"), 1, 16, 0),
     has_next=False, last_rows=[9, 24, 39], max_len=15)
for M in (5, 16, 40):          # a ragged next projection behind the half-tile and the full-tile consumers
    _add(f"llama-M{M}-ragged", (M, *LL, 1003), HALF if M <= 16 else MSPLIT)
for M in (1, 16, 17, 64):                                                                                      # 8
    _add(f"gpt2-M{M}", (M, 768, 768, 3072, 384), sk(2, 4), None, ("random",), norm="layer", act="gelu", biases=True)
for H in (192, 256):                                                                                           # 9
    for M in (3, 40):
        for tag, mult in (("", {}), ("-mults", dict(attention_multiplier=0.7, residual_multiplier=0.22))):
            # q_width 512: the O projection's 16 k-steps split in two; FFN-down then finds a pending add and adds into x
            _add(f"falcon-H{H}-M{M}{tag}", (M, H, 512, 512, 384), sk(2, 0), None, ("random",), norm="layer", act="gelu",
                 block="parallel", **mult)
# 10: the tile kernel's split-K: 2 x 16 (5 x 16) tiles, K = 2048: 2 slices (K / 4 = 512), 4 slices (K / 8 = 256 < 512: stop)
BIG = (2048, 2048, 2048)
_add("tile-M130", (130, *BIG, 384), sk(4, 4, form="tile"), None, ("random", "exact"), max_len=130)
_add("tile-M520", (520, *BIG, 384), sk(4, 4, "tile16", "tile16", form="tile"), None, ("random",), max_len=520)
# key 26 = 0 (the tile split off): at 130 rows the projections then fall to the DECODE kernel's 64-row groups (2 x 16 tiles
# are fewer than g_chunk_min_tiles), adding in the launch; only at 520 rows (> g_chunk_max_m) does the tile kernel's own
# fused add run
_add("groups-M130-key26=0", (130, *BIG, 384), sk(0, 0, form="groups"), {26: 0}, ("random",), max_len=130)
_add("tile-M520-fused", (520, *BIG, 384), sk(0, 0, form="tile"), {26: 0}, ("random",), max_len=520)


def make_inputs(case, family):
    c = CASES[case]
    kw = dict(c["kw"])
    if family == "exact":
        if "residual_multiplier" not in kw:
            kw["residual_multiplier"] = 0.0
        return exact_inputs(*c["shape"], **kw)
    return random_inputs(*c["shape"], **kw)


OP_KEYS = ("bo", "norm_b", "b1", "b2", "next_norm_b", "norm", "act", "block", "residual_multiplier", "attention_multiplier",
           "norm_eps", "max_len", "last_rows", "has_next")


def op_args(inp):
    """the arguments of ops.dense_stages"""
    pos = [inp[k] for k in ("x", "attn_out", "wo", "norm_w", "w1", "w2", "next_norm_w", "wn")]
    return pos, {k: inp[k] for k in OP_KEYS if k in inp}


# ---- the assertions ---------------------------------------------------------------------------------------------------
def _ratio(dev, f64, emu):
    den = row_rms(emu - f64)
    assert (den > 0).all(), "the emulation does not differ from float64: the ratio is undefined"
    return row_rms(_f64(dev) - f64) / den


def _resid_exact_bound(xin, a, w, bias, alpha):
    """worst-case error of an fp32 evaluation of xin + alpha (a . w^T + bias) in any order, elementwise"""
    K = a.shape[1]
    mag = np.abs(_f64(a)) @ np.abs(_f64(w)).T + (0.0 if bias is None else np.abs(_f64(bias)))
    return (K + 2) * U24 * abs(alpha) * mag + 2 * U24 * (np.abs(_f64(xin)) + abs(alpha) * mag)


def check_operand(x_dev, op, rs, w, b, inp, figures, stage, rows=None):
    """the operand a projection reads, from the device's own x: bit for bit + derived partial bounds on the deferred path,
    the rms ratio on the norm path"""
    H = x_dev.shape[1]
    xs = x_dev if rows is None else x_dev[rows]
    if rs is not None:
        assert rows is None
        assert np.array_equal(op, xn_raw32(x_dev, w)), f"{stage}: xn_raw is not bf16(fp32(x) * fp32(w))"
        tiles = rs.shape[1]
        n = H // tiles
        want = partials64(x_dev, tiles)
        rel = np.abs(_f64(rs) - want) / np.where(want > 0, want, 1.0)
        print(f"{stage}: partials [{rs.shape[0]}][{tiles}] rel err {rel.max():.2e} (bound {(n + 1) * U24:.2e})")
        assert np.isfinite(rs).all() and rel.max() <= (n + 1) * U24, f"{stage}: an x^2 partial is off"
        r_dev, r_64 = rstd_of(rs, H, inp["norm_eps"]), rstd_of(want, H, inp["norm_eps"])
        assert (np.abs(r_dev - r_64) <= 1e-6 * r_64).all(), f"{stage}: rstd from the device's partials"
        if inp["family"] == "exact" and stage == "op1":       # (x2 holds the device's h: no integers any more)
            assert np.array_equal(_f64(rs), want), f"{stage}: partials are not exact"
            assert np.array_equal(_f64(rs).sum(1), want.sum(1)), f"{stage}: row sums of the partials"
        return
    kind = inp.get("norm", "rms")
    f64 = norm64(xs, w, b, inp["norm_eps"], kind)
    assert np.isfinite(op).all(), f"{stage}: NaN in a normed operand"
    figures[stage] = _ratio(op, f64, _r64(f64))


def check_stages(inp, out, bound, name=""):
    """every stage of out against the reference fed the stage before -> {stage: per-row ratios} (random family)"""
    fam, fig = inp["family"], {}
    a_o, a_d = alphas(inp)
    last = not inp.get("has_next", True)
    rows = np.asarray(inp["last_rows"] if inp.get("last_rows") is not None else np.arange(inp["x"].shape[0])) if last else None
    for k in ("x1", "op1", "h", "x2", "op2", "yn"):
        assert np.isfinite(out[k]).all(), f"{name}: NaN in {k}: something no launch wrote was read"
    # x1
    if fam == "exact":
        assert np.array_equal(_f64(out["x1"]), resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a_o, False)), f"{name}: x1 is not exact"
    else:
        f64 = resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a_o, False)
        fig["x1"] = _ratio(out["x1"], f64, resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a_o, True))
    # FFN-up's operand.  The parallel block normalises the layer's INPUT (the op runs that norm first)
    src = inp["x"] if inp.get("block") == "parallel" else out["x1"]
    check_operand(src, out["op1"], out["rs1"], inp["norm_w"], inp.get("norm_b"), inp, fig, "op1")
    # h
    h64 = ffn_h(out["op1"], out["rs1"], inp, False)
    if fam == "exact":
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(h64), 1e-300))) - 7)
        tol = 0.5 * ulp + H_F32_MARGIN * H_F32_REL * np.abs(h64)
        bad = np.abs(_f64(out["h"]) - h64) > tol
        assert not bad.any(), f"{name}: h off in rows {np.flatnonzero(bad.any(1))[:8]}"
    else:
        fig["h"] = _ratio(out["h"], h64, ffn_h(out["op1"], out["rs1"], inp, True))
    # x2 from the device's x1 and h
    f64 = resid(out["x1"], out["h"], inp["w2"], inp.get("b2"), a_d, False)
    if fam == "exact" or inp.get("fmt"):      # (quantized: h and W~ are both exact in bf16 — the emulation IS float64, no ratio)
        err = np.abs(_f64(out["x2"]) - f64)
        assert (err <= _resid_exact_bound(out["x1"], out["h"], inp["w2"], inp.get("b2"), a_d)).all(), f"{name}: x2 beyond the fp32 dot product bound"
    else:
        fig["x2"] = _ratio(out["x2"], f64, resid(out["x1"], out["h"], inp["w2"], inp.get("b2"), a_d, True))
    # the next operand: from x2 — on the last_rows form from x_end, whose listed rows the norm completed
    xsrc = out["x2"]
    if last and out["rs2"] is None:
        assert np.array_equal(out["x_end"][rows], out["x2"][rows]), f"{name}: the rows the final norm read are not complete in x"
    check_operand(xsrc, out["op2"], out["rs2"], inp["next_norm_w"], inp.get("next_norm_b"), inp, fig, "op2",
                  rows if (last and out["rs2"] is None) else None)
    # yn
    op2, rs2 = out["op2"], out["rs2"]
    if last and rs2 is not None:
        op2, rs2 = op2[rows], rs2[rows]
    y64r = next_y(op2, rs2, inp, True)
    assert out["yn"].shape == y64r.shape, (out["yn"].shape, y64r.shape)
    e = np.abs(_f64(out["yn"]) - y64r).max() / np.abs(y64r).max()
    print(f"{name}: yn against the float64 product of its bf16 operands: {e:.2e} of max")
    assert e <= F32_TOL, f"{name}: yn"
    if fam != "exact" and not inp.get("wn_quantized"):      # (a quantized wn is exact in bf16, like its operand: F32_TOL above holds yn)
        fig["yn"] = _ratio(out["yn"], next_y(op2, rs2, inp, False), y64r)
    for stage, r in fig.items():
        print(f"{name} {stage}: max row ratio {r.max():.4f} (row {int(r.argmax())})")
    for stage, r in fig.items():
        assert r.max() <= bound, (name, stage, float(r.max()), int(r.argmax()))
    return fig


# ---- quantized weights (tests/test_dense_q_ops_gpu.py; ops.dense_stages(..., weight_format=...)) ----------------------
# The op quantizes wo, w1, w2 (and wn where a model would) itself — the upload quantizer, then finalize's fuse_w1 and
# registration —; the reference computes with W~ of the bit-exact numpy mirrors (moe_reference.mirror), so quantization
# error is in no figure.  W~ is exact in bf16: every rounding point above is unchanged, the projections' weight operand just
# has nothing left to round.  Where BOTH operands of a product are exact in bf16 — x2 = x1 + alpha h . W~2^T from the
# device's own h, and yn behind a quantized wn — the emulation equals float64 and a ratio is undefined: x2 is held to the
# exact family's fp32 dot product bound instead (in both families), yn to F32_TOL alone.
import moe_reference as MR

Q_FORMATS = (("fp8", 0), ("mxfp4", 0), ("int4", 32), ("int4", 64), ("int4", 128))      # (format, INT4 group)
Q_WEIGHTS = ("wo", "w1", "w2", "wn")


def next_is_quantized(fmt, has_next):
    """what quantize_next = -1 decides, as a model: the next layer's QKV follows the format; the LM head only under fp8"""
    return fmt != "bf16" and (has_next or fmt == "fp8")


def exact_int4(rng, n, k, g):
    """test_int4_weights_gpu.exact_weights with e = 0: integers (q - z), q = 0 and q = 15 present in every group of g ->
    range 15, s = 1, W~ == w bit for bit.  (-1, 0, 1 do NOT survive INT4: their range 2 gives s = 2 / 15.)"""
    from test_int4_weights_gpu import exact_weights
    w, e = exact_weights(rng, n, k, g)                       # (q - z) 2^e per group
    return (w.reshape(n, k // g, g) * np.exp2(-e)).astype(np.float32).reshape(n, k)


def exact_inputs_q(M, H, qw, F, Nn, fmt, g, **kw):
    """exact_inputs whose weights survive the format unchanged.  fp8 / MXFP4: the family's {-1, 0, 1} as they are.  INT4:
    exact_int4 weights up to +-15 — with attn_out thinned to 16 non-zeros per row (|x1| stays below 256: xn_raw's integers fit
    bf16, every partial sum stays below 2^24) and the norm weights 2^-9..2^-7 instead of 2^-5..2^-3 (the pre-activations g, u
    keep the size they have with {-1, 0, 1} weights, for which H_F32_REL was worked out).  exact_inputs' own assertions run on
    the result."""
    if fmt != "int4":
        return exact_inputs(M, H, qw, F, Nn, **kw)
    r = np.random.default_rng(11 * M + H + qw + F + Nn + g)
    attn = np.zeros((M, qw), np.float32)
    for m in range(M):
        attn[m, r.permutation(qw)[:16]] = r.integers(-1, 2, 16)
    p2 = lambda: (2.0 ** r.integers(-9, -6, H)).astype(np.float32)
    return exact_inputs(M, H, qw, F, Nn, attn_out=attn, wo=exact_int4(r, H, qw, g), w1=exact_int4(r, 2 * F, H, g),
                        w2=exact_int4(r, H, F, g), wn=exact_int4(r, Nn, H, g), norm_w=p2(), next_norm_w=p2(), **kw)


def crafted_rows(w, fmt, g, seed):
    """the crafted groups of the format's weight test in the first rows of w (moe_reference.crafted_experts on one matrix)"""
    return MR.crafted_experts(np.asarray(w, np.float32)[None], fmt, g, seed)[0]


def quantize(inp, fmt, g, crafted=True):
    """inp with wo, w1, w2 (and wn, where a model quantizes it) replaced by W~ of the mirror; raw_*: what the op is given"""
    mir = MR.mirror(fmt)
    out = dict(inp, fmt=fmt, g=g, wn_quantized=next_is_quantized(fmt, inp.get("has_next", True)))
    for i, k in enumerate(Q_WEIGHTS):
        raw = crafted_rows(inp[k], fmt, g, 21 + i) if crafted else np.asarray(inp[k], np.float32)
        out["raw_" + k] = raw
        out[k] = mir(raw, g)["wt"] if (k != "wn" or out["wn_quantized"]) else raw
    return out


def q_formats(case):
    """the (format, group) pairs a case runs in: INT4 groups that divide hidden, q_width and ffn"""
    _, H, qw, F, _ = CASES_Q[case]["shape"]
    return [(f, g) for f, g in Q_FORMATS if f != "int4" or (H % g == 0 and qw % g == 0 and F % g == 0)]


def quantized_inputs(case, family, fmt, g):
    c = CASES_Q[case]
    kw = dict(c["kw"])
    if family == "exact":
        kw.setdefault("residual_multiplier", 0.0)
        inp = quantize(exact_inputs_q(*c["shape"], fmt, g, **kw), fmt, g, crafted=False)
        for k in Q_WEIGHTS:
            assert np.array_equal(inp[k].view(np.uint32), inp["raw_" + k].view(np.uint32)), f"{case}: {k} does not survive {fmt}"
        return inp
    return quantize(random_inputs(*c["shape"], **kw), fmt, g)


def op_args_q(inp):
    """the arguments of ops.dense_stages for quantized inputs: the raw weights, the format"""
    pos = [inp[k] for k in ("x", "attn_out", "raw_wo", "norm_w", "raw_w1", "raw_w2", "next_norm_w", "raw_wn")]
    kw = {k: inp[k] for k in OP_KEYS if k in inp}
    return pos, dict(kw, weight_format=inp["fmt"], group_size=inp["g"])


def check_wt(out, inp):
    """W~ as the device holds it after finalize (fuse_w1's interleave undone) equals the mirror bit for bit"""
    for k in Q_WEIGHTS:
        got = out["wt_" + k[1:]]
        if k == "wn" and not inp["wn_quantized"]:
            assert got is None, "wt_n of a projection that stays bf16"
            continue
        want = inp[k]
        assert got is not None and got.shape == want.shape, (k, None if got is None else got.shape, want.shape)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"W~ of {k} differs from the {inp['fmt']} mirror at {len(bad)} places, first (matrix, row, k) = {(k, *map(int, bad[0]))}"


# The case table of the quantized file: the bf16 cases it keeps, by name, with their literals — gemm.h: "every weight format
# takes the same decisions" —, and the shapes the bf16 file does not have.  New literals by hand from resid_gemm / the launchers:
#  ragged-*   K = 768 = 24 k-steps in both residual projections.  Deferred: g_msplit_ks = 8 -> 24 / 8 = 3 < 4 -> ks = 4, six
#             k-steps a wave: waves 1 and 3 start at k = 192 and 576, inside a 128-group.  The form is the ladder's (half tiles
#             at 5 rows, m_split at 40).  Key 3 = 0, key 1 = 2: two slices of 12 k-steps each, cut at k = 384.
#  wide-*     F = 8192: FFN-up has 2 F / 64 = 256 groups -> the wide kernel (rows > 16) reading rs_in, PASSES at 100 rows
#             (256 / NTB % 8 == 0); FFN-down runs K = 8192 (256 k-steps, ks = 8) as the ladder's producer: m_split up to 64
#             rows, 64-row groups at 100 (16 weight blocks, a multiple of 8: one launch).
CASES_Q = {}
for _n in (["llama-M%d" % M for M in (1, 5, 16, 17, 32, 33, 64, 65, 100, 128, 129)] + ["llama-M100-serial", "llama-M5-nohalf"] +
           ["llama-M%d-key3=0%s" % (M, t) for M in (1, 17, 64) for t in ("", "-key1=2", "-key1=4")] +
           ["llama-M%d-key3=%d" % (M, k) for M in (5, 40) for k in (2, 3)] + ["h2048-M8", "wide-H4096-M8"] +
           ["llama-last-M5", "llama-last-M40", "llama-last-rows"] + ["gpt2-M%d" % M for M in (1, 17, 64)] +
           ["falcon-H%d-M%d" % (H, M) for H in (192, 256) for M in (3, 40)] + ["tile-M130", "tile-M520", "groups-M130-key26=0"]):
    CASES_Q[_n] = CASES[_n]
for _n in ("h2048-M8", "wide-H4096-M8"):
    CASES_Q[_n] = dict(CASES[_n], families=("random",))
for M in (5, 40):
    CASES_Q[f"ragged-M{M}"] = dict(shape=(M, 256, 768, 768, 384), ran=HALF if M <= 16 else MSPLIT, keys={}, families=("random", "exact"), kw={})
    CASES_Q[f"ragged-M{M}-key3=0-key1=2"] = dict(shape=(M, 256, 768, 768, 384), ran=sk(2, 2), keys={3: 0, 1: 2}, families=("random", "exact"), kw={})
for M in (17, 33, 64, 100):
    CASES_Q[f"wide-F8192-M{M}"] = dict(shape=(M, 256, 256, 8192, 384), ran=MSPLIT if M <= 64 else GROUPS, keys={}, families=("random",), kw={})
Q_PARAMS = [(n, fam, f, g) for n, c in CASES_Q.items() for fam in c["families"] for f, g in q_formats(n)]


def _scaled_from(m, fmt, rows_from=None, groups_from=None, zero_points=True):
    """W~ of a mirror result m with every row's scales (and zero points) taken from row rows_from[r], every group's from
    group groups_from[j] of the same row: what a kernel computes that fetches the wrong scale"""
    wt = _f64(m["wt"])
    N, K = wt.shape
    rf = np.arange(N) if rows_from is None else np.asarray(rows_from)
    if fmt == "fp8":
        s = _f64(m["s"])
        return round_bf16((wt / s[:, None] * s[rf][:, None]).astype(np.float32))
    G = m["s"].shape[1]
    gf = np.arange(G) if groups_from is None else np.asarray(groups_from)
    if fmt == "mxfp4":
        e = m["s"].astype(np.int64)
        return np.ldexp(wt.reshape(N, G, -1), (e[rf][:, gf] - e)[:, :, None]).reshape(N, K).astype(np.float32)
    c = m["codes"]
    q = np.stack([c & 15, c >> 4], -1).reshape(N, G, -1).astype(np.float64)
    s, z = _f64(m["s"])[rf][:, gf], _f64(m["z"])[rf][:, gf] * (1.0 if zero_points else 0.0)
    return round_bf16((s[:, :, None] * (q - z[:, :, None])).astype(np.float32)).reshape(N, K)


Q_MUTATIONS = ("w1_scales_before_interleave", "group_off_by_one_at_wave_start", "zero_point_dropped", "slice_last_kstep_skipped",
               "rstd_on_the_scale", "second_group_first_scales", "wt1_interleaved")


def _mutated_weights(inp, ran, mut):
    """the weights a kernel with the mutation computes with (the stand-in still REPORTS the mirror's W~)"""
    fmt, g = inp.get("fmt"), inp.get("g", 0)
    if fmt is None or mut not in ("w1_scales_before_interleave", "group_off_by_one_at_wave_start", "zero_point_dropped"):
        return {}
    mir = MR.mirror(fmt)
    if mut == "w1_scales_before_interleave":      # device row p holds canonical row idx[p] but keeps the scales of canonical row p
        F = inp["w1"].shape[0] // 2
        idx = np.arange(2 * F).reshape(2, F // 16, 16).transpose(1, 0, 2).reshape(-1)      # fuse_w1's interleave
        src = np.empty(2 * F, np.int64)
        src[idx] = np.arange(2 * F)
        return dict(w1=_scaled_from(mir(inp["raw_w1"], g), fmt, rows_from=src))
    if mut == "zero_point_dropped":
        assert fmt == "int4"
        return dict(wo=_scaled_from(mir(inp["raw_wo"], g), fmt, zero_points=False))
    # the O projection's producer form: ks waves of K / 32 / ks k-steps each; a wave's first k-step takes the group before its own
    assert fmt in ("mxfp4", "int4") and ran["o"]["producer"]
    K = inp["wo"].shape[1]
    ks = 8
    while ks > 1 and (K // 32) // ks < 4:
        ks //= 2
    m = mir(inp["raw_wo"], g)
    per = g if fmt == "int4" else 32
    bad = _scaled_from(m, fmt, groups_from=np.maximum(np.arange(K // per) - 1, 0))
    wo = np.array(inp["wo"], np.float32)
    for w in range(1, ks):
        k0 = w * (K // 32 // ks) * 32
        wo[:, k0:k0 + 32] = bad[:, k0:k0 + 32]
    return dict(wo=wo)


# ---- a stand-in for ops.dense_stages made of the reference alone (tests/test_dense_reference_host.py) ----------------
MUTATIONS = ("slice_dropped", "bias_every_slice", "alpha_on_x", "tile_missing", "eps_left_out", "normalised_before_rounding",
             "rows_15_16_swapped", "second_group_first_rstd", "gate_up_swapped", "multiplier_skipped") + Q_MUTATIONS


def emulated_device(inp, ran, mut=None):
    """float64 with the kernels' bf16 roundings, stored as fp32, in the shape of ops.dense_stages' result; mut: one of
    MUTATIONS, applied where the kernel would go wrong.  Quantized inputs (quantized_inputs): computes with W~ and reports it
    as wt_o / wt_1 / wt_2 / wt_n."""
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    given = inp
    inp = dict(inp, **_mutated_weights(inp, ran, mut))
    a_o, a_d = alphas(inp)
    eps, kind = inp["norm_eps"], inp.get("norm", "rms")
    M, H = inp["x"].shape
    last = not inp.get("has_next", True)
    rows = np.asarray(inp["last_rows"] if inp.get("last_rows") is not None else np.arange(M)) if last else None

    def residual(xin, a, w, bias, alpha, slices):
        s = max(slices, 1)
        K = a.shape[1]
        cuts = [K * i // s for i in range(s + 1)]
        ends = [c - 32 if (mut == "slice_last_kstep_skipped" and s > 1) else c for c in cuts]
        parts = [_r64(a)[:, cuts[i]:ends[i + 1]] @ _r64(w)[:, cuts[i]:ends[i + 1]].T for i in range(s)]
        b = 0.0 if bias is None else _f64(bias)
        if mut == "slice_dropped" and s > 1:
            parts = parts[:-1]
        nb = len(parts) if mut == "bias_every_slice" else 1
        al = 1.0 if (mut == "multiplier_skipped" and s > 1) else np.float64(np.float32(alpha))
        if mut == "alpha_on_x":
            return al * _f64(xin) + (sum(parts) + nb * b)
        return _f64(xin) + al * (sum(parts) + nb * b)

    def operand(xc, w, b, tiles, sel=None):
        if tiles:
            rs = f32(partials64(f32(xc), tiles))
            if mut == "tile_missing":
                rs[:, tiles // 2] = 0.0
            if mut == "normalised_before_rounding":
                return round_bf16(f32(norm64(f32(xc), w, None, eps, "rms"))), rs
            return xn_raw32(f32(xc), w), rs
        xs = f32(xc) if sel is None else f32(xc)[sel]
        return round_bf16(f32(norm64(xs, w, b, 0.0 if mut == "eps_left_out" else eps, kind))), None

    x1 = residual(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a_o, ran["o"]["slices"])
    if mut == "second_group_first_scales" and M > 64:
        # the 64-row groups of one launch: weight block b of group 1 fetching the scales of block b // 2 (an index that
        # forgot the groups are interleaved with the weight blocks)
        m = MR.mirror(inp["fmt"])(inp["raw_wo"], inp["g"])
        n = inp["wo"].shape[0]
        wo_bad = _scaled_from(m, inp["fmt"], rows_from=(np.arange(n) // 16 // 2) * 16 + np.arange(n) % 16)
        x1[64:] = residual(inp["x"], inp["attn_out"], wo_bad, inp.get("bo"), a_o, ran["o"]["slices"])[64:]
    if mut == "rows_15_16_swapped" and M > 16:
        x1[[15, 16]] = x1[[16, 15]]
    src = inp["x"] if inp.get("block") == "parallel" else x1
    op1, rs1 = operand(src, inp["norm_w"], inp.get("norm_b"), ran["rs1_tiles"])
    rs_h = rs1
    if rs1 is not None and mut == "eps_left_out":
        rs_h = rs1 - np.float32(eps * H / rs1.shape[1])
    if rs1 is not None and mut == "second_group_first_rstd" and M > 64:
        rs_h = rs1.copy()
        rs_h[64:] = rs1[:M - 64]
    if rs1 is not None and mut == "rstd_on_the_scale":
        # rstd folded into the dequantized weight, W~' = bf16(rstd W~), instead of scaling the fp32 accumulator: one more rounding
        rstd = rstd_of(rs1, H, eps)
        h = np.concatenate([ffn_h(op1[m:m + 1], None, dict(inp, w1=round_bf16(f32(rstd[m] * _f64(inp["w1"])))), True) for m in range(M)])
        h = f32(h)
    else:
        h = f32(ffn_h(op1, rs_h, inp, True, swap=(mut == "gate_up_swapped")))
    x2 = residual(f32(x1), h, inp["w2"], inp.get("b2"), a_d, ran["down"]["slices"])
    sel = rows if (last and not ran["rs2_tiles"]) else None
    op2, rs2 = operand(x2, inp["next_norm_w"], inp.get("next_norm_b"), ran["rs2_tiles"], sel)
    o2, r2 = (op2, rs2) if not (last and rs2 is not None) else (op2[rows], rs2[rows])
    yn = f32(next_y(o2, r2, inp, True))
    out = dict(x1=f32(x1), op1=op1, rs1=rs1, h=h, x2=f32(x2), op2=op2, rs2=rs2, yn=yn, x_end=f32(x2), ran=ran)
    if given.get("fmt"):
        out.update({"wt_" + k[1:]: (given[k].copy() if (k != "wn" or given["wn_quantized"]) else None) for k in Q_WEIGHTS})
        if mut == "wt1_interleaved":
            F = given["w1"].shape[0] // 2
            out["wt_1"] = given["w1"][np.arange(2 * F).reshape(2, F // 16, 16).transpose(1, 0, 2).reshape(-1)]
    return out


# ---- the MoE chain: O projection (producer) -> moe(deferred_norm) -> pending moe_part (ops.dense_moe_stages) ----------
# (moe_reference's softmax / route / tolerances: the routing is held exactly as test_moe_ops_gpu.py holds it)

MOE_SHAPE = dict(H=256, qw=256, E=8, k=2, I=64)
# (M, tuning keys, MoE form, ran): E = 8 -> moe_down_slices = 4 slices left in moe_part; the O projection is the producer
# (half tiles up to 16 rows), no norm launch; the down projection is no resid_gemm, its record holds the slices only
MOE_CASES = [(M, keys, form, _ran(P(1, 1 if M <= 16 else 0, "msplit"), P(0, 0, "tile", 4), 0, 32 if M <= 16 else 16, 0))
             for M in (1, 16, 40) for keys, form in (({}, "dense_fused"), ({31: 0}, "dense"))]


# quantized experts (tests/test_moe_q_ops_gpu.py): the same chain per format (INT4 g = 64) with W~ in inp, and one
# Granite-shaped case — 64 rows, E = 32, k = 8, I = 512, INT4 g = 128: MT = 4 and the wide up form under the deferred scale
# (fmt, group, M, keys, form, ran, shape)
GRANITE_SHAPE = dict(H=256, qw=256, E=32, k=8, I=512)
MOE_Q_CASES = ([(fmt, 64, M, keys, form, ran, MOE_SHAPE) for fmt in MR.FORMATS for M, keys, form, ran in MOE_CASES]
               + [("int4", 128, 64, {}, "dense_fused", _ran(P(1, 0, "msplit"), P(0, 0, "tile", 4), 0, 16, 0), GRANITE_SHAPE)])


def moe_inputs_q(M, fmt, g, shape=None):
    """moe_inputs with W~ of the format in w_in / w_out (the reference's experts) and the unquantized ones, which the op
    is given, in raw_in / raw_out"""
    return MR.quantized(moe_inputs(M, shape=shape), fmt, g)


def moe_inputs(M, seed=0, shape=None):
    s = shape or MOE_SHAPE
    r = np.random.default_rng(977 * M + seed)
    n = lambda *sh: r.standard_normal(sh, dtype=np.float32)
    inp = dict(x=n(M, s["H"]), attn_out=n(M, s["qw"]), wo=n(s["H"], s["qw"]) * 0.05, norm_w=1.0 + 0.3 * n(s["H"]),
               router=n(s["H"], s["E"]) * 0.3, w_in=n(s["E"], 2 * s["I"], s["H"]) * 0.1, w_out=n(s["E"], s["H"], s["I"]) * 0.1,
               next_norm_w=1.0 + 0.3 * n(s["H"]), k=s["k"], norm_eps=1e-5, family="random", residual_multiplier=0.0)
    inp["x"][3::7] *= 1e-3
    inp["attn_out"][3::7] *= 1e-3
    return inp


def moe_logits(op, rs, inp):
    """rstd x the raw product: float64 from the device's operand and partials, the router through bf16"""
    return (_f64(op) @ _r64(inp["router"])) * rstd_of(rs, op.shape[1], inp["norm_eps"])[:, None]


def moe_experts(op, rs, inp, gate, rounded):
    """sum_e W_out[e] bf16(silu(g) u gate[m][e]), [g | u] = rstd (op . W_in[e]^T) — the dense forms fold the gate before h's
    rounding (moe_reference.experts_emulated), the operand is scaled after the product"""
    cv = _r64 if rounded else _f64
    E, _, I = inp["w_out"].shape
    rstd, gate = rstd_of(rs, op.shape[1], inp["norm_eps"]), _f64(gate)
    y = np.zeros(op.shape)
    for e in range(E):
        rows = np.flatnonzero(gate[:, e])
        if rows.size:
            gu = (_f64(op)[rows] @ cv(inp["w_in"][e]).T) * rstd[rows, None]
            h = silu(gu[:, :I]) * gu[:, I:] * gate[rows, e][:, None]
            y[rows] += (_r64(h) if rounded else h) @ cv(inp["w_out"][e]).T
    return y


def check_moe_chain(inp, out, bound, name=""):
    """x1 and the deferred operand as in check_stages; the router logits against rstd x the raw product (F32_TOL of the
    largest); the routing fed the device's logits (moe_reference's rules and tolerances); y per row against the experts fed
    the device's x1, operand, partials and gate"""
    a = alphas(inp)[0]
    k = inp["k"]
    for key in ("x1", "op1", "router_logits", "gate", "y"):
        assert np.isfinite(out[key]).all(), f"{name}: NaN in {key}: something no launch wrote was read"
    assert out["rs1"] is not None, f"{name}: the O projection did not carry the FFN norm"
    fig = {}
    f64 = resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a, False)
    fig["x1"] = _ratio(out["x1"], f64, resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a, True))
    check_operand(out["x1"], out["op1"], out["rs1"], inp["norm_w"], None, inp, fig, "op1")
    lg, want = _f64(out["router_logits"]), moe_logits(out["op1"], out["rs1"], inp)
    e_lg = float(np.abs(lg - want).max() / np.abs(want).max())
    got = _f64(out["gate"])
    chosen = got != 0
    assert (chosen.sum(1) == k).all(), f"{name}: a row without exactly k experts"
    lo, hi = np.where(chosen, lg, np.inf).min(1), np.where(chosen, -np.inf, lg).max(1)
    p = np.where(chosen, MR.softmax(lg), 0.0)
    wantg = p / p.sum(1, keepdims=True)
    e_w = float((np.abs(got - wantg).max(1) / wantg.max(1)).max())
    print(f"{name}: router logits {e_lg:.2e} of max, gate weights {e_w:.2e}")
    assert e_lg <= F32_TOL, f"{name}: the router logits are not rstd x the raw product"
    assert (lo >= hi - MR.SOFTMAX_TOL * np.abs(lg).max()).all(), f"{name}: an unchosen logit above a chosen one"
    assert e_w <= MR.SOFTMAX_TOL, f"{name}: gate weights"
    y64 = _f64(out["x1"]) + np.float64(np.float32(a)) * moe_experts(out["op1"], out["rs1"], inp, out["gate"], False)
    yem = _f64(out["x1"]) + np.float64(np.float32(a)) * moe_experts(out["op1"], out["rs1"], inp, out["gate"], True)
    fig["y"] = _ratio(out["y"], y64, yem)
    for stage, r in fig.items():
        print(f"{name} {stage}: max row ratio {r.max():.4f} (row {int(r.argmax())})")
        assert r.max() <= bound, (name, stage, float(r.max()), int(r.argmax()))
    return fig


MOE_MUTATIONS = ("router_without_rstd", "up_without_rstd", "neighbour_rstd")


def emulated_moe_device(inp, ran, form, mut=None):
    """the stand-in for ops.dense_moe_stages; mut: the router / the expert up projection forgetting the deferred scale, or
    taking the next row's (a wrong stride into the partials)"""
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    a = alphas(inp)[0]
    x1 = f32(resid(inp["x"], inp["attn_out"], inp["wo"], inp.get("bo"), a, True))
    op1, rs1 = xn_raw32(x1, inp["norm_w"]), f32(partials64(x1, ran["rs1_tiles"]))
    H = x1.shape[1]
    ones = np.full_like(rs1, (1.0 - inp["norm_eps"]) * H / rs1.shape[1])            # partials that give rstd = 1
    rs_r = ones if mut == "router_without_rstd" else rs1
    rs_u = ones if mut == "up_without_rstd" else (np.roll(rs1, -1, 0) if mut == "neighbour_rstd" else rs1)
    lg = f32(moe_logits(op1, rs_r, inp))
    gate = f32(MR.route(lg, inp["k"]))
    y = f32(_f64(x1) + np.float64(np.float32(a)) * moe_experts(op1, rs_u, inp, gate, True))
    return dict(x1=x1, op1=op1, rs1=rs1, router_logits=lg, gate=gate, y=y, form=form, ran=ran)
