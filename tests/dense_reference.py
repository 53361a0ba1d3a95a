"""The dense layer tail (generic_model.go:320-326,383-418: O projection, FFN norm, FFN-up, FFN-down, the next norm, the
next projection) in float64, stage by stage — numpy only, test infrastructure like tests/moe_reference.py — plus the
inputs, the case table and the assertions tests/test_dense_ops_gpu.py and tests/test_dense_reference_host.py share.

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
    if fam == "exact":
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
    if fam != "exact":
        fig["yn"] = _ratio(out["yn"], next_y(op2, rs2, inp, False), y64r)
    for stage, r in fig.items():
        print(f"{name} {stage}: max row ratio {r.max():.4f} (row {int(r.argmax())})")
    for stage, r in fig.items():
        assert r.max() <= bound, (name, stage, float(r.max()), int(r.argmax()))
    return fig


# ---- a stand-in for ops.dense_stages made of the reference alone (tests/test_dense_reference_host.py) ----------------
MUTATIONS = ("slice_dropped", "bias_every_slice", "alpha_on_x", "tile_missing", "eps_left_out", "normalised_before_rounding",
             "rows_15_16_swapped", "second_group_first_rstd", "gate_up_swapped", "multiplier_skipped")


def emulated_device(inp, ran, mut=None):
    """float64 with the kernels' bf16 roundings, stored as fp32, in the shape of ops.dense_stages' result; mut: one of
    MUTATIONS, applied where the kernel would go wrong"""
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    a_o, a_d = alphas(inp)
    eps, kind = inp["norm_eps"], inp.get("norm", "rms")
    M, H = inp["x"].shape
    last = not inp.get("has_next", True)
    rows = np.asarray(inp["last_rows"] if inp.get("last_rows") is not None else np.arange(M)) if last else None

    def residual(xin, a, w, bias, alpha, slices):
        s = max(slices, 1)
        K = a.shape[1]
        cuts = [K * i // s for i in range(s + 1)]
        parts = [_r64(a)[:, cuts[i]:cuts[i + 1]] @ _r64(w)[:, cuts[i]:cuts[i + 1]].T for i in range(s)]
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
    h = f32(ffn_h(op1, rs_h, inp, True, swap=(mut == "gate_up_swapped")))
    x2 = residual(f32(x1), h, inp["w2"], inp.get("b2"), a_d, ran["down"]["slices"])
    sel = rows if (last and not ran["rs2_tiles"]) else None
    op2, rs2 = operand(x2, inp["next_norm_w"], inp.get("next_norm_b"), ran["rs2_tiles"], sel)
    o2, r2 = (op2, rs2) if not (last and rs2 is not None) else (op2[rows], rs2[rows])
    yn = f32(next_y(o2, r2, inp, True))
    return dict(x1=f32(x1), op1=op1, rs1=rs1, h=h, x2=f32(x2), op2=op2, rs2=rs2, yn=yn, x_end=f32(x2), ran=ran)


# ---- the MoE chain: O projection (producer) -> moe(deferred_norm) -> pending moe_part (ops.dense_moe_stages) ----------
import moe_reference as MR        # (its softmax / route / tolerances: the routing is held exactly as test_moe_ops_gpu.py holds it)

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
