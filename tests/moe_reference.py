"""The MoE block (MoELayer.Forward, moe.go:43-128) in float64, stage by stage — numpy only, test infrastructure like
tests/mamba_reference.py — plus the inputs, cases and assertions tests/test_moe_ops_gpu.py and
tests/test_moe_reference_host.py share.

Every stage's reference is FED THE DEVICE'S OWN OUTPUT of the stage before: route() runs on the device's router logits,
the expert references on the device's gate matrix.  A near-tie at the top-k boundary is then no reason to leave a row
out: whichever expert the device's logits favour is the one the reference routes to, and the logits themselves are held
to the float64 product separately.

Where the device rounds to bf16 (experts_emulated mirrors exactly these points and no others; all sums are fp32 on the
device and float64 here):
  x, W_in, W_out   on upload: the MFMA operands of both projections (convert_2d_kernel; the router and its operand too).
  dense forms      gemm.h epilogue_swiglu4<bf16_t, MOE>: v = silu(g) * u in fp32, v *= moe_gate[m][e] in fp32, then
                   act_store4 rounds v once — h = bf16(silu(g) * u * gate[m][e]).  The down projection sums over all
                   experts' columns (K = E * I) in fp32; its K slices are fp32 partials which the next norm
                   (norm_row_kernel / tap_hidden_kernel, slice order) adds into x in fp32: no further rounding.
  sorted forms     epilogue_swiglu4<bf16_t, false>: h = bf16(silu(g) * u).  The grouped down projection stores fp32 rows
                   eo; moe_combine_kernel (or the same arithmetic in norm_row_kernel / tap_hidden_kernel) takes
                   sum_rank w[m][rank] * eo[slot] in rank order, fp32 weight times fp32 row: no further rounding.
The gate weights are fp32 everywhere and never rounded."""
import numpy as np

from bf16_emulator import round_bf16

DENSE_FORMS, SORTED_FORMS = ("dense_fused", "dense"), ("plan", "grouped")
F32_TOL = 2e-5        # tests/test_ops_gpu.py's file-wide bound on fp32 results of bf16-rounded operands, relative to max
SOFTMAX_TOL = 1e-5    # the bound test_softmax holds the fp32 softmax to


def _r64(a):
    return round_bf16(a).astype(np.float64)


def router_logits(x, router):
    """float64 product of the bf16-rounded operands: x [M][H], router [H][E] -> [M][E]"""
    return _r64(x) @ _r64(router)


def softmax(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def route(logits, k):
    """softmax over E, top-k by descending probability with ties to the lower expert index, weights renormalised over
    the chosen k (moe.go:63-103) -> the dense gate matrix [M][E], 0 where an expert was not picked"""
    p = softmax(logits)
    order = np.argsort(-p, axis=1, kind="stable")[:, :k]
    gate = np.zeros_like(p)
    w = np.take_along_axis(p, order, 1)
    np.put_along_axis(gate, order, w / w.sum(1, keepdims=True), 1)
    return gate


def _experts(x, w_in, w_out, gate, rounded, fold_gate):
    M, H = x.shape
    E, _, I = w_out.shape
    cv = _r64 if rounded else (lambda a: np.asarray(a, np.float64))
    rh = _r64 if rounded else (lambda a: a)
    x, gate = cv(x), np.asarray(gate, np.float64)
    y = np.zeros((M, H))
    for e in range(E):
        rows = np.flatnonzero(gate[:, e])
        if rows.size == 0:
            continue
        gu = x[rows] @ cv(w_in[e]).T
        g, u = gu[:, :I], gu[:, I:]
        h = g / (1.0 + np.exp(-g)) * u
        w = gate[rows, e][:, None]
        wo = cv(w_out[e]).T
        y[rows] += rh(h * w) @ wo if fold_gate else w * (rh(h) @ wo)
    return y


def experts_f64(x, w_in, w_out, gate):
    """sum_e gate[m][e] * W_out[e] (silu(g) * u), [g | u] = W_in[e] x — float64 on the unrounded inputs.
    x [M][H], w_in [E][2I][H] (gate rows, then up rows), w_out [E][H][I], gate [M][E] -> [M][H]"""
    return _experts(x, w_in, w_out, gate, False, False)


def experts_emulated(x, w_in, w_out, gate, form):
    """the same in float64 with a bf16 rounding at each of the kernels' operand points (module docstring)"""
    assert form in DENSE_FORMS + SORTED_FORMS, form
    return _experts(x, w_in, w_out, gate, True, form in DENSE_FORMS)


def row_rms(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).mean(1))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def random_inputs(M, E, k, H, I, seed=None):
    """as tests/test_ops_gpu.py::test_moe: x ~ N(0, 1), router x 0.3, expert weights x 0.1"""
    r = np.random.default_rng(1000 * M + 10 * E + k + H + I if seed is None else seed)
    return dict(x=r.standard_normal((M, H), dtype=np.float32), router=r.standard_normal((H, E), dtype=np.float32) * 0.3,
                w_in=r.standard_normal((E, 2 * I, H), dtype=np.float32) * 0.1,
                w_out=r.standard_normal((E, H, I), dtype=np.float32) * 0.1, k=k)


ROW_KINDS = ("boundary_tie", "inner_tie", "all_equal", "distinct")


def crafted_routing_inputs(M, E, k, H=64, I=64):
    """Logits that are exact in every path: x rows one-hot (row r hot at r % H), router entries multiples of 1/8 in
    [-4, 4] — a logit is one router entry, gaps are 0 or >= 1/8.  Row r is of kind ROW_KINDS[r % 4]: a two-way tie across
    the top-k boundary, a tie inside the top-k, all experts equal, all distinct."""
    assert M <= H and E <= 65
    inp = random_inputs(M, E, k, H, I)
    r = np.random.default_rng(7 * M + E)
    router = (r.integers(0, 65, (H, E)) - 32) / 8.0
    for row in range(M):
        v = (r.permutation(65)[:E] - 32) / 8.0
        order = np.argsort(-v, kind="stable")
        kind = ROW_KINDS[row % 4]
        if kind == "boundary_tie" and k < E:
            v[order[k]] = v[order[k - 1]]
        elif kind == "inner_tie" and k >= 2:
            v[order[1]] = v[order[0]]
        elif kind == "all_equal":
            v[:] = v[0]
        router[row % H] = v
    x = np.zeros((M, H), np.float32)
    x[np.arange(M), np.arange(M) % H] = 1.0
    inp.update(x=x, router=router.astype(np.float32))
    return inp


SKEWS = ("two_experts", "one_token_each", "row0_only")


def skew_inputs(skew):
    """(20, 8, 2, 64, 64) with the routing dictated: x[:, :20] is 4 x the identity, router rows 0..19 hold 8 and 7 at the
    two experts their token is to pick and 0 elsewhere (logits 32 and 28 against |noise| of the random rest below 10).
      two_experts     every token on experts 2 and 5: six experts are never picked
      one_token_each  rows 0..15 on experts 0 and 1; experts 2..7 picked by exactly one token each, expert 7 only by the
                      LAST row of the batch
      row0_only       expert 0 picked by row 0 alone"""
    M, E, k, H, I = 20, 8, 2, 64, 64
    inp = random_inputs(M, E, k, H, I, seed=50 + SKEWS.index(skew))
    if skew == "two_experts":
        picks = [(2, 5)] * M
    elif skew == "one_token_each":
        picks = [(0, 1)] * 16 + [(2, 3), (4, 5), (6, 0), (7, 1)]
    else:
        picks = [(0, 1)] + [(1 + r % 6, 2 + r % 6) for r in range(1, M)]
    inp["x"][:, :M] = 4.0 * np.eye(M, dtype=np.float32)
    inp["router"][:M] = 0.0
    for row, (a, b) in enumerate(picks):
        inp["router"][row, a], inp["router"][row, b] = 8.0, 7.0
    inp["picks"] = picks
    return inp


# ---- cases (M, E, k, H, I) -----------------------------------------------------------------------------------------------
ROUTING_CASES = [(3, 8, 2), (20, 8, 2), (16, 64, 8), (17, 40, 8), (5, 5, 5), (64, 32, 1)]       # (M, E, k) at H = 64
DENSE_CASES = [
    (1, 8, 2, 64, 64),        # 1
    (5, 5, 2, 128, 96),       # 2  one slice and five waves; an expert is 3 k-steps: tail only
    (16, 6, 1, 64, 32),       # 3  three slices; an expert is one k-step
    (17, 40, 8, 64, 64),      # 4  MT = 2; ten waves per slice
    (33, 64, 8, 64, 160),     # 5  MT = 4, U = 2; 16 waves; two blocks plus tail
    (64, 32, 8, 256, 512),    # 6  Granite-1B's E, k, I: the wide up form (and the narrow one under key 2 = 1)
    (4, 4, 4, 64, 64),        # 7  k = E: every expert live for every row
    (32, 4, 2, 64, 4096),     # 8  full 32-bit mask at U = 4
    (33, 4, 2, 64, 2048),     # 9  full 32-bit mask at U = 2
    (32, 4, 2, 64, 4160),     # 10 32 blocks plus a tail, let through by the integer division in moe_dense_ok
]
REFUSED_CASES = [(33, 4, 2, 64, 4096), (32, 4, 2, 64, 4224),      # live mask too narrow
                 (8, 34, 2, 64, 64)]                               # 17 waves per slice
PREFILL_CASES = [(65, 8, 2, 128, 64), (300, 32, 4, 256, 256)]


# ---- the assertions of tests/test_moe_ops_gpu.py (out: what ops.moe_stages returns, or a stand-in for it) ------------
def check_routing_exact(inp, out):
    """crafted_routing_inputs: logits bit for bit, the selection exactly, the weights to SOFTMAX_TOL of the row maximum"""
    k = inp["k"]
    want_logits = router_logits(inp["x"], inp["router"])
    assert np.array_equal(out["router_logits"].astype(np.float64), want_logits), "router logits are not exact"
    want = route(want_logits, k)
    got = out["gate"].astype(np.float64)
    assert np.array_equal(got != 0, want != 0), f"selection differs in rows {np.flatnonzero(((got != 0) != (want != 0)).any(1))}"
    err = np.abs(got - want).max(1) / want.max(1)
    print(f"routing exact M={got.shape[0]} E={got.shape[1]} k={k}: weights {err.max():.2e} row sums {np.abs(got.sum(1) - 1).max():.2e}")
    assert err.max() <= SOFTMAX_TOL
    assert (np.abs(got.sum(1) - 1.0) <= SOFTMAX_TOL).all()
    for row in range(2, got.shape[0], 4):      # all_equal rows: experts 0 .. k-1, 1/k each
        assert np.array_equal(np.flatnonzero(got[row]), np.arange(k)) and np.abs(got[row, :k] - 1.0 / k).max() <= SOFTMAX_TOL / k
    if k == 1:
        assert (out["gate"].max(1) == np.float32(1.0)).all()


def check_routing_random(inp, out):
    """the reference fed the device's own router logits; no row is excluded"""
    k = inp["k"]
    lg = out["router_logits"].astype(np.float64)
    got = out["gate"].astype(np.float64)
    want_lg = router_logits(inp["x"], inp["router"])
    e_lg = float(np.abs(lg - want_lg).max() / np.abs(want_lg).max())
    chosen = got != 0
    assert (chosen.sum(1) == k).all(), "a row without exactly k experts"
    lo = np.where(chosen, lg, np.inf).min(1)
    hi = np.where(chosen, -np.inf, lg).max(1) if k < lg.shape[1] else np.full(lg.shape[0], -np.inf)
    p = np.where(chosen, softmax(lg), 0.0)
    want = p / p.sum(1, keepdims=True)
    e_w = float((np.abs(got - want).max(1) / want.max(1)).max())
    print(f"routing M={lg.shape[0]} E={lg.shape[1]} k={k}: logits {e_lg:.2e} weights {e_w:.2e}")
    assert np.isfinite(lg).all() and np.isfinite(got).all()
    assert e_lg <= F32_TOL
    assert (lo >= hi - SOFTMAX_TOL * np.abs(lg).max()).all(), "an unchosen logit above a chosen one"
    assert e_w <= SOFTMAX_TOL


def expert_ratio(inp, out):
    """per row: rms(y_dev - y_f64) / rms(y_emulated - y_f64), both references fed the device's gate"""
    y64 = experts_f64(inp["x"], inp["w_in"], inp["w_out"], out["gate"])
    yem = experts_emulated(inp["x"], inp["w_in"], inp["w_out"], out["gate"], out["form"])
    return row_rms(out["y"].astype(np.float64) - y64) / row_rms(yem - y64)


def check_experts(inp, out, bound, name=""):
    assert np.isfinite(out["y"]).all(), "a NaN in y: something no launch wrote was read"
    ratio = expert_ratio(inp, out)
    print(f"experts {name} {out['form']}: max row ratio {ratio.max():.4f} (row {int(ratio.argmax())})")
    assert ratio.max() <= bound, (float(ratio.max()), int(ratio.argmax()))
    return ratio


def emulated_device(inp, form):
    """a stand-in for ops.moe_stages made of the reference alone: how the inputs and bounds are proved usable without a GPU"""
    lg = router_logits(inp["x"], inp["router"]).astype(np.float32)
    gate = route(lg, inp["k"]).astype(np.float32)
    y = experts_emulated(inp["x"], inp["w_in"], inp["w_out"], gate, form).astype(np.float32)
    return dict(y=y, router_logits=lg, gate=gate, form=form)


# ---- quantized experts (tests/test_moe_q_ops_gpu.py; ops.moe_stages(..., expert_format=...)) ---------------------------
# The device quantizes the experts itself (the upload quantizer, then finalize's layouts); the reference computes with W~,
# the values those codes and scales stand for, from the bit-exact numpy mirrors of the three formats.  Quantization error is
# no kernel error: every check above is reused unchanged on W~, which is exact in bf16, so the kernels' rounding points are
# those of the bf16 kernels — x on upload, h once.  The decode kernels form W~ = bf16(scale x code) (fp8: w8_frag; INT4:
# bf16(s (q - z))) or an exact product of a power of two (MXFP4) in registers before the MFMA, the same values the
# dequantize kernels write: no further rounding point, and the deferred-norm chain scales the fp32 accumulator by rstd after
# the product, as for bf16 experts.
FORMATS = ("fp8", "mxfp4", "int4")
U24 = 2.0 ** -24


def _silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def mirror(fmt):
    """the format's mirror as rows [N][K] -> dict(wt=W~, ...codes and scales as the mirror returns them)"""
    if fmt == "fp8":
        from test_fp8_weights_gpu import ref_w8
        return lambda w, g: dict(zip(("codes", "s", "wt"), ref_w8(w)))
    if fmt == "mxfp4":
        from test_mxfp4_weights_gpu import ref_mx
        return lambda w, g: dict(zip(("codes", "s", "wt"), ref_mx(w)))
    assert fmt == "int4", fmt
    from test_int4_weights_gpu import ref_gq
    return lambda w, g: dict(zip(("codes", "s", "z", "wt"), ref_gq(w, g)))


def w_tilde(w3, fmt, g=0):
    """W~ of [E][out][in] experts: the mirror applied per row of [E out][in], as nvl_upload_tensor takes MOE_IN / MOE_OUT"""
    E, N, K = w3.shape
    return mirror(fmt)(np.ascontiguousarray(w3, np.float32).reshape(E * N, K), g)["wt"].reshape(E, N, K)


def crafted_experts(w3, fmt, g, seed):
    """w3 with the crafted() groups of the format's weight test in the first rows of EVERY expert, scaled by a power of two
    (ties stay ties) to the size of the other weights: an all-zero group, one-signed groups, exact ties, an outlier among
    tiny values, and for INT4 a range below the fp16 scale floor 2^-24"""
    w = np.array(w3, np.float32)
    E, N, K = w.shape
    rng = np.random.default_rng(seed)
    for e in range(E):
        if fmt == "fp8":          # the scale is per row: whole rows (zero | midpoints of consecutive codes under amax = 448 | outlier)
            from test_fp8_weights_gpu import crafted
            w[e, :3] = crafted(rng, K, 3).T * np.float32(2.0 ** -9)
        elif fmt == "mxfp4":      # the first 32-block of five rows (zero | ties, amax 4 | ties, amax 5 | saturating | outlier)
            from test_mxfp4_weights_gpu import crafted
            w[e, :5, :32] = crafted(rng, K, 8, False).T[:5, :32] * np.float32(2.0 ** -4)
        else:                     # the first group of six rows (zero | positive | negative | ties | outlier | scale floor)
            from test_int4_weights_gpu import crafted
            w[e, :6, :g] = crafted(rng, K, 6, g).T[:, :g] * np.float32(0.25)
    return w


def quantized(inp, fmt, g=0, crafted=False):
    """inp with w_in / w_out replaced by W~ (what the reference computes with); raw_in / raw_out are what the op is given"""
    raw_in, raw_out = inp["w_in"], inp["w_out"]
    if crafted:
        raw_in, raw_out = crafted_experts(raw_in, fmt, g, 11), crafted_experts(raw_out, fmt, g, 12)
    return dict(inp, w_in=w_tilde(raw_in, fmt, g), w_out=w_tilde(raw_out, fmt, g), raw_in=raw_in, raw_out=raw_out, fmt=fmt, g=g)


# (M, E, k, H, I), the INT4 group: the bf16 file's dense cases at the edges of the quantized kernels
Q_CASES = [
    ((1, 8, 2, 64, 64), 64),          # 1  one row; an expert is one 64-group (INT4) / two MX blocks
    ((5, 5, 2, 128, 96), 32),         # 2  one slice (E prime), an expert is 3 k-steps: tail only
    ((16, 6, 1, 64, 32), 32),         # 3  an expert is one k-step = one MX block = one group; three slices
    ((17, 40, 8, 64, 64), 64),        # 4  MT = 2; ten experts per slice
    ((33, 64, 8, 64, 160), 32),       # 5  MT = 4: U = 2 (fp8 / MXFP4), INT4 one k-step per register set; five k-steps
    ((64, 32, 8, 256, 512), 128),     # 6  Granite-1B's E, k, I: the wide up form (and the narrow one under key 2 = 1)
    ((4, 4, 4, 64, 64), 32),          # 7  k = E: every expert live for every row
    ((32, 4, 2, 64, 4096), 64),       # 8  full 32-bit live-block mask at U = 4
    ((32, 4, 2, 64, 4160), 32),       # 9  32 blocks plus a tail, let through by the integer division in moe_dense_ok
]
Q_CRAFTED = (1, 3, 6)                 # the cases (numbered as above) that carry crafted groups
# the mask edge at 33 rows, per format: (shape, group, form) — U = 2 (fp8 / MXFP4): 64 k-steps fill the mask, 66 overflow
# it; INT4 (U = 1): 32 k-steps fill it, 33 overflow it.  moe_dense_ok refuses the overflow: the sorted "plan" form runs.
Q_MASK_EDGES = {
    "fp8": [((33, 4, 2, 64, 2048), 0, "dense"), ((33, 4, 2, 64, 2112), 0, "plan")],
    "mxfp4": [((33, 4, 2, 64, 2048), 0, "dense"), ((33, 4, 2, 64, 2112), 0, "plan")],
    "int4": [((33, 4, 2, 64, 1024), 64, "dense"), ((33, 4, 2, 64, 1056), 32, "plan")],
}


def check_wt(out, inp_q):
    """W~ as the device holds it after finalize (gather_rows_q, moe_cat_down_w*, read through the dequantize kernels of the
    grouped forms) equals the mirror bit for bit"""
    for key in ("w_in", "w_out"):
        got, want = out["wt_" + key[2:]], inp_q[key]
        assert got.shape == want.shape, (key, got.shape, want.shape)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"W~ of {key} differs from the {inp_q['fmt']} mirror at {len(bad)} places, first (expert, row, k) = {tuple(bad[0])}"


def pre_activation(inp):
    """the default [g | u] of check_h: (expert, rows, rounded) -> x[rows] . W_in[e]^T in float64"""
    def gu(e, rows, rounded):
        cv = _r64 if rounded else (lambda a: np.asarray(a, np.float64))
        return cv(inp["x"])[rows] @ cv(inp["w_in"][e]).T
    return gu


def h_ratio(inp_q, out, gu=None):
    """the dense forms' h = bf16(silu(g) u gate[m][e]) after the up projection.  Untouched experts all NaN (the skip really
    skipped: the 0xFF pre-fill is still there); a live expert finite everywhere and exactly 0 in the rows that did not pick it;
    -> {(row, expert): rms(h_dev - h_f64) / rms(h_emulated - h_f64)} over the picked pairs, both references fed the device's gate"""
    gate = out["gate"].astype(np.float64)
    M, E = gate.shape
    I = inp_q["w_out"].shape[2]
    h = out["h"].reshape(M, E, I)
    gu = gu or pre_activation(inp_q)
    ratios = {}
    for e in range(E):
        rows = np.flatnonzero(gate[:, e])
        if rows.size == 0:
            assert np.isnan(h[:, e]).all(), f"expert {e} was picked by no row, yet its h columns were written"
            continue
        assert np.isfinite(h[:, e]).all(), f"expert {e} is live, yet its h columns hold NaN"
        rest = np.setdiff1d(np.arange(M), rows)
        assert (h[rest, e] == 0).all(), f"expert {e}: h of rows that did not pick it is not exactly 0"
        ref = []
        for rounded in (False, True):
            a = gu(e, rows, rounded)
            v = _silu(a[:, :I]) * a[:, I:] * gate[rows, e][:, None]
            ref.append(_r64(v) if rounded else v)
        den = np.sqrt(((ref[1] - ref[0]) ** 2).mean(1))
        assert (den > 0).all(), "the emulation does not differ from float64: the ratio is undefined"
        num = np.sqrt(((h[rows, e].astype(np.float64) - ref[0]) ** 2).mean(1))
        for r, v in zip(rows, num / den):
            ratios[(int(r), e)] = float(v)
    return ratios


def check_h(inp_q, out, bound, name="", gu=None):
    assert out["form"] in DENSE_FORMS, out["form"]
    ratios = h_ratio(inp_q, out, gu)
    worst = max(ratios, key=ratios.get)
    print(f"h {name} {out['form']}: max (row, expert) ratio {ratios[worst]:.4f} at {worst}, {len(ratios)} pairs")
    assert ratios[worst] <= bound, (ratios[worst], worst)
    return ratios


def down_error(inp_q, out, base=None, alpha=1.0):
    """the down projection fed the DEVICE'S OWN h: y = base + alpha sum_e h_dev[:, e] . W~_out[e]^T.  Both operands are
    exact in bf16, so the float64 product is the exact result and what the device may add is fp32 summation error alone:
    elementwise at most (K + 8) 2^-24 alpha sum |h| |w| (K = E I terms in any order, the slices' and the residual's adds)
    + 2 x 2^-24 |y|, the bound dense_reference._resid_exact_bound takes.  -> (|y_dev - y_exact|, bound), elementwise"""
    M, E = out["gate"].shape
    I = inp_q["w_out"].shape[2]
    h = np.where(np.isnan(out["h"]), 0.0, out["h"].astype(np.float64)).reshape(M, E, I)       # (untouched experts are skipped: check_h)
    w = inp_q["w_out"].astype(np.float64)
    y = np.einsum("mei,ehi->mh", h, w)
    mag = np.einsum("mei,ehi->mh", np.abs(h), np.abs(w))
    b = 0.0 if base is None else np.asarray(base, np.float64)
    want = b + alpha * y
    bound = (E * I + 8) * U24 * abs(alpha) * mag + 2 * U24 * (np.abs(b) + abs(alpha) * mag)
    return np.abs(out["y"].astype(np.float64) - want), bound


def check_down(inp_q, out, name="", base=None, alpha=1.0):
    err, bound = down_error(inp_q, out, base, alpha)
    frac = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"down {name} {out['form']}: |y - down(h_dev)| at most {frac:.3f} of the fp32 summation bound")
    assert (err <= bound).all(), f"y is not the down projection of the device's own h: {frac:.1f} x the fp32 bound at {np.unravel_index((err - bound).argmax(), err.shape)}"


def emulated_h(inp_q, gate, untouched=np.nan, gu=None):
    """h of the stand-in: bf16(silu(g) u gate) for live experts (0 where the gate is 0), `untouched` elsewhere"""
    M, E = gate.shape
    I = inp_q["w_out"].shape[2]
    h = np.full((M, E, I), untouched, np.float32)
    gu = gu or pre_activation(inp_q)
    for e in range(E):
        rows = np.flatnonzero(gate[:, e])
        if rows.size:
            a = gu(e, rows, True)
            h[:, e] = 0.0
            h[rows, e] = round_bf16(_silu(a[:, :I]) * a[:, I:] * gate[rows, e].astype(np.float64)[:, None])
    return h.reshape(M, E * I)


def emulated_device_q(inp_q, form, compute_with=None, untouched=np.nan):
    """the stand-in for ops.moe_stages(..., expert_format=...): it REPORTS W~ of the mirror (wt_in / wt_out) and computes h
    and y with compute_with (default: the same W~; a mutation test passes the experts a wrong kernel would compute with)"""
    c = dict(inp_q, **(compute_with or {}))
    out = emulated_device(c, form)
    out.update(wt_in=inp_q["w_in"].copy(), wt_out=inp_q["w_out"].copy())
    M, E = out["gate"].shape
    if form in DENSE_FORMS:
        out["h"] = emulated_h(c, out["gate"], untouched)
    else:
        out["h"] = np.full((M, E * inp_q["w_out"].shape[2]), np.nan, np.float32)
    return out


def check_all_q(inp_q, out, bound, name=""):
    """what tests/test_moe_q_ops_gpu.py asserts of one call (the form literal apart)"""
    check_wt(out, inp_q)
    check_routing_random(inp_q, out)
    if out["form"] in DENSE_FORMS:
        check_h(inp_q, out, bound, name)
        check_down(inp_q, out, name)
    else:
        assert np.isnan(out["h"]).all(), "a sorted form wrote moe_hall"
    return check_experts(inp_q, out, bound, name)
