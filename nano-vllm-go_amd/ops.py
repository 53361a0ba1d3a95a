"""purego/tensor's leaf functions on the device, one call each, through the nvl_op_* entry points
(host fp32 in, host fp32 out).  Names follow the reference (tensor.go / rope.go / transformer.go /
moe.go); used by the parity tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mat_mul(a, b, precision="bf16", device=0):                 # MatMul tensor.go:62
    a, b = _f(a), _f(b)
    m, k = a.shape
    _, n = b.shape
    c = np.empty((m, n), np.float32)
    L.check(L.lib().nvl_op_matmul(device, L.PRECISION[precision], _p(a), _p(b), _p(c), m, k, n))
    return c


def layer_norm(x, weight, bias, eps, device=0):                # LayerNorm tensor.go:193
    x, w = _f(x), _f(weight)
    b = None if bias is None else _f(bias)
    y = np.empty_like(x)
    L.check(L.lib().nvl_op_layernorm(device, _p(x), _p(w), _p(b), eps, _p(y), x.shape[0], x.shape[1]))
    return y


def softmax(x, device=0):                                      # Softmax tensor.go:128
    x = _f(x)
    y = np.empty_like(x)
    L.check(L.lib().nvl_op_softmax(device, _p(x), _p(y), x.shape[0], x.shape[1]))
    return y


def gelu(x, device=0):                                         # GELU tensor.go:181
    x = _f(x)
    y = np.empty_like(x)
    L.check(L.lib().nvl_op_gelu(device, _p(x), _p(y), x.size))
    return y


def silu(x, device=0):                                         # SiLU mamba2.go:360
    x = _f(x)
    y = np.empty_like(x)
    L.check(L.lib().nvl_op_silu(device, _p(x), _p(y), x.size))
    return y


def apply_rope_single_tensor(t, start_pos, base, max_seq, device=0):   # rope.go:153
    t = _f(t).copy()
    heads, seq, hd = t.shape
    L.check(L.lib().nvl_op_rope(device, _p(t), heads, seq, hd, start_pos, base, max_seq))
    return t


def attention(q, k, v, scale=0.0, precision="bf16", device=0):  # attention.go:354-470 / mqa.go:184
    q, k, v = _f(q), _f(k), _f(v)
    nH, S, hd = q.shape
    nKV, T, _ = k.shape
    out = np.empty_like(q)
    L.check(L.lib().nvl_op_attention(device, L.PRECISION[precision], _p(q), _p(k), _p(v), nH, nKV, S, T, hd,
                                     scale, _p(out)))
    return out


def attention_mq(q, k, v, scale=0.0, device=0):   # the multi-position decode attention of a verify pass (bf16, S = 2..8)
    q, k, v = _f(q), _f(k), _f(v)
    nH, S, hd = q.shape
    nKV, T, _ = k.shape
    out = np.empty_like(q)
    L.check(L.lib().nvl_op_attention_mq(device, _p(q), _p(k), _p(v), nH, nKV, S, T, hd, scale, _p(out)))
    return out


def mamba_mixer(proj, seq_len, seq_pos, seq_slot, state, nh, hd, ss, ng, K, conv_w, conv_b=None, a_log=None, D=None,
                dt_bias=None, norm_w=None, tail=None, chain=0, precision="bf16", device=0):   # mamba2.go:107-170
    """The Mamba2 mixer between its projections through the model's dispatch (csrc/mamba.h): proj [M][EH + conv_dim + nh],
    sequence i = seq_len[i] rows from position seq_pos[i] in slot seq_slot[i] of state [n_slots][nh][hd][ss] (and of tail
    [n_slots][K-1][conv_dim]).  chain: 0 zero padding, 1 / 2 a chained prefill of one sequence, 3 the carried window of
    NVL_MAMBA_CONV_CARRIED for any batch (csrc/mamba.h MambaArgs::chain).  -> dict(xbc, delta, y (before gating), normed, state, tail); state / tail are new arrays."""
    proj, conv_w = _f(proj), _f(conv_w)
    opt = [None if v is None else _f(v) for v in (conv_b, a_log, D, dt_bias, norm_w)]
    sl, sp, so = (np.ascontiguousarray(v, dtype=np.int32) for v in (seq_len, seq_pos, seq_slot))
    state = _f(state).copy()
    tail = None if tail is None else _f(tail).copy()
    M, EH, conv_dim = proj.shape[0], nh * hd, nh * hd + 2 * ng * ss
    if proj.shape != (M, EH + conv_dim + nh) or conv_w.shape != (conv_dim, K) or M != int(sl.sum()) or not sl.size == sp.size == so.size:
        raise ValueError("mamba_mixer: shapes do not match the geometry")
    if state.ndim != 4 or state.shape[1:] != (nh, hd, ss) or (tail is not None and tail.shape != (state.shape[0], K - 1, conv_dim)):
        raise ValueError("mamba_mixer: state / tail shape")
    out = dict(xbc=np.empty((M, conv_dim), np.float32), delta=np.empty((M, nh), np.float32), y=np.empty((M, EH), np.float32),
               normed=np.empty((M, EH), np.float32))
    L.check(L.lib().nvl_op_mamba_mixer(device, L.PRECISION[precision], _p(proj), sl.size, _p(sl), _p(sp), _p(so), state.shape[0],
                                       nh, hd, ss, ng, K, _p(conv_w), *[_p(v) for v in opt], _p(state), _p(tail), chain,
                                       _p(out["xbc"]), _p(out["delta"]), _p(out["y"]), _p(out["normed"])))
    out["state"], out["tail"] = state, tail
    return out


def lookup_draft(history, k, ngram=3):
    """nvl_lookup_draft (host only): -> (draft [k], number of real draft tokens)."""
    h = np.ascontiguousarray(history, dtype=np.int32)
    draft = np.empty(k, np.int32)
    n_real = L.check(L.lib().nvl_lookup_draft(_p(h), h.size, int(k), int(ngram), _p(draft)))
    return draft, n_real


def matmul_fp8w(a, w, device=0):                              # MatMul tensor.go:62 with 8-bit weights (w8.h)
    """a [M][K], w [K][N] ([in, out]) -> (c, codes, scales): w quantized by the model's upload quantizer (codes [N][K]
    uint8, scales [N]), c = bf16(a) @ W~ through the model's GEMM dispatch, W~ = bf16(scales[:, None] * e4m3(codes))."""
    a, w = _f(a), _f(w)
    m, k = a.shape
    _, n = w.shape
    c = np.empty((m, n), np.float32)
    codes = np.empty((n, k), np.uint8)
    scales = np.empty(n, np.float32)
    L.check(L.lib().nvl_op_matmul_fp8w(device, _p(a), _p(w), m, n, k, _p(c), _p(codes), _p(scales)))
    return c, codes, scales


def matmul_mxfp4w(a, w, device=0):                            # MatMul tensor.go:62 with MXFP4 weights (w4.h)
    """a [M][K], w [K][N] ([in, out]) -> (c, codes, scales): w quantized by the model's upload quantizer (codes [N][K/2]
    uint8, two e2m1 codes per byte with even k in the low nibble; scales [N][K/32] e8m0 bytes), c = bf16(a) @ W~ through
    the model's GEMM dispatch, W~ = grid[codes] * 2^(scales - 127)."""
    a, w = _f(a), _f(w)
    m, k = a.shape
    _, n = w.shape
    c = np.empty((m, n), np.float32)
    codes = np.empty((n, k // 2), np.uint8)
    scales = np.empty((n, k // 32), np.uint8)
    L.check(L.lib().nvl_op_matmul_mxfp4w(device, _p(a), _p(w), m, n, k, _p(c), _p(codes), _p(scales)))
    return c, codes, scales


def matmul_int4w(a, w, group, device=0):                      # MatMul tensor.go:62 with INT4 group-quantized weights (w4g.h)
    """a [M][K], w [K][N] ([in, out]) -> (c, codes, scales, zeros): w quantized by the model's upload quantizer with groups
    of `group` input features (codes [N][K/2] uint8, even k in the low nibble; scales [N][K/group] float16; zeros
    [N][K/group] uint8), c = bf16(a) @ W~ through the model's GEMM dispatch, W~ = bf16(scales * (codes - zeros))."""
    a, w = _f(a), _f(w)
    m, k = a.shape
    _, n = w.shape
    c = np.empty((m, n), np.float32)
    codes = np.empty((n, k // 2), np.uint8)
    scales = np.empty((n, k // group), np.float16)
    zeros = np.empty((n, k // group), np.uint8)
    L.check(L.lib().nvl_op_matmul_int4w(device, _p(a), _p(w), m, n, k, int(group), _p(c), _p(codes), _p(scales), _p(zeros)))
    return c, codes, scales, zeros


def matmul_w8a8(a, w, device=0):                              # MatMul tensor.go:62 with 8-bit weights and activations (a8.h)
    """a [M][K], w [K][N] ([in, out]) -> (c, a_codes, a_scales): matmul_fp8w's dispatch in W8A8 mode.  The tile form
    quantizes bf16(a) per row (a_codes [M][K] uint8, a_scales [M]) and returns c = (e4m3(a_codes) @ e4m3(w codes)^T) * a_scales
    * w scales; the decode form (small M) is matmul_fp8w's bf16(a) @ W~ and leaves a_codes 0, a_scales 1."""
    a, w = _f(a), _f(w)
    m, k = a.shape
    _, n = w.shape
    c = np.empty((m, n), np.float32)
    codes = np.empty((m, k), np.uint8)
    scales = np.empty(m, np.float32)
    L.check(L.lib().nvl_op_matmul_w8a8(device, _p(a), _p(w), m, n, k, _p(c), _p(codes), _p(scales)))
    return c, codes, scales


def act_quant_fp8(a, lda=None, device=0):                     # the W8A8 activation quantizer alone (a8.h)
    """a [M][K] -> (codes [M][K] uint8, scales [M]) of bf16(a), read as a fragment-major operand of row width lda >= K"""
    a = _f(a)
    m, k = a.shape
    codes = np.empty((m, k), np.uint8)
    scales = np.empty(m, np.float32)
    L.check(L.lib().nvl_op_act_quant_fp8(device, _p(a), m, k, int(lda or k), _p(codes), _p(scales)))
    return codes, scales


def fp8_kv_roundtrip(x, scale=1.0, device=0):                  # the 8-bit KV cache's quantizer + read path (kv8.h)
    """-> (codes uint8, back fp32): codes = e4m3fn(x / scale), back = scale * bf16(code), both computed on the device."""
    x = _f(x)
    codes = np.empty(x.shape, np.uint8)
    back = np.empty_like(x)
    L.check(L.lib().nvl_op_fp8_kv_roundtrip(device, _p(x), x.size, scale, _p(codes), _p(back)))
    return codes, back


def attention_kv8(q, k, v, scale=0.0, k_scale=1.0, v_scale=1.0, device=0):   # attention() over an 8-bit cache (bf16)
    q, k, v = _f(q), _f(k), _f(v)
    nH, S, hd = q.shape
    nKV, T, _ = k.shape
    out = np.empty_like(q)
    L.check(L.lib().nvl_op_attention_kv8(device, _p(q), _p(k), _p(v), nH, nKV, S, T, hd, scale, k_scale, v_scale,
                                         _p(out)))
    return out


def feed_forward(x, w1, b1, w2, b2, swiglu, precision="bf16", device=0):   # FeedForward.Forward transformer.go:40
    x, w1, w2 = _f(x), _f(w1), _f(w2)
    b1 = None if b1 is None else _f(b1)
    b2 = None if b2 is None else _f(b2)
    rows, hidden = x.shape
    y = np.empty((rows, hidden), np.float32)
    L.check(L.lib().nvl_op_ffn(device, L.PRECISION[precision], _p(x), _p(w1), _p(b1), _p(w2), _p(b2), rows, hidden,
                               w2.shape[0], int(swiglu), _p(y)))
    return y


def moe_forward(x, router, w_in, w_out, top_k, precision="bf16", device=0):   # MoELayer.Forward moe.go:43
    x, router, w_in, w_out = _f(x), _f(router), _f(w_in), _f(w_out)
    rows, hidden = x.shape
    y = np.empty((rows, hidden), np.float32)
    L.check(L.lib().nvl_op_moe(device, L.PRECISION[precision], _p(x), _p(router), _p(w_in), _p(w_out), rows, hidden,
                               router.shape[1], top_k, w_out.shape[2], _p(y)))
    return y


MOE_FORMS = {1: "dense_fused", 2: "dense", 3: "plan", 4: "grouped"}      # NVL_MOE_FORM_*


EXPERT_FORMATS = {"bf16": 0, "fp8": 1, "mxfp4": 2, "int4": 3}             # NVL_OP_EXPERTS_*


def _expert_outputs(out, expert_format, M, E, I, hidden):
    """the optional outputs of the *_q entry points: W~ of quantized experts, and h of the dense-masked forms"""
    if expert_format not in EXPERT_FORMATS:
        raise ValueError(f"expert_format must be one of {sorted(EXPERT_FORMATS)}")
    out["h"] = np.full((M, E * I), np.nan, np.float32)
    if expert_format != "bf16":
        out["wt_in"], out["wt_out"] = np.full((E, 2 * I, hidden), np.nan, np.float32), np.full((E, hidden, I), np.nan, np.float32)
    return [_p(out.get("wt_in")), _p(out.get("wt_out")), _p(out["h"])]


def moe_stages(x, router, w_in, w_out, top_k, precision="bf16", device=0, expert_format="bf16", group_size=0):   # MoELayer.Forward moe.go:43
    """The MoE block as a layer of the model runs it (nvl_op_moe_stages_q: the decode form wherever a model would take it,
    every scratch buffer pre-filled with NaN).  x [rows][H], router [H][E], w_in [E][2I][H], w_out [E][H][I] ->
    dict(y [rows][H], router_logits [rows][E], gate [rows][E] (0 = not picked), form (a MOE_FORMS name), h [rows][E I] (the
    dense forms' intermediate after the up projection; NaN where no launch wrote)).  expert_format "fp8" | "mxfp4" | "int4"
    (group_size 32 / 64 / 128): the experts quantized and finalized as a model's, and wt_in / wt_out, W~ as the device holds it."""
    x, router, w_in, w_out = _f(x), _f(router), _f(w_in), _f(w_out)
    rows, hidden = x.shape
    E, I = router.shape[1], w_out.shape[2]
    if router.shape != (hidden, E) or w_in.shape != (E, 2 * I, hidden) or w_out.shape != (E, hidden, I):
        raise ValueError("moe_stages: shapes do not match")
    out = dict(y=np.empty((rows, hidden), np.float32), router_logits=np.empty((rows, E), np.float32),
               gate=np.empty((rows, E), np.float32))
    extra = _expert_outputs(out, expert_format, rows, E, I, hidden)
    form = C.c_int32(0)
    L.check(L.lib().nvl_op_moe_stages_q(device, L.PRECISION[precision], _p(x), _p(router), _p(w_in), _p(w_out), rows, hidden, E,
                                        int(top_k), I, EXPERT_FORMATS[expert_format], int(group_size), _p(out["y"]),
                                        _p(out["router_logits"]), _p(out["gate"]), C.cast(C.byref(form), C.c_void_p), *extra))
    out["form"] = MOE_FORMS[form.value]
    return out


RESID_FORMS = {0: "tile", 1: "msplit", 2: "groups", 3: "groups_serial", 4: "decode"}      # NVL_RESID_FORM_*
NORM_RAN = {0: None, 1: "row", 2: "row_idx", 3: "tile16", 4: "wave"}                        # NVL_NORM_RAN_*


def dense_stages(x, attn_out, wo, norm_w, w1, w2, next_norm_w, wn, bo=None, norm_b=None, b1=None, b2=None, next_norm_b=None,
                 norm="rms", act="swiglu", block="sequential", residual_multiplier=0.0, attention_multiplier=0.0, norm_eps=1e-5,
                 max_len=1, last_rows=None, has_next=True, precision="bf16", device=0):   # generic_model.go:320-418
    """The dense layer tail as a layer of the model runs it, stage by stage (nvl_op_dense_stages; bf16 only).  x [M][H],
    attn_out [M][qw], wo [H][qw], w1 [2F][H] (gate rows | up rows; GELU: [F][H]), w2 [H][F], wn [Nn][H]; has_next=False is
    the last layer: last_rows (default: every row, a decode pass) feed the final norm and wn as the LM head.
    -> dict(x1, op1, rs1 (None = op1 is already normalised, else the x^2 partials [M][tiles]), h, x2, op2, rs2, yn, x_end,
    ran = dict(o=..., down=..., norms, rs1_tiles, rs2_tiles) with o / down = dict(producer, half, form (a RESID_FORMS
    name), slices, consumer (a NORM_RAN name)))."""
    x, attn_out, wo, norm_w, w1, w2, next_norm_w, wn = (_f(a) for a in (x, attn_out, wo, norm_w, w1, w2, next_norm_w, wn))
    opt = [None if a is None else _f(a) for a in (bo, norm_b, b1, b2, next_norm_b)]
    M, H = x.shape
    qw, Nn, swiglu = attn_out.shape[1], wn.shape[0], act == "swiglu"
    F = w2.shape[1]
    if attn_out.shape != (M, qw) or wo.shape != (H, qw) or w1.shape != ((2 * F if swiglu else F), H) or w2.shape != (H, F) or \
            wn.shape != (Nn, H) or norm_w.shape != (H,) or next_norm_w.shape != (H,):
        raise ValueError("dense_stages: shapes do not match")
    lr = None
    if not has_next:
        lr = np.ascontiguousarray(np.arange(M) if last_rows is None else last_rows, dtype=np.int32)
    elif last_rows is not None:
        raise ValueError("dense_stages: last_rows belong to the last layer")
    n_out = M if lr is None else len(lr)
    nan = lambda *s: np.full(s, np.nan, np.float32)
    out = dict(x1=nan(M, H), op1=nan(M, H), rs1=nan(M, H // 8), h=nan(M, F), x2=nan(M, H), op2=nan(M, H), rs2=nan(M, H // 8),
               yn=nan(n_out, Nn), x_end=nan(M, H))
    ran = np.zeros(14, np.int32)
    d = L.DenseStagesC(struct_bytes=C.sizeof(L.DenseStagesC), rows=M, hidden=H, q_width=qw, ffn=F, n_next=Nn,
                       norm_type=1 if norm == "rms" else 0, activation_type=1 if swiglu else 0,
                       block_style=1 if block == "parallel" else 0, max_len=int(max_len), has_next=1 if has_next else 0,
                       n_last_rows=0 if lr is None else len(lr), residual_multiplier=residual_multiplier,
                       attention_multiplier=attention_multiplier, norm_eps=norm_eps)
    keep = dict(x=x, attn_out=attn_out, wo=wo, bo=opt[0], norm_w=norm_w, norm_b=opt[1], w1=w1, b1=opt[2], w2=w2, b2=opt[3],
                next_norm_w=next_norm_w, next_norm_b=opt[4], wn=wn, last_rows=lr, ran=ran, **out)
    for k, v in keep.items():
        setattr(d, k, None if v is None else v.ctypes.data)
    L.check(L.lib().nvl_op_dense_stages(device, L.PRECISION[precision], C.byref(d)))
    t1, t2 = int(ran[12]), int(ran[13])
    out["rs1"] = out["rs1"][:, :t1].copy() if t1 else None
    out["rs2"] = out["rs2"][:, :t2].copy() if t2 else None
    if not t2:
        out["op2"] = out["op2"][:n_out]
    proj = lambda p: dict(producer=int(ran[4 * p]), half=int(ran[4 * p + 1]), form=RESID_FORMS[int(ran[4 * p + 2])],
                          slices=int(ran[4 * p + 3]), consumer=NORM_RAN[int(ran[9 + p])])
    out["ran"] = dict(o=proj(0), down=proj(1), norms=int(ran[8]), rs1_tiles=t1, rs2_tiles=t2)
    return out


def dense_moe_stages(x, attn_out, wo, norm_w, router, w_in, w_out, next_norm_w, top_k, bo=None, residual_multiplier=0.0,
                     norm_eps=1e-5, precision="bf16", device=0, expert_format="bf16", group_size=0):   # generic_model.go:320-389 around moe.go:43
    """The layer tail with a MoE block, decode (nvl_op_dense_moe_stages_q): the O projection carries the FFN norm, moe() reads
    the deferred operand, its down projection stays pending.  router [H][E], w_in [E][2I][H], w_out [E][H][I] ->
    dict(x1, op1, rs1 (x^2 partials, None = op1 is normalised), router_logits, gate, y (x after the block), form (a
    MOE_FORMS name), ran as dense_stages gives it; ran["down"]["slices"] = what moe() left pending; h, and for a quantized
    expert_format wt_in / wt_out, as moe_stages gives them)."""
    x, attn_out, wo, norm_w, router, w_in, w_out, next_norm_w = (_f(a) for a in (x, attn_out, wo, norm_w, router, w_in, w_out, next_norm_w))
    bo = None if bo is None else _f(bo)
    M, H = x.shape
    qw, E, I = attn_out.shape[1], router.shape[1], w_out.shape[2]
    if attn_out.shape != (M, qw) or wo.shape != (H, qw) or router.shape != (H, E) or w_in.shape != (E, 2 * I, H) or \
            w_out.shape != (E, H, I) or norm_w.shape != (H,) or next_norm_w.shape != (H,):
        raise ValueError("dense_moe_stages: shapes do not match")
    nan = lambda *s: np.full(s, np.nan, np.float32)
    out = dict(x1=nan(M, H), op1=nan(M, H), rs1=nan(M, H // 8), router_logits=nan(M, E), gate=nan(M, E), y=nan(M, H))
    ran, form = np.zeros(14, np.int32), np.zeros(1, np.int32)
    extra = _expert_outputs(out, expert_format, M, E, I, H)
    L.check(L.lib().nvl_op_dense_moe_stages_q(device, L.PRECISION[precision], _p(x), _p(attn_out), _p(wo), _p(bo), _p(norm_w), _p(router),
                                              _p(w_in), _p(w_out), _p(next_norm_w), M, H, qw, E, int(top_k), I, residual_multiplier,
                                              norm_eps, EXPERT_FORMATS[expert_format], int(group_size), _p(out["x1"]), _p(out["op1"]),
                                              _p(out["rs1"]), _p(out["router_logits"]), _p(out["gate"]), _p(out["y"]), _p(form), _p(ran),
                                              *extra))
    t1 = int(ran[12])
    out["rs1"] = out["rs1"][:, :t1].copy() if t1 else None
    proj = lambda p: dict(producer=int(ran[4 * p]), half=int(ran[4 * p + 1]), form=RESID_FORMS[int(ran[4 * p + 2])],
                          slices=int(ran[4 * p + 3]), consumer=NORM_RAN[int(ran[9 + p])])
    out["ran"] = dict(o=proj(0), down=proj(1), norms=int(ran[8]), rs1_tiles=t1, rs2_tiles=0)
    out["form"] = MOE_FORMS[int(form[0])]
    return out


ATTN_OP_FORMS = {"plain": 0, "fused": 1, "mq": 2, "kv8": 3}                                  # NVL_ATTN_OP_*
ATTN_RAN = {1: "f32", 2: "prefill", 3: "prefill_kv8", 4: "decode", 5: "decode_fused", 6: "decode_kv8", 7: "decode_mq",
            8: "decode_stamped"}                                                                 # NVL_ATTN_RAN_*


def attention_batch(q, k_pool, v_pool, block_table, seq_len, seq_pos, nH, form="plain", scale=0.0, rope_base=0.0, max_seq=0,
                    k_scale=1.0, v_scale=1.0, precision="bf16", device=0):   # generic_model.go:276 over block tables
    """One layer's attention on a batch laid out as the paged front end lays it out, through the model's own dispatch
    (nvl_op_attention_batch): k_pool / v_pool [n_blocks][nKV][block_size][hd], block_table [n_seqs][tbl_stride] (passed
    verbatim), sequence i = seq_len[i] new rows behind seq_pos[i] cached keys.  q [tokens][nH][hd]; form "fused": the fp32
    QKV rows [n_seqs][(nH + 2 nKV) hd] of a decode step (RoPE with rope_base, 0 = none; K / V appended by the kernel).
    max_seq 0 = what the table covers.  -> dict(out [tokens][nH][hd], ran (an ATTN_RAN name), nw, nsplit, part_cnt [32],
    and for "fused" k_pool / v_pool after the launch)."""
    k_pool, v_pool = _f(k_pool).copy(), _f(v_pool).copy()
    q = _f(q)
    tbl = np.ascontiguousarray(block_table, dtype=np.int32)
    sl, sp = np.ascontiguousarray(seq_len, dtype=np.int32), np.ascontiguousarray(seq_pos, dtype=np.int32)
    n_blocks, nKV, bs, hd = k_pool.shape
    n_seqs, stride = tbl.shape
    tokens = int(sl.sum())
    if v_pool.shape != k_pool.shape or sl.shape != (n_seqs,) or sp.shape != (n_seqs,) or \
            q.shape != ((n_seqs, (nH + 2 * nKV) * hd) if form == "fused" else (tokens, nH, hd)):
        raise ValueError("attention_batch: shapes do not match")
    out = np.empty((tokens, nH, hd), np.float32)
    ran, cnt = np.zeros(3, np.int32), np.zeros(32, np.int32)
    L.check(L.lib().nvl_op_attention_batch(device, L.PRECISION[precision], ATTN_OP_FORMS[form], nH, nKV, hd, scale, n_seqs, _p(sl),
                                           _p(sp), _p(k_pool), _p(v_pool), n_blocks, bs, _p(tbl), stride, _p(q), float(rope_base),
                                           int(max_seq) if max_seq else stride * bs, k_scale, v_scale, _p(out), _p(ran), _p(cnt)))
    res = dict(out=out, ran=ATTN_RAN[int(ran[0])], nw=int(ran[1]), nsplit=int(ran[2]), part_cnt=cnt)
    if form == "fused":
        res.update(k_pool=k_pool, v_pool=v_pool)
    return res


QKV_FORMS = {1: "f32_store_rope", 2: "decode_store_rope", 3: "groups_store_rope", 4: "epilogue", 5: "store_rope_kv8",
             6: "store_only"}                                                                    # NVL_QKV_FORM_*
GEMM_RAN = {0: None, 1: "tile1", 2: "tile2", 3: "tile3", 5: "pingpong", 6: "hd128_4x2", 7: "hd128_pingpong", 8: "decode",
            9: "groups"}                                                                         # NVL_GEMM_RAN_*
EMBED_RAN = {0: None, 1: "f32", 2: "bf16", 3: "w8", 4: "w4"}                                    # NVL_EMBED_RAN_*


def qkv_stages(x, w_qkv, k_pool, v_pool, block_table, seq_len, seq_pos, nH, b_qkv=None, norm_w=None, norm_b=None, norm="rms",
               norm_eps=1e-5, rope_base=0.0, max_seq=0, kv8=False, k_scale=1.0, v_scale=1.0, tokens=None, tok_pos=None, emb=None,
               pos_emb=None, embedding_multiplier=0.0, precision="bf16", device=0):   # generic_model.go:295-318 + rope.go:153
    """The front of an attention layer on a paged batch, stage by stage (nvl_op_qkv_stages): x [tokens][hidden] (None with the
    embedding stage: tokens / tok_pos [tokens], emb [V][hidden], pos_emb [P][hidden] or None), the attention norm (norm_w
    None: x is the operand already), w_qkv [(nH + 2 nKV) hd][hidden] (+ b_qkv), RoPE with rope_base (0: none), Q into the
    operand buffer, K / V into k_pool / v_pool [n_blocks][nKV][block][hd] through block_table [n_seqs][stride]; sequence i =
    seq_len[i] rows behind seq_pos[i] cached keys.  max_seq 0 = what the table covers.
    -> dict(x (the embedding stage's), op [tokens][hidden], qkv [tokens][n_qkv] (NaN in the epilogue form), q [round_up(tokens,
    256)][nH hd], k_pool, v_pool after the pass (kv8: dequantized, plus k_codes / v_codes), ran = dict(form (a QKV_FORMS
    name), gemm (GEMM_RAN), norm (NORM_RAN), embed (EMBED_RAN)))."""
    k_pool, v_pool, w_qkv = _f(k_pool).copy(), _f(v_pool).copy(), _f(w_qkv)
    tbl = np.ascontiguousarray(block_table, dtype=np.int32)
    sl, sp = np.ascontiguousarray(seq_len, dtype=np.int32), np.ascontiguousarray(seq_pos, dtype=np.int32)
    n_blocks, nKV, bs, hd = k_pool.shape
    if tbl.ndim != 2 or sl.ndim != 1 or sp.ndim != 1:
        raise ValueError("qkv_stages: shapes do not match")
    n_seqs, stride = tbl.shape
    M, (N, H) = int(sl.sum()), w_qkv.shape
    opt = {k: None if a is None else _f(a) for k, a in dict(b_qkv=b_qkv, norm_w=norm_w, norm_b=norm_b, emb=emb, pos_emb=pos_emb).items()}
    ints = {k: None if a is None else np.ascontiguousarray(a, dtype=np.int32) for k, a in dict(tokens=tokens, tok_pos=tok_pos).items()}
    x = np.full((M, H), np.nan, np.float32) if tokens is not None else _f(x).copy()
    if v_pool.shape != k_pool.shape or sl.shape != (n_seqs,) or sp.shape != (n_seqs,) or N != (nH + 2 * nKV) * hd or x.shape != (M, H) or \
            any(a is not None and a.shape != s for a, s in ((opt["b_qkv"], (N,)), (opt["norm_w"], (H,)), (opt["norm_b"], (H,)),
                                                            (ints["tokens"], (M,)), (ints["tok_pos"], (M,)))) or \
            any(a is not None and (a.ndim != 2 or a.shape[1] != H) for a in (opt["emb"], opt["pos_emb"])):
        raise ValueError("qkv_stages: shapes do not match")
    nan = lambda *s: np.full(s, np.nan, np.float32)
    Mq = -(-M // 256) * 256
    out = dict(op=nan(M, H), qkv=nan(M, N), q=nan(Mq, nH * hd))
    codes = dict(k_codes=np.zeros(k_pool.shape, np.uint8), v_codes=np.zeros(k_pool.shape, np.uint8)) if kv8 else {}
    ran = np.zeros(4, np.int32)
    d = L.QkvStagesC(struct_bytes=C.sizeof(L.QkvStagesC), kv8=1 if kv8 else 0, nH=nH, nKV=nKV, hd=hd, hidden=H, n_seqs=n_seqs,
                     tbl_stride=stride, n_blocks=n_blocks, block_size=bs, max_seq=int(max_seq) if max_seq else stride * bs,
                     norm_type=1 if norm == "rms" else 0, vocab=0 if opt["emb"] is None else opt["emb"].shape[0],
                     pos_rows=0 if opt["pos_emb"] is None else opt["pos_emb"].shape[0], norm_eps=norm_eps, k_scale=k_scale,
                     v_scale=v_scale, embedding_multiplier=embedding_multiplier, rope_base=float(rope_base))
    keep = dict(seq_len=sl, seq_pos=sp, block_table=tbl, w_qkv=w_qkv, x=x, k_pool=k_pool, v_pool=v_pool, ran=ran, **opt, **ints, **out, **codes)
    for k, v in keep.items():
        setattr(d, k, None if v is None else v.ctypes.data)
    L.check(L.lib().nvl_op_qkv_stages(device, L.PRECISION[precision], C.byref(d)))
    out.update(k_pool=k_pool, v_pool=v_pool, **codes)
    if tokens is not None:
        out["x"] = x
    out["ran"] = dict(form=QKV_FORMS[int(ran[0])], gemm=GEMM_RAN[int(ran[1])], norm=NORM_RAN[int(ran[2])], embed=EMBED_RAN[int(ran[3])])
    return out


def argmax(x, device=0):                                       # argmax cmd/ask/main.go:389
    x = _f(x)
    if x.ndim == 1:
        x = x[None]
    out = np.empty(x.shape[0], np.int32)
    L.check(L.lib().nvl_op_argmax(device, _p(x), x.shape[0], x.shape[1], _p(out)))
    return out


def logprobs(logits, targets, top_k=0, logits_scaling=0.0, ld=None, device=0):   # logprob.h on host logits
    """Per row of logits [rows, V]: the log-probability of targets[row] (-1 = none -> 0.0) under softmax(logits /
    logits_scaling) (0 = no scaling), the greedy id, and the top_k ids / log-probabilities.
    ld=None: the rows are passed densely.  ld=n: `logits` is the float32 view buf[:, :V] of a buffer buf [rows, n] and the
    rows are passed as they lie in memory, pad columns included (what the model's [rows][Vpad] logits look like).
    -> (logprobs [rows], argmax [rows], topk_ids [rows, top_k] or None, topk_logprobs or None)."""
    if ld is None:
        lg = _f(logits)
        if lg.ndim == 1:
            lg = lg[None]
        rows, V = lg.shape
        stride = V
    else:
        lg, stride = logits, int(ld)
        if not isinstance(lg, np.ndarray) or lg.dtype != np.float32 or lg.ndim != 2:
            raise ValueError("logprobs: with ld, logits must be a 2-D float32 numpy view")
        rows, V = lg.shape
        if V > stride or lg.strides != (stride * 4, 4) or lg.base is None or lg.base.size < rows * stride:
            raise ValueError(f"logprobs: logits is not the [:, :{V}] view of a [rows, {stride}] buffer")
    tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    if tg.size != rows:
        raise ValueError(f"logprobs: {tg.size} targets for {rows} rows")
    top_k = int(top_k)
    lp, am = np.empty(rows, np.float32), np.empty(rows, np.int32)
    ti = np.empty((rows, top_k), np.int32) if top_k > 0 else None
    tl = np.empty((rows, top_k), np.float32) if top_k > 0 else None
    L.check(L.lib().nvl_op_logprobs(device, _p(lg), rows, V, stride, float(logits_scaling), _p(tg), top_k, _p(lp), _p(am),
                                    _p(ti), _p(tl)))
    return lp, am, ti, tl


def _histories(histories, rows):
    """-> (pointer array, int32 lengths, keep-alive list) for `rows` token histories (None = no history)."""
    arrs = [np.ascontiguousarray([] if h is None else h, dtype=np.int32) for h in (histories or [None] * rows)]
    ptrs = (C.c_void_p * rows)(*[a.ctypes.data_as(C.c_void_p).value if a.size else None for a in arrs])
    lens = np.asarray([a.size for a in arrs], np.int32)
    return ptrs, lens, arrs


def sample_with_history(logits, histories, uniforms, *, temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2,
                        return_probs=False, device=0):        # SampleWithHistory sampling.go:33, u = rand.Float32()
    lg = _f(logits)
    if lg.ndim == 1:
        lg = lg[None]
    rows, V = lg.shape
    ptrs, lens, keep = _histories(histories, rows)
    u = _f(uniforms).reshape(rows)
    out = np.empty(rows, np.int32)
    probs = np.empty((rows, V), np.float32) if return_probs else None
    sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
    L.check(L.lib().nvl_op_sample(device, _p(lg), rows, V, C.byref(sp), ptrs, _p(lens), _p(u), _p(out), _p(probs)))
    return (out, probs) if return_probs else out


def sample_drafts(logits, token_rows, k, histories, uniforms, *, temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2,
                  return_probs=False, device=0):
    """nvl_op_sample_drafts: the sampler of a sampled verify pass + its accept kernel on host logits [n_seqs * (1+k), V].
    token_rows [n_seqs, 1+k]; histories[i] ends with token_rows[i][0]; uniforms [n_seqs, 1+k].
    -> (sampled [n_seqs, 1+k], n_accepted [n_seqs], out_tokens [n_seqs, 1+k][, probs [n_seqs * (1+k), V]])."""
    lg = _f(logits)
    k = int(k)
    if lg.ndim != 2 or not 0 <= k <= 7 or lg.shape[0] % (1 + k):
        raise ValueError("sample_drafts: logits must be [n_seqs * (1+k), V] with k in [0, 7]")
    M, V = lg.shape
    n = M // (1 + k)
    toks = np.ascontiguousarray(token_rows, dtype=np.int32)
    if toks.size != M:
        raise ValueError(f"sample_drafts: {toks.size} tokens for {M} rows")
    if histories is None or len(histories) != n or any(h is None or len(h) == 0 for h in histories):
        raise ValueError(f"sample_drafts: {n} sequences need {n} non-empty histories")
    u = _f(uniforms)
    if u.size != M:
        raise ValueError(f"sample_drafts: {u.size} uniforms for {M} rows")
    ptrs, lens, keep = _histories(histories, n)
    sampled, acc, out = np.empty((n, 1 + k), np.int32), np.empty(n, np.int32), np.empty((n, 1 + k), np.int32)
    probs = np.empty((M, V), np.float32) if return_probs else None
    sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
    L.check(L.lib().nvl_op_sample_drafts(device, _p(lg), n, k, V, C.byref(sp), _p(toks), ptrs, _p(lens), _p(u), _p(sampled),
                                         _p(acc), _p(out), _p(probs)))
    return (sampled, acc, out, probs) if return_probs else (sampled, acc, out)


def spec_reject(p, q, token_rows, accept_uniforms, final_uniforms, device=0):
    """nvl_op_spec_reject: the rejection kernel of speculative sampling with a draft model on host distributions.
    p [n_seqs, 1+k, V] (the target's rows), q [n_seqs, k, V] (the draft's steps), token_rows [n_seqs, 1+k] (column 0 unused,
    column j+1 the draft's id of step j), accept_uniforms [n_seqs, k], final_uniforms [n_seqs].
    -> (n_accepted [n_seqs], out_tokens [n_seqs, 1+k], accept_prob [n_seqs, k, 2] = {p_j(d_j), q_j(d_j)})."""
    p, q = _f(p), _f(q)
    if p.ndim != 3 or q.ndim != 3 or p.shape[0] != q.shape[0] or p.shape[1] != q.shape[1] + 1 or p.shape[2] != q.shape[2]:
        raise ValueError("spec_reject: p must be [n_seqs, 1+k, V] and q [n_seqs, k, V]")
    n, k, V = q.shape
    if not 1 <= k <= 7:
        raise ValueError("spec_reject: k must be in [1, 7]")
    toks = np.ascontiguousarray(token_rows, dtype=np.int32)
    ua, uf = _f(accept_uniforms), _f(final_uniforms)
    if toks.size != n * (1 + k) or ua.size != n * k or uf.size != n:
        raise ValueError(f"spec_reject: {toks.size} tokens / {ua.size} accept draws / {uf.size} final draws for {n} x (1 + {k}) rows")
    acc, out, ap = np.empty(n, np.int32), np.empty((n, 1 + k), np.int32), np.empty((n, k, 2), np.float32)
    L.check(L.lib().nvl_op_spec_reject(device, _p(p), _p(q), _p(toks), n, k, V, _p(ua), _p(uf), _p(acc), _p(out), _p(ap)))
    return acc, out, ap
