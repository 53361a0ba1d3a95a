"""nvl_op_dense_stages with the longer struct (nvl_dense_stages_q: the weights in a quantized format) on the CPU, no GPU:
what it refuses arrives as NVL_ERR_INVALID before the device probe — not as NVL_ERR_NO_DEVICE on a machine without a GPU —,
the ctypes mirror matches the header field for field, and the shorter struct is still accepted."""
import ctypes as C
import re

import numpy as np
import pytest

INVALID, NO_DEVICE = -1, -8
z = lambda *s: np.zeros(s, np.float32)


def call(pkg, M=2, H=256, qw=256, F=512, Nn=384, **kw):
    return pkg.ops.dense_stages(z(M, H), z(M, qw), z(H, qw), z(H), z(2 * F, H), z(H, F), z(H), z(Nn, H), **kw)


def reaches_the_device(fn):
    """the call was not refused: it ran, or only the device probe stopped it"""
    try:
        fn()
    except Exception as e:
        return getattr(e, "code", None) == NO_DEVICE
    return True


def raw_call(pkg, struct_bytes=None, precision="bf16", wt=(), weight_format=0, group_size=0, quantize_next=-1):
    """the long struct filled by hand (what ops.dense_stages would not send: an unknown format code, a stray wt_*)"""
    L = pkg._lib
    M, H, qw, F, Nn = 2, 256, 256, 512, 384
    keep = dict(x=z(M, H), attn_out=z(M, qw), wo=z(H, qw), norm_w=z(H), w1=z(2 * F, H), w2=z(H, F), next_norm_w=z(H), wn=z(Nn, H),
                x1=z(M, H), op1=z(M, H), rs1=z(M, H // 8), h=z(M, F), x2=z(M, H), op2=z(M, H), rs2=z(M, H // 8), yn=z(M, Nn),
                x_end=z(M, H), ran=np.zeros(14, np.int32))
    d = L.DenseStagesC(struct_bytes=C.sizeof(L.DenseStagesQC) if struct_bytes is None else struct_bytes, rows=M, hidden=H,
                       q_width=qw, ffn=F, n_next=Nn, norm_type=1, activation_type=1, block_style=0, max_len=1, has_next=1,
                       n_last_rows=0, norm_eps=1e-5)
    for k, v in keep.items():
        setattr(d, k, v.ctypes.data)
    bufs = {k: z(2 * F, H) for k in wt}
    whole = L.DenseStagesQC(s=d, weight_format=weight_format, group_size=group_size, quantize_next=quantize_next,
                            **{k: v.ctypes.data for k, v in bufs.items()})
    return pkg.lib().nvl_op_dense_stages(0, L.PRECISION[precision], C.cast(C.byref(whole), C.POINTER(L.DenseStagesC)))


def test_refusals_arrive_before_the_device_probe(pkg):
    for kw in (dict(weight_format="fp8", precision="f32"),                    # f32 precision
               dict(weight_format="int4", group_size=48),                      # a group that is not 32 / 64 / 128
               dict(weight_format="int4", group_size=0),
               dict(weight_format="int4", group_size=128, H=192, qw=512),      # ... that does not divide hidden
               dict(weight_format="int4", group_size=128, qw=192),             # ... q_width
               dict(weight_format="int4", group_size=128, F=448),              # ... ffn
               dict(weight_format="mxfp4", H=96),                              # a K that is no multiple of 32 (nvl_create's % 64)
               dict(weight_format="int4", group_size=64, has_next=False, quantize_next=True),      # an INT4 LM head
               dict(weight_format="bf16", quantize_next=True)):
        with pytest.raises(pkg.NvlError) as e:
            call(pkg, **kw)
        assert e.value.code == INVALID, (kw, e.value)
    with pytest.raises(ValueError):
        call(pkg, weight_format="fp4")
    size = C.sizeof(pkg._lib.DenseStagesQC)
    for q in (dict(weight_format=4), dict(weight_format=-1),                  # an unknown format
              dict(wt=("wt_o",)), dict(wt=("wt_1",)), dict(wt=("wt_2",)), dict(wt=("wt_n",)),      # wt_* with bf16 weights
              dict(weight_format=1, quantize_next=0, wt=("wt_n",)),            # ... of a wn that stays bf16
              dict(weight_format=1, quantize_next=2),
              dict(weight_format=1, struct_bytes=size - 8), dict(weight_format=1, struct_bytes=size + 8),      # any other struct_bytes
              dict(weight_format=1, precision="f32")):
        rc = raw_call(pkg, **q)
        assert rc == INVALID, (q, rc, pkg.lib().nvl_last_error(None))


def test_struct_matches_the_header(pkg):
    L = pkg._lib
    text = L.HEADER.read_text()
    body = re.search(r"typedef struct nvl_dense_stages_q \{(.*?)\} nvl_dense_stages_q;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"[*\s,]([a-z_0-9]+)\s*[,;]", body)
    assert names == [n for n, _ in L.DenseStagesQC._fields_], names
    assert re.search(r"\bnvl_dense_stages s;", body) and L.DenseStagesQC._fields_[0][1] is L.DenseStagesC
    kinds = dict(L.DenseStagesQC._fields_)
    assert all(kinds[n] is C.c_int32 for n in ("weight_format", "group_size", "quantize_next", "pad"))
    assert all(kinds[n] is C.c_void_p for n in ("wt_o", "wt_1", "wt_2", "wt_n"))
    assert re.search(r"int32_t weight_format;\s*int32_t group_size;\s*int32_t quantize_next;\s*int32_t pad;\s*float \*wt_o, \*wt_1, \*wt_2, \*wt_n;", body)
    assert C.sizeof(L.DenseStagesQC) == C.sizeof(L.DenseStagesC) + 16 + 4 * C.sizeof(C.c_void_p)
    assert L.DenseStagesQC.weight_format.offset == C.sizeof(L.DenseStagesC)
    for name, code in pkg.ops.EXPERT_FORMATS.items():           # weight_format reuses the experts' codes
        assert re.search(rf"NVL_OP_EXPERTS_{name.upper()} = {code}\b", text), name


def test_the_short_struct_and_the_good_long_ones_are_accepted(pkg):
    assert reaches_the_device(lambda: call(pkg))                                         # the short struct, as before
    assert reaches_the_device(lambda: call(pkg, weight_format="bf16", quantize_next=False))      # the long one with bf16 weights
    for kw in (dict(weight_format="fp8"), dict(weight_format="mxfp4"), dict(weight_format="int4", group_size=128),
               dict(weight_format="fp8", has_next=False), dict(weight_format="mxfp4", has_next=False, quantize_next=True),
               dict(weight_format="int4", group_size=32, has_next=False)):
        assert reaches_the_device(lambda: call(pkg, **kw)), kw
