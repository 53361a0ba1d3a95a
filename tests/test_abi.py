"""The drop-in boundary without a GPU: the library loads, exports every symbol include/nvllm.h declares,
its structs match the ctypes mirrors, and it refuses to compute without a device (no CPU fallback)."""
import ctypes as C
import re

import pytest


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.lib()
    names = pkg.declared_symbols()
    assert len(names) >= 30 and "nvl_forward" in names and "nvl_runner_run" in names and "nvl_op_moe_stages" in names
    assert "nvl_op_attention_batch" in names and "nvl_op_dense_stages" in names and "nvl_op_dense_moe_stages" in names
    assert "nvl_op_moe_stages_q" in names and "nvl_op_dense_moe_stages_q" in names and "nvl_op_qkv_stages" in names
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert L.nvl_abi_version() == 3                                 # (nvl_op_moe_stages / nvl_op_attention_batch / nvl_op_dense_stages and the *_q entry points are additions: the version stays)


def test_header_cites_the_reference_for_every_entry_point(pkg):
    text = pkg._lib.HEADER.read_text()
    for must in ("generic_model.go:276-480", "tensor_model_runner.go:55-97", "model_runner.go:9-16",
                 "generic_loader.go", "cmd/ask/main.go:389-402", "tensor.go:62-88", "rope.go:153-205", "moe.go:43-128"):
        assert must in text, must
    assert 'extern "C"' in text and "torch" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_struct_mirrors_match_the_header(pkg):
    L = pkg._lib
    lib = pkg.lib()
    assert C.sizeof(L.ModelConfigC) == lib.nvl_sizeof(0) == 144     # 13 x i32, pad, f64, f32, i32, 3 x i32, 4 x f32, 6 x i32 (Mamba2), 2 x u64
    assert C.sizeof(L.RuntimeOptsC) == lib.nvl_sizeof(1) == 40
    assert C.sizeof(L.StatsC) == lib.nvl_sizeof(2) == 16 * 8
    assert C.sizeof(L.SamplingParamsC) == lib.nvl_sizeof(3) == 16
    assert [n for n, _ in L.ModelConfigC._fields_][:3] == ["vocab_size", "hidden", "num_layers"]
    assert len(L.SLOTS) == 33 and L.SLOT_ID["moe_out"] == 24 and L.SLOT_ID["mamba_out_proj"] == 32      # NVL_T_COUNT


def test_no_cpu_fallback(pkg):
    L = pkg.lib()
    if L.nvl_device_count() > 0:
        pytest.skip("a GPU is visible here")
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(pkg.NvlError) as e:
        pkg.HipTransformerModel(cfg, pkg.synth.make_weights(cfg))
    assert e.value.code == -8                                      # NVL_ERR_NO_DEVICE
    import numpy as np
    with pytest.raises(pkg.NvlError) as e:
        pkg.ops.mat_mul(np.zeros((1, 64), np.float32), np.zeros((64, 16), np.float32))
    assert e.value.code == -8


def test_moe_stages_refuses_bad_arguments_before_touching_a_device(pkg):
    """nvl_op_moe_stages is bf16 only, and its shape rules are checked before the device probe (NVL_ERR_INVALID, not
    NVL_ERR_NO_DEVICE, on a machine without a GPU)."""
    import numpy as np
    z = np.zeros
    for kw, shape in ((dict(precision="f32"), (2, 64, 4, 64)), (dict(), (2, 64, 4, 48)), (dict(top_k=5), (2, 64, 4, 64)),
                      (dict(), (2, 64, 65, 64))):
        M, H, E, I = shape
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.moe_stages(z((M, H), np.float32), z((H, E), np.float32), z((E, 2 * I, H), np.float32), z((E, H, I), np.float32),
                               kw.get("top_k", 2), precision=kw.get("precision", "bf16"))
        assert e.value.code == -1, (kw, shape)                      # NVL_ERR_INVALID
    # the expert format: what the format's setter would refuse — an unknown format, an INT4 group that is not 32 / 64 / 128 or
    # does not divide hidden and inter, f32 — is refused the same way, in both entry points
    M, H, E, I = 2, 256, 4, 96
    args = (z((M, H), np.float32), z((H, E), np.float32), z((E, 2 * I, H), np.float32), z((E, H, I), np.float32), 2)
    for kw in (dict(expert_format="int4", group_size=64), dict(expert_format="int4", group_size=16), dict(expert_format="int4"),
               dict(expert_format="fp8", precision="f32"), dict(expert_format="mxfp4", precision="f32")):
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.moe_stages(*args, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(ValueError):
        pkg.ops.moe_stages(*args, expert_format="fp4")
    I = 192
    chain = (z((M, H), np.float32), z((M, H), np.float32), z((H, H), np.float32), z(H, np.float32), z((H, E), np.float32),
             z((E, 2 * I, H), np.float32), z((E, H, I), np.float32), z(H, np.float32), 2)
    for kw in (dict(expert_format="int4", group_size=128), dict(expert_format="int4", group_size=48), dict(expert_format="fp8", precision="f32")):
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.dense_moe_stages(*chain, **kw)
        assert e.value.code == -1, kw
    assert pkg.ops.EXPERT_FORMATS == {"bf16": 0, "fp8": 1, "mxfp4": 2, "int4": 3}
    assert re.search(r"NVL_OP_EXPERTS_BF16 = 0, NVL_OP_EXPERTS_FP8 = 1, NVL_OP_EXPERTS_MXFP4 = 2, NVL_OP_EXPERTS_INT4 = 3", pkg._lib.HEADER.read_text())
    assert pkg.ops.MOE_FORMS == {1: "dense_fused", 2: "dense", 3: "plan", 4: "grouped"}
    text = pkg._lib.HEADER.read_text()
    for code, name in enumerate(("DENSE_FUSED", "DENSE", "PLAN", "GROUPED"), 1):
        assert re.search(rf"NVL_MOE_FORM_{name} = {code}\b", text), name


def test_dense_stages_refuses_bad_arguments_before_touching_a_device(pkg):
    """nvl_op_dense_stages is bf16 only and refuses what nvl_create refuses, before the device probe (NVL_ERR_INVALID /
    NVL_ERR_POSITION, not NVL_ERR_NO_DEVICE, on a machine without a GPU); its struct and codes match the header."""
    import numpy as np
    z = lambda *s: np.zeros(s, np.float32)

    def call(M=2, H=256, qw=256, F=512, Nn=384, **kw):
        return pkg.ops.dense_stages(z(M, H), z(M, qw), z(H, qw), z(H), z(2 * F, H), z(H, F), z(H), z(Nn, H), **kw)
    for kw, code in ((dict(precision="f32"), -1), (dict(H=96), -1), (dict(F=96), -1), (dict(qw=32), -1), (dict(M=4096), -1),
                     (dict(attention_multiplier=-1.0), -1), (dict(norm="layer"), -1), (dict(max_len=0), -1),
                     (dict(has_next=False, last_rows=[0, 2]), -2), (dict(has_next=False, last_rows=[0], max_len=1), -1)):
        with pytest.raises(pkg.NvlError) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)
    with pytest.raises(ValueError):
        call(last_rows=[0])                                         # last_rows belong to the last layer
    text = pkg._lib.HEADER.read_text()
    assert C.sizeof(pkg._lib.DenseStagesC) == 64 + 24 * C.sizeof(C.c_void_p)
    fields = re.search(r"typedef struct nvl_dense_stages \{(.*?)\} nvl_dense_stages;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n for n in re.findall(r"[*\s,]([a-z_0-9]+)\s*[,;]", fields)]
    assert names == [n for n, _ in pkg._lib.DenseStagesC._fields_], names
    for table, prefix in ((pkg.ops.RESID_FORMS, "NVL_RESID_FORM_"), (pkg.ops.NORM_RAN, "NVL_NORM_RAN_")):
        for code, name in table.items():
            if name is not None:
                assert re.search(rf"{prefix}{name.upper()} = {code}\b", text), name
    assert re.search(r"NVL_DENSE_RAN_INTS = 14\b", text)
    for kw in (dict(M=65), dict(H=96), dict(I=96), dict(k=9), dict(qw=32)):            # the MoE chain: decode rows, nvl_create's widths
        a = dict(M=2, H=256, qw=256, E=8, k=2, I=64)
        a.update(kw)
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.dense_moe_stages(z(a["M"], a["H"]), z(a["M"], a["qw"]), z(a["H"], a["qw"]), z(a["H"]), z(a["H"], a["E"]),
                                     z(a["E"], 2 * a["I"], a["H"]), z(a["E"], a["H"], a["I"]), z(a["H"]), a["k"])
        assert e.value.code == -1, (kw, e.value)


def test_attention_batch_refuses_bad_arguments_before_touching_a_device(pkg):
    """nvl_op_attention_batch checks what the paged front end checks, and every table entry, before the device probe
    (NVL_ERR_INVALID / NVL_ERR_POSITION, not NVL_ERR_NO_DEVICE, on a machine without a GPU)."""
    import numpy as np
    nH, nKV, hd, bs = 8, 2, 64, 64
    pool = np.zeros((3, nKV, bs, hd), np.float32)
    ok = dict(q=np.zeros((2, nH, hd), np.float32), k_pool=pool, v_pool=pool, block_table=[[0, 1], [2, 2]], seq_len=[1, 1],
              seq_pos=[70, 3], nH=nH)
    for over, code in ((dict(block_table=[[0, 1], [2, 3]]), -1), (dict(block_table=[[0, 1], [-1, 2]]), -1), (dict(seq_pos=[70, -1]), -1),
                       (dict(seq_pos=[128, 3], max_seq=256), -1), (dict(max_seq=70), -2), (dict(seq_len=[1, 0], q=np.zeros((1, nH, hd), np.float32)), -1),
                       (dict(form="kv8", v_scale=float("inf")), -1), (dict(form="mq", precision="f32"), -1),
                       (dict(form="fused", q=np.zeros((2, (nH + 2 * nKV) * hd), np.float32), seq_len=[1, 2], seq_pos=[70, 3]), -1)):
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.attention_batch(**{**ok, **over})
        assert e.value.code == code, (over, e.value)
    assert pkg.ops.ATTN_OP_FORMS == {"plain": 0, "fused": 1, "mq": 2, "kv8": 3}
    text = pkg._lib.HEADER.read_text()
    for code, name in pkg.ops.ATTN_RAN.items():
        assert re.search(rf"NVL_ATTN_RAN_{name.upper()} = {code}\b", text), name
    for name, code in pkg.ops.ATTN_OP_FORMS.items():
        assert re.search(rf"NVL_ATTN_OP_{name.upper()} = {code}\b", text), name


def test_qkv_stages_struct_and_codes_match_the_header(pkg):
    """nvl_op_qkv_stages is an addition (the ABI version stays 3): its struct mirror and the names ops.qkv_stages reports
    match include/nvllm.h.  (Its refusals before the device probe: tests/test_qkv_reference_host.py.)"""
    text = pkg._lib.HEADER.read_text()
    assert pkg.lib().nvl_abi_version() == 3
    assert C.sizeof(pkg._lib.QkvStagesC) == 80 + 20 * C.sizeof(C.c_void_p)
    fields = re.search(r"typedef struct nvl_qkv_stages \{(.*?)\} nvl_qkv_stages;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n for n in re.findall(r"[*\s,]([A-Za-z_0-9]+)\s*[,;]", fields)]
    assert names == [n for n, _ in pkg._lib.QkvStagesC._fields_], names
    for table, prefix in ((pkg.ops.QKV_FORMS, "NVL_QKV_FORM_"), (pkg.ops.GEMM_RAN, "NVL_GEMM_RAN_"), (pkg.ops.EMBED_RAN, "NVL_EMBED_RAN_"),
                          (pkg.ops.NORM_RAN, "NVL_NORM_RAN_")):
        for code, name in table.items():
            if name is not None:
                assert re.search(rf"{prefix}{name.upper()} = {code}\b", text), name
    assert re.search(r"NVL_QKV_RAN_FORM = 0, NVL_QKV_RAN_GEMM = 1, NVL_QKV_RAN_NORM = 2, NVL_QKV_RAN_EMBED = 3, NVL_QKV_RAN_INTS = 4\b", text)
    with pytest.raises(pkg.NvlError) as e:          # a struct of another size is refused
        d = pkg._lib.QkvStagesC(struct_bytes=8)
        pkg._lib.check(pkg.lib().nvl_op_qkv_stages(0, 0, C.byref(d)))
    assert e.value.code == -1


def test_product_package_never_imports_the_oracle(pkg):
    from pathlib import Path
    root = Path(pkg.__file__).resolve().parent
    for p in list(root.rglob("*.py")) + list(root.rglob("*.h")) + list(root.rglob("*.hip")) + list(root.rglob("Makefile")):
        text = p.read_text()
        assert "purego_oracle" not in text and "import oracle" not in text and "from oracle" not in text, p


def test_create_validates_options_before_touching_a_device(pkg):
    """A zero-valued host options struct (max_seqs = 0) must be refused, not turned into a 0-block KV cache
    (the check runs before the device probe, so it is testable without a GPU)."""
    import ctypes as C
    L = pkg._lib
    lib = pkg.lib()
    from importlib import import_module
    cfgc = import_module("nano-vllm-go_amd.model")._cfg_struct(pkg.synth.tiny_config("llama"))
    h = C.c_void_p()
    for bad in (dict(max_seqs=0), dict(max_seqs=-3), dict(max_seqs=2, max_batch_tokens=-1), dict(max_seqs=2, kv_num_blocks=-1)):
        opts = L.RuntimeOptsC(device=0, precision=0, tp_size=1, **bad)
        assert lib.nvl_create(C.byref(cfgc), C.byref(opts), C.byref(h)) == -1, bad     # NVL_ERR_INVALID
        assert not h.value
        assert b"nvl_create" in lib.nvl_last_error(None)
