"""8-bit (e4m3fn) KV cache, the parts that need no GPU: the ABI additions, nvl_create's refusals before any
device is touched, the op entry points' argument checks, and the register budgets of the 8-bit attention kernels
(hipcc cross-compiles them here)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def _create(pkg, kv_cache_dtype, precision, tp_size=1):
    L = pkg._lib
    cfg = L.ModelConfigC()
    cfg.vocab_size, cfg.hidden, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads = 256, 128, 2, 4, 2
    cfg.head_dim, cfg.ffn_dim, cfg.max_seq_len = 64, 256, 128
    cfg.attention_type, cfg.norm_type, cfg.position_type = L.ATTN["gqa"], L.NORM["rmsnorm"], L.POS["rope"]
    cfg.activation_type, cfg.rope_base, cfg.norm_eps = L.ACT["swiglu"], 10000.0, 1e-5
    opts = L.RuntimeOptsC()
    opts.device, opts.precision, opts.max_seqs, opts.max_batch_tokens = 0, precision, 2, 64
    opts.kv_cache_dtype = kv_cache_dtype
    opts.tp_size = tp_size
    h = C.c_void_p()
    rc = L.lib().nvl_create(C.byref(cfg), C.byref(opts), C.byref(h))
    if rc == 0:
        L.lib().nvl_destroy(h)
    return rc, L.lib().nvl_last_error(None).decode()


def test_abi_additions(pkg):
    L = pkg._lib
    names = pkg.declared_symbols()
    new = ("nvl_op_fp8_kv_roundtrip", "nvl_op_attention_kv8", "nvl_set_kv_scales")
    assert all(n in names for n in new) and all(hasattr(L.lib(), n) for n in new)
    assert [f for f, _ in L.RuntimeOptsC._fields_][-1] == "kv_cache_dtype"
    assert C.sizeof(L.RuntimeOptsC) == L.lib().nvl_sizeof(1) == 40
    assert L.lib().nvl_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "nvllm.h")).read()
    assert re.search(r"NVL_KV_AUTO\s*=\s*0", hdr) and re.search(r"NVL_KV_FP8_E4M3\s*=\s*1", hdr)
    assert L.KV_CACHE_DTYPE == {"auto": 0, "fp8_e4m3": 1}


@pytest.mark.parametrize("kv_cache_dtype,precision", [(7, 0), (-1, 0), (1, 1)])
def test_create_refuses_bad_kv_cache_dtype_before_the_device(pkg, kv_cache_dtype, precision):
    """Unknown values and fp8 with f32 precision are NVL_ERR_INVALID, on a machine with or without a GPU (the checks run
    before the device probe, which would answer NVL_ERR_NO_DEVICE here)."""
    rc, msg = _create(pkg, kv_cache_dtype, precision)
    assert rc == -1, (rc, msg)
    assert "kv_cache_dtype" in msg or "fp8" in msg


def test_create_refuses_fp8_with_tensor_parallelism(pkg):
    rc, msg = _create(pkg, 1, 0, tp_size=2)
    assert rc == -1 and "tensor parallel" in msg, (rc, msg)


def test_python_option_is_checked(pkg):
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(pkg.synth.tiny_config("llama"), None, kv_cache_dtype="int4")


def test_kv8_ops_check_arguments_before_the_device(pkg):
    L = pkg._lib
    x = np.ones(8, np.float32)
    codes = np.empty(8, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.lib().nvl_op_fp8_kv_roundtrip(0, p(x), 8, bad, p(codes), p(x.copy())) == -1
    q = np.ones((2, 1, 64), np.float32)
    k = np.ones((1, 4, 64), np.float32)
    out = np.empty_like(q)
    for ks, vs in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert L.lib().nvl_op_attention_kv8(0, p(q), p(k), p(k), 2, 1, 1, 4, 64, 0.0, ks, vs, p(out)) == -1
    assert L.lib().nvl_op_attention_kv8(0, p(q), p(k), p(k), 2, 1, 1, 4, 96, 0.0, 1.0, 1.0, p(out)) == -1   # hd


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_kv8_kernel_register_budgets(tmp_path):
    """Every 8-bit attention instantiation the library launches compiles without spills; the hd-64 decode kernels keep
    two waves per SIMD (<= 256 registers, VGPR + AGPR), the prefill kernels their launch bounds."""
    src = tmp_path / "kv8_isa.hip"
    inst = []
    for hd in (64, 128):
        for nw in (2, 4, 8):
            inst.append(f"template __global__ void nvl::attn_decode_kv8_kernel<{hd}, {nw}>(const int32_t*, const int32_t*, "
                        "int, int, int, int, nvl::AttnArgs, float, float);")
        inst.append(f"template __global__ void nvl::attn_prefill_kv8_kernel<{hd}>(nvl::AttnArgs, float, float);")
    src.write_text('#include "kv8.h"\n' + "\n".join(inst) + "\n")
    asm = tmp_path / "kv8_isa.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=6",
                        "-Wno-unused-function", "-Wno-unused-variable", "--cuda-device-only", "-S",
                        "-I", os.path.join(ROOT, "nano-vllm-go_amd", "csrc"), str(src), "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    text = asm.read_text()
    kern = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        g = lambda k: int(re.search(r"\." + k + r": *(\d+)", blk).group(1))
        kern[re.search(r"\.name: *(\S+)", blk).group(1)] = dict(
            agpr=int(re.match(r" *(\d+)", blk).group(1)), vgpr=g("vgpr_count"), spill=g("vgpr_spill_count"))
    dec = {k: v for k, v in kern.items() if "attn_decode_kv8_kernel" in k}
    pre = {k: v for k, v in kern.items() if "attn_prefill_kv8_kernel" in k}
    assert len(dec) == 6 and len(pre) == 2, sorted(kern)
    for k, v in {**dec, **pre}.items():
        assert v["spill"] == 0, (k, v)
    for k, v in dec.items():
        if "ILi64E" in k:
            assert v["vgpr"] + v["agpr"] <= 256, (k, v)
    for k, v in pre.items():
        assert v["vgpr"] + v["agpr"] <= (128 if "ILi64E" in k else 256), (k, v)
