"""8-bit activations (act_dtype="fp8_e4m3"), the parts that need no GPU: the ABI additions and their
Python mirrors, and the W8A8 kernels as hipcc builds them for gfx950 (the scaled FP8 MFMA in each, no spills, LDS within a
CU's 160 KiB)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
HEADER = os.path.join(ROOT, "include", "nvllm.h")
NEW = ("nvl_set_act_dtype", "nvl_op_matmul_w8a8", "nvl_op_act_quant_fp8")


def test_abi_additions(pkg):
    L = pkg._lib
    assert all(n in pkg.declared_symbols() for n in NEW)
    assert all(hasattr(L.lib(), n) for n in NEW)
    assert L.lib().nvl_abi_version() == 3


def test_python_mirrors_match_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_ACT_(?:AUTO|FP8_E4M3))\s*=\s*(\d+)", text))
    assert enum == {"NVL_ACT_AUTO": 0, "NVL_ACT_FP8_E4M3": 1}
    assert pkg._lib.ACT_DTYPE == {"auto": enum["NVL_ACT_AUTO"], "fp8_e4m3": enum["NVL_ACT_FP8_E4M3"]}
    assert re.search(r"int nvl_set_act_dtype\(nvl_model\* m, int dtype\);", text)
    assert re.search(r"int nvl_op_matmul_w8a8\(int device, const float\* a, const float\* w, int M, int N, int K, float\* c, "
                     r"uint8_t\* a_codes_out,\s+float\* a_scales_out\);", text)
    lib = pkg._lib.lib()
    assert len(lib.nvl_set_act_dtype.argtypes) == 2
    assert len(lib.nvl_op_matmul_w8a8.argtypes) == 9
    assert len(lib.nvl_op_act_quant_fp8.argtypes) == 7


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_act_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_set_act_dtype(None, 0) == -1


def test_model_option_needs_fp8_weights(pkg):
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, act_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, weight_dtype="fp8_e4m3", act_dtype="int8")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_w8a8_kernels_build_for_gfx950(tmp_path):
    s = tmp_path / "nvllm.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=6",
                           "-Wno-unused-function", "-Wno-unused-variable", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "nano-vllm-go_amd", "csrc", "nvllm.hip"), "-o", str(s)],
                          stderr=subprocess.DEVNULL, timeout=900)
    text = s.read_text()
    bodies = dict((m.group(1), m.group(2)) for m in
                  re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M))
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name: *(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s: *(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
    gemm = [k for k in bodies if "gemm_w8a8_pp_kernel" in k]
    quant = [k for k in bodies if "a8_quant_kernel" in k]
    # every epilogue: STORE fp32 / bf16, RESID, SWIGLU, GELU on both forms, QKV on four (head 64 and 128)
    assert len(gemm) == 14 and len(quant) == 1, gemm
    for k in gemm:
        assert re.search(r"v_mfma_scale_f32_(32x32x64|16x16x128)_f8f6f4", bodies[k]), k
        bm, bn = map(int, re.search(r"Li(\d+)ELi(\d+)ELi\d+EEEvNS_8GemmArgs", k).groups())
        lds = 4 * (bm + bn) * 64 + meta[k]["group_segment_fixed_size"]      # the 4-slot ring is dynamic LDS
        assert lds <= 160 * 1024, (k, lds)
    for k in gemm + quant:
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["sgpr_spill_count"] == 0, (k, meta[k])
        assert meta[k]["vgpr_count"] <= 256, (k, meta[k])
    for k in quant:
        assert "v_cvt_pk_fp8_f32" in bodies[k]
