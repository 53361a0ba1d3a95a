"""MXFP4 (e2m1 + e8m0 block scale) projection weights, the parts that need no GPU: the ABI additions and
their Python mirrors, the option's ValueErrors, and the register budgets of the MXFP4-weight decode kernels next to the
unchanged bf16 / fp8 ones (hipcc cross-compiles them here)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
HEADER = os.path.join(ROOT, "include", "nvllm.h")
NEW = ("nvl_set_mx_weight_dtype", "nvl_upload_tensor_mxfp4", "nvl_op_matmul_mxfp4w")


def test_abi_additions(pkg):
    L = pkg._lib
    assert all(n in pkg.declared_symbols() for n in NEW)
    assert all(hasattr(L.lib(), n) for n in NEW)
    assert L.lib().nvl_abi_version() == 3


def test_python_mirrors_match_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_MX_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_MX_NONE": 0, "NVL_MX_FP4_E2M1": 1}
    assert pkg._lib.MX_WEIGHT_DTYPE == {"none": enum["NVL_MX_NONE"], "fp4_e2m1": enum["NVL_MX_FP4_E2M1"]}
    assert len(pkg._lib.lib().nvl_set_mx_weight_dtype.argtypes) == 2
    assert len(pkg._lib.lib().nvl_upload_tensor_mxfp4.argtypes) == 8
    assert len(pkg._lib.lib().nvl_op_matmul_mxfp4w.argtypes) == 9
    assert re.search(r"int nvl_upload_tensor_mxfp4\(nvl_model\* m, int kind, int layer, const uint8_t\* codes, const uint8_t\* scales,"
                     r"\s+int64_t rows,\s+int64_t cols, int layout\);", text)
    assert re.search(r"int nvl_op_matmul_mxfp4w\(int device, const float\* a, const float\* w, int M, int N, int K, float\* c,"
                     r"\s+uint8_t\* codes_out,\s+uint8_t\* scales_out\);", text)


def test_the_8bit_weight_enum_is_unchanged(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_W_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_W_AUTO": 0, "NVL_W_FP8_E4M3": 1}
    assert pkg._lib.WEIGHT_DTYPE == {"auto": 0, "fp8_e4m3": 1}


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_mx_weight_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_upload_tensor_mxfp4(None, 0, 0, None, None, 1, 32, 1) == -1


def test_option_value_errors(pkg):
    """raised before the library is asked for a device"""
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_weight_dtype="fp4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_weight_dtype="fp4_e2m1", weight_dtype="fp8_e4m3")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_mxfp4_decode_kernel_budgets(tmp_path):
    """the MXFP4-weight decode kernels (narrow and wide, MT 1 / 2 / 4) are held to the fp8 forms' budgets (<= 12 spilled
    registers, <= 512 VGPRs), and the bf16 / fp8w kernels test_fp8_weights_host.py pins still exist under their names"""
    s = tmp_path / "nvllm.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=6",
                           "-Wno-unused-function", "-Wno-unused-variable", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "nano-vllm-go_amd", "csrc", "nvllm.hip"), "-o", str(s)],
                          stderr=subprocess.DEVNULL, timeout=900)
    meta = s.read_text()
    kern = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name: *(\S+)", blk).group(1)
        kern[name] = (int(re.search(r"\.vgpr_count: *(\d+)", blk).group(1)),
                      int(re.search(r"\.vgpr_spill_count: *(\d+)", blk).group(1)))
    mx = {k: v for k, v in kern.items() if "gemm_skinny_mxfp4w_kernel" in k or "gemm_skinny_wide_mxfp4w_kernel" in k}
    for mt in (1, 2, 4):
        assert [k for k in mx if re.search(r"gemm_skinny_mxfp4w_kernelILi%dE" % mt, k)], mt
        assert [k for k in mx if re.search(r"gemm_skinny_wide_mxfp4w_kernelILi%dE" % mt, k)], mt
    assert len([k for k in mx if "wide" in k]) >= 8 and len([k for k in mx if "wide" not in k]) >= 20
    bad = {k: v for k, v in mx.items() if v[1] > 12 or v[0] > 512}
    assert not bad, bad
    fp8 = [k for k in kern if "gemm_skinny_fp8w_kernel" in k or "gemm_skinny_wide_fp8w_kernel" in k]
    assert len([k for k in fp8 if "wide" in k]) >= 8 and len([k for k in fp8 if "wide" not in k]) >= 20
    for name in ("_ZN3nvl23gemm_skinny_bf16_kernelILi1ELi1ELi4ELi0EfLb0ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_bf16_kernelILi4ELi1ELi2ELi1EfLb1ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl28gemm_skinny_wide_bf16_kernelILi2ELi2ELi4ELi2EDF16bLb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_fp8w_kernelILi1ELi1ELi4ELi0EfLb0ELb0EEEvNS_8GemmArgsEPKf"):
        assert name in kern, name
