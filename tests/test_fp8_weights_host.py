"""8-bit (e4m3fn) projection weights, the parts that need no GPU: the ABI additions and their Python
mirrors, and the register budgets of the fp8-weight decode kernels next to the unchanged bf16 ones (hipcc cross-compiles
them here)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
HEADER = os.path.join(ROOT, "include", "nvllm.h")


def test_abi_additions(pkg):
    L = pkg._lib
    new = ("nvl_set_weight_dtype", "nvl_op_matmul_fp8w", "nvl_upload_tensor_fp8")
    assert all(n in pkg.declared_symbols() for n in new)
    assert all(hasattr(L.lib(), n) for n in new)
    assert L.lib().nvl_abi_version() == 3


def test_python_mirrors_match_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_W_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_W_AUTO": 0, "NVL_W_FP8_E4M3": 1}
    assert pkg._lib.WEIGHT_DTYPE == {"auto": enum["NVL_W_AUTO"], "fp8_e4m3": enum["NVL_W_FP8_E4M3"]}
    assert len(pkg._lib.lib().nvl_op_matmul_fp8w.argtypes) == 9
    assert len(pkg._lib.lib().nvl_set_weight_dtype.argtypes) == 2
    assert len(pkg._lib.lib().nvl_upload_tensor_fp8.argtypes) == 8
    assert re.search(r"int nvl_upload_tensor_fp8\(nvl_model\* m, int kind, int layer, const uint8_t\* codes, const float\* scales, int64_t rows,"
                     r"\s+int64_t cols, int layout\);", text)


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_weight_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_upload_tensor_fp8(None, 0, 0, None, None, 1, 1, 1) == -1


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_fp8_decode_kernel_budgets(tmp_path):
    """the fp8-weight decode kernels are held to check_isa.sh's budgets for the bf16 forms (<= 12 spilled registers), and
    the bf16 decode kernels still exist under their mangled names"""
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
    fp8 = {k: v for k, v in kern.items() if "gemm_skinny_fp8w_kernel" in k or "gemm_skinny_wide_fp8w_kernel" in k}
    assert len([k for k in fp8 if "wide" in k]) >= 8 and len([k for k in fp8 if "wide" not in k]) >= 20
    bad = {k: v for k, v in fp8.items() if v[1] > 12 or v[0] > 512}
    assert not bad, bad
    for name in ("_ZN3nvl23gemm_skinny_bf16_kernelILi1ELi1ELi4ELi0EfLb0ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_bf16_kernelILi4ELi1ELi2ELi1EfLb1ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl28gemm_skinny_wide_bf16_kernelILi2ELi2ELi4ELi2EDF16bLb0ELb0EEEvNS_8GemmArgsE"):
        assert name in kern, name
