"""MXFP4 MoE expert weights (mx_expert_dtype="fp4_e2m1", nvl_set_mx_expert_dtype), the parts that need no
GPU: the ABI addition and its Python mirror, the option's ValueErrors, and the MoE MXFP4 decode kernels as hipcc builds them
for gfx950 (held to the decode kernels' register budget) next to the unchanged bf16 / fp8w / mxfp4w / moe_fp8w kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
HEADER = os.path.join(ROOT, "include", "nvllm.h")


def test_abi_addition(pkg):
    L = pkg._lib
    assert "nvl_set_mx_expert_dtype" in pkg.declared_symbols()
    assert hasattr(L.lib(), "nvl_set_mx_expert_dtype")
    assert L.lib().nvl_abi_version() == 3
    text = open(HEADER).read()
    assert re.search(r"int nvl_set_mx_expert_dtype\(nvl_model\* m, int dtype\);", text)


def test_python_mirror_matches_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_MXE_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_MXE_NONE": 0, "NVL_MXE_FP4_E2M1": 1}
    assert pkg._lib.MX_EXPERT_DTYPE == {"none": enum["NVL_MXE_NONE"], "fp4_e2m1": enum["NVL_MXE_FP4_E2M1"]}
    assert len(pkg._lib.lib().nvl_set_mx_expert_dtype.argtypes) == 2
    # the enums the other host tests pin, and their mirrors, are unchanged
    for prefix, want, mirror in (("NVL_MX_", {"NVL_MX_NONE": 0, "NVL_MX_FP4_E2M1": 1}, pkg._lib.MX_WEIGHT_DTYPE),
                                 ("NVL_EXPERT_", {"NVL_EXPERT_AUTO": 0, "NVL_EXPERT_FP8_E4M3": 1}, pkg._lib.EXPERT_DTYPE)):
        got = dict((k, int(v)) for k, v in re.findall(r"\b(%s[A-Z0-9_]+)\s*=\s*(\d+)" % prefix, text))
        assert got == want and sorted(mirror.values()) == [0, 1] and len(mirror) == 2, prefix


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_mx_expert_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_set_mx_expert_dtype(None, 0) == -1


def test_option_value_errors(pkg):
    """raised before the library is asked for a device"""
    cfg = pkg.synth.tiny_config("granite_moe")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_weight_dtype="fp4_e2m1", mx_expert_dtype="fp4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_expert_dtype="fp4_e2m1")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, weight_dtype="fp8_e4m3", mx_expert_dtype="fp4_e2m1")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_moe_mxfp4_decode_kernels_build_for_gfx950(tmp_path):
    """the MoE MXFP4 decode kernels (narrow SwiGLU / K-split down at (MT, U) = (1, 4), (2, 4), (4, 2), wide SwiGLU at MT 1 / 2 /
    4 with 2 and 4 tiles per wave) exist with <= 12 spilled registers and <= 512 VGPRs, beside the kernels the other host
    tests pin under their unchanged names"""
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
    narrow = {k: v for k, v in kern.items() if "gemm_skinny_moe_mxfp4w_kernel" in k}
    wide = {k: v for k, v in kern.items() if "gemm_skinny_wide_moe_mxfp4w_kernel" in k}
    for mt, u in ((1, 4), (2, 4), (4, 2)):
        # down: EPI_RESID (1), fp32 out, NTW 1; up: EPI_SWIGLU (2), bf16 out, NTW 2 (narrow) / NTB 2 and 4 (wide)
        assert f"_ZN3nvl29gemm_skinny_moe_mxfp4w_kernelILi{mt}ELi1ELi{u}ELi1EfEEvNS_8GemmArgsEPKh" in narrow, mt
        assert f"_ZN3nvl29gemm_skinny_moe_mxfp4w_kernelILi{mt}ELi2ELi{u}ELi2EDF16bEEvNS_8GemmArgsEPKh" in narrow, mt
        for ntb in (2, 4):
            assert f"_ZN3nvl34gemm_skinny_wide_moe_mxfp4w_kernelILi{mt}ELi{ntb}ELi{u}ELi2EDF16bEEvNS_8GemmArgsEPKh" in wide, (mt, ntb)
    bad = {k: v for k, v in {**narrow, **wide}.items() if v[1] > 12 or v[0] > 512}
    assert not bad, bad
    for name in ("_ZN3nvl23gemm_skinny_bf16_kernelILi1ELi1ELi4ELi0EfLb0ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_bf16_kernelILi4ELi1ELi2ELi1EfLb1ELb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl28gemm_skinny_wide_bf16_kernelILi2ELi2ELi4ELi2EDF16bLb0ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_bf16_kernelILi4ELi1ELi2ELi1EfLb0ELb1ELb0EEEvNS_8GemmArgsE",
                 "_ZN3nvl28gemm_skinny_wide_bf16_kernelILi2ELi2ELi4ELi2EDF16bLb0ELb1EEEvNS_8GemmArgsE",
                 "_ZN3nvl23gemm_skinny_fp8w_kernelILi1ELi1ELi4ELi0EfLb0ELb0EEEvNS_8GemmArgsEPKf",
                 "_ZN3nvl23gemm_skinny_fp8w_kernelILi1ELi1ELi4ELi1EfLb0ELb0EEEvNS_8GemmArgsEPKf",
                 "_ZN3nvl28gemm_skinny_wide_fp8w_kernelILi2ELi2ELi4ELi2EDF16bLb0EEEvNS_8GemmArgsEPKf"):
        assert name in kern, name
    for mt, u in ((1, 4), (2, 4), (4, 2)):
        assert f"_ZN3nvl27gemm_skinny_moe_fp8w_kernelILi{mt}ELi1ELi{u}ELi1EfEEvNS_8GemmArgsEPKf" in kern, mt
        assert f"_ZN3nvl32gemm_skinny_wide_moe_fp8w_kernelILi{mt}ELi2ELi{u}ELi2EDF16bEEvNS_8GemmArgsEPKf" in kern, mt
    mx = [k for k in kern if "gemm_skinny_mxfp4w_kernel" in k or "gemm_skinny_wide_mxfp4w_kernel" in k]
    assert len([k for k in mx if "wide" in k]) >= 8 and len([k for k in mx if "wide" not in k]) >= 20
