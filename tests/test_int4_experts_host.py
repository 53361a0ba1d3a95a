"""INT4 group-quantized MoE expert weights (gq_expert_dtype="uint4", nvl_set_gq_expert_dtype), the parts
that need no GPU: the ABI addition and its Python mirror, the option's ValueErrors, and the MoE INT4 decode kernels as hipcc
builds them for gfx950 (every form the MXFP4 MoE wrappers have, held to their register budget) with the two expert-layout
kernels of w4g.h."""
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
    assert "nvl_set_gq_expert_dtype" in pkg.declared_symbols()
    assert hasattr(L.lib(), "nvl_set_gq_expert_dtype")
    assert L.lib().nvl_abi_version() == 3
    text = open(HEADER).read()
    assert re.search(r"int nvl_set_gq_expert_dtype\(nvl_model\* m, int dtype\);", text)
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_GQE_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_GQE_NONE": 0, "NVL_GQE_UINT4": 1}


def test_python_mirror_matches_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_GQE_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert pkg._lib.GQ_EXPERT_DTYPE == {"none": enum["NVL_GQE_NONE"], "uint4": enum["NVL_GQE_UINT4"]}
    assert len(pkg._lib.lib().nvl_set_gq_expert_dtype.argtypes) == 2
    # the enum of the projection weights is not touched by the new prefix
    gq = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_GQ_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert gq == {"NVL_GQ_NONE": 0, "NVL_GQ_UINT4": 1}
    assert [pkg._lib.lib().nvl_sizeof(i) for i in range(4)] == [144, 40, 128, 16] and len(pkg._lib.SLOTS) == 33


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_gq_expert_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_set_gq_expert_dtype(None, 0) == -1


def test_option_value_errors(pkg):
    """raised before the library is asked for a device"""
    cfg = pkg.synth.tiny_config("granite_moe")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_weight_dtype="uint4", gq_group_size=64, gq_expert_dtype="int4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_expert_dtype="uint4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_weight_dtype="fp4_e2m1", gq_expert_dtype="uint4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, weight_dtype="fp8_e4m3", gq_expert_dtype="uint4")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_moe_int4_decode_kernels_build_for_gfx950(tmp_path):
    """the MoE INT4 decode kernels exist at MT 1 / 2 / 4 in every form the MXFP4 MoE wrappers have (the same template arguments
    under the other kernel name, but for U, the k-steps per register set), none above 12 spilled registers or 512 VGPRs; the
    concatenated-down builder and the down dequantize of w4g.h are in the code object"""
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
    gq = {k: v for k, v in kern.items() if "gemm_skinny_moe_int4w_kernel" in k or "gemm_skinny_wide_moe_int4w_kernel" in k}
    mx = [k for k in kern if "gemm_skinny_moe_mxfp4w_kernel" in k or "gemm_skinny_wide_moe_mxfp4w_kernel" in k]
    assert len(mx) >= 12
    for mt in (1, 2, 4):
        assert [k for k in gq if re.search(r"gemm_skinny_moe_int4w_kernelILi%dE" % mt, k)], mt
        assert [k for k in gq if re.search(r"gemm_skinny_wide_moe_int4w_kernelILi%dE" % mt, k)], mt
    strip = lambda k, a, b: re.sub(r"(kernelILi\d+ELi\d+E)Li\d+E", r"\1", re.sub(r"^_ZN3nvl\d+", "", k).replace(a, b).rsplit("EEvNS_8GemmArgs", 1)[0])
    have = {strip(k, "int4w", "Xw") for k in gq}
    missing = [k for k in mx if strip(k, "mxfp4w", "Xw") not in have]
    assert not missing, missing
    bad = {k: v for k, v in gq.items() if v[1] > 12 or v[0] > 512}
    assert not bad, bad
    assert [k for k in kern if "moe_cat_down_w4g_kernel" in k] and [k for k in kern if "e4g_dequant_down_kernel" in k]
