"""MXFP4 LM head and tied token embedding (mx_head_dtype="fp4_e2m1", nvl_set_mx_head_dtype), the parts
that need no GPU: the ABI addition and its Python mirror, and the option's ValueErrors."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvllm.h")


def test_abi_addition(pkg):
    L = pkg._lib
    assert "nvl_set_mx_head_dtype" in pkg.declared_symbols()
    assert hasattr(L.lib(), "nvl_set_mx_head_dtype")
    assert L.lib().nvl_abi_version() == 3
    text = open(HEADER).read()
    assert re.search(r"int nvl_set_mx_head_dtype\(nvl_model\* m, int dtype\);", text)


def test_python_mirror_matches_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_MXH_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_MXH_NONE": 0, "NVL_MXH_FP4_E2M1": 1}
    assert pkg._lib.MX_HEAD_DTYPE == {"none": enum["NVL_MXH_NONE"], "fp4_e2m1": enum["NVL_MXH_FP4_E2M1"]}
    assert len(pkg._lib.lib().nvl_set_mx_head_dtype.argtypes) == 2
    # the enums the other host tests pin, and their mirrors, are unchanged
    for prefix, want, mirror in (("NVL_MX_", {"NVL_MX_NONE": 0, "NVL_MX_FP4_E2M1": 1}, pkg._lib.MX_WEIGHT_DTYPE),
                                 ("NVL_MXE_", {"NVL_MXE_NONE": 0, "NVL_MXE_FP4_E2M1": 1}, pkg._lib.MX_EXPERT_DTYPE)):
        got = dict((k, int(v)) for k, v in re.findall(r"\b(%s[A-Z0-9_]+)\s*=\s*(\d+)" % prefix, text))
        assert got == want and mirror == {"none": 0, "fp4_e2m1": 1}, prefix


def test_null_model_is_refused(pkg):
    assert pkg._lib.lib().nvl_set_mx_head_dtype(None, 1) == -1
    assert pkg._lib.lib().nvl_set_mx_head_dtype(None, 0) == -1


def test_option_value_errors(pkg):
    """raised before the library is asked for a device"""
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_weight_dtype="fp4_e2m1", mx_head_dtype="fp4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, mx_head_dtype="fp4_e2m1")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, weight_dtype="fp8_e4m3", mx_head_dtype="fp4_e2m1")
