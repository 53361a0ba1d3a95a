"""nvl_set_mamba_rollback, the parts that need no GPU: the ABI additions and the refusals answered
before a device is touched.  (The setter's other refusals need a created model: test_mamba_verify_gpu.py.)"""
import re

import pytest


def test_header_and_exports(pkg):
    text = pkg._lib.HEADER.read_text()
    L = pkg.lib()
    for name in ("nvl_set_mamba_rollback", "nvl_op_mamba_verify"):
        assert name in pkg.declared_symbols() and hasattr(L, name), name
    assert re.search(r"NVL_MAMBA_ROLLBACK_NONE\s*=\s*0", text) and re.search(r"NVL_MAMBA_ROLLBACK_VERIFY\s*=\s*1", text)
    assert L.nvl_abi_version() == 3
    assert pkg._lib.MAMBA_ROLLBACK == {"none": 0, "verify": 1}
    assert callable(pkg.ops.mamba_verify)


def test_null_model_and_bad_option_are_refused_before_the_device(pkg):
    assert pkg.lib().nvl_set_mamba_rollback(None, 1) == -1       # NVL_ERR_INVALID, not NVL_ERR_NO_DEVICE (-8)
    for bad in ("x", "VERIFY", None, 1):
        with pytest.raises(ValueError):
            pkg.HipTransformerModel(pkg.synth.tiny_config("granite_hybrid"), None, mamba_rollback=bad)
