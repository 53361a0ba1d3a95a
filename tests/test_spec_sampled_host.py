"""Sampled speculative decoding, host side: the new entry points are declared (with their citations), exported and bound,
the Python wrappers exist, refuse mismatched arguments before any library call, and nothing computes without a device."""
import ctypes as C
import re

import numpy as np
import pytest

NEW = ("nvl_verify_sampled", "nvl_verify_sampled_paged", "nvl_decode_sampled_lookup", "nvl_op_sample_drafts")


def test_prototypes_in_header_with_citations(pkg):
    text = pkg._lib.HEADER.read_text()
    declared = pkg.declared_symbols()
    for s in NEW:
        assert s in declared, s
        # the comment right above the prototype cites the sampler and the runner step it replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + s + r"\s*\(", text, flags=re.S)
        assert m, s
        assert "sampling.go:33-102" in m.group(1) and "tensor_model_runner.go:89-93" in m.group(1), s
    assert "#define NVL_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", text)
    assert "nvl_verify_sampled*" in text and "key 38" in text                  # key 38 names the sampled passes too


def test_exported_and_bound(pkg):
    L = pkg.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.nvl_verify_sampled.argtypes) == 11
    assert len(L.nvl_verify_sampled_paged.argtypes) == 13
    assert len(L.nvl_decode_sampled_lookup.argtypes) == 13
    assert len(L.nvl_op_sample_drafts.argtypes) == 14
    assert L.nvl_abi_version() == 3


def test_python_surface(pkg):
    for name in ("verify_sampled", "verify_sampled_paged", "sampled_lookup"):
        assert callable(getattr(pkg.HipTransformerModel, name)), name
    assert callable(pkg.ops.sample_drafts)


class _NoLibrary:
    """stands in for the ctypes library: any call is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _shell(pkg):
    hm = object.__new__(pkg.HipTransformerModel)
    hm.lib, hm.h = _NoLibrary(), None
    return hm


def test_mismatched_lengths_raise_before_any_library_call(pkg):
    hm = _shell(pkg)
    try:
        h, u = [[1, 2, 3]], np.zeros((1, 4), np.float32)
        rows = [[3, 5, 6, 7]]
        with pytest.raises(ValueError):
            hm.verify_sampled([0], rows, 3, h + h, u)                          # two histories for one sequence
        with pytest.raises(ValueError):
            hm.verify_sampled([0], rows, 3, None, u)
        with pytest.raises(ValueError):
            hm.verify_sampled([0], rows, 3, [[]], u)                           # an empty history
        with pytest.raises(ValueError):
            hm.verify_sampled([0], rows, 3, h, u[:, :3])                       # 3 draws for 4 rows
        with pytest.raises(ValueError):
            hm.verify_sampled([0], [[3, 5, 6]], 3, h, u)                       # 3 tokens for 1 + k = 4 rows
        with pytest.raises(ValueError):
            hm.verify_sampled([0], rows, 8, h, u)                              # k outside [0, 7]
        with pytest.raises(ValueError):
            hm.verify_sampled([], [], 3, [], [])
        with pytest.raises(ValueError):
            hm.verify_sampled_paged(rows, 3, [0], [[0], [1]], h, u)            # two block tables for one sequence
        with pytest.raises(ValueError):
            hm.verify_sampled_paged(rows, 3, [0], [[0]], h, u[:, :2])
        with pytest.raises(ValueError):
            hm.verify_sampled_paged([[3, 5]], 3, [0], [[0]], h, u)
        with pytest.raises(ValueError):
            hm.sampled_lookup([0], [3], 5, h, np.zeros((4, 1), np.float32))    # 4 rows of draws for 5 steps
        with pytest.raises(ValueError):
            hm.sampled_lookup([0], [3, 4], 5, h, np.zeros((5, 1), np.float32))
        with pytest.raises(ValueError):
            hm.sampled_lookup([0, 1], [3, 3], 5, h, np.zeros((5, 2), np.float32))
        with pytest.raises(ValueError):
            hm.sampled_lookup([0], [3], 0, h, np.zeros((0, 1), np.float32))
    finally:
        hm.h = None                                                            # (__del__ has nothing to close)
    lg = np.zeros((4, 16), np.float32)
    with pytest.raises(ValueError):
        pkg.ops.sample_drafts(lg, [[3, 1, 2]], 3, [[3]], np.zeros(4))          # 3 tokens for 4 rows
    with pytest.raises(ValueError):
        pkg.ops.sample_drafts(lg, [[3, 1, 2, 0]], 3, [[3]], np.zeros(3))
    with pytest.raises(ValueError):
        pkg.ops.sample_drafts(lg, [[3, 1, 2, 0]], 3, [[3], [3]], np.zeros(4))
    with pytest.raises(ValueError):
        pkg.ops.sample_drafts(lg, [[3, 1, 2, 0]], 2, [[3]], np.zeros(4))       # 4 rows are no multiple of 1 + k = 3


def test_no_cpu_fallback(pkg):
    L = pkg.lib()
    sp = pkg._lib.sampling_params()
    # a NULL handle is refused, not served by some host path
    assert L.nvl_verify_sampled(None, 1, None, None, 1, C.byref(sp), None, None, None, None, None) < 0
    assert L.nvl_verify_sampled_paged(None, 1, None, 1, None, None, None, C.byref(sp), None, None, None, None, None) < 0
    assert L.nvl_decode_sampled_lookup(None, 1, None, None, 1, 1, 1, C.byref(sp), None, None, None, None, None) < 0
    if L.nvl_device_count() > 0:
        return                                                                 # (the GPU file covers a machine with a device)
    with pytest.raises(pkg.NvlError) as e:
        pkg.ops.sample_drafts(np.zeros((2, 16), np.float32), [[3, 1]], 1, [[5, 3]], [0.5, 0.5])
    assert e.value.code == -8                                                  # NVL_ERR_NO_DEVICE
    # the model-level calls need a model, and no model exists without a device
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(pkg.NvlError) as e:
        pkg.HipTransformerModel(cfg, pkg.synth.make_weights(cfg))
    assert e.value.code == -8
