"""Token log-probabilities, the part that needs no GPU: the four entry points are declared with
their reference citations and exported, the Python surface exists and refuses mismatched lengths before it touches the
library, and without a device the op answers NVL_ERR_NO_DEVICE (no CPU fallback)."""
import re

import numpy as np
import pytest

SYMBOLS = ("nvl_logprobs", "nvl_score", "nvl_score_paged", "nvl_op_logprobs")


def test_symbols_declared_with_citations_and_exported(pkg):
    text = pkg._lib.HEADER.read_text()
    L = pkg.lib()
    for name in SYMBOLS:
        assert name in pkg.declared_symbols(), name
        assert hasattr(L, name), name
        # the comment block right above the declaration cites the reference lines it extends
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", text, flags=re.S)
        assert m, name
        assert re.search(r"generic_model\.go:\d+-\d+", m.group(1)), name
    for must in ("generic_model.go:467-470", "generic_model.go:595-604", "cmd/check-logits/main.go"):
        assert must in text, must
    assert "key 37" in text                               # the row-chunk tuning key is documented with the others
    assert L.nvl_abi_version() == 3


def test_python_surface_exists(pkg):
    assert callable(pkg.ops.logprobs)
    for name in ("score", "score_paged", "logprobs"):
        assert callable(getattr(pkg.HipTransformerModel, name)), name


def test_length_mismatches_raise_before_any_library_call(pkg):
    with pytest.raises(ValueError):
        pkg.ops.logprobs(np.zeros((3, 10), np.float32), [0, 1])                  # 2 targets, 3 rows
    buf = np.zeros((2, 16), np.float32)
    with pytest.raises(ValueError):
        pkg.ops.logprobs(buf[:, :10], [0, 1], ld=12)                             # not a view of a 12-wide buffer
    m = object.__new__(pkg.HipTransformerModel)                                  # no handle: a library call would crash
    m.h = None
    with pytest.raises(ValueError):
        m.score([0, 1], [[1, 2, 3]], [0, 0])                                     # 2 ids, 1 token list
    with pytest.raises(ValueError):
        m.score([0], [[1, 2, 3]], [0], targets=[[2, 3]])                         # 3 tokens, 2 targets
    with pytest.raises(ValueError):
        m.score([0], [[1, 2, 3]], [0], targets=[[2, 3, -1], [1]])                # 2 target lists, 1 sequence
    with pytest.raises(ValueError):
        m.score_paged([[1, 2]], [0, 0], [[0]])                                   # 1 sequence, 2 offsets
    with pytest.raises(ValueError):
        m.score([0], [[1, 2, 3]], [0], top_k=9)


def test_default_targets_are_the_next_tokens(pkg):
    m = object.__new__(pkg.HipTransformerModel)
    lens, toks, tg, out = m._score_args([[5, 6, 7], [9]], None, 2)
    assert lens.tolist() == [3, 1] and toks.tolist() == [5, 6, 7, 9]
    assert tg.tolist() == [6, 7, -1, -1]
    assert out[0].shape == (4,) and out[2].shape == (4, 2)


def test_no_cpu_fallback(pkg):
    if pkg.lib().nvl_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(pkg.NvlError) as e:
        pkg.ops.logprobs(np.zeros((2, 10), np.float32), [1, -1])
    assert e.value.code == -8
