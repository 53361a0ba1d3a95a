"""Greedy speculative decoding, host side: nvl_lookup_draft (prompt-lookup drafting, no device needed) against a restatement
of its contract, and the presence of the new entry points in the header and the library."""
import ctypes as C

import numpy as np
import pytest


def restated(h, k, ngram):
    """include/nvllm.h, nvl_lookup_draft, in ten lines"""
    n = len(h)
    for g in range(min(ngram, n - 1), 0, -1):
        for s in range(n - g - 1, -1, -1):
            if h[s:s + g] == h[n - g:]:
                got = h[s + g:s + g + k]
                return got + [got[-1]] * (k - len(got)), len(got)
    return [h[-1]] * k, 0


def both(pkg, h, k, ngram):
    draft, n_real = pkg.ops.lookup_draft(h, k, ngram)
    assert (draft.tolist(), n_real) == restated(list(h), k, ngram), (h, k, ngram)
    return draft.tolist(), n_real


def test_lookup_draft_named_cases(pkg):
    # no match at any g: every entry is the last token
    assert both(pkg, [1, 2, 3, 4], 3, 3) == ([4, 4, 4], 0)
    # a match at g < ngram: "7 8" occurs before, "6 7 8" does not
    assert both(pkg, [5, 7, 8, 9, 10, 11, 6, 7, 8], 3, 3) == ([9, 10, 11], 3)
    # the latest of several matches wins (largest s)
    assert both(pkg, [1, 2, 30, 1, 2, 40, 1, 2], 1, 2) == ([40], 1)
    # the continuation runs off the end: padding repeats the last token taken
    assert both(pkg, [1, 2, 3, 1, 2], 4, 2) == ([3, 1, 2, 2], 3)
    # n = 1: nothing to match
    assert both(pkg, [9], 2, 3) == ([9, 9], 0)
    # k = 7 over a periodic history: the LATEST match leaves one period to copy
    assert both(pkg, [1, 2, 3] * 5, 7, 3) == ([1, 2, 3, 3, 3, 3, 3], 3)
    # the longest g is preferred over a later, shorter match
    assert both(pkg, [1, 2, 3, 50, 9, 3, 60, 1, 2, 3], 1, 3) == ([50], 1)


@pytest.mark.parametrize("seed", range(6))
def test_lookup_draft_seeded_histories(pkg, seed):
    r = np.random.default_rng(seed)
    for _ in range(200):
        n = int(r.integers(1, 40))
        h = r.integers(0, int(r.integers(2, 6)), n).tolist()          # tiny alphabets: matches at every g
        both(pkg, h, int(r.integers(1, 8)), int(r.integers(1, 5)))


def test_lookup_draft_refusals(pkg):
    L = pkg.lib()
    h = np.asarray([1, 2, 3], np.int32)
    out = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.nvl_lookup_draft(None, 3, 2, 2, p(out)) == -1
    assert L.nvl_lookup_draft(p(h), 0, 2, 2, p(out)) == -1
    assert L.nvl_lookup_draft(p(h), 3, 0, 2, p(out)) == -1
    assert L.nvl_lookup_draft(p(h), 3, 2, 2, None) == -1
    assert L.nvl_lookup_draft(p(h), 3, 2, 0, p(out)) == 0 and out[:2].tolist() == [3, 3]     # ngram < 1: no match


def test_prototypes_in_header_and_library(pkg):
    new = ("nvl_verify_greedy", "nvl_verify_greedy_paged", "nvl_seq_truncate", "nvl_lookup_draft",
           "nvl_decode_greedy_lookup", "nvl_op_attention_mq")
    declared = pkg.declared_symbols()
    for s in new:
        assert s in declared, s
        assert hasattr(pkg.lib(), s), s
    text = (pkg._lib.HEADER).read_text()
    assert "cmd/ask/main.go:315-360" in text and "generic_model.go:276-480" in text
    assert "key 38" in text
