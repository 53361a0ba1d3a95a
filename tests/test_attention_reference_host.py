"""tests/attention_reference.py and the bounds of tests/test_attention_ops_gpu.py proved without a GPU.

The float64 statement is checked against the oracle; the emulation (attention_reference.emulated_device, which reads the
POOLS through the block table as a kernel does, and emulates the fused forms' patch / append and the key-split merge)
stands in for the device: unmutated it must pass every assertion of the GPU file on every batch of the GPU file, and each
mutation — the kernel errors that 2e-2 of a tensor's maximum or an equality between two forms cannot see — must break the
bound or census aimed at it, on a batch the GPU file runs."""
import numpy as np
import pytest

import attention_reference as R
from test_attention_ops_gpu import ATTN_RATIO_BOUND, DECODE_FORMS, PREFILL_RAN, RAN


def forms_of(name):
    return DECODE_FORMS if name in R.DECODE_CASES else (["plain"] if name in R.MQ_CASES else ["plain", "kv8"])


def stand_in(b, mutation=None, seq=0):
    name = b["name"]
    if name in R.DECODE_CASES:
        return R.emulated_device(b, RAN[b["form"]], *b["expect"], mutation=mutation, seq=seq)
    return R.emulated_device(b, "decode_mq" if name in R.MQ_CASES else PREFILL_RAN[b["form"]], 8, 1, mutation=mutation, seq=seq)


def test_reference_against_the_oracle(oracle):
    """one contiguous sequence (pos = 0): attention_f64 == oracle.gqa_core to fp32 rounding, hd 64 and 128"""
    for nH, nKV, S, hd in ((8, 2, 70, 64), (4, 1, 33, 128)):
        r = np.random.default_rng(S)
        q, k, v = (r.standard_normal(s, dtype=np.float32) for s in ((nH, S, hd), (nKV, S, hd), (nKV, S, hd)))
        want = oracle.gqa_core(q, k, v)
        got = R.attention_f64(q.transpose(1, 0, 2), k, v, 0, 1.0 / np.sqrt(hd)).transpose(1, 0, 2)
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()


def test_rope_against_the_oracle_convention():
    """rotate-half: pair (i, i + hd/2) turns by pos x base^(-2i/hd)"""
    hd, pos, base = 64, 37, 10000.0
    x = np.random.default_rng(1).standard_normal((3, hd))
    y = R.rope_f64(x, pos, base, 64)
    ang = pos * base ** (-np.arange(hd // 2) * 2.0 / hd)
    want = np.concatenate([x[:, :32] * np.cos(ang) - x[:, 32:] * np.sin(ang), x[:, 32:] * np.cos(ang) + x[:, :32] * np.sin(ang)], -1)
    assert np.abs(y - want).max() <= 1e-6
    assert np.array_equal(R.rope_f64(x, pos, 0.0, 64), x)


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_batches_are_what_they_claim(name):
    """gather() through the table returns each sequence's own keys; everything else in the pools is the garbage; unused
    table entries name the poison block; block ids are distinct"""
    for form in forms_of(name):
        b = R.batch(name, form)
        used = set()
        for i, (pos, n) in enumerate(zip(b["seq_pos"], b["seq_len"])):
            T = pos + n - (1 if form.startswith("fused") else 0)
            nb = -(-(pos + n) // b["block"])
            assert (b["table"][i, nb:] == b["poison"]).all() and b["poison"] not in b["table"][i, :nb]
            assert not used & set(b["table"][i, :nb].tolist())
            used |= set(b["table"][i, :nb].tolist())
            if form != "kv8":
                assert np.array_equal(R.gather(b["k_pool"], b["table"][i], T, b["block"]), b["K"][i][:, :T])
                assert np.array_equal(R.gather(b["v_pool"], b["table"][i], T, b["block"]), b["V"][i][:, :T])
            rest = R.gather(b["v_pool"], b["table"][i], nb * b["block"], b["block"])[:, T:]
            assert (rest == R.GARBAGE_V).all()
        others = [x for x in range(b["k_pool"].shape[0]) if x not in used]
        assert len(others) >= 3 and (b["v_pool"][others] == R.GARBAGE_V).all() and np.abs(b["k_pool"][others]).max() > 32
        assert np.isfinite(b["k_pool"]).all() and np.array_equal(R.bf16(b["k_pool"]), b["k_pool"].astype(np.float64))
        assert np.array_equal(R.bf16(b["q"]), b["q"].astype(np.float64))


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_unmutated_emulation_passes(name):
    """the emulation within element_bound (with the draws' headroom) and within the ratio bound on every GPU batch, the
    key-split stand-in — another correct rounding order — included"""
    for form in forms_of(name):
        b = R.batch(name, form)
        res = stand_in(b)
        worst, top = R.check_bf16(b, res, ATTN_RATIO_BOUND)
        assert worst <= R.HEADROOM or b["expect"] and b["expect"][1] > 1
        if form.startswith("fused"):
            R.check_append(b, res)


@pytest.mark.parametrize("name", R.CENSUS_CASES)
def test_unmutated_census_passes(name):
    for form in (["plain", "fused", "kv8"] if name in R.DECODE_CASES else ["plain", "kv8"]):
        b = R.batch(name, form, census=True)
        for must in (b["seq_pos"][-1] - 1, b["seq_pos"][-1], b["seq_pos"][-1] + b["seq_len"][-1] - 1):       # last cached key, new keys
            if must >= 0:
                assert (b["V"][-1][0, must] > 0).any(), (name, must)
        res = stand_in(b)
        R.check_census(b, res)
        if form == "fused":
            R.check_append(b, res)


def breaks(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


#            mutation                  batches (case, form, sequence) whose bounds (a)/(b) it must break
BOUND_MUTATIONS = [
    ("drop_key", [("D2", "plain", 0), ("D6", "kv8", 0), ("P1", "plain", 1), ("M1", "plain", 2)]),
    ("extra_key", [("D1", "plain", 1), ("D7", "kv8", 0), ("P1", "kv8", 1)]),
    ("swap_blocks", [("D3", "plain", 0), ("D7", "fused", 2), ("P1", "plain", 1), ("M1", "plain", 2)]),
    ("poison_tile", [("D2", "plain", 0), ("D5", "kv8", 0), ("P3", "plain", 0)]),
    ("merge_scale_one", [("D2", "plain", 0), ("D3", "fused", 1), ("D4", "kv8", 0), ("D6", "plain", 3)]),
    ("next_position", [("D2", "plain", 0), ("D6p", "kv8", 1), ("P1", "plain", 0), ("M2", "plain", 1)]),
    ("wrong_kv_head", [("D1", "plain", 2), ("D8", "fused_norope", 4), ("P3", "kv8", 0)]),
    ("patch_skipped", [("D1", "fused", 0), ("D3", "fused", 0), ("D6", "fused_norope", 2)]),
    ("rope_position_minus_one", [("D2", "fused", 1), ("D7", "fused", 3)]),
]


@pytest.mark.parametrize("mutation,where", BOUND_MUTATIONS, ids=[m for m, _ in BOUND_MUTATIONS])
def test_mutation_breaks_the_bounds(mutation, where):
    for name, form, seq in where:
        b = R.batch(name, form)
        breaks(R.check_bf16, b, stand_in(b, mutation, seq), ATTN_RATIO_BOUND)


CENSUS_MUTATIONS = [
    ("drop_key", [("D3", "plain", 0), ("P1", "kv8", 1)]),           # (the dropped key (T - 1) // 2 is marked in neither: 1/(T-1) for 1/T ...
    ("extra_key", [("D1", "plain", 1), ("D3", "kv8", 1), ("D7", "fused", 0), ("P1", "plain", 1)]),
    ("swap_blocks", [("D3", "plain", 0), ("D7", "kv8", 3), ("P1", "plain", 2)]),
    ("poison_tile", [("D3", "fused", 0), ("D7", "plain", 3), ("P1", "kv8", 2)]),
    ("next_position", [("D1", "plain", 1), ("D7", "kv8", 0), ("P1", "plain", 0)]),
    ("patch_skipped", [("D1", "fused", 0), ("D3", "fused", 0), ("D7", "fused", 1)]),
]


@pytest.mark.parametrize("mutation,where", CENSUS_MUTATIONS, ids=[m for m, _ in CENSUS_MUTATIONS])
def test_mutation_breaks_the_census(mutation, where):
    for name, form, seq in where:
        if mutation == "drop_key" and name == "D3":
            continue      # ... which at 1025 keys is inside 2^-8: the census sees a dropped key only where it is a marked one)
        b = R.batch(name, form, census=True)
        breaks(R.check_census, b, stand_in(b, mutation, seq))


@pytest.mark.parametrize("mutation", ["append_row_off", "append_block_off", "rope_position_minus_one"])
def test_mutation_breaks_the_append_check(mutation):
    for name, seq in (("D1", 1), ("D3", 0), ("D7", 2)):
        for form in (["fused"] if mutation.startswith("rope") else ["fused", "fused_norope"]):
            b = R.batch(name, form)
            breaks(R.check_append, b, stand_in(b, mutation, seq))
