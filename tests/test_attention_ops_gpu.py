"""The attention kernels of attn.h and kv8.h as a model runs them — batched, paged, key-split and fused — through
nvl_op_attention_batch (ops.attention_batch: the model's own attention() / attention_kv8() on a batch laid out as the paged
front end lays it out) against the float64 statement of tests/attention_reference.py.

Every test asserts the kernel form that ran and its launch shape (waves per workgroup, workgroups per (sequence, kv
head)), so a fallback cannot pass for the form under test, and that `out` is finite: the op fills the output rows and the
split scratch with NaN bytes first.  The pools hold large finite garbage wherever no key of the batch lives, every unused
table entry names a poison block, and block ids are a seeded permutation (attention_reference.py): a wrong block, row,
head or mask limit gives wrong numbers, never an access outside the pool.

Bounds (attention_reference.py derives them).  bf16 forms: (a) per element |dev - f64| <= 1.05 element_bound + 1e-6
max|f64|, element_bound = 2^-9 (A + 2 |f64|); (b) per (sequence, kv head), pooled over its rows, rms(dev - f64) <=
ATTN_RATIO_BOUND x rms(emulated - f64).  ATTN_RATIO_BOUND = 1.25 x the largest ratio measured on the MI355X over all cases
of this file (profiles/attention_op_tests.txt, written by scripts/attention_op_figures.py), never above 2 — the rule of
test_moe_ops_gpu.py.  f32: 5e-5 of the row maximum, per row.  Census: q = 0, V marks one key per output dimension; the
output is exactly 0 where the marked key is invisible and within 2^-8 of 1 / (seq_pos + j + 1) where it is visible; a
garbage row counted shows as about 1024 / T.  tests/test_attention_reference_host.py shows on the CPU that each bound
fails under the mutation it is aimed at.

What the op-level tests before this file never ran, and the test here that does:
 1. a block table with more than one entry, permuted blocks, stale entries, Tmax no power of two  -> every case; D7, P3
 2. a batch: seq_tok_start, ragged seq_len / seq_pos, a short sequence beside a long one           -> D1-D8, P1, M2
 3. the key-split decode form for bf16 K/V: records, ticket, merge, idle workgroups, the reset     -> D2-D6, test_split_*
 4. the fused decode form: RoPE, the operand patch of the tile holding the new key, the append     -> test_decode (fused forms), test_census
 5. per-element and per-(sequence, kv head) bounds instead of 2e-2 of the tensor's maximum          -> every case
 6. a visibility census of the one-position decode forms and both prefill kernels                   -> test_census
What building it found (read in the launch code while sizing P1; the old sizing was never run on P1): attention_launch sized attn_f32_kernel's score buffer (dynamic LDS) by Tmax, the tokens of ONE KV block;
in paged mode a row sees up to blocks_per_seq blocks, so the scores of a context longer than one block were written and
read outside the workgroup's LDS allocation (P1 at f32: 1001 keys over 64-key blocks).  It is now sized by blocks_per_seq
x Tmax (slab mode: unchanged)."""
import numpy as np
import pytest

import attention_reference as R

pytestmark = pytest.mark.gpu

ATTN_RATIO_BOUND = 1.550         # 1.25 x the largest measured device / emulation rms ratio, 1.2397 (profiles/attention_op_tests.txt)

DECODE_FORMS = ["plain", "fused", "fused_norope", "kv8"]
RAN = {"plain": "decode", "fused": "decode_fused", "fused_norope": "decode_fused", "kv8": "decode_kv8"}
PREFILL_RAN = {"plain": "prefill", "kv8": "prefill_kv8"}


class Tuning:
    """nvl_set_tuning keys for a block, restored afterwards"""
    def __init__(self, gpu, keys):
        self.lib, self.keys, self.old = gpu.lib(), keys, {}

    def __enter__(self):
        for key, value in self.keys.items():
            self.old[key] = self.lib.nvl_set_tuning(key, value)

    def __exit__(self, *exc):
        for key, value in self.old.items():
            self.lib.nvl_set_tuning(key, value)


def run(gpu, b, precision="bf16", keys=None):
    """the op on a batch of attention_reference.batch()"""
    form = {"fused_norope": "fused"}.get(b["form"], b["form"])
    with Tuning(gpu, keys or {}):
        return gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"], form=form,
                                       scale=0.0, rope_base=b["rope_base"], max_seq=b["max_seq"], k_scale=b.get("k_scale", 1.0),
                                       v_scale=b.get("v_scale", 1.0), precision=precision)


def ran_as(res, ran, shape, tag=""):
    assert (res["ran"], res["nw"], res["nsplit"]) == (ran,) + tuple(shape), (tag, res["ran"], res["nw"], res["nsplit"])
    assert np.isfinite(res["out"]).all(), tag


@pytest.mark.parametrize("form", DECODE_FORMS)
@pytest.mark.parametrize("name", list(R.DECODE_CASES))
def test_decode(gpu, name, form):
    b = R.batch(name, form)
    res = run(gpu, b)
    ran_as(res, RAN[form], b["expect"], (name, form))
    R.check_bf16(b, res, ATTN_RATIO_BOUND)
    if form.startswith("fused"):
        R.check_append(b, res)
    if b["expect"][1] == 1:
        assert not res["part_cnt"].any()


@pytest.mark.parametrize("name", ["D1", "D2"])
def test_decode_wave_counts_and_load_policy(gpu, name):
    """nvl_set_tuning key 15 (2 / 4 / 8 waves per workgroup, which also turns the key split off) under both bounds; key 35
    (non-temporal K/V loads never / always) changes no bit"""
    for form in DECODE_FORMS:
        b = R.batch(name, form)
        for nw in (2, 4, 8):
            res = run(gpu, b, keys={15: nw})
            ran_as(res, RAN[form], (nw, 1), (name, form, nw))
            R.check_bf16(b, res, ATTN_RATIO_BOUND, f"key 15 = {nw}")
        base = run(gpu, b)
        for nt in (0, 2):
            res = run(gpu, b, keys={35: nt})
            ran_as(res, RAN[form], b["expect"], (name, form, nt))
            assert np.array_equal(res["out"], base["out"]), (name, form, "key 35", nt)


@pytest.mark.parametrize("name", R.SPLIT_CASES)
def test_split_tickets_reset_and_order(gpu, name):
    """every key-split launch leaves its tickets at zero, and three runs agree bit for bit (the merge sums in z order
    whichever workgroup arrives last)"""
    for form in DECODE_FORMS:
        b = R.batch(name, form)
        outs = []
        for _ in range(3):
            res = run(gpu, b)
            ran_as(res, RAN[form], b["expect"], (name, form))
            assert not res["part_cnt"].any(), (name, form, res["part_cnt"])
            outs.append(res["out"])
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (name, form)


@pytest.mark.parametrize("form", ["plain", "kv8"])
@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_prefill(gpu, name, form):
    b = R.batch(name, form)
    res = run(gpu, b)
    ran_as(res, PREFILL_RAN[form], (8, 1), (name, form))
    R.check_bf16(b, res, ATTN_RATIO_BOUND)


def test_prefill_f32(gpu):
    b = R.batch("P1", "plain")
    res = run(gpu, b, precision="f32")
    ran_as(res, "f32", (4, 1), "P1 f32")
    R.check_f32(b, res)


def test_prefill_long_block_table(gpu):
    """129 table entries per sequence: the bf16 prefill kernel keeps the table in a 128-entry LDS array and refuses; the
    8-bit kernel reads it from global memory and runs"""
    with pytest.raises(gpu.NvlError) as e:
        run(gpu, R.batch("P4", "plain"))
    assert e.value.code == -1 and "more than 128 KV blocks" in str(e.value)
    b = R.batch("P4", "kv8")
    res = run(gpu, b)
    ran_as(res, "prefill_kv8", (8, 1), "P4 kv8")
    R.check_bf16(b, res, ATTN_RATIO_BOUND)


@pytest.mark.parametrize("name", list(R.MQ_CASES))
def test_verify_pass(gpu, name):
    b = R.batch(name, "plain")
    res = gpu.ops.attention_batch(b["q"], b["k_pool"], b["v_pool"], b["table"], b["seq_len"], b["seq_pos"], b["nH"], form="mq")
    ran_as(res, "decode_mq", b["expect"], name)
    R.check_bf16(b, res, ATTN_RATIO_BOUND)


@pytest.mark.parametrize("name", R.CENSUS_CASES)
def test_census(gpu, name):
    decode = name in R.DECODE_CASES
    for form in (["plain", "fused", "kv8"] if decode else ["plain", "kv8"]):
        b = R.batch(name, form, census=True)
        res = run(gpu, b)
        ran_as(res, RAN[form] if decode else PREFILL_RAN[form], b["expect"] or (8, 1), (name, form))
        R.check_census(b, res)
        if form == "fused":
            R.check_append(b, res)


def test_refusals(gpu):
    """what the paged front end refuses, and any table entry outside the pool, before a kernel sees it"""
    b = R.batch("D1", "plain")

    def call(**over):
        a = dict(q=b["q"], k_pool=b["k_pool"], v_pool=b["v_pool"], block_table=b["table"], seq_len=b["seq_len"], seq_pos=b["seq_pos"],
                 nH=b["nH"])
        a.update(over)
        with pytest.raises(gpu.NvlError) as e:
            gpu.ops.attention_batch(**a)
        return e.value.code

    bad = np.array(b["table"])
    bad[2, 1] = b["k_pool"].shape[0]
    assert call(block_table=bad) == -1
    bad[2, 1] = -1
    assert call(block_table=bad) == -1
    assert call(seq_pos=[0, -1, 64]) == -1
    assert call(seq_pos=[0, 63, 128], max_seq=256) == -1           # the table covers 128 keys
    assert call(max_seq=64) == -2                                  # NVL_ERR_POSITION
    assert call(form="kv8", k_scale=0.0) == -1
    assert call(form="fused", precision="f32", q=np.zeros((3, 12 * 64), np.float32)) == -1
