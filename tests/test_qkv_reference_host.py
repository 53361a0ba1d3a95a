"""tests/qkv_reference.py on the CPU, no GPU: the float64 statement agrees with bf16_emulator.layer's q / k / v, the builders
give what they promise, the op refuses bad arguments before it touches a device, a stand-in device made of the reference
passes every check of tests/test_qkv_ops_gpu.py under each case's own ran literals, and each check fails under the mutation
it is aimed at:
  rope_position_minus_one       RoPE with the row before's angle                 -> Q / K of a store form
  rope_skipped_on_k             K stored unrotated                               -> K of the epilogue form
  rope_applied_to_v             V rotated like K                                 -> V bit for bit
  partner_at_32_in_hd128        the hd-64 partner distance inside an hd-128 head -> Q / K of the hd-128 epilogue
  cos_sin_halves_swapped        each half rotated with the other half's formula  -> Q / K
  k_row_at_pos_plus_one         K one row down (V in place)                      -> untouched sentinels, exact K
  other_sequences_table_row     tok_tbl of the next sequence                     -> untouched sentinels
  kv_heads_swapped              K / V heads in reverse order                     -> exact K / V
  bias_omitted                  no bias                                          -> Q / K / V of the epilogue form
  bias_shifted_one_head         head h adds head h - 1's bias                    -> qkv
  last_ragged_tile_not_written  the last m-tile's rows missing                   -> NaN in Q
  padded_row_written            row m = M stored                                 -> the q buffer's NaN rows
  q_hd64_row_stride_in_hd128    Q rows nH * 64 apart in an hd-128 case            -> exact Q
  v_truncated                   V cut to bf16 instead of rounded to nearest even -> V bit for bit"""
import numpy as np
import pytest

import bf16_emulator as E
import qkv_reference as R
from attention_reference import bf16, bf16_ulp_distance

BOUND = 1.6          # the operand's rms ratio a case may show before it counts as a finding; the stand-in device sits at 1.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulated_device_passes_every_check(name):
    inp = R.make_inputs(name)
    fig = R.check(inp, R.emulated_device(inp, R.CASES[name]["ran"]), BOUND, name)
    assert all(v <= 1.0 + 1e-9 for v in fig.values()), fig


def test_case_table_reaches_what_it_promises():
    """every EPI_QKV instance, both rope_kv_kernel types, the 8-bit writer and both embedding kernels have a case; every
    batch crosses a block boundary inside an m-tile, starts one sequence mid-block and names a poison block"""
    rans = [c["ran"] for c in R.CASES.values()]
    assert {r["gemm"] for r in rans if r["form"] == "epilogue"} == set(R.EPILOGUE_INSTANCES)
    assert {r["form"] for r in rans} == {"f32_store_rope", "decode_store_rope", "groups_store_rope", "epilogue", "store_rope_kv8", "store_only"}
    assert {r["embed"] for r in rans} == {None, "bf16", "f32"}
    for batch in (R.B131, R.B259, R.B37):
        seq, pos = R.token_rows(*batch)
        assert any(p % R.BLOCK for p in batch[1]) and any((np.diff(pos // R.BLOCK) == 1) & (np.diff(seq) == 0))
    assert sum(R.B131[0]) == 131 and 131 % 128 == 3 and sum(R.B259[0]) == 259 and 259 % 256 == 3
    inp = R.make_inputs("epi-tile1-4x2-M131")
    t = inp["table"]
    used = np.concatenate([t[0, :2], t[1, :3], t[2, :2]])               # 70, 131 and 110 positions
    assert (t == inp["poison"]).sum() == t.size - 7 and inp["poison"] not in used and len(set(used)) == 7
    assert list(used) != sorted(used)
    for pool, s in ((inp["k_pool"], 1.0), (inp["v_pool"], 1.0)):
        flat = pool.ravel()
        assert np.isfinite(flat).all() and (flat[1:] != flat[:-1]).all() and np.array_equal(bf16(flat), flat.astype(np.float64))
    inp8 = R.make_inputs("kv8-M131")
    assert np.array_equal(R.kv8_dequantized(inp8["v_pool"], 0.25), inp8["v_pool"].astype(np.float64))
    ex = R.make_inputs("epi-tile3-3x1-M131-exact")
    p64, S = R.projection64(ex, ex["x"])
    assert np.array_equal(p64, np.round(p64)) and S.max() <= 128 and np.array_equal(bf16(p64), p64)


def test_reference_agrees_with_the_bf16_emulator():
    """one prompt from position 0, Llama-shaped: bf16_emulator.layer's xn / q / k / v (float64 with the same roundings, its own
    tables and matrix products) against the stand-in device's operand, Q buffer and pools — at most one bf16 step apart
    (the two sum in different orders), and on all but 1e-3 of the elements equal"""
    name = "store-decode-llama-M37"
    inp = R.make_inputs(name)
    dev = R.emulated_device(inp, dict(R.CASES[name]["ran"], form="epilogue"))      # (no fp32 round trip of the projection)
    nH, nKV, hd, M = inp["nH"], inp["nKV"], inp["hd"], inp["M"]
    w = bf16(inp["w_qkv"])
    weights = {("attn_norm_w", 0): inp["norm_w"].astype(np.float64), ("wq", 0): w[:nH * hd].T, ("wk", 0): w[nH * hd:(nH + nKV) * hd].T,
               ("wv", 0): w[(nH + nKV) * hd:].T, ("wo", 0): np.zeros((nH * hd, inp["K"])), ("ffn_norm_w", 0): np.ones(inp["K"]),
               ("w1", 0): np.zeros((inp["K"], 128)), ("w2", 0): np.zeros((64, inp["K"]))}
    cfg = dict(num_heads=nH, num_kv_heads=nKV, head_dim=hd, ffn_dim=64, norm_eps=1e-5, rope_base=inp["rope"])
    tap = {}
    E.layer(inp["x"].astype(np.float64), weights, 0, cfg, {"xn", "q", "k", "v"}, tap)
    got = dict(xn=dev["op"], q=dev["q"][:M].reshape(M, nH, hd), k=R.gathered(inp, dev["k_pool"]), v=R.gathered(inp, dev["v_pool"]))
    for what in ("xn", "q", "k", "v"):
        d = bf16_ulp_distance(got[what], tap[what].astype(np.float32))
        print(f"{what}: {int((d > 0).sum())} of {d.size} elements differ, by at most {int(d.max())} step(s)")
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3, what


STORE_CASES = [n for n, c in R.CASES.items() if c["ran"]["form"] in ("decode_store_rope", "groups_store_rope") and c["rope"]]


def test_float32_rotation_rarely_leaves_the_rounded_float64_value():
    """the share of Q / K elements on which a float32 evaluation of x1 c - x2 s / x2 c + x1 s, rounded to bf16, differs from
    bf16 of the float64 value, over the store-form cases with RoPE: below 1e-4, a tenth of MISMATCH_CAP"""
    worst = 0.0
    for name in STORE_CASES:
        inp = R.make_inputs(name)
        dev = R.emulated_device(inp, R.CASES[name]["ran"])
        _, pos = R.token_rows(inp["seq_len"], inp["seq_pos"])
        cos, sin = (t[pos].astype(np.float32)[:, None, :] for t in R.rope_tables(inp["rope"], inp["max_seq"], inp["hd"]))
        h = inp["hd"] // 2
        diff = total = 0
        for t in R.heads_of(inp, dev["qkv"])[:2]:
            x1, x2 = t[..., :h], t[..., h:]
            y32 = np.concatenate([x1 * cos[..., :h] + (-x2) * sin[..., :h], x2 * cos[..., h:] + x1 * sin[..., h:]], -1)
            assert y32.dtype == np.float32
            diff += int((bf16(y32) != bf16(R.rotate(inp, t)[0].astype(np.float32))).sum())
            total += y32.size
        print(f"{name}: {diff} of {total}")
        worst = max(worst, diff / total)
    assert len(STORE_CASES) >= 6 and worst < 1e-4, worst


AIMED = [("rope_position_minus_one", "store-decode-4x2-M37"), ("rope_skipped_on_k", "epi-tile1-4x2-M131"),
         ("rope_applied_to_v", "store-groups-4x2-M131"), ("partner_at_32_in_hd128", "epi-hd128-4x2-M259"),
         ("cos_sin_halves_swapped", "epi-tile2-4x2-M131"), ("k_row_at_pos_plus_one", "store-groups-M131-exact"),
         ("other_sequences_table_row", "epi-tile3-3x1-M131-exact"), ("kv_heads_swapped", "epi-pingpong-4x2-M131-exact"),
         ("bias_omitted", "epi-tile1-4x2-M259"), ("bias_shifted_one_head", "store-gpt2-M131"),
         ("last_ragged_tile_not_written", "epi-tile1-3x1-M131"), ("padded_row_written", "epi-tile3-4x2-M259"),
         ("q_hd64_row_stride_in_hd128", "epi-hd128-3x1-M259-exact"), ("v_truncated", "store-decode-3x1-M37"),
         ("v_truncated", "epi-tile2-3x1-M131"), ("rope_position_minus_one", "kv8-M131"), ("kv_heads_swapped", "kv8-M37"),
         ("k_row_at_pos_plus_one", "f32-M131"), ("bias_omitted", "f32-M131-3x1-gpt2")]


@pytest.mark.parametrize("mut,name", AIMED, ids=[f"{m}-{n}" for m, n in AIMED])
def test_each_mutation_fails_its_check(mut, name):
    assert mut in R.MUTATIONS
    inp = R.make_inputs(name)
    ran = R.CASES[name]["ran"]
    R.check(inp, R.emulated_device(inp, ran), BOUND, name)                             # sound without the mutation
    with pytest.raises(AssertionError):
        R.check(inp, R.emulated_device(inp, ran, mut), BOUND, f"{name} {mut}")


def test_every_mutation_is_aimed_at():
    assert sorted({a[0] for a in AIMED}) == sorted(R.MUTATIONS)


def test_qkv_stages_refuses_bad_arguments_before_touching_a_device(pkg):
    """nvl_op_qkv_stages checks what the paged front end checks, every table entry and every token id before the device
    probe (NVL_ERR_INVALID / NVL_ERR_POSITION, not NVL_ERR_NO_DEVICE, on a machine without a GPU)"""
    inp = R.make_inputs("store-decode-4x2-M37")
    ok = R.op_kwargs(inp)
    bad_table = inp["table"].copy()
    bad_table[1, -1] = inp["n_blocks"]                          # an entry no position reaches
    neg_table = inp["table"].copy()
    neg_table[0, 0] = -1
    z = lambda *s: np.zeros(s, np.float32)
    emb = dict(tokens=np.zeros(37, np.int32), tok_pos=np.zeros(37, np.int32), emb=z(10, 192), x=None)
    for over, code in ((dict(block_table=bad_table), -1), (dict(block_table=neg_table), -1), (dict(seq_pos=(0, -1, 50)), -1),
                       (dict(max_seq=100), -2), (dict(seq_pos=(0, 130, 250), max_seq=1024), -1),               # beyond max_seq; beyond the table
                       (dict(seq_len=(20, 0, 17)), -1), (dict(kv8=True, precision="f32"), -1), (dict(kv8=True, v_scale=0.0), -1),
                       (dict(kv8=True, k_scale=float("inf")), -1), (dict(rope_base=-1.0), -1), (dict(rope_base=float("nan")), -1),
                       (dict(norm="layer"), -1), (dict(norm_eps=-1.0), -1),
                       (dict(w_qkv=z(512, 96), x=z(37, 96), norm_w=z(96)), -1),                   # hidden % 64
                       (dict(emb, tokens=np.full(37, 10, np.int32)), -1), (dict(emb, tokens=np.full(37, -1, np.int32)), -1),
                       (dict(emb, tok_pos=np.full(37, -1, np.int32)), -1), (dict(emb, norm_w=None), -1)):
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.qkv_stages(**{**ok, **over})
        assert e.value.code == code, (over, e.value)
    pools96 = z(inp["n_blocks"], 2, 64, 96)
    with pytest.raises(pkg.NvlError) as e:                                                        # head_dim 96
        pkg.ops.qkv_stages(**{**ok, "k_pool": pools96, "v_pool": pools96, "w_qkv": z(8 * 96, 192), "b_qkv": None})
    assert e.value.code == -1
    pools32 = z(inp["n_blocks"] * 2, 2, 32, 64)
    with pytest.raises(pkg.NvlError) as e:                                                        # block_size % 64
        pkg.ops.qkv_stages(**{**ok, "k_pool": pools32, "v_pool": pools32})
    assert e.value.code == -1
    with pytest.raises(ValueError):
        pkg.ops.qkv_stages(**{**ok, "b_qkv": z(511)})
    if pkg.lib().nvl_device_count() == 0:
        with pytest.raises(pkg.NvlError) as e:
            pkg.ops.qkv_stages(**ok)
        assert e.value.code == -8                                                                  # NVL_ERR_NO_DEVICE: the arguments were fine
