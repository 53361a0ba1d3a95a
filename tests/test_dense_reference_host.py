"""tests/dense_reference.py on the CPU, no GPU: the builders give what they promise (the exact family really is exact),
a stand-in device made of the emulation passes every check of tests/test_dense_ops_gpu.py under the case's own ran
literals, and each check fails under the mutation it is aimed at — the gaps of the model-level suite listed in
test_dense_ops_gpu.py's docstring, one mutation each:
  slice_dropped               one K slice missing from a pending sum            -> x1 ratio          (gap 3)
  bias_every_slice            the bias in every slice, not in slice 0 alone     -> x1 ratio          (gap 3)
  alpha_on_x                  alpha x + product instead of x + alpha product    -> x1 ratio          (gap 5)
  tile_missing                one x^2 tile lost at H = 2048                     -> partial bound     (gap 1)
  eps_left_out                rstd without eps                                  -> h ratio on the rows whose mean(x^2) ~ eps
  normalised_before_rounding  bf16(x w rstd) where bf16(x w) belongs            -> xn_raw bit for bit
  rows_15_16_swapped          two rows across a 16-row tile edge                -> x1 exact          (gap 4)
  second_group_first_rstd     rows 64.. scaled with rows 0..'s rstd             -> h ratio           (gap 2)
  gate_up_swapped             silu(u) g                                         -> h ratio
  multiplier_skipped          a pending add summed without the multiplier       -> x2 ratio          (gap 5)"""
import numpy as np
import pytest

import dense_reference as R

BOUND = 1.6          # what the issue allows a case before it counts as a finding; the stand-in device sits at 1.0

SMALL = [n for n, c in R.CASES.items() if c["shape"][1] <= 2048 and c["shape"][0] <= 130]


@pytest.mark.parametrize("name", SMALL)
def test_emulated_device_passes_every_check(name):
    c = R.CASES[name]
    for fam in c["families"]:
        inp = R.make_inputs(name, fam)
        fig = R.check_stages(inp, R.emulated_device(inp, c["ran"]), BOUND, f"{name} {fam}")
        assert all(abs(r.max() - 1.0) < 0.05 for r in fig.values())


AIMED = [("slice_dropped", "gpt2-M17", "random"), ("bias_every_slice", "gpt2-M17", "random"),
         ("alpha_on_x", "llama-M5-alpha0.22", "random"), ("tile_missing", "h2048-M8", "random"),
         ("eps_left_out", "llama-M5", "random"), ("normalised_before_rounding", "llama-M5", "random"),
         ("rows_15_16_swapped", "llama-M17", "exact"), ("second_group_first_rstd", "llama-M100", "random"),
         ("gate_up_swapped", "llama-M5", "random"), ("multiplier_skipped", "llama-M5-alpha0.22-key3=0", "random")]


@pytest.mark.parametrize("mut,name,fam", AIMED, ids=[a[0] for a in AIMED])
def test_each_mutation_fails_its_check(mut, name, fam):
    assert mut in R.MUTATIONS
    c = R.CASES[name]
    inp = R.make_inputs(name, fam)
    R.check_stages(inp, R.emulated_device(inp, c["ran"]), BOUND, name)                 # sound without the mutation
    with pytest.raises(AssertionError):
        R.check_stages(inp, R.emulated_device(inp, c["ran"], mut), BOUND, f"{name} {mut}")


def test_every_mutation_is_aimed_at():
    assert sorted(a[0] for a in AIMED) == sorted(R.MUTATIONS)


def test_h_f32_term():
    """the float32 evaluation of rstd * acc -> silu(g) * u against float64 over the exact cases: H_F32_REL covers it"""
    worst = 0.0
    for name in ("llama-M5", "llama-M40-key3=2", "llama-M100", "llama-M5-alpha0.5"):
        c = R.CASES[name]
        inp = R.make_inputs(name, "exact")
        dev = R.emulated_device(inp, c["ran"])
        H, F = inp["x"].shape[1], inp["w2"].shape[1]
        acc = (dev["op1"].astype(np.float64) @ inp["w1"].astype(np.float64).T).astype(np.float32)
        s = dev["rs1"].astype(np.float32).sum(1, dtype=np.float32)
        rstd = (np.float32(1.0) / np.sqrt(s * np.float32(1.0 / H) + np.float32(inp["norm_eps"]))).astype(np.float32)
        g, u = acc[:, :F] * rstd[:, None], acc[:, F:] * rstd[:, None]
        h32 = (g / (np.float32(1.0) + np.exp(-g))) * u
        assert h32.dtype == np.float32
        h64 = R.ffn_h(dev["op1"], dev["rs1"], inp, False)
        nz = h64 != 0
        worst = max(worst, float((np.abs(h32.astype(np.float64) - h64)[nz] / np.abs(h64[nz])).max()))
    print(f"float32 evaluation of h: largest relative error {worst:.3e} (H_F32_REL {R.H_F32_REL:.1e})")
    assert worst <= R.H_F32_REL


@pytest.mark.parametrize("M", [1, 16, 40])
def test_moe_chain_stand_in_and_mutations(M):
    """the MoE chain's checks pass on the emulation and fail when the router or the expert up projection forgets the
    deferred scale, or reads the next row's partials (M > 1)"""
    _, _, form, ran = next(c for c in R.MOE_CASES if c[0] == M)
    inp = R.moe_inputs(M)
    fig = R.check_moe_chain(inp, R.emulated_moe_device(inp, ran, form), BOUND, f"moe M={M}")
    assert all(abs(r.max() - 1.0) < 0.05 for r in fig.values())
    for mut in R.MOE_MUTATIONS:
        if mut == "neighbour_rstd" and M == 1:
            continue
        with pytest.raises(AssertionError):
            R.check_moe_chain(inp, R.emulated_moe_device(inp, ran, form, mut), BOUND, f"moe M={M} {mut}")
