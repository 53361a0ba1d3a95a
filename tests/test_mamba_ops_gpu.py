"""csrc/mamba.h stage by stage through nvl_op_mamba_mixer (the model's own dispatch, nvllm.hip mamba_mixer) against the
float64 statement of tests/mamba_reference.py.

Every stage is compared with the reference FED THE DEVICE'S OWN OUTPUT of the stage before — the reference scan runs on
the device's xbc and delta, the reference gate-norm on the device's y — so one stage's error neither masks nor excuses
another's.  Scan errors are taken per (sequence, head), relative to that head's own largest reference value, and the
decay regimes live side by side as heads of one call (slow: A dt = -0.004, 0.77 carried per chunk; mid: -0.2; fast: -8,
s_cum near -500 inside a chunk; the last head has D = 0): a lost carry is 0.3 .. 0.8 on a slow head and invisible on a
fast one, an inclusive / exclusive slip in the decay is 0.25 .. 1.2 on mid and fast heads and 1e-2 on a slow one.

Bounds.  fp32 conv, delta and gate-norm: 1e-5 of the largest value (tests/test_ops_gpu.py's bound for layernorm, SiLU,
softmax).  fp32 scan outputs and states: 1e-4 per head (tests/test_mamba_gpu.py's fp32 bound; a float32 numpy run of the
recurrence is 1.3e-6 from float64 over 600 tokens, the device's worst values are in profiles/mamba_op_tests.txt).  bf16
gate-norm: |got - want| <= 2^-8 |want| + 1e-30, twice one bf16 rounding.  bf16 SSD y and final state: (1) 1.5e-2 per
(sequence, head), the project's bf16 bound; (2) per head, over all tokens of the case, the device's rms error against
the float64 reference is at most SSD_RATIO_BOUND x the rms error of the rounding emulation (mamba_reference.ssd_scan) on
the same inputs.  SSD_RATIO_BOUND = 1.25 x the largest ratio measured on the MI355X (profiles/mamba_op_tests.txt, written
by scripts/mamba_op_figures.py), and never above 2.

The gaps of the model-level suite (tests/test_mamba_gpu.py) and the test here that closes each:
 1. SSD instantiations (64, 32), (64, 64), (32, 128) never ran          -> test_ssd_scan (all six, three forms)
 2. mamba_scan_kernel<16> never ran                                     -> test_sequential_scan[(64, 64)], test_ssd_scan key 0
 3. lane groups SG = 1, 2, 32, 64 (hd 256, 128, 8, 4) never ran         -> test_sequential_scan
 4. second round of the prefix loop (more than 4 chunks) never ran      -> test_ssd_scan key 1: 9 chunks = rounds of 4, 4, 1
 5. chunk-parallel form never entered on a carried state                -> test_ssd_scan key 1: 257 tokens at position 40
                                                                           (+ test_mamba_gpu.py two-call case)
 6. sequence index and slot index never told apart                      -> every test: slots are a permutation, spare
                                                                           slots pre-filled and compared bit for bit
 7. fast synthetic decays hide carry / decay errors                     -> the regimes above, errors per (sequence, head)
 8. NULL parameter paths never ran                                      -> test_null_parameters
 9. conv: K = 3, 4 only, chained tail only through the runner           -> test_conv_softplus, test_chained_conv

What the hard bound (1) found: with a token's own term dt_t (C_t . B_t) u_t inside the bf16 decay matrix, the one-token
sequence (position 7) of the (64, 128) case was at 1.23e-1 on its fast head in both SSD forms (every other (sequence,
head) at most 6.9e-3) — there y = u x (D + dt C.B) = u x (0.943 - 0.998), the carried state having decayed by exp(-7), so
one bf16 rounding of dt C.B was 0.12 of the largest |y| = 0.053; about one random one-token sequence in twenty did this
in the emulation too.  The kernel now keeps that term in fp32 beside the D skip (mamba.h), and the emulation with it.

test_ssd_scan with key 30 = 1 really takes the three-launch form: the dispatch takes it when nh * n_seqs < 128 (here 24),
max_chunks >= 4 (here 9) and the scratch is below 256 MB (here 7 MB at most); the kernel-site statistics count the three
launches as one mamba_scan site, so they cannot tell the forms apart and are not consulted."""
import numpy as np
import pytest

import mamba_reference as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

F32_ELEM, F32_SCAN, BF16_HARD = 1e-5, 1e-4, 1.5e-2
SSD_RATIO_BOUND = 1.25          # 1.25 x the largest measured device / emulation rms ratio, 1.0003 (profiles/mamba_op_tests.txt)

SSD_CASES = [(32, 32, 1), (32, 64, 2), (32, 128, 4), (64, 32, 2), (64, 64, 4), (64, 128, 1)]      # (hd, ss, ng), nh = 4
SSD_LENS, SSD_POS, SSD_SLOTS = (520, 1, 15, 64, 65, 257), (0, 7, 0, 100, 0, 40), (5, 0, 7, 2, 6, 3)
SEQ_CASES = [(32, 32, 4, 1), (32, 64, 4, 2), (64, 64, 4, 4), (64, 128, 4, 1),                       # (hd, ss, nh, ng): PER 4, 8, 16, 32
             (4, 256, 16, 2), (8, 128, 8, 4), (128, 64, 4, 1), (256, 32, 4, 2)]                     # SG 64, 32, 2, 1
SEQ_LENS = {"f32": (37, 1, 150), "bf16": (15, 1, 9)}
SEQ_POS, SEQ_SLOTS = (0, 5, 30), (2, 0, 3)
NULL_LENS, NULL_POS, NULL_SLOTS = (300, 20, 64), (0, 4, 0), (1, 3, 0)


class Tuning:
    """one nvl_set_tuning key for a block, restored afterwards"""
    def __init__(self, gpu, key, value):
        self.lib, self.key, self.value = gpu.lib(), key, value

    def __enter__(self):
        self.old = self.lib.nvl_set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        self.lib.nvl_set_tuning(self.key, self.old)


def run(gpu, g, inp, lens, pos, slots, state, precision, tail=None, chain=0):
    return gpu.ops.mamba_mixer(inp["proj"], lens, pos, slots, state, g.nh, g.hd, g.ss, g.ng, g.K, inp["conv_w"], inp["conv_b"],
                               inp["a_log"], inp["D"], inp["dt_bias"], inp["norm_w"], tail=tail, chain=chain, precision=precision)


def col_err(got, want):
    """per column, relative to the column's largest value (the heads' dt differ by a factor of 40)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want).max(0) / (np.abs(want).max(0) + 1e-300)).max())


def check_conv(g, inp, out, lens, pos, slots, tail=None, chain=0):
    xbc, delta, new_tail = R.conv_softplus(g, inp["proj"], lens, pos, slots, inp["conv_w"], inp["conv_b"], inp["dt_bias"], tail, chain)
    e_x, e_d = rel_err(out["xbc"], xbc), col_err(out["delta"], delta)
    print(f"conv K={g.K} chain={chain}: xbc {e_x:.2e} delta {e_d:.2e}")
    assert np.isfinite(out["xbc"]).all() and np.isfinite(out["delta"]).all()
    assert e_x <= F32_ELEM and e_d <= F32_ELEM
    return new_tail


def check_gate_norm(g, inp, out, precision):
    want = R.gate_norm(g, out["y"], inp["proj"], inp["norm_w"])
    got = out["normed"].astype(np.float64)
    assert np.isfinite(got).all()
    if precision == "f32":
        e = rel_err(got, want)
        print(f"gate-norm f32 EH={g.EH}: {e:.2e}")
        assert e <= F32_ELEM
    else:
        excess = np.abs(got - want) - (2.0 ** -8 * np.abs(want) + 1e-30)
        print(f"gate-norm bf16 EH={g.EH}: worst |err|/|want| {float((np.abs(got - want) / (np.abs(want) + 1e-300)).max()):.2e}")
        assert (excess <= 0).all(), float(excess.max())


def scan_figures(gpu, g, inp, lens, pos, slots, n_slots, precision, seed):
    """One op call on pre-filled states, checked at the conv and gate-norm stages -> the scan stage's figures: per
    (sequence, head) errors of y and state against the float64 scan of the device's xbc / delta, and the pieces of the
    emulation comparison."""
    state = np.random.default_rng(seed).standard_normal((n_slots, g.nh, g.hd, g.ss)).astype(np.float32)
    out = run(gpu, g, inp, lens, pos, slots, state, precision)
    check_conv(g, inp, out, lens, pos, slots)
    y, st = R.scan(g, out["xbc"], out["delta"], lens, pos, slots, state, inp["a_log"], inp["D"])
    assert np.isfinite(out["y"]).all() and np.isfinite(out["state"]).all()
    spare = [s for s in range(state.shape[0]) if s not in slots]
    assert np.array_equal(out["state"][spare], state[spare]), "a slot no sequence uses was written"
    check_gate_norm(g, inp, out, precision)
    return dict(out=out, state_in=state, y_ref=y, st_ref=st, ey=R.head_errors(g, out["y"], y, lens),
                es=R.state_head_errors(out["state"], st, slots))


def ssd_figures(gpu, g, inp, lens, pos, slots, n_slots, key30, seed):
    """scan_figures of a bf16 call under tuning key 30 + per head the device / emulation rms ratios (y, state)."""
    with Tuning(gpu, 30, key30):
        f = scan_figures(gpu, g, inp, lens, pos, slots, n_slots, "bf16", seed)
    out = f["out"]
    y_b, st_b = R.ssd_scan(g, out["xbc"], out["delta"], lens, pos, slots, f["state_in"], inp["a_log"], inp["D"], rounding=True)
    used = list(slots)
    f["ry"] = R.head_rms(g, out["y"], f["y_ref"]) / R.head_rms(g, y_b, f["y_ref"])
    f["rs"] = R.head_rms(g, out["state"][used], f["st_ref"][used]) / R.head_rms(g, st_b[used], f["st_ref"][used])
    return f


def ssd_inputs(hd, ss, ng):
    g = R.Geom(4, hd, ss, ng, 4)
    return g, R.make_inputs(g, SSD_LENS, np.random.default_rng(1000 + hd + ss))


def null_inputs(K=4):
    g = R.Geom(4, 32, 64, 2, K)
    return g, R.make_inputs(g, NULL_LENS, np.random.default_rng(77), null_params=True)


def seq_inputs(hd, ss, nh, ng, precision):
    g = R.Geom(nh, hd, ss, ng, 4)
    return g, R.make_inputs(g, SEQ_LENS[precision], np.random.default_rng(2000 + hd + ss))


def assert_ssd(f, key30, what):
    print(f"{what} key30={key30}: y per (seq, head) max {f['ey'].max():.2e}, state {f['es'].max():.2e}; "
          f"rms ratio to the emulation y {np.round(f['ry'], 3).tolist()} state {np.round(f['rs'], 3).tolist()}")
    if key30 == 0:                                   # the sequential scan: fp32 arithmetic also in the bf16 mode
        assert f["ey"].max() <= F32_SCAN and f["es"].max() <= F32_SCAN
        return
    assert f["ey"].max() <= BF16_HARD, f["ey"]
    assert f["es"].max() <= BF16_HARD, f["es"]
    assert f["ry"].max() <= SSD_RATIO_BOUND and f["rs"].max() <= SSD_RATIO_BOUND, (f["ry"], f["rs"])


@pytest.mark.parametrize("key30", [1, 2, 0])
@pytest.mark.parametrize("hd,ss,ng", SSD_CASES)
def test_ssd_scan(gpu, hd, ss, ng, key30):
    """All six (head_dim, state) instantiations of mamba_ssd_kernel in the chunk-parallel three-launch form (key 30 = 1:
    9 chunks = three rounds of the prefix loop, the last a round of one; a 5-chunk sequence entering on a carried state;
    sequences of 1 and 15 tokens inside the launch), chunk after chunk (2) and on the sequential scan (0)."""
    g, inp = ssd_inputs(hd, ss, ng)
    assert_ssd(ssd_figures(gpu, g, inp, SSD_LENS, SSD_POS, SSD_SLOTS, 8, key30, seed=hd + ss), key30, f"ssd ({hd}, {ss})")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("hd,ss,nh,ng", SEQ_CASES)
def test_sequential_scan(gpu, hd, ss, nh, ng, precision):
    """mamba_scan_kernel in its four PER instantiations and at the lane-group extremes the host accepts; bf16 calls with
    every sequence shorter than 16 tokens take it too.  Fresh and carried sequences mixed, slots permuted."""
    g, inp = seq_inputs(hd, ss, nh, ng, precision)
    f = scan_figures(gpu, g, inp, SEQ_LENS[precision], SEQ_POS, SEQ_SLOTS, 5, precision, seed=hd + ss)
    print(f"scan {precision} ({hd}, {ss}): y per (seq, head) max {f['ey'].max():.2e}, state {f['es'].max():.2e}")
    assert f["ey"].max() <= F32_SCAN and f["es"].max() <= F32_SCAN


@pytest.mark.parametrize("form", ["ssd1", "ssd2", "seq_f32"])
def test_null_parameters(gpu, form):
    """conv_b, a_log, D, dt_bias and norm_w all NULL (no decay at all: A = 0), through both SSD forms and the sequential scan."""
    g, inp = null_inputs()
    if form == "seq_f32":
        f = scan_figures(gpu, g, inp, NULL_LENS, NULL_POS, NULL_SLOTS, 4, "f32", seed=5)
        print(f"null f32: y {f['ey'].max():.2e} state {f['es'].max():.2e}")
        assert f["ey"].max() <= F32_SCAN and f["es"].max() <= F32_SCAN
    else:
        key30 = int(form[-1])
        assert_ssd(ssd_figures(gpu, g, inp, NULL_LENS, NULL_POS, NULL_SLOTS, 4, key30, seed=5), key30, "null")


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_conv_softplus(gpu, K):
    """Every conv width the host accepts at a conv_dim (384) that is no multiple of the 256 threads; raw dt on both sides
    of softplus's x > 20 branch; chain = 0 zero-pads also at seq_pos > 0 and leaves the tails alone."""
    g = R.Geom(10, 32, 32, 1, K)
    lens, pos, slots = (5, 1, 12), (0, 3, 9), (2, 0, 1)
    rng = np.random.default_rng(K)
    inp = R.make_inputs(g, lens, rng)
    M = sum(lens)
    inp["proj"][:, g.EH + g.conv_dim:] = rng.permutation(np.linspace(-30.0, 40.0, M * g.nh)).reshape(M, g.nh).astype(np.float32)
    inp["dt_bias"] = np.zeros(g.nh, np.float32)
    state = rng.standard_normal((3, g.nh, g.hd, g.ss)).astype(np.float32)
    tail = rng.standard_normal((3, K - 1, g.conv_dim)).astype(np.float32)
    out = run(gpu, g, inp, lens, pos, slots, state, "f32", tail=tail)
    assert out["delta"].min() < 1e-9 and out["delta"].max() > 39.0
    check_conv(g, inp, out, lens, pos, slots)                               # the reference call WITHOUT a tail: zero padding
    assert np.array_equal(out["tail"], tail)


@pytest.mark.parametrize("K,chunks", [(4, (64, 64, 2, 1, 19)), (8, (3, 2, 9))])
def test_chained_conv(gpu, K, chunks):
    """A chained prefill (chain 1, then 2) of one sequence gives the one-shot call's xbc rows, keeps exactly the last K-1
    raw rows after every chunk (chunks shorter than the window included) in its own slot only, and — the state carrying
    on — the one-shot call's y."""
    g = R.Geom(10, 32, 32, 1, K)
    n = sum(chunks)
    rng = np.random.default_rng(10 + K)
    inp = R.make_inputs(g, (n,), rng)
    state0 = rng.standard_normal((3, g.nh, g.hd, g.ss)).astype(np.float32)
    tail0 = rng.standard_normal((3, K - 1, g.conv_dim)).astype(np.float32)
    one = run(gpu, g, inp, (n,), (0,), (1,), state0, "f32")
    check_conv(g, inp, one, (n,), (0,), (1,))
    raw = np.concatenate([np.zeros((K - 1, g.conv_dim), np.float32), inp["proj"][:, g.EH:g.EH + g.conv_dim]])
    state, tail, p, parts = state0, tail0, 0, []
    for i, c in enumerate(chunks):
        part = dict(inp, proj=inp["proj"][p:p + c])
        out = run(gpu, g, part, (c,), (p,), (1,), state, "f32", tail=tail, chain=1 if i == 0 else 2)
        check_conv(g, part, out, (c,), (p,), (1,), tail=tail, chain=1 if i == 0 else 2)
        p += c
        assert np.array_equal(out["tail"][1], raw[p:p + K - 1]), f"tail after chunk {i}"
        assert np.array_equal(out["tail"][[0, 2]], tail0[[0, 2]])
        state, tail = out["state"], out["tail"]
        parts.append(out)
    xbc = np.concatenate([o["xbc"] for o in parts])
    assert rel_err(xbc, one["xbc"]) <= F32_ELEM
    y = np.concatenate([o["y"] for o in parts])
    y_ref, st_ref = R.scan(g, xbc, np.concatenate([o["delta"] for o in parts]), (n,), (0,), (1,), state0, inp["a_log"], inp["D"])
    assert R.head_errors(g, y, y_ref, (n,)).max() <= F32_SCAN
    assert R.state_head_errors(state, st_ref, (1,)).max() <= F32_SCAN


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("with_norm_w", [False, True])
@pytest.mark.parametrize("nh,hd", [(2, 32), (10, 32), (16, 64), (17, 64)])         # EH 64, 320, 1024, 1088
def test_gate_norm(gpu, nh, hd, with_norm_w, precision):
    """Widths below, at and just past the 1024 floats one pass of the store loop covers, and no multiple of 256; an
    all-zero y row (the first token of a fresh sequence with u = 0) comes out as zeros, not as 0 / 0."""
    g = R.Geom(nh, hd, 32, 1, 4)
    lens, pos, slots = (3, 5), (0, 2), (1, 0)
    inp = R.make_inputs(g, lens, np.random.default_rng(nh * hd))
    inp["conv_b"] = None
    inp["proj"][0, g.EH:2 * g.EH] = 0.0                                     # u of token 0 = SiLU(0) = 0, its state was reset
    if not with_norm_w:
        inp["norm_w"] = None
    state = np.random.default_rng(1).standard_normal((2, g.nh, g.hd, g.ss)).astype(np.float32)
    out = run(gpu, g, inp, lens, pos, slots, state, precision)
    assert not out["y"][0].any() and out["y"][1].any()
    check_gate_norm(g, inp, out, precision)
    assert not out["normed"][0].any()


def test_refusals(gpu):
    """Geometry the kernels do not cover is an error code before anything is launched."""
    def call(nh=4, hd=32, ss=32, ng=1, K=4, lens=(3,), chain=0):
        g = R.Geom(nh, hd, ss, ng, K)
        inp = R.make_inputs(g, lens, np.random.default_rng(0))
        n = len(lens)
        state = np.zeros((n, nh, hd, ss), np.float32)
        tail = np.zeros((n, K - 1, g.conv_dim), np.float32)
        return run(gpu, g, inp, lens, (0,) * n, tuple(range(n)), state, "f32", tail=tail, chain=chain)
    call()                                                                  # the good call these are variations of
    for bad in (dict(hd=48),                                                # 256 % hd != 0
                dict(nh=16, hd=4, ss=32),                                   # SG = 64 does not divide the state
                dict(ss=96),                                                # PER = 12: no such scan instantiation
                dict(K=9), dict(ng=3),
                dict(lens=(3, 2), chain=1)):                                # a chained prefill is one sequence
        with pytest.raises(gpu.NvlError) as e:
            call(**bad)
        assert e.value.code == -1, bad                                      # NVL_ERR_INVALID
