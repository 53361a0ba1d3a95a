"""tests/mamba_reference.py checked against itself, without a GPU: the chunked (SSD) emulation with its roundings off is
the sequential float64 recurrence, and with them on it is a finite, small distance away — the distance the GPU op tests
(tests/test_mamba_ops_gpu.py) hold the MFMA scan to."""
import numpy as np
import pytest

import mamba_reference as R

LENS, POS, SLOTS = (200, 1, 15, 64, 65, 129), (0, 7, 0, 100, 0, 40), (5, 0, 7, 2, 6, 3)


def _case(hd, ss, ng, seed, null_params=False):
    g = R.Geom(4, hd, ss, ng, 4)
    rng = np.random.default_rng(seed)
    inp = R.make_inputs(g, LENS, rng, null_params)
    state = rng.standard_normal((8, g.nh, g.hd, g.ss))
    xbc, delta, _ = R.conv_softplus(g, inp["proj"], LENS, POS, SLOTS, inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    return g, inp, state, xbc, delta


@pytest.mark.parametrize("hd,ss,ng", [(32, 32, 1), (64, 64, 2), (32, 128, 4)])
@pytest.mark.parametrize("null_params", [False, True])
def test_unrounded_ssd_form_is_the_sequential_recurrence(hd, ss, ng, null_params):
    g, inp, state, xbc, delta = _case(hd, ss, ng, 3, null_params)
    y_a, s_a = R.scan(g, xbc, delta, LENS, POS, SLOTS, state, inp["a_log"], inp["D"])
    y_b, s_b = R.ssd_scan(g, xbc, delta, LENS, POS, SLOTS, state, inp["a_log"], inp["D"], rounding=False)
    assert np.isfinite(y_a).all() and np.isfinite(y_b).all()
    assert R.head_errors(g, y_b, y_a, LENS).max() <= 1e-10
    assert R.state_head_errors(s_b, s_a, SLOTS).max() <= 1e-10
    unused = [s for s in range(8) if s not in SLOTS]
    assert np.array_equal(s_a[unused], state[unused]) and np.array_equal(s_b[unused], state[unused])
    # a sequence at position 0 ignores what its slot held
    zeroed = state.copy()
    zeroed[[SLOTS[i] for i, p in enumerate(POS) if p == 0]] = 0.0
    y_z, s_z = R.scan(g, xbc, delta, LENS, POS, SLOTS, zeroed, inp["a_log"], inp["D"])
    assert np.array_equal(y_z, y_a) and np.array_equal(s_z[list(SLOTS)], s_a[list(SLOTS)])


@pytest.mark.parametrize("hd,ss,ng", [(32, 32, 1), (64, 64, 2), (32, 128, 4), (64, 128, 1)])
def test_rounded_ssd_form_stays_within_the_bf16_bound(hd, ss, ng):
    g, inp, state, xbc, delta = _case(hd, ss, ng, 4)
    y_a, s_a = R.scan(g, xbc, delta, LENS, POS, SLOTS, state, inp["a_log"], inp["D"])
    y_b, s_b = R.ssd_scan(g, xbc, delta, LENS, POS, SLOTS, state, inp["a_log"], inp["D"], rounding=True)
    ey, es = R.head_errors(g, y_b, y_a, LENS), R.state_head_errors(s_b, s_a, SLOTS)
    print("y", ey.min(), ey.max(), "state", es.min(), es.max())
    assert np.isfinite(y_b).all() and np.isfinite(s_b).all()
    assert 0 < ey.max() <= 1.5e-2 and 0 < es.max() <= 1.5e-2              # the device's hard bound leaves room for it
    assert (R.head_rms(g, y_b, y_a) > 0).all() and (R.head_rms(g, s_b[list(SLOTS)], s_a[list(SLOTS)]) > 0).all()


def test_regimes_are_what_the_op_tests_say():
    g = R.Geom(4, 32, 32, 1, 4)
    inp = R.make_inputs(g, (600,), np.random.default_rng(0))
    _, delta, _ = R.conv_softplus(g, inp["proj"], (600,), (0,), (0,), inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    adt = -np.exp(inp["a_log"].astype(np.float64)) * delta
    for h, name in enumerate(inp["regimes"]):
        assert abs(adt[:, h].mean() / R.REGIMES[name] - 1) < 0.1, (h, name)
        assert 0.2 < delta[:, h].std() / delta[:, h].mean() < 0.4          # about +-30 %
    assert 0.7 < np.exp(adt[:64, 0].sum()) < 0.82                           # slow: about 0.76 carried per chunk
    assert np.cumsum(adt[:64, 2]).min() < -400                              # fast: s_cum near -500 inside a chunk
    assert inp["D"][-1] == 0.0


@pytest.mark.parametrize("K,chunks", [(4, (64, 64, 2, 1, 19)), (8, (3, 2, 9)), (1, (5, 6)), (2, (1, 1, 3))])
def test_chained_conv_of_the_reference_equals_one_shot(K, chunks):
    g = R.Geom(10, 32, 32, 1, K)
    n = sum(chunks)
    inp = R.make_inputs(g, (n,), np.random.default_rng(K))
    one, _, _ = R.conv_softplus(g, inp["proj"], (n,), (0,), (1,), inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    tail = np.random.default_rng(1).standard_normal((2, K - 1, g.conv_dim))
    raw = inp["proj"][:, g.EH:g.EH + g.conv_dim].astype(np.float64)
    pos = 0
    for i, c in enumerate(chunks):
        got, _, tail = R.conv_softplus(g, inp["proj"][pos:pos + c], (c,), (pos,), (1,), inp["conv_w"], inp["conv_b"], inp["dt_bias"],
                                       tail=tail, chain=1 if i == 0 else 2)
        pos += c
        assert np.abs(got - one[pos - c:pos]).max() <= 1e-12
        want_tail = np.concatenate([np.zeros((K - 1, g.conv_dim)), raw[:pos]])[-(K - 1):] if K > 1 else raw[:0]
        assert np.array_equal(tail[1], want_tail)
    # naive statement of the convolution at one token
    t, c = n - 1, 7
    s = sum(raw[t - (K - 1) + k, c] * float(inp["conv_w"][c, k]) for k in range(K) if t - (K - 1) + k >= 0) + float(inp["conv_b"][c])
    assert abs(one[t, c] - s / (1 + np.exp(-s))) <= 1e-12
