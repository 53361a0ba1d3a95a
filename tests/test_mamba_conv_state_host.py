"""The carried Mamba2 convolution window, the parts that need no GPU: the float64 reference of the
contract against the one-shot convolution, the ABI additions, and the refusals that are answered before a device is
touched.  (The setter's refusals that need a created model — called after nvl_finalize, an unknown mode, a model without
Mamba2 layers — are in test_mamba_conv_state_gpu.py: nvl_create itself needs a device.)"""
import ctypes as C
import re

import numpy as np
import pytest

import mamba_conv_state_reference as CR
import mamba_reference as R

SYMBOLS = ("nvl_set_mamba_conv_state", "nvl_get_mamba_conv_state")


@pytest.mark.parametrize("K", [2, 3, 4, 8])
@pytest.mark.parametrize("split", [(1, 2, 1, 30), (2, 1, 1, 1, 7, 22), (1, 1, 1, 1, 1, 1, 1, 1, 1, 25), (34,), (2, 32), (17, 1, 16)])
def test_reference_split_any_way_equals_the_one_shot_convolution(K, split):
    """The contract's float64 statement, fed a sequence in pieces (pieces of 1 and 2 tokens at the start: shorter than
    the window), equals mamba_reference.conv_softplus(chain=0) over the whole sequence, and keeps the last K-1 raw rows
    (zeros before position 0) after every piece."""
    g = R.Geom(2, 32, 32, 1, K)
    n = sum(split)
    rng = np.random.default_rng(100 * K + len(split))
    inp = R.make_inputs(g, (n,), rng)
    want_x, want_d, _ = R.conv_softplus(g, inp["proj"], (n,), (0,), (0,), inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    raw = np.concatenate([np.zeros((K - 1, g.conv_dim)), inp["proj"][:, g.EH:g.EH + g.conv_dim].astype(np.float64)])
    ref = CR.Carried(g, inp["conv_w"], inp["conv_b"], inp["dt_bias"])
    p, xs, ds = 0, [], []
    for c in split:
        x, d, tails = ref.call(inp["proj"][p:p + c], ["s"], (c,), (p,))
        p += c
        assert np.array_equal(tails["s"], raw[p:p + K - 1]), p
        xs.append(x)
        ds.append(d)
    assert np.abs(np.concatenate(xs) - want_x).max() <= 1e-14 * np.abs(want_x).max()
    assert np.array_equal(np.concatenate(ds), want_d)


def test_reference_restart_at_position_zero_forgets_the_history():
    g = R.Geom(2, 32, 32, 1, 4)
    inp = R.make_inputs(g, (9,), np.random.default_rng(3))
    ref = CR.Carried(g, inp["conv_w"], inp["conv_b"])
    ref.call(inp["proj"][:5], ["s"], (5,), (0,))
    x, _, tails = ref.call(inp["proj"][5:], ["s"], (4,), (0,))
    fresh = CR.Carried(g, inp["conv_w"], inp["conv_b"]).call(inp["proj"][5:], ["t"], (4,), (0,))
    assert np.array_equal(x, fresh[0]) and np.array_equal(tails["s"], fresh[2]["t"])


def test_header_and_exports(pkg):
    text = pkg._lib.HEADER.read_text()
    L = pkg.lib()
    for name in SYMBOLS:
        assert name in pkg.declared_symbols(), name
        assert hasattr(L, name), name
    assert re.search(r"NVL_MAMBA_CONV_PER_CALL\s*=\s*0", text) and re.search(r"NVL_MAMBA_CONV_CARRIED\s*=\s*1", text)
    assert "mamba2.go:181-254" in text and "mamba2.go:27,181-254,356" in text
    assert "key 39" in text                                   # the tuning key is documented with the others
    assert L.nvl_abi_version() == 3
    assert pkg._lib.MAMBA_CONV_STATE == {"per_call": 0, "carried": 1}
    assert callable(pkg.HipTransformerModel.get_mamba_conv_state)


def test_null_model_is_refused_before_the_device(pkg):
    L = pkg.lib()
    for mode in (0, 1, 7):
        assert L.nvl_set_mamba_conv_state(None, mode) == -1    # NVL_ERR_INVALID, not NVL_ERR_NO_DEVICE (-8)
    out = np.zeros(4, np.float32)
    assert L.nvl_get_mamba_conv_state(None, 0, 0, out.ctypes.data_as(C.c_void_p)) == -1


def test_python_option_is_checked(pkg):
    cfg = pkg.synth.tiny_config("granite_hybrid")
    for bad in ("x", "", "CARRIED", None, 1):
        with pytest.raises(ValueError):
            pkg.HipTransformerModel(cfg, None, mamba_conv_state=bad)


def test_op_chain_is_checked_before_the_device(pkg):
    """chain = 4 does not exist, and chain = 3 needs a tail when K > 1: NVL_ERR_INVALID before the device probe."""
    g = R.Geom(4, 32, 32, 1, 4)
    lens = (1, 1)
    inp = R.make_inputs(g, lens, np.random.default_rng(0))
    state = np.zeros((2, g.nh, g.hd, g.ss), np.float32)
    tail = np.zeros((2, g.K - 1, g.conv_dim), np.float32)

    def call(**kw):
        return pkg.ops.mamba_mixer(inp["proj"], lens, (0, 0), (0, 1), state, g.nh, g.hd, g.ss, g.ng, g.K, inp["conv_w"],
                                   precision="f32", **kw)
    for kw in (dict(chain=4, tail=tail), dict(chain=-1, tail=tail), dict(chain=3), dict(chain=2, tail=tail)):
        with pytest.raises(pkg.NvlError) as e:
            call(**kw)
        assert e.value.code == -1, (kw, e.value)
