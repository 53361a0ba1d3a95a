"""Attention at head_dim 256: attn256.h's prefill and decode kernels through ops.attention_batch against
tests/attention_reference.py's float64 statement — its pools, draws and bounds (a) / (b), ATTN_RATIO_BOUND of
tests/test_attention_ops_gpu.py (the contracts are the same: prefill sums the rounded P, decode the unrounded).  The cases are
the hd-64 ones at 256: each the smallest that reaches one thing.  Windowed cases go through test_attention_window_gpu.py's run
and check (the windowed reference).  Figures: profiles/attention_hd256_op_tests.txt."""
import pytest

import attention_reference as R
import test_attention_window_gpu as W
from test_attention_ops_gpu import ATTN_RATIO_BOUND

pytestmark = pytest.mark.gpu

R.ALL_CASES.update({
    "G1": R._c(hd=256, pos=(0, 63, 64)),                               # empty cache, tile edge, fresh block
    "G2": R._c(hd=256, block=256, pos=(1023, 70)),                     # 16 tiles: key split; the short sequence leaves workgroups idle
    "G3": R._c(hd=256, block=256, pos=(1024, 960)),                    # 17 tiles over 16 virtual waves: one wave takes two
    "G4": R._c(hd=256, block=192, pos=(191, 192, 383, 500)),           # a block size that is not a power of two; four waves
    "G5": R._c(hd=256, nH=20, nKV=1, block=256, pos=(1100, 5)),        # two query tiles, the second with 4 heads
    # ragged rows, a 128-row tile boundary, 16 tiles through 2 slots.  The hd-64 case P1 has 5 rows at position 0; at 256 columns
    # R.batch finds no draw for that (its own emulation sits at 0.95 - 1.24 of bound (a) on rows of 1 - 5 keys, HEADROOM is
    # 0.9, 16 draws): 2 rows, as the verify case G9 has them
    "G6": R._c(hd=256, pos=(0, 60, 1000), lens=(2, 70, 1)),
    "G7": R._c(hd=256, nH=71, nKV=1, pos=(30,), lens=(4,)),            # 284 rows: three query tiles, the last ragged
    "G8": R._c(hd=256, block=192, pos=(200,), lens=(40,)),             # a block size that is not a power of two
    "G9": R._c(hd=256, pos=(62, 0, 1030), lens=(4, 2, 4)),             # a verify pass
})
# (case, form, window, precision) -> the kernel that must have run; nsplit > 1 where the keys must have been split
CASES = ([(n, "plain", 0, "bf16", "decode_hd256") for n in ("G1", "G2", "G3", "G4", "G5")] +
         [(n, "plain", 0, "bf16", "prefill_hd256") for n in ("G6", "G7", "G8")] + [("G9", "mq", 0, "bf16", "prefill_hd256")] +
         [("G2", "plain", 100, "bf16", "decode_hd256"), ("G6", "plain", 100, "bf16", "prefill_hd256")] +
         [("G4", "plain", 0, "f32", "f32"), ("G8", "plain", 0, "f32", "f32")])
SPLIT = {"G2", "G3", "G5"}


@pytest.mark.parametrize("name,form,window,precision,ran", CASES)
def test_hd256(gpu, name, form, window, precision, ran):
    b, res = W.run(gpu, name, form, window, precision)
    assert res["ran"] == ran, (name, form, res["ran"])
    if precision == "f32":
        R.check_f32(b, res)
    elif window:
        assert res["nsplit"] == 1, res["nsplit"]          # (the launch shape follows the keys read: 163 at most)
        W.check(b, res, window, f"{name} {form} W={window}")
    else:
        assert (res["nsplit"] > 1) == (name in SPLIT), (name, res["nw"], res["nsplit"])
        R.check_bf16(b, res, ATTN_RATIO_BOUND, tag=form)
