"""The weight-format setters through the C ABI against tests/wf_state_reference.py: seeded random walks over all eight setters on
four kinds of model, every return code compared with the restatement's; then one 2-D upload (and one expert upload on the MoE
model), after which the setters whose window that closes return NVL_ERR_STATE while the others still follow their own rule
(nvl_set_act_dtype until nvl_finalize; the expert setters of a model that never uploads an expert).  No kernel runs but the
uploads' own."""
import numpy as np
import pytest

import wf_state_reference as R

pytestmark = pytest.mark.gpu

N_CALLS = 300
KINDS = {     # name -> (family, constructor keywords, f32, tp)
    "llama_bf16": ("llama", dict(precision="bf16"), False, False),
    "moe_bf16": ("granite_moe", dict(precision="bf16"), False, False),
    "llama_f32": ("llama", dict(precision="f32"), True, False),
    "llama_tp_forced": ("llama", dict(precision="bf16", tp_force_single=True), False, True),
}


def call(hm, c):
    name, value, g = c
    fn = getattr(hm.lib, name)
    return fn(hm.h, value, g) if name == "nvl_set_gq_weight_dtype" else fn(hm.h, value)


def walk(hm, facts, state, rng, n):
    """n random calls; -> the state the restatement ends in"""
    all_calls = R.calls()
    for i in range(n):
        c = all_calls[int(rng.integers(len(all_calls)))]
        want, state = R.step(state, facts, c)
        got = call(hm, c)
        assert got == want, (i, c, got, want, state, facts)
    return state


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_walk(gpu, kind, seed):
    family, kw, f32, tp = KINDS[kind]
    cfg = gpu.synth.tiny_config(family)
    w = gpu.synth.make_weights(cfg, seed=1, scale=0.05)
    moe = bool(cfg["use_moe"])
    facts = R.Facts(f32=f32, tp=tp, moe=moe, H=cfg["hidden"], F=cfg["ffn_dim"], finalized=False, w2d_uploaded=False,
                    expert_uploaded=False)
    rng = np.random.default_rng(1000 * seed + sorted(KINDS).index(kind))
    hm = gpu.HipTransformerModel(cfg, None, max_seqs=2, max_batch_tokens=64, **kw)
    try:
        state = walk(hm, facts, R.START, rng, N_CALLS)
        hm.upload("wo", 0, w[("wo", 0)])
        facts = facts._replace(w2d_uploaded=True)
        if moe:
            hm.upload("moe_in", 0, w[("moe_in", 0)])
            facts = facts._replace(expert_uploaded=True)
        for c in R.calls():
            want, state = R.step(state, facts, c)
            got = call(hm, c)
            assert got == want, (c, got, want, state, facts)
            name = c[0]
            if name != "nvl_set_act_dtype" and (moe or "expert" not in name):
                assert got == R.STATE, (c, got)
        walk(hm, facts, state, rng, 40)      # nvl_set_act_dtype (and a dense model's expert setters) still move
    finally:
        hm.close()
