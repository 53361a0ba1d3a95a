"""The weight-format setters of include/nvllm.h (nvl_set_weight_dtype, nvl_set_mx_weight_dtype, nvl_set_gq_weight_dtype, their
expert and head setters, nvl_set_act_dtype) restated as one pure function, setter by setter as the header describes them:

    step(state, facts, call) -> (code, state)

state  (wf, ef, hf, a8): the stored format of the projections, the experts and the LM head, and whether activations are 8-bit.
       A format is BF16, FP8, MXFP4 or int4(g), the group size above the low byte as the library keeps it.
facts  what the rules read of the model: f32, tp (tensor parallel, forced single rank included), moe, H, F (hidden and FFN /
       expert width), and the three "too late" flags finalized, w2d_uploaded, expert_uploaded.
call   (setter name, value, group size); the group size counts for nvl_set_gq_weight_dtype only.

A refused call leaves the state as it was.  Test infrastructure only: the library does not read this file."""
from collections import namedtuple

OK, INVALID, STATE = 0, -1, -7
BF16, FP8, MXFP4, INT4 = 0, 1, 2, 3

State = namedtuple("State", "wf ef hf a8")
Facts = namedtuple("Facts", "f32 tp moe H F finalized w2d_uploaded expert_uploaded")
START = State(BF16, BF16, BF16, False)

SETTERS = ("nvl_set_weight_dtype", "nvl_set_mx_weight_dtype", "nvl_set_gq_weight_dtype", "nvl_set_expert_dtype",
           "nvl_set_mx_expert_dtype", "nvl_set_gq_expert_dtype", "nvl_set_mx_head_dtype", "nvl_set_act_dtype")
GROUPS = (32, 64, 128)


def int4(g):
    return INT4 | (g << 8)


def base(wf):
    return wf & 0xFF


def group(wf):
    return wf >> 8


def step(s, f, call):
    name, value, g = call
    on = value == 1
    late_2d = f.finalized or f.w2d_uploaded
    late_expert = f.finalized or f.expert_uploaded
    known = value in (0, 1)

    if name == "nvl_set_weight_dtype":
        if late_2d:
            return STATE, s
        if not known or (on and (f.f32 or f.tp or s.wf == MXFP4 or base(s.wf) == INT4)):
            return INVALID, s
        if on:
            return OK, s._replace(wf=FP8)
        if s.wf == FP8:                     # 8-bit experts and activations need 8-bit weights: they go with them
            return OK, State(BF16, BF16, s.hf, False)
        return OK, s

    if name == "nvl_set_mx_weight_dtype":
        if late_2d:
            return STATE, s
        if not known or (on and (f.f32 or f.tp or s.wf == FP8 or base(s.wf) == INT4)):
            return INVALID, s
        if not on and (s.ef == MXFP4 or s.hf == MXFP4):     # MXFP4 experts / an MXFP4 head hold the MXFP4 weights
            return INVALID, s
        if on:
            return OK, s._replace(wf=MXFP4)
        return OK, s._replace(wf=BF16) if s.wf == MXFP4 else s

    if name == "nvl_set_gq_weight_dtype":
        if late_2d:
            return STATE, s
        if not known or g not in GROUPS:                    # (the group size is checked for NVL_GQ_NONE too)
            return INVALID, s
        if on and (f.f32 or f.tp or s.wf == FP8 or s.wf == MXFP4):
            return INVALID, s
        if base(s.ef) == INT4 and (not on or int4(g) != s.ef):      # INT4 experts hold INT4 weights of their group size
            return INVALID, s
        if on:
            return OK, s._replace(wf=int4(g))
        return OK, s._replace(wf=BF16) if base(s.wf) == INT4 else s

    if name in ("nvl_set_expert_dtype", "nvl_set_mx_expert_dtype", "nvl_set_gq_expert_dtype"):
        fam = {"nvl_set_expert_dtype": FP8, "nvl_set_mx_expert_dtype": MXFP4, "nvl_set_gq_expert_dtype": INT4}[name]
        if late_expert:
            return STATE, s
        if not known:
            return INVALID, s
        if on:
            if not f.moe or f.f32 or base(s.wf) != fam:
                return INVALID, s
            if fam == INT4 and (f.H % group(s.wf) or f.F % group(s.wf)):
                return INVALID, s
            return OK, s._replace(ef=s.wf)
        return OK, s._replace(ef=BF16) if base(s.ef) == fam else s

    if name == "nvl_set_mx_head_dtype":
        if late_2d:
            return STATE, s
        if not known or (on and (f.f32 or s.wf != MXFP4)):
            return INVALID, s
        return OK, s._replace(hf=MXFP4 if on else BF16)

    if name == "nvl_set_act_dtype":
        if f.finalized:
            return STATE, s
        if not known or (on and s.wf != FP8):
            return INVALID, s
        return OK, s._replace(a8=on)

    raise ValueError(name)


def calls():
    """every call the tests draw from: off, on and an unknown value of each setter; nvl_set_gq_weight_dtype at the three group
    sizes and one bad one"""
    out = []
    for name in SETTERS:
        for value in (0, 1, 7):
            for g in ((32, 64, 128, 48) if name == "nvl_set_gq_weight_dtype" else (0,)):
                out.append((name, value, g))
    return out
