// wfmt.h — the stored weight formats as the host sees them, without a device: the format ids, what a format stores per element
// and per row, which tensor kinds it covers, and wf_decide(): the one place that answers every dtype request of the
// nvl_set_*_dtype entry points (include/nvllm.h).  Host-only and HIP-free, so that a plain C++ program can drive it
// (tests/wf_state_driver.cpp).  The device side of a format is w8.h / w4.h / w4g.h; its launches are in wq.h.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/nvllm.h"

namespace nvl {

// the weight storage format of a kernel's weight operand (w8.h / w4.h / w4g.h)
enum { WF_BF16 = 0, WF_FP8 = 1, WF_MXFP4 = 2, WF_INT4 = 3 };

// ---- the format table ----
// A host format id is the kernels' WF_* in its low byte; INT4 carries its group size g above it (wf_int4(g)), so that one
// id answers every question below.  wf_base() is the WF_* of the kernels, wf_gshift() = log2(g / 32) their group argument.
inline int wf_int4(int g) { return WF_INT4 | (g << 8); }
inline int wf_base(int wf) { return wf & 0xff; }
inline int wf_group(int wf) { return wf >> 8; }
inline int wf_gshift(int wf) { return wf_group(wf) == 128 ? 2 : (wf_group(wf) == 64 ? 1 : 0); }
// bytes of `elems` codes (fp8: one per element; MXFP4 / INT4: two codes per byte)
inline int64_t wf_code_bytes(int wf, int64_t elems) { return wf_base(wf) != WF_FP8 ? elems / 2 : elems; }
// bytes of the scales of `rows` rows of K inputs (fp8: one fp32 per row; MXFP4: one e8m0 byte per 32 inputs of a row,
// [rows/16][K/32][16], so whole 16-row tiles are contiguous in both; INT4: one 4-byte word {fp16 s, z} per group of g inputs
// of a row, [rows/16][K/g][16] words)
inline int64_t wf_scale_bytes(int wf, int64_t rows, int64_t K) {
    return wf == WF_MXFP4 ? rows * K / 32 : (wf_base(wf) == WF_INT4 ? rows * (K / wf_group(wf)) * 4 : rows * 4);
}
// the name of the format in error messages
inline const char* wf_name(int wf) { return wf == WF_MXFP4 ? "MXFP4" : (wf_base(wf) == WF_INT4 ? "INT4" : "8-bit"); }
// what the input width of a stored tensor must be a multiple of (fp8: the kernels' 32-wide k-steps; MXFP4: its 32-blocks; INT4:
// its groups, themselves multiples of 32), and how a shape refusal says so
inline int64_t wf_in_multiple(int wf) { return wf_base(wf) == WF_INT4 ? wf_group(wf) : 32; }
inline const char* wf_in_multiple_hint(int wf) { return wf == WF_MXFP4 ? ", in % 32 == 0" : (wf_base(wf) == WF_INT4 ? ", in % group size == 0" : ""); }
// what the upload quantizer of the format refuses, as its message says it
inline const char* wf_quant_refuses(int wf) { return wf_base(wf) == WF_INT4 ? "NaN / Inf, and a group whose scale exceeds the fp16 range" : "NaN / Inf"; }
// traffic estimates, bytes per weight.  Stored: the code, and INT4's group words (4 / g bytes per weight, a quarter of the codes
// at g = 32); the row and block scales are not counted.  A dequantize: the code and its share of the scales in, 2 bytes out.
inline double wf_stored_bytes(int wf) { return wf_code_bytes(wf, 2) / 2.0 + (wf_base(wf) == WF_INT4 ? 4.0 / wf_group(wf) : 0.0); }
inline double wf_dequant_bytes(int wf) { return wf == WF_MXFP4 ? 2.53 : (wf_base(wf) == WF_INT4 ? 2.5 + 4.0 / wf_group(wf) : 3.0); }
// does the format cover this 2-D tensor kind (experts: when the expert format `ef` is set too; LM head: the head format
// `hf`)?  Attention and FFN projections in both; the LM head, and the token embedding when it is the (tied) LM head, in
// fp8 always and in MXFP4 when nvl_set_mx_head_dtype asked for it.  Position embedding, router and Mamba2 projections stay bf16.
// INT4 (hf = WF_BF16 always) covers the attention and FFN projections, as AWQ / GPTQ checkpoints do, and the MoE experts when
// nvl_set_gq_expert_dtype asked for them (ef = wf then, the group size included).
inline bool wf_covers(int wf, int ef, int hf, int kind, bool tied_embedding) {
    switch (kind) {
        case NVL_T_WQ: case NVL_T_WK: case NVL_T_WV: case NVL_T_WKV: case NVL_T_WO: case NVL_T_W1: case NVL_T_W2: return wf != WF_BF16;
        case NVL_T_LM_HEAD: return wf == WF_FP8 || (wf != WF_BF16 && hf == wf);
        case NVL_T_TOK_EMB: return (wf == WF_FP8 || (wf != WF_BF16 && hf == wf)) && tied_embedding;
        case NVL_T_MOE_IN: case NVL_T_MOE_OUT: return wf != WF_BF16 && ef == wf;
        default: return false;
    }
}

// ---- the dtype requests ----
// What a model stores: the format of the projections (wf), of the MoE experts (ef) and of the LM head (hf; WF_BF16 under fp8,
// whose head always follows wf), and whether the tile path quantizes its activations to 8 bits (a8).
struct WfState { int wf = WF_BF16, ef = WF_BF16, hf = WF_BF16; bool a8 = false; };
// what the rules read of the model
struct WfFacts {
    bool f32, tp;              // fp32 precision; tensor parallel (a forced single rank included)
    bool moe;                  // has MoE layers
    int H, F;                  // hidden width, FFN / expert width
    bool finalized, w2d_uploaded, expert_uploaded;     // the three ways of being too late
};
enum { WT_PROJ = 0, WT_EXPERT = 1, WT_HEAD = 2, WT_ACT = 3 };     // what a request sets
enum { WFAM_FP8 = 0, WFAM_MX = 1, WFAM_GQ = 2 };                  // the family of setters it came through
// value: the entry point's own enum (0: off, 1: on in every one of them); group: nvl_set_gq_weight_dtype's group size;
// fn: the entry point's name, for the message
struct WfRequest { int target, family, value, group; const char* fn; };
struct WfDecision { int code; WfState state; char msg[192]; };     // (refused: the state as it was, and why; else "")

struct WfFamily { int base; const char* unknown; const char* setter[3]; };     // setter[]: of WT_PROJ, WT_EXPERT, WT_HEAD
inline const WfFamily& wf_family(int family) {
    static const WfFamily table[3] = {
        {WF_FP8, "", {"nvl_set_weight_dtype", "nvl_set_expert_dtype", ""}},
        {WF_MXFP4, "MX ", {"nvl_set_mx_weight_dtype", "nvl_set_mx_expert_dtype", "nvl_set_mx_head_dtype"}},
        {WF_INT4, "group-quantized ", {"nvl_set_gq_weight_dtype", "nvl_set_gq_expert_dtype", ""}},
    };
    return table[family];
}

// The rules, each written once:
//   too late      projections and head before the first 2-D upload, experts before the first expert upload, activations before
//                 nvl_finalize
//   exclusivity   one family holds the projections; turning one on while another holds them is refused
//   needs         experts, head and 8-bit activations need their own family's projections first (experts: a MoE model; INT4
//                 experts: widths that are multiples of the group size, a group of the concatenated down matrix lying inside
//                 one expert)
//   holds         while MXFP4 / INT4 experts or an MXFP4 head are set, their projections can be neither turned off nor (INT4)
//                 given another group size
//   fp8 cascade   turning fp8 projections off takes the 8-bit experts and activations with them instead
// Turning something off that another family holds, or that is off already, changes nothing and succeeds.
inline WfDecision wf_decide(const WfState& s0, const WfFacts& f, const WfRequest& r) {
    const WfFamily& fam = wf_family(r.family);
    const char* name = wf_name(fam.base);
    WfDecision d{NVL_OK, s0, ""};
    auto refuse = [&](int code, const char* fmt, auto... args) {     // (every format starts with the entry point's name)
        snprintf(d.msg, sizeof d.msg, fmt, r.fn, args...);
        d.code = code;
        return d;
    };
    // what the request would store, as the messages call it: "<an><name><noun> need<s> ..."
    static const char* const target_word[4] = {"weight", "expert", "head", "activation"};
    static const char* const noun[4] = {" weights", " experts", " LM head", " activations"};
    const char *an = r.target == WT_HEAD ? "an " : "", *need = r.target == WT_HEAD ? "needs" : "need";

    if (f.finalized || (r.target == WT_EXPERT && f.expert_uploaded) || ((r.target == WT_PROJ || r.target == WT_HEAD) && f.w2d_uploaded)) {
        if (r.target == WT_ACT) return refuse(NVL_ERR_STATE, "%s: call it before nvl_finalize");
        return refuse(NVL_ERR_STATE, "%s: call it after %s and before the first %s upload", r.target == WT_PROJ ? "nvl_create" : fam.setter[WT_PROJ],
                      r.target == WT_EXPERT ? "expert" : "2-D weight");
    }
    if (r.value != 0 && r.value != 1) return refuse(NVL_ERR_INVALID, "%s: unknown %s%s dtype", fam.unknown, target_word[r.target]);
    const bool on = r.value == 1, gq = r.family == WFAM_GQ;
    if (r.target == WT_PROJ && gq && r.group != 32 && r.group != 64 && r.group != 128)     // (asked of NVL_GQ_NONE too)
        return refuse(NVL_ERR_INVALID, "%s: the group size must be 32, 64 or 128");
    WfState& s = d.state;

    if (r.target != WT_PROJ) {     // experts, head, activations: they need their family's projections
        if (on) {
            if (r.target == WT_EXPERT && !f.moe) return refuse(NVL_ERR_INVALID, "%s: the model has no MoE layers");
            if (r.target != WT_ACT && f.f32) return refuse(NVL_ERR_INVALID, "%s: %s%s%s %s bf16 precision", an, name, noun[r.target], need);
            if (wf_base(s.wf) != fam.base)
                return refuse(NVL_ERR_INVALID, "%s: %s%s%s %s %s %sweights (%s first)", an, name, noun[r.target], need, name,
                              r.target == WT_ACT ? "" : "projection ", fam.setter[WT_PROJ]);
            if (r.target == WT_EXPERT && gq && (f.H % wf_group(s.wf) != 0 || f.F % wf_group(s.wf) != 0))
                return refuse(NVL_ERR_INVALID, "%s: the hidden width and the expert width must be multiples of the group size");
        }
        if (r.target == WT_EXPERT) s.ef = on ? s.wf : (wf_base(s.ef) == fam.base ? WF_BF16 : s.ef);
        else if (r.target == WT_HEAD) s.hf = on ? s.wf : WF_BF16;
        else s.a8 = on;
        return d;
    }

    const int mine = gq ? wf_int4(r.group) : fam.base;     // the projections
    if (on) {
        if (f.f32) return refuse(NVL_ERR_INVALID, "%s: %s weights need bf16 precision", name);
        if (f.tp) return refuse(NVL_ERR_INVALID, "%s: %s weights are not available with tensor parallelism", name);
        for (int o = 0; o < 3; o++)     // exclusivity
            if (o != r.family && wf_base(s.wf) == wf_family(o).base)
                return refuse(NVL_ERR_INVALID, "%s: the model stores %s weights (%s)", wf_name(wf_family(o).base), wf_family(o).setter[WT_PROJ]);
    }
    if (r.family != WFAM_FP8) {         // holds: what depends on these projections keeps them as they are
        if (wf_base(s.ef) == fam.base && (!on || mine != s.ef))
            return refuse(NVL_ERR_INVALID, "%s: the model stores %s experts (%s), which need %s weights%s", name, fam.setter[WT_EXPERT], name,
                          gq ? " of their group size" : "");
        if (wf_base(s.hf) == fam.base && !on)
            return refuse(NVL_ERR_INVALID, "%s: the model stores an %s LM head (%s), which needs %s weights", name, fam.setter[WT_HEAD], name);
    }
    if (on) s.wf = mine;
    else if (wf_base(s.wf) == fam.base) {
        s.wf = WF_BF16;
        if (r.family == WFAM_FP8) { s.ef = WF_BF16; s.a8 = false; }     // the fp8 cascade
    }
    return d;
}

}  // namespace nvl
