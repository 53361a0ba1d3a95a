// wq.h — the host side of a quantized weight, whatever its format (gemm.h WF_FP8: w8.h, WF_MXFP4: w4.h, WF_INT4: w4g.h): the format table
// (what a format stores per element and per row), the dequantize launch of the tile path and the GEMM dispatch.
// The numerics and the device layouts of each format are described in w8.h / w4.h / w4g.h.
#pragma once
#include "w8.h"
#include "w4.h"
#include "w4g.h"
#include "a8.h"

namespace nvl {

// ---- the format table: every host decision that depends on the stored format is answered here ----
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
// (the pad scales — fp32 1.0 / e8m0 127 = 2^0 — are written where the scales are allocated: nvllm.hip q_alloc_scales)

// W~ of rows [row0, row0 + rows) (whole 16-row tiles) into dst, fragment-major
static inline void wf_dequant_rows(hipStream_t st, int wf, const void* codes, const void* qs, int64_t K, int64_t row0, int64_t rows,
                                   bf16_t* dst) {
    const int64_t n8 = rows * K / 8;
    const uint8_t* c = (const uint8_t*)codes + wf_code_bytes(wf, row0 * K);
    const uint8_t* s = (const uint8_t*)qs + wf_scale_bytes(wf, row0, K);
    if (wf == WF_MXFP4) hipLaunchKernelGGL(w4_dequant_kernel, dim3((unsigned)cdiv(n8, 256)), dim3(256), 0, st, c, s, n8, dst);
    else if (wf_base(wf) == WF_INT4)
        hipLaunchKernelGGL(w4g_dequant_kernel, dim3((unsigned)cdiv(n8, 256)), dim3(256), 0, st, c, (const uint32_t*)s, K >> 5, wf_gshift(wf), n8, dst);
    else hipLaunchKernelGGL(w8_dequant_kernel, dim3((unsigned)cdiv(n8, 256)), dim3(256), 0, st, c, (const float*)s, K, n8, dst);
}

// The GEMM of a quantized weight (a.W: codes, qs: its scales, w_rows_pad: its allocated rows).  Decode-sized calls go where
// the bf16 dispatch (launch_gemm_bf16) sends them, on the kernels of format WF; the rest run the bf16 dispatch on W~ in
// `scratch` (scratch_elems bf16 elements); a W~ that does not fit runs in row chunks (EPI_STORE with fp32 output only: the
// LM head).  fp8 only: with a8 (8-bit activations, a8.h) the tile step is the W8A8 kernel on the codes instead.
// INT4 only: g, the group size of the weight (the decode kernels' gshift and the dequantize launch need it).
template <int EPI, typename OutT, int WF>
static inline void launch_gemm_q(hipStream_t st, const GemmArgs& a, const void* qs, int64_t w_rows_pad, bf16_t* scratch,
                                 int64_t scratch_elems, const A8Buf* a8 = nullptr, int g = 0) {
    static_assert(WF == WF_FP8 || WF == WF_MXFP4 || WF == WF_INT4, "launch_gemm_q: a quantized format");
    auto err = [](const char* tail) { return std::runtime_error(std::string("gemm: ") + (WF == WF_FP8 ? "an 8-bit" : (WF == WF_INT4 ? "an INT4" : "an MXFP4")) + tail); };
    const int wfid = WF == WF_INT4 ? wf_int4(g) : WF, gsh = wf_gshift(wfid);     // (gsh: 0 for the other formats)
    if (a.tile_map || a.seg || a.a_rows) throw err(" weight in a gathered / grouped launch");
    const float* ws = (const float*)qs;     // (the launchers' scale argument; the MXFP4 kernels take it back as bytes)
    if (a.moe_gate) {     // quantized MoE experts, the decode (dense-masked) form: the only launch that reads their codes
        if (launch_gemm_skinny_bf16<EPI, OutT, WF>(st, a, ws, gsh)) return;
        throw err(" MoE projection did not fit the decode kernels");
    }
    if (launch_gemm_skinny_bf16<EPI, OutT, WF>(st, a, ws, gsh)) return;
    if constexpr (EPI != EPI_QKV) {
        if (skinny_groups_ok(a)) {     // (the 64-row-group condition of launch_gemm_bf16)
            GemmArgs c = a;
            c.m_passes = cdiv(a.M, 64);
            const bool ok = g_pass_interleave ? launch_gemm_skinny_bf16<EPI, OutT, WF>(st, c, ws, gsh)
                                              : launch_skinny_passes_serial<EPI, OutT, WF>(st, c, ws, gsh);
            if (ok) return;
        }
    }
    if (a.rs_in || a.rs_out) throw std::runtime_error("gemm: a deferred-RMSNorm projection did not fit the decode kernels");
    if constexpr (WF == WF_FP8) {
        if (a8) {
            launch_gemm_w8a8<EPI, OutT>(st, a, ws, *a8);
            return;
        }
    }
    if (w_rows_pad * a.K <= scratch_elems) {
        wf_dequant_rows(st, wfid, a.W, qs, a.K, 0, w_rows_pad, scratch);
        GemmArgs c = a;
        c.W = scratch;
        launch_gemm_bf16<EPI, OutT>(st, c);
        return;
    }
    if constexpr (EPI == EPI_STORE && std::is_same<OutT, float>::value) {
        const int64_t chunk = (scratch_elems / a.K) / W_ROW_PAD * W_ROW_PAD;     // whole padded tiles per chunk
        if (chunk < W_ROW_PAD) throw err(" weight's scratch holds no whole row tile");
        for (int64_t n0 = 0; n0 < a.N; n0 += chunk) {
            const int64_t rows = std::min<int64_t>(chunk, w_rows_pad - n0);
            wf_dequant_rows(st, wfid, a.W, qs, a.K, n0, rows, scratch);
            GemmArgs c = a;
            c.W = scratch;
            c.N = (int)std::min<int64_t>(chunk, a.N - n0);
            c.C = (float*)a.C + n0;
            if (a.bias) c.bias = a.bias + n0;
            launch_gemm_bf16<EPI, OutT>(st, c);
        }
        return;
    }
    throw err(" weight larger than its dequantize scratch");
}

}  // namespace nvl
