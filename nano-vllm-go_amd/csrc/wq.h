// wq.h — the device side of a quantized weight as the host drives it, whatever its format (wfmt.h WF_FP8: w8.h, WF_MXFP4: w4.h,
// WF_INT4: w4g.h).  What a format is, what it covers and which dtype requests a model accepts is wfmt.h (host-only, DESIGN.md
// §9); here is every launch and every walk over codes and scales that differs by format, each as one wf_* function that
// switches on the format once: pad scales, the upload quantizer, the prequantized upload's checks and placement, the scale
// gather of a tile permutation, the experts' concatenated down matrix and its dequantize, the read-backs, the dequantize
// launch of the tile path and the GEMM dispatch.  The callers (nvllm.hip, ops_impl.h) allocate and pass a format id.
// The numerics and the device layouts of each format are described in w8.h / w4.h / w4g.h.
#pragma once
#include "elem.h"
#include "w8.h"
#include "w4.h"
#include "w4g.h"
#include "a8.h"

namespace nvl {

// every scale of `rows` rows of K inputs at the pad value of the format: fp32 1.0, the e8m0 byte 127 (2^0), or the INT4 group
// word {s = 1, z = 0}
static inline void wf_fill_pad_scales(hipStream_t st, int wf, void* qs, int64_t rows, int64_t K) {
    const size_t nb = (size_t)wf_scale_bytes(wf, rows, K);
    switch (wf_base(wf)) {
        case WF_MXFP4: NVL_HIP(hipMemsetAsync(qs, 127, nb, st)); break;
        case WF_INT4: {
            const std::vector<uint32_t> pad(nb / 4, W4G_PAD_WORD);
            NVL_HIP(hipMemcpy(qs, pad.data(), nb, hipMemcpyHostToDevice));
            break;
        }
        default: {
            const std::vector<float> ones((size_t)rows, 1.0f);
            NVL_HIP(hipMemcpy(qs, ones.data(), nb, hipMemcpyHostToDevice));   // (synchronous: `ones` is pageable and local)
        }
    }
}

// the upload quantizer: fp32 f [N][K] on the device -> codes + scales in the format's device layout; *bad is set when a weight
// is not finite (INT4: or a group's scale exceeds the fp16 range)
static inline void wf_quant_rows(hipStream_t st, int wf, const float* f, int64_t N, int64_t K, void* codes, void* qs, int* bad) {
    switch (wf_base(wf)) {
        case WF_MXFP4: hipLaunchKernelGGL(w4_quant_rows_kernel, dim3((unsigned)N), dim3(64), 0, st, f, K, (uint8_t*)codes, (uint8_t*)qs, bad); break;
        case WF_INT4: hipLaunchKernelGGL(w4g_quant_rows_kernel, dim3((unsigned)N), dim3(64), 0, st, f, K, wf_gshift(wf), (uint8_t*)codes, (uint32_t*)qs, bad); break;
        default: hipLaunchKernelGGL(w8_quant_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, f, K, (uint8_t*)codes, (float*)qs, bad);
    }
}

// ---- the prequantized upload (nvl_upload_tensor_fp8 / _mxfp4 / _int4): codes, scales and zero points in the ABI packing ----
// bytes of the scales and of the zero points of [rows][cols] as the caller passes them: fp8 one fp32 per row; MXFP4 one e8m0
// byte per 32 inputs; INT4 one fp16 scale and one zero-point byte per group
static inline int64_t wf_abi_scale_bytes(int wf, int64_t rows, int64_t cols) {
    return wf_base(wf) == WF_INT4 ? rows * (cols / wf_group(wf)) * 2 : wf_scale_bytes(wf, rows, cols);
}
static inline int64_t wf_abi_zero_bytes(int wf, int64_t rows, int64_t cols) { return wf_base(wf) == WF_INT4 ? rows * (cols / wf_group(wf)) : 0; }
// what the caller's values must satisfy: nullptr, or the refusal (a format that takes the entry point's name)
static inline const char* wf_check_prequant(int wf, const uint8_t* codes, const void* scales, const uint8_t* zeros, int64_t rows, int64_t cols) {
    switch (wf_base(wf)) {
        case WF_MXFP4:
            for (int64_t i = 0; i < rows * (cols / 32); i++)
                if (((const uint8_t*)scales)[i] < W4_E_MIN + 127 || ((const uint8_t*)scales)[i] > W4_E_MAX + 127)
                    return "%s: a scale byte is outside [7, 252] (0xff is the e8m0 NaN)";
            return nullptr;
        case WF_INT4:
            for (int64_t i = 0; i < rows * (cols / wf_group(wf)); i++) {
                if (zeros[i] > 15) return "%s: a zero point is above 15";
                const uint16_t h = ((const uint16_t*)scales)[i];     // fp16 bits: positive (sign 0, not zero) and finite (exponent field below 31)
                if ((h & 0x8000) || h == 0 || (h & 0x7c00) == 0x7c00) return "%s: scales must be finite and positive";
            }
            return nullptr;
        default:
            for (int64_t i = 0; i < rows * cols; i++)
                if ((codes[i] & 0x7F) == 0x7F) return "%s: NaN code (0x7f / 0xff)";
            for (int64_t r = 0; r < rows; r++)
                if (!(((const float*)scales)[r] > 0.f) || !std::isfinite(((const float*)scales)[r])) return "%s: scales must be finite and positive";
            return nullptr;
    }
}
// device copies of the caller's arrays -> the format's device layout (fp8: one scale per row, the layout is the caller's;
// MXFP4 / INT4: the scales move beside the 16-row tiles with the codes)
static inline void wf_place(hipStream_t st, int wf, const uint8_t* raw, const void* raw_s, const uint8_t* raw_z, int64_t rows, int64_t cols,
                            void* codes, void* qs) {
    switch (wf_base(wf)) {
        case WF_MXFP4:
            hipLaunchKernelGGL(w4_place_kernel, dim3((unsigned)cdiv(rows * cols / 8, 256)), dim3(256), 0, st, raw, (const uint8_t*)raw_s, rows, cols,
                               (uint8_t*)codes, (uint8_t*)qs);
            break;
        case WF_INT4:
            hipLaunchKernelGGL(w4g_place_kernel, dim3((unsigned)cdiv(rows * cols / 8, 256)), dim3(256), 0, st, raw, (const uint16_t*)raw_s, raw_z, rows,
                               cols, wf_gshift(wf), (uint8_t*)codes, (uint32_t*)qs);
            break;
        default:
            NVL_HIP(hipMemcpyAsync(qs, raw_s, (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(w8_place_kernel, dim3((unsigned)cdiv(rows * cols / 4, 256)), dim3(256), 0, st, raw, rows, cols, (uint8_t*)codes);
    }
}

// ---- a row permutation in 16-row tiles (nvllm.hip gather_rows_q): the scales of the moved tiles ----
// idx: source row of every destination row (-1: pad); d_tiles: the same per tile, on the device.  Pad rows get, fp8: scale 1
// (the per-row scales are permuted on the host); MXFP4: zero scale bytes, a tile's K/2 scale bytes being contiguous like its
// codes; INT4: zero group words, moved the same way (W~ = 0 every way; pad outputs are never stored)
static inline void wf_gather_scales(hipStream_t st, int wf, const void* src_qs, int64_t src_rows_pad, const std::vector<int32_t>& idx,
                                    const int32_t* d_tiles, void* dst_qs, int64_t K) {
    if (wf_base(wf) != WF_FP8) {
        hipLaunchKernelGGL((gather_rows_kernel<uint8_t>), dim3((unsigned)(idx.size() / 16)), dim3(256), 0, st, (const uint8_t*)src_qs, d_tiles,
                           (uint8_t*)dst_qs, wf_scale_bytes(wf, 16, K));
        return;
    }
    std::vector<float> ssrc((size_t)src_rows_pad), sc;
    NVL_HIP(hipMemcpy(ssrc.data(), src_qs, ssrc.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t i : idx) sc.push_back(i < 0 ? 1.0f : ssrc[(size_t)i]);
    NVL_HIP(hipMemcpy(dst_qs, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));     // (synchronous: `sc` is pageable and local)
}

// ---- quantized MoE experts: the down matrices concatenated over K = E*I, codes [H_pad][E*I] (the decode form's layout) ----
// where their scales live: fp8 one row of H_pad scales per expert, [E * H_pad] rows of I inputs; MXFP4 / INT4 block scales /
// group words over the same K as the codes, [H_pad] rows of E*I inputs
static inline void wf_down_scale_dims(int wf, int64_t hp, int64_t E, int64_t I, int64_t* rows, int64_t* K) {
    const bool per_expert = wf_base(wf) == WF_FP8;
    *rows = per_expert ? E * hp : hp;
    *K = per_expert ? I : E * I;
}
// src / src_qs: the uploaded [E*H][I] tensor (src_rows_pad allocated rows); dst zeroed, dst_qs at the pad value
static inline void wf_cat_down(hipStream_t st, int wf, const void* src, const void* src_qs, int64_t src_rows_pad, void* dst, void* dst_qs,
                               int64_t H, int64_t I, int64_t E) {
    const dim3 grid((unsigned)(H / 16), (unsigned)E);
    switch (wf_base(wf)) {
        case WF_MXFP4:     // block scales, moved with the code tiles
            hipLaunchKernelGGL(moe_cat_down_w4_kernel, grid, dim3(256), 0, st, (const uint8_t*)src, (const uint8_t*)src_qs, (uint8_t*)dst,
                               (uint8_t*)dst_qs, (int)H, (int)I, (int)E);
            break;
        case WF_INT4:      // group words (pad rows: {s = 1, z = 0}), moved with the code tiles
            hipLaunchKernelGGL(moe_cat_down_w4g_kernel, grid, dim3(256), 0, st, (const uint8_t*)src, (const uint32_t*)src_qs, (uint8_t*)dst,
                               (uint32_t*)dst_qs, (int)H, (int)I, (int)E, wf_gshift(wf));
            break;
        default: {         // row scales: one row per expert, through the host
            hipLaunchKernelGGL(moe_cat_down_w8_kernel, grid, dim3(256), 0, st, (const uint8_t*)src, (uint8_t*)dst, (int)H, (int)I, (int)E);
            const int64_t hp = round_up(H, W_ROW_PAD);
            std::vector<float> sd((size_t)src_rows_pad);
            NVL_HIP(hipMemcpy(sd.data(), src_qs, sd.size() * 4, hipMemcpyDeviceToHost));
            for (int64_t e = 0; e < E; e++)
                NVL_HIP(hipMemcpy((float*)dst_qs + e * hp, &sd[(size_t)(e * H)], (size_t)H * 4, hipMemcpyHostToDevice));
        }
    }
}
// the grouped forms: W~ of those down matrices into dst, [E][H][I] fragment-major per expert
static inline void wf_dequant_down(hipStream_t st, int wf, const void* codes, const void* qs, int H, int I, int E, bf16_t* dst) {
    const int64_t n8 = (int64_t)E * H * I / 8;
    const dim3 grid((unsigned)cdiv(n8, 256));
    switch (wf_base(wf)) {
        case WF_MXFP4: hipLaunchKernelGGL(e4_dequant_down_kernel, grid, dim3(256), 0, st, (const uint8_t*)codes, (const uint8_t*)qs, H, I, E, n8, dst); break;
        case WF_INT4:
            hipLaunchKernelGGL(e4g_dequant_down_kernel, grid, dim3(256), 0, st, (const uint8_t*)codes, (const uint32_t*)qs, H, I, E, wf_gshift(wf), n8, dst);
            break;
        default:
            hipLaunchKernelGGL(e8_dequant_down_kernel, grid, dim3(256), 0, st, (const uint8_t*)codes, (const float*)qs, H, I, E, round_up(H, W_ROW_PAD), n8, dst);
    }
}

// ---- read-backs (host copies of the device layout: codes of [rows_pad][K], their scales) ----
// W~ of element (n, k), the value every GEMM path computes with: fp8 bf16_rne(s * e4m3(q)); MXFP4 +-grid[q] * 2^e; INT4
// bf16_rne(s * (q - z))
static inline float wf_value_at(int wf, const uint8_t* codes, const void* scales, int64_t n, int64_t k, int64_t K) {
    switch (wf_base(wf)) {
        case WF_MXFP4: return w4_value(w4_code_at(codes, n, k, K), ((const uint8_t*)scales)[w4_scale_index(n, k >> 5, K >> 5)]);
        case WF_INT4: {
            const int64_t g = wf_group(wf);
            return w4g_value(w4_code_at(codes, n, k, K), ((const uint32_t*)scales)[w4g_word_index(n, k / g, K / g)]);
        }
        default: return w8_value(codes[fm_index(n, k, K)], ((const float*)scales)[n]);
    }
}
// the first N rows in the ABI packing of the prequantized upload; a null output is skipped (zeros_out: INT4 only)
static inline void wf_to_abi(int wf, const uint8_t* codes, const void* scales, int64_t N, int64_t K, uint8_t* codes_out, void* scales_out,
                             uint8_t* zeros_out) {
    switch (wf_base(wf)) {
        case WF_MXFP4: {
            std::vector<uint8_t> co((size_t)N * K / 2), so((size_t)N * K / 32);
            w4_to_abi(codes, (const uint8_t*)scales, N, K, co.data(), so.data());
            if (codes_out) memcpy(codes_out, co.data(), co.size());
            if (scales_out) memcpy(scales_out, so.data(), so.size());
            break;
        }
        case WF_INT4: w4g_to_abi(codes, (const uint32_t*)scales, N, K, wf_group(wf), codes_out, (uint16_t*)scales_out, zeros_out); break;
        default:
            if (scales_out) memcpy(scales_out, scales, (size_t)N * 4);
            if (codes_out)
                for (int64_t n = 0; n < N; n++)
                    for (int64_t k = 0; k < K; k++) codes_out[n * K + k] = codes[(size_t)fm_index(n, k, K)];
    }
}

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
