// w4g.h — INT4 group-quantized projection weights (nvl_set_gq_weight_dtype): the W4A16 format of
// AWQ / GPTQ checkpoints — unsigned 4-bit codes with one fp16 scale and one 4-bit zero point per group of g = 32 / 64 / 128
// consecutive k of one output row.  The quantizer every upload uses, the placement of pre-quantized input, the dequantize
// kernel of the tile path and the host read-back.  The host side shared with fp8 / MXFP4 (format table, dispatch) is wq.h.
//
// Numerics, per group, all fp32 with correctly rounded division and round-half-even: lo = min(0, min w), hi = max(0, max w),
// r = hi - lo; r == 0: s = 1, z = 0, q = 0; else s = fp16_rne(r / 15) (2^-24 when that rounds to 0; r / 15 > 65504 and any
// non-finite weight refuse the upload), z = clamp(rint(-lo / s), 0, 15), q = clamp(rint(w / s) + z, 0, 15).
// The model computes with W~ = bf16_rne(fp32(s) * (q - z)) — the product is exact in fp32, one rounding — on every path:
//   decode: gemm_skinny_int4w_kernel / gemm_skinny_wide_int4w_kernel, the shared decode bodies with the fragment built from 4
//       code bytes + the group's word (gemm.h w4g_frag) — the same launch decisions as in bf16 mode;
//   everything else: w4g_dequant_kernel writes W~ in the bf16 fragment-major layout into the tile-path scratch.
// Storage: codes exactly as MXFP4's (w4.h: nibble-packed fragment-major, 256 bytes per 16-row x 32-k block, even k in the low
// nibble); one 32-bit word per (row, group), {fp16 s in bits 0-15, z in bits 16-19}, [rows_pad/16][K/g][16]: the 16 rows of
// a tile side by side, one 4-byte load beside the codes (pad rows: codes 0, s = 1, z = 0).
// MoE experts (nvl_set_gq_expert_dtype, §9 f-19): the same contract with one word per g input features of one (expert, output
// row).  Decode streams the codes through gemm_skinny_moe_int4w_kernel / gemm_skinny_wide_moe_int4w_kernel; every other MoE
// launch runs the unchanged grouped GEMMs on one layer's W~, dequantized (up, then down) into a scratch buffer.  No checkpoint
// reading: no AWQ / GPTQ MoE layout is mapped by the loader, the experts arrive through the upload calls.
#pragma once
#include "gemm.h"

namespace nvl {

constexpr uint32_t W4G_PAD_WORD = 0x3c00u;     // {s = 1.0, z = 0}

// word offset of row r's group gi (ng = K/g groups per row)
__host__ __device__ __forceinline__ int64_t w4g_word_index(int64_t r, int64_t gi, int64_t ng) { return ((r >> 4) * ng + gi) * 16 + (r & 15); }

// x fp32 row-major [rows][K] -> codes + group words in the device layout; one wave per row, a lane per group of 32 << gshift.
// A non-finite element or a group whose scale would exceed the fp16 range sets *bad (the upload is refused).
__global__ __launch_bounds__(64) void w4g_quant_rows_kernel(const float* __restrict__ x, int64_t K, int gshift, uint8_t* __restrict__ codes,
                                                            uint32_t* __restrict__ words, int* __restrict__ bad) {
    const int64_t r = blockIdx.x, ng = (K >> 5) >> gshift;
    const int g = 32 << gshift;
    bool ok = true;
    for (int64_t gi = threadIdx.x; gi < ng; gi += 64) {
        const float* xg = x + r * K + gi * g;
        float lo = 0.f, hi = 0.f;
        bool fin = true;
        for (int k = 0; k < g; k++) {
            const float w = xg[k];
            if ((__builtin_bit_cast(uint32_t, w) & 0x7fffffffu) >= 0x7f800000u) fin = false;
            lo = fminf(lo, w); hi = fmaxf(hi, w);
        }
        const float range = hi - lo, step = __fdiv_rn(range, 15.0f);
        if (!fin || !(step <= 65504.0f)) { ok = false; fin = false; }
        uint32_t sb = 0x3c00u, z = 0;
        float s = 1.0f;
        const bool flat = !fin || range == 0.f;
        if (!flat) {
            sb = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)step);
            if (sb == 0) sb = 1;                                  // the smallest fp16, 2^-24
            s = (float)__builtin_bit_cast(_Float16, (uint16_t)sb);
            z = (uint32_t)fminf(fmaxf(rintf(__fdiv_rn(-lo, s)), 0.f), 15.f);
        }
        words[w4g_word_index(r, gi, ng)] = sb | (z << 16);
        for (int f = 0; f < g / 8; f++) {     // fragments of 8 codes
            uint32_t c = 0;
            for (int k = 0; k < 8; k++) {
                const uint32_t q = flat ? 0u : (uint32_t)fminf(fmaxf(rintf(__fdiv_rn(xg[8 * f + k], s)) + (float)z, 0.f), 15.f);
                c |= q << (4 * k);
            }
            *(uint32_t*)(codes + (fm_index(r, gi * g + 8 * f, K) >> 1)) = c;
        }
    }
    if (!ok) atomicOr(bad, 1);
}

// pre-quantized input in the ABI packing (codes [rows][K/2], fp16 scales and zero points [rows][K/g], nvl_upload_tensor_int4)
// -> the device layout; a thread per 4 code bytes (one fragment), the first thread of a group also writes its word
__global__ __launch_bounds__(256) void w4g_place_kernel(const uint8_t* __restrict__ src, const uint16_t* __restrict__ src_scales,
                                                        const uint8_t* __restrict__ src_zeros, int64_t rows, int64_t K, int gshift,
                                                        uint8_t* __restrict__ dst, uint32_t* __restrict__ dst_words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // fragment index, row-major: [rows][K/8]
    if (i >= rows * (K >> 3)) return;
    const int64_t r = i / (K >> 3), k = (i - r * (K >> 3)) * 8, ng = (K >> 5) >> gshift;
    *(uint32_t*)(dst + (fm_index(r, k, K) >> 1)) = *(const uint32_t*)(src + i * 4);
    if ((k & ((32 << gshift) - 1)) == 0) {
        const int64_t gi = (k >> 5) >> gshift;
        dst_words[w4g_word_index(r, gi, ng)] = (uint32_t)src_scales[r * ng + gi] | ((uint32_t)(src_zeros[r * ng + gi] & 15) << 16);
    }
}

// codes + group words -> W~ (bf16, the fragment-major layout): n8 fragments starting at a 16-row tile boundary, nks = K/32
__global__ __launch_bounds__(256) void w4g_dequant_kernel(const uint8_t* __restrict__ codes, const uint32_t* __restrict__ words,
                                                          int64_t nks, int gshift, int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // fragment index: (tile, k-step, lane)
    if (i >= n8) return;
    const int64_t blk = i >> 6, tile = blk / nks, ks = blk - tile * nks;
    *(bf16x8*)(out + i * 8) = w4g_frag(*(const uint32_t*)(codes + i * 4), words[(tile * (nks >> gshift) + (ks >> gshift)) * 16 + (i & 15)]);
}

// INT4 MoE experts (nvl_set_gq_expert_dtype).  As for MXFP4 experts (w4.h) the down codes are stored once, in
// the decode form's layout: [H_pad][E*I/2] bytes, fragment-major with K = E*I (expert e's k-steps e*I/32 .. (e+1)*I/32 - 1 of
// every 16-row tile), the group words [H_pad/16][E*I/g][16] over the same K (expert e's groups e*I/g .. (e+1)*I/g - 1: I % g
// == 0, no group straddles two experts).  moe_cat_down_w4g_kernel builds both from the uploaded [E*H][I] codes and words
// (moe_cat_down_w4_kernel with words for scale bytes; H % 16 == 0: an expert starts on a tile boundary).
__global__ __launch_bounds__(256) void moe_cat_down_w4g_kernel(const uint8_t* __restrict__ src, const uint32_t* __restrict__ src_words,
                                                               uint8_t* __restrict__ dst, uint32_t* __restrict__ dst_words, int H, int I, int E,
                                                               int gshift) {
    const int nt = blockIdx.x, e = blockIdx.y, kbs = I >> 5, ngs = kbs >> gshift;     // k-steps and groups per expert row
    const int64_t stile = (int64_t)e * (H >> 4) + nt, dtile = nt;
    const uint32_t* s4 = (const uint32_t*)(src + stile * kbs * 256);
    uint32_t* d4 = (uint32_t*)(dst + (dtile * E + e) * kbs * 256);
    for (int i = threadIdx.x; i < kbs * 64; i += 256) d4[i] = s4[i];
    const uint32_t* sw = src_words + stile * ngs * 16;
    uint32_t* dw = dst_words + (dtile * E + e) * ngs * 16;
    for (int i = threadIdx.x; i < ngs * 16; i += 256) dw[i] = sw[i];
}

// the tile path's per-expert W~ of the down projection from the stored concatenated codes: out [E][H][I] bf16, fragment-major
// per expert (expert e at e*H*I: the grouped GEMMs' w_expert_stride), n8 = E*H*I/8 fragments, H % 16 == 0
__global__ __launch_bounds__(256) void e4g_dequant_down_kernel(const uint8_t* __restrict__ codes, const uint32_t* __restrict__ words,
                                                               int H, int I, int E, int gshift, int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int64_t per_e = (int64_t)H * I / 8, kbs = I >> 5;
    const int64_t e = i / per_e, j = i - e * per_e;            // j = (tile * kbs + ks) * 64 + lane
    const int64_t lane = j & 63, blk = j >> 6, tile = blk / kbs, ks = blk - tile * kbs;
    const int64_t sblk = (tile * E + e) * kbs + ks;            // the (tile, k-step) block over K = E*I; its group: sblk >> gshift
    *(bf16x8*)(out + i * 8) = w4g_frag(*(const uint32_t*)(codes + (sblk * 64 + lane) * 4), words[(sblk >> gshift) * 16 + (lane & 15)]);
}

// ---- host ----
inline float w4g_half_value(uint16_t h) {     // fp16 bits -> fp32 (finite inputs)
    const int e = (h >> 10) & 31, f = h & 1023;
    const float v = e == 0 ? std::ldexp((float)f, -24) : std::ldexp((float)(f | 1024), e - 25);
    return (h & 0x8000) ? -v : v;
}
// W~ of one code under its group's word (the read-back of nvl_get_weight)
inline float w4g_value(uint8_t q, uint32_t word) {
    const float p = w4g_half_value((uint16_t)word) * (float)((int)q - (int)((word >> 16) & 15));
    uint32_t u;
    memcpy(&u, &p, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;     // RNE to bf16 (p is finite)
    float v;
    memcpy(&v, &u, 4);
    return v;
}
// device layout (host copies) -> the ABI packing: codes [N][K/2] (even k in the low nibble), scales / zeros [N][K/g]
inline void w4g_to_abi(const uint8_t* codes, const uint32_t* words, int64_t N, int64_t K, int g, uint8_t* codes_out, uint16_t* scales_out,
                       uint8_t* zeros_out) {
    const int64_t ng = K / g;
    for (int64_t r = 0; r < N; r++) {
        if (codes_out) for (int64_t k = 0; k < K; k += 2) codes_out[r * (K / 2) + k / 2] = codes[fm_index(r, k, K) >> 1];
        for (int64_t gi = 0; gi < ng; gi++) {
            const uint32_t w = words[w4g_word_index(r, gi, ng)];
            if (scales_out) scales_out[r * ng + gi] = (uint16_t)w;
            if (zeros_out) zeros_out[r * ng + gi] = (uint8_t)((w >> 16) & 15);
        }
    }
}

}  // namespace nvl
