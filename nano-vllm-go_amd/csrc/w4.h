// w4.h — MXFP4 projection weights (nvl_set_mx_weight_dtype): OCP e2m1 elements with one e8m0 scale
// per block of 32 consecutive k of one output row.  The quantizer every upload uses, the placement of pre-quantized input,
// and the dequantize kernel of the tile path.  The host side shared with fp8 (format table, GEMM dispatch) is wq.h.
//
// Numerics, per 32-block: e = clamp(floor(log2(amax)) - 2, -120, 125) (0 for an all-zero block), stored E = e + 127;
// q = e2m1_rne(|w| / 2^e) on {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even mantissa bit, saturating at 6; sign in bit 3.
// The model computes with W~ = +-grid[q] * 2^e, exact in bf16 and never denormal, on every path:
//   decode (every call the bf16 dispatch sends to the weight-streaming kernels): gemm_skinny_mxfp4w_kernel /
//       gemm_skinny_wide_mxfp4w_kernel, the fp8-weight bodies with the fragment built from 4 code bytes + the block's E
//       (gemm.h w4_frag: v_cvt_scalef32_pk_bf16_fp4) — the same launch decisions as in bf16 mode;
//   everything else (prefill, the tile and ping-pong kernels): w4_dequant_kernel writes W~ in the bf16 fragment-major
//       layout into the tile-path scratch and the unchanged bf16 GEMM runs on it.
// Storage: codes in the bf16 fragment-major order, two per byte ([rows_pad][K/2] bytes: a 16-row x 32-k block is 256
// bytes, a lane's fragment 4 of them, even k in the low nibble); scales [rows_pad/16][K/32][16] bytes, a block's 16 rows
// side by side (pad rows: codes 0, E = 127).  A fm_index() element offset halved is the byte of its code pair.
// MoE experts (nvl_set_mx_expert_dtype, §9 f-10): the same contract with one scale per 32 input features of one (expert,
// output row).  Decode streams the codes through gemm_skinny_moe_mxfp4w_kernel / gemm_skinny_wide_moe_mxfp4w_kernel; every
// other MoE launch runs the unchanged grouped GEMMs on one layer's W~, dequantized (up, then down) into a scratch buffer.
#pragma once
#include "gemm.h"

namespace nvl {

constexpr int W4_E_MIN = -120, W4_E_MAX = 125;     // block exponents; E = e + 127 in [7, 252]

// byte offset of row r's scale of k-step ks (K/32 k-steps per row)
__host__ __device__ __forceinline__ int64_t w4_scale_index(int64_t r, int64_t ks, int64_t nks) {
    return ((r >> 4) * nks + ks) * 16 + (r & 15);
}

// the e2m1 code of |w| * 2^-e (v >= 0, finite): round to nearest, ties to the even mantissa bit, saturate at 6
__device__ __forceinline__ uint32_t w4_code(float v) {
    return (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) + (uint32_t)(v > 2.5f) +
           (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
}

// x fp32 row-major [rows][K] -> codes + scales in the device layout; one wave per row, a lane per 32-block.
// Any non-finite element sets *bad (the upload is refused).  Plain arithmetic: the chip's fp4 quantizing instruction is
// not used (its ties and saturation are not pinned against the contract; the upload is not a hot path).
__global__ __launch_bounds__(64) void w4_quant_rows_kernel(const float* __restrict__ x, int64_t K, uint8_t* __restrict__ codes,
                                                           uint8_t* __restrict__ scales, int* __restrict__ bad) {
    const int64_t r = blockIdx.x, nks = K >> 5;
    bool fin = true;
    for (int64_t ks = threadIdx.x; ks < nks; ks += 64) {
        const uint32_t* xb = (const uint32_t*)(x + r * K + ks * 32);
        uint32_t amax = 0;                                   // |w| as bits: the order of non-negative floats, no denormal mode involved
        for (int k = 0; k < 32; k++) amax = max(amax, xb[k] & 0x7fffffffu);
        if (amax >= 0x7f800000u) { fin = false; amax = 0; }
        const int e = amax == 0 ? 0 : min(max((int)(amax >> 23) - 127 - 2, W4_E_MIN), W4_E_MAX);     // (denormal amax: field 0, clamped)
        const float inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);                      // 2^-e, a normal number
        scales[w4_scale_index(r, ks, nks)] = (uint8_t)(e + 127);
        for (int fg = 0; fg < 4; fg++) {
            uint32_t c = 0;
            for (int k = 0; k < 8; k++) {
                const uint32_t u = xb[8 * fg + k];
                const uint32_t q = fin ? w4_code(__builtin_bit_cast(float, u & 0x7fffffffu) * inv) : 0u;
                c |= (q | ((u >> 28) & 8u)) << (4 * k);
            }
            *(uint32_t*)(codes + (fm_index(r, ks * 32 + 8 * fg, K) >> 1)) = c;
        }
    }
    if (!fin) atomicOr(bad, 1);
}

// pre-quantized input in the ABI packing (codes [rows][K/2], scales [rows][K/32], nvl_upload_tensor_mxfp4) -> the device
// layout; a thread per 4 code bytes (one fragment), the first thread of a 32-block also moves its scale
__global__ __launch_bounds__(256) void w4_place_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_scales,
                                                       int64_t rows, int64_t K, uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_scales) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // fragment index, row-major: [rows][K/8]
    if (i >= rows * (K >> 3)) return;
    const int64_t r = i / (K >> 3), k = (i - r * (K >> 3)) * 8;
    *(uint32_t*)(dst + (fm_index(r, k, K) >> 1)) = *(const uint32_t*)(src + i * 4);
    if ((k & 31) == 0) dst_scales[w4_scale_index(r, k >> 5, K >> 5)] = src_scales[r * (K >> 5) + (k >> 5)];
}

// codes + scales -> W~ (bf16, the fragment-major layout): n8 fragments starting at a 16-row tile boundary
__global__ __launch_bounds__(256) void w4_dequant_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                         int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // fragment index: (block, lane)
    if (i >= n8) return;
    *(bf16x8*)(out + i * 8) = w4_frag(*(const uint32_t*)(codes + i * 4), (uint32_t)scales[(i >> 6) * 16 + (i & 15)]);
}

// MXFP4 LM head / tied embedding table (nvl_set_mx_head_dtype): the head is one more [Vpad][H] weight of
// the layout above, streamed by the same decode kernels; the two kernels below gather rows of it.
// embed_kernel<bf16_t, true> over the MXFP4 (tied) table: each gathered element is W~.  A thread takes the 8 codes of one
// fragment (4 bytes, one load) and the byte of their block; H % 32 == 0.
__global__ __launch_bounds__(256) void embed_w4_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ tok_pos,
                                                       const uint8_t* __restrict__ emb, const uint8_t* __restrict__ escales,
                                                       const bf16_t* __restrict__ pos_emb, int max_seq, float mult,
                                                       float* __restrict__ x, int H) {
    const int t = blockIdx.x;
    const int tok = tokens[t];
    const int pos = tok_pos[t];
    const bool use_pos = pos_emb && pos < max_seq;
    float* xr = x + (int64_t)t * H;
    for (int j = threadIdx.x * 8; j < H; j += 256 * 8) {
        const bf16x8 e = w4_frag(*(const uint32_t*)(emb + (fm_index(tok, j, H) >> 1)), (uint32_t)escales[w4_scale_index(tok, j >> 5, H >> 5)]);
        bf16x8 pe = {};
        if (use_pos) pe = *(const bf16x8*)(pos_emb + fm_index(pos, j, H));
        f32x4 lo, hi;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float f = (float)e[k];
            if (use_pos) f += (float)pe[k];
            if (mult != 0.f) f *= mult;
            if (k < 4) lo[k] = f; else hi[k - 4] = f;
        }
        *(f32x4*)(xr + j) = lo;
        *(f32x4*)(xr + j + 4) = hi;
    }
}

// decode_seam_kernel (elem.h) over the MXFP4 (tied) embedding table: the same launch, the gathered row is W~.  A thread
// keeps the 4 elements norm_row_finish expects of it: it loads its fragment's 4 code bytes and converts its half of them.
__global__ __launch_bounds__(256) void decode_seam_w4_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                          int chunks, const int32_t* __restrict__ sampled,
                                                          int32_t* __restrict__ hist, int64_t hist_stride,
                                                          int32_t* __restrict__ hist_len, int32_t* __restrict__ argmax_out,
                                                          int32_t* __restrict__ ring_out, const int32_t* __restrict__ ring_pos0,
                                                          int ring_rows, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ tok_pos, int32_t* __restrict__ seq_pos,
                                                          const uint8_t* __restrict__ emb, const uint8_t* __restrict__ escales, const bf16_t* __restrict__ pos_emb,
                                                          int max_seq, float mult, float* __restrict__ x,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float eps, bf16_t* __restrict__ y, int H) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    __shared__ float red[4];
    __shared__ int tok_s, pos_s;
    const int r = blockIdx.x;
    if (threadIdx.x < 64) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        if (!sampled) {
            for (int c = threadIdx.x; c < chunks; c += 64) argmax_merge(best, bi, pval[r * chunks + c], pidx[r * chunks + c]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        }
        if (threadIdx.x == 0) {
            int t = (bi == 0x7fffffff) ? 0 : bi;
            if (sampled) {                 // the token comes from sample_row_kernel; it joins the sequence's history
                t = sampled[r];
                const int n = hist_len[r];
                hist[(int64_t)r * hist_stride + n] = t;
                hist_len[r] = n + 1;
            }
            const int pos = tok_pos[r] + 1;
            // ring row = steps since the loop started (from the positions, so every step's launch has the same arguments)
            argmax_out[r] = t; ring_out[(int64_t)(pos - 1 - ring_pos0[r]) * ring_rows + r] = t; tokens[r] = t;
            tok_pos[r] = pos; seq_pos[r] = pos;          // (one token per sequence: row r IS sequence r)
            tok_s = t; pos_s = pos;
        }
    }
    __syncthreads();
    const int tok = tok_s, pos = pos_s;
    const bool use_pos = pos_emb && pos < max_seq;
    float* xr = x + (int64_t)r * H;
    const int H4 = H >> 2;
    f32x4 v[NORM_ROW_MAXCH], ww[NORM_ROW_MAXCH], bb[NORM_ROW_MAXCH];
#pragma unroll
    for (int c = 0; c < NORM_ROW_MAXCH; c++) {
        const int j = threadIdx.x + c * 256;
        v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < H4) {
            const int k8 = (j * 4) & ~7;                                                   // the fragment of this thread's 4 elements
            const uint32_t code8 = *(const uint32_t*)(emb + (fm_index(tok, k8, H) >> 1));
            const uint32_t code4 = code8 >> (16 * (j & 1));                                // its 4 codes in the low 2 bytes
            const float es = __builtin_bit_cast(float, (uint32_t)escales[w4_scale_index(tok, j >> 3, H >> 5)] << 23);
            const bf16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(code4, es, 0), hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(code4, es, 1);
            const bf16x4 e = {lo[0], lo[1], hi[0], hi[1]};                                 // W~ of the 4 gathered codes
            bf16x4 pe = {};
            if (use_pos) pe = *(const bf16x4*)(pos_emb + fm_index(pos, j * 4, H));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float f = (float)e[k];
                if (use_pos) f += (float)pe[k];
                if (mult != 0.f) f *= mult;
                v[c][k] = f;
            }
            *(f32x4*)(xr + j * 4) = v[c];
            ww[c] = *(const f32x4*)(w + j * 4);
            if (b) bb[c] = *(const f32x4*)(b + j * 4);
        }
    }
    norm_row_finish<bf16_t>(v, ww, bb, b, eps, y, r, H, red);
}

// MXFP4 MoE experts (nvl_set_mx_expert_dtype).  The down codes are stored once, in the decode form's
// layout: [H_pad][E*I/2] bytes, fragment-major with K = E*I (expert e's k-steps e*I/32 .. (e+1)*I/32 - 1 of every 16-row
// tile), the block scales [H_pad/16][E*I/32][16] over the same K.  moe_cat_down_w4_kernel builds both from the uploaded
// [E*H][I] codes and scales (moe_cat_down_w8_kernel's nibble form; H % 16 == 0: an expert starts on a tile boundary).
__global__ __launch_bounds__(256) void moe_cat_down_w4_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_scales,
                                                              uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_scales, int H, int I, int E) {
    const int nt = blockIdx.x, e = blockIdx.y, kbs = I >> 5;
    const int64_t sblk = ((int64_t)e * (H >> 4) + nt) * kbs, dblk = ((int64_t)nt * E + e) * kbs;     // first (tile, k-step) block
    const uint32_t* s4 = (const uint32_t*)(src + sblk * 256);
    uint32_t* d4 = (uint32_t*)(dst + dblk * 256);
    for (int i = threadIdx.x; i < kbs * 64; i += 256) d4[i] = s4[i];
    const uint32_t* ss = (const uint32_t*)(src_scales + sblk * 16);
    uint32_t* ds = (uint32_t*)(dst_scales + dblk * 16);
    for (int i = threadIdx.x; i < kbs * 4; i += 256) ds[i] = ss[i];
}

// the tile path's per-expert W~ of the down projection from the stored concatenated codes: out [E][H][I] bf16, fragment-major
// per expert (expert e at e*H*I: the grouped GEMMs' w_expert_stride), n8 = E*H*I/8 fragments, H % 16 == 0
__global__ __launch_bounds__(256) void e4_dequant_down_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                              int H, int I, int E, int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int64_t per_e = (int64_t)H * I / 8, kbs = I >> 5;
    const int64_t e = i / per_e, j = i - e * per_e;            // j = (tile * kbs + ks) * 64 + lane
    const int64_t lane = j & 63, blk = j >> 6, tile = blk / kbs, ks = blk - tile * kbs;
    const int64_t sblk = (tile * E + e) * kbs + ks;
    *(bf16x8*)(out + i * 8) = w4_frag(*(const uint32_t*)(codes + (sblk * 64 + lane) * 4), (uint32_t)scales[sblk * 16 + (lane & 15)]);
}

// ---- host ----
inline float w4_grid(uint8_t q) {
    static const float g[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return (q & 8) ? -g[q & 7] : g[q & 7];
}
// W~ of one code under the block scale byte E (the read-back of nvl_get_weight)
inline float w4_value(uint8_t q, uint8_t E) { return std::ldexp(w4_grid(q), (int)E - 127); }
// device layout (host copies) -> the code of element (r, k) and its block's scale byte
inline uint8_t w4_code_at(const uint8_t* codes, int64_t r, int64_t k, int64_t K) { return (codes[fm_index(r, k, K) >> 1] >> (4 * (k & 1))) & 15; }
// device layout -> the ABI packing: codes [N][K/2] (even k in the low nibble), scales [N][K/32]
inline void w4_to_abi(const uint8_t* codes, const uint8_t* scales, int64_t N, int64_t K, uint8_t* codes_out, uint8_t* scales_out) {
    for (int64_t r = 0; r < N; r++) {
        for (int64_t k = 0; k < K; k += 2) codes_out[r * (K / 2) + k / 2] = codes[fm_index(r, k, K) >> 1];
        for (int64_t ks = 0; ks < K / 32; ks++) scales_out[r * (K / 32) + ks] = scales[w4_scale_index(r, ks, K / 32)];
    }
}

}  // namespace nvl
