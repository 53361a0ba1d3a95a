// w8.h — 8-bit (OCP e4m3fn) projection weights with one fp32 scale per output row (nvl_set_weight_dtype, DESIGN.md §3 and
// §9 f-6): the quantizer every upload uses, the dequantize kernel of the tile path, the embedding gather of a quantized
// tied table.  The host side shared with MXFP4 (format table, GEMM dispatch) is wq.h.
//
// Numerics: s_n = amax_n / 448 (1 when the row is all zeros), q = e4m3fn_rne(w / s_n) through kv8.h's quantizer; the model
// computes with W~ = bf16_rne(s_n * e4m3(q)) (fp32 product, one rounding), on every path:
//   decode (every call the bf16 dispatch sends to the weight-streaming kernels): gemm_skinny_fp8w_kernel /
//       gemm_skinny_wide_fp8w_kernel, the bf16 kernels' bodies with the weight fragment built from 8 codes per lane
//       (gemm.h w8_frag) — the same launch decisions, deferred RMSNorm, K split and 64-row groups as in bf16 mode;
//   everything else (prefill, the tile and ping-pong kernels): w8_dequant_kernel writes W~ in the bf16 fragment-major
//       layout into one scratch buffer and the unchanged bf16 GEMM runs on it; an LM head larger than the scratch runs in
//       row chunks that fit.
// Storage: the codes in the bf16 fragment-major order, one byte per element ([rows_pad][K] bytes), scales [rows_pad]
// (pad rows: codes 0, scale 1).
// MoE experts (nvl_set_expert_dtype, §9 f-8): the same contract with one scale per (expert, output row).  Decode streams the
// codes through gemm_skinny_moe_fp8w_kernel / gemm_skinny_wide_moe_fp8w_kernel; every other MoE launch runs the unchanged
// grouped GEMMs on one layer's W~, dequantized (up, then down) into a scratch buffer.
#pragma once
#include "kv8.h"
#include "gemm.h"

namespace nvl {

// x fp32 row-major [rows][K] -> codes (fragment-major bytes) + scale[row]; one 256-thread block per row.
// Any non-finite element sets *bad (the upload is refused).
__global__ __launch_bounds__(256) void w8_quant_rows_kernel(const float* __restrict__ x, int64_t K, uint8_t* __restrict__ codes,
                                                            float* __restrict__ scale, int* __restrict__ bad) {
    __shared__ float red[4];
    __shared__ int nonfin;
    const int64_t r = blockIdx.x;
    const float* xr = x + r * K;
    if (threadIdx.x == 0) nonfin = 0;
    __syncthreads();
    float amax = 0.f;
    bool fin = true;
    for (int64_t k = threadIdx.x; k < K; k += 256) {
        const float v = fabsf(xr[k]);
        if (!(v <= 3.402823466e38f)) fin = false;
        amax = fmaxf(amax, v);
    }
    if (!fin) nonfin = 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = (nonfin || amax == 0.f) ? 1.0f : amax / 448.f;
    if (threadIdx.x == 0) {
        scale[r] = s;
        if (nonfin) atomicOr(bad, 1);
    }
    for (int64_t k = (int64_t)threadIdx.x * 4; k < K; k += 1024)     // K % 32 == 0: 4 consecutive k are 4 consecutive bytes
        *(uint32_t*)(codes + fm_index(r, k, K)) = kv8_quant4(*(const f32x4*)(xr + k), s);
}

// pre-quantized codes, row-major [rows][K] -> the fragment-major byte layout (nvl_upload_tensor_fp8); 4 codes per thread
__global__ __launch_bounds__(256) void w8_place_kernel(const uint8_t* __restrict__ src, int64_t rows, int64_t K, uint8_t* __restrict__ dst) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * K) return;
    const int64_t r = i / K, k = i - r * K;
    *(uint32_t*)(dst + fm_index(r, k, K)) = *(const uint32_t*)(src + i);
}

// codes -> W~ (bf16, the same fragment-major layout): n8 groups of 8 codes starting at a 16-row tile boundary
__global__ __launch_bounds__(256) void w8_dequant_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale,
                                                         int64_t K, int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int64_t e = i * 8;
    const int64_t row = (e / (16 * K)) * 16 + ((e >> 3) & 15);
    *(bf16x8*)(out + e) = w8_frag(*(const u32x2*)(codes + e), scale[row]);
}

// embed_kernel<bf16_t, true> over a quantized (tied) table: each gathered element is W~
__global__ void embed_w8_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ tok_pos,
                                const uint8_t* __restrict__ emb, const float* __restrict__ escale, const bf16_t* __restrict__ pos_emb,
                                int max_seq, float mult, float* __restrict__ x, int H) {
    const int t = blockIdx.x;
    const int tok = tokens[t];
    const int pos = tok_pos[t];
    const bool use_pos = pos_emb && pos < max_seq;
    const float s = escale[tok];
    float* xr = x + (int64_t)t * H;
    for (int j = threadIdx.x; j < H; j += blockDim.x) {
        const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)emb[fm_index(tok, j, H)], false);
        float v = (float)(__bf16)(c[0] * s);
        if (use_pos) v += (float)pos_emb[fm_index(pos, j, H)];
        if (mult != 0.f) v *= mult;
        xr[j] = v;
    }
}

// decode_seam_kernel (elem.h) over a quantized (tied) embedding table: the same launch, the gathered row is W~
__global__ __launch_bounds__(256) void decode_seam_w8_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                          int chunks, const int32_t* __restrict__ sampled,
                                                          int32_t* __restrict__ hist, int64_t hist_stride,
                                                          int32_t* __restrict__ hist_len, int32_t* __restrict__ argmax_out,
                                                          int32_t* __restrict__ ring_out, const int32_t* __restrict__ ring_pos0,
                                                          int ring_rows, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ tok_pos, int32_t* __restrict__ seq_pos,
                                                          const uint8_t* __restrict__ emb, const float* __restrict__ escale, const bf16_t* __restrict__ pos_emb,
                                                          int max_seq, float mult, float* __restrict__ x,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float eps, bf16_t* __restrict__ y, int H) {
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
            const uint32_t code4 = *(const uint32_t*)(emb + fm_index(tok, j * 4, H));      // W~ of the 4 gathered codes
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)code4, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)code4, true);
            const float es = escale[tok];
            const bf16x4 e = {(__bf16)(lo[0] * es), (__bf16)(lo[1] * es), (__bf16)(hi[0] * es), (__bf16)(hi[1] * es)};
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

// 8-bit MoE experts (nvl_set_expert_dtype).  The down codes are stored once, in the decode form's layout:
// [H_pad][E*I] bytes, fragment-major with K = E*I (expert e's k-steps e*I/32 .. (e+1)*I/32 - 1 of every 16-row tile), scales
// [E][H_pad].  moe_cat_down_w8_kernel builds it from the uploaded [E*H][I] codes (moe_cat_down_kernel's byte form).
__global__ __launch_bounds__(256) void moe_cat_down_w8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int I, int E) {
    const int nt = blockIdx.x, e = blockIdx.y, kbs = I >> 5;
    const u32x2* s8 = (const u32x2*)(src + ((int64_t)e * H * I + (int64_t)nt * kbs * 512));
    u32x2* d8 = (u32x2*)(dst + ((int64_t)nt * E * kbs + (int64_t)e * kbs) * 512);
    for (int i = threadIdx.x; i < kbs * 64; i += 256) d8[i] = s8[i];
}

// the tile path's per-expert W~ of the down projection from the stored [H_pad][E*I] codes: out [E][H][I] bf16, fragment-major
// per expert (expert e at e*H*I: the grouped GEMMs' w_expert_stride), n8 = E*H*I/8 groups of 8 elements, H % 16 == 0
__global__ __launch_bounds__(256) void e8_dequant_down_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale,
                                                              int H, int I, int E, int64_t hp, int64_t n8, bf16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int64_t per_e = (int64_t)H * I / 8, kbs = I >> 5;
    const int64_t e = i / per_e, j = i - e * per_e;            // j = (tile * kbs + ks) * 64 + lane
    const int64_t lane = j & 63, blk = j >> 6, tile = blk / kbs, ks = blk - tile * kbs;
    const int64_t src = ((tile * E * kbs + e * kbs + ks) * 64 + lane) * 8;
    *(bf16x8*)(out + i * 8) = w8_frag(*(const u32x2*)(codes + src), scale[e * hp + tile * 16 + (lane & 15)]);
}

// host: W~ of one code (the read-back of nvl_get_weight)
inline float w8_value(uint8_t c, float s) {
    const float p = s * e4m3fn_value(c);
    uint32_t u;
    memcpy(&u, &p, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;     // RNE to bf16 (p is finite)
    float v;
    memcpy(&v, &u, 4);
    return v;
}

}  // namespace nvl
