// qknorm.h — per-head QK RMSNorm (HF Qwen3Attention: q_norm / k_norm over the head dimension, after the projection and its
// bias, before RoPE).  For token row t and every Q head and K head, x [hd] fp32:
//     y[d] = x[d] * (1 / sqrt(mean_d(x[d]^2) + eps)) * w[d]        w = q_norm_w (Q heads) / k_norm_w (K heads), [hd], fp32
// then RoPE on y; V is untouched.  Three places apply it, all through common.h's qk_norm_scale:
//   qk_norm_rope_kv_kernel (here)          the store forms: fp32 QKV rows -> Q operand rows + K / V cache rows
//   epilogue_qkv_head<TH, true> (gemm.h)   the EPI_QKV tile epilogue
//   attn_decode_bf16_kernel<128, .., QKNORM = true> (attn.h)   the fused decode prologue
#pragma once
#include "kv8.h"

namespace nvl {

// one DPP step of a butterfly: v + (v of the lane the control word names).  Every lane of the row is active at the calls.
template <int CTRL>
__device__ __forceinline__ float qk_dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false);
    return v + __builtin_bit_cast(float, o);
}
// sum over the LPH = 8 or 16 adjacent lanes of one head (aligned groups inside a 16-lane DPP row): quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, (16: row_mirror).  After each step the lanes that were combined hold equal sums,
// so a mirror reaches the other half's total.  All lanes end with the same value, summed in the same order.
// LPH = 32 (hd 256: two heads per wave, a head = two adjacent DPP rows): one step more across the row pair, both rows'
// totals exchanged by v_permlane16_swap (rows 0 <-> 1 and 2 <-> 3 trade places) and added: commutative, so still one value
// and one order for all 32 lanes.
template <int LPH>
__device__ __forceinline__ float qk_head_sum(float v) {
    static_assert(LPH == 8 || LPH == 16 || LPH == 32, "a head spans 8, 16 or 32 lanes");
    v = qk_dpp_add<0xB1>(v);
    v = qk_dpp_add<0x4E>(v);
    v = qk_dpp_add<0x141>(v);
    if constexpr (LPH >= 16) v = qk_dpp_add<0x140>(v);
    if constexpr (LPH == 32) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    return v;
}

__device__ __forceinline__ void qk_store4(float* d, f32x4 v) { *(f32x4*)d = v; }
__device__ __forceinline__ void qk_store4(bf16_t* d, f32x4 v) { *(bf16x4*)d = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]}; }

// ---------------------------------------------------------------------------------------
// The store forms' second launch for a QK-norm layer: rope_kv_kernel / rope_kv8_kernel with the norm in front of the rotation.
// Those give a (token, head) a block of hd/2 threads, one rotation pair each: no cheap place for a sum over the head.
// Here the unit is the wave.  A lane owns d0 .. d0+3 and d0 + hd/2 .. +3 of ONE head (d0 = 4 * (lane % LPH), LPH = hd/8):
// two 16-byte fp32 loads; the eight values are both its terms of the head's sum of squares and four whole RoPE pairs, so the
// rotation needs nothing from another lane, and the sum is a DPP butterfly over the head's LPH lanes — no LDS, no barrier.
// A wave covers 64 / LPH = 8 (hd 64) or 4 (hd 128) consecutive heads of one token; the heads of a token [Q | K | V] are dealt
// to ceil((nH + 2 nKV) / HPW) waves, the last of which may be partly filled: its spare lanes load nothing (zeros), take
// part in the butterfly (whose groups never mix heads) and store nothing.  V heads ride along as converts / quantizes.
// Stores: 16 bytes (f32), 8 bytes (bf16) or 4 bytes (e4m3 codes, the cache's own quantizer) per lane and half.
// grid = ceil(tokens * waves_per_token / 4) blocks of 256 threads.
// ---------------------------------------------------------------------------------------
template <typename ActT, int HD, bool KV8>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_kernel(const float* __restrict__ qkv, int qkv_stride, int tokens,
                                                              const int32_t* __restrict__ tok_pos, const int32_t* __restrict__ tok_tbl,
                                                              const int32_t* __restrict__ blk_table,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              const float* __restrict__ q_norm_w, const float* __restrict__ k_norm_w, float eps,
                                                              ActT* __restrict__ q_out, int q_stride, void* __restrict__ kcache, void* __restrict__ vcache,
                                                              int64_t slot_stride, int Tmax, int nH, int nKV, float ksc, float vsc) {
    constexpr int LPH = HD / 8, HPW = 64 / LPH, HALF = HD / 2;
    static_assert(!KV8 || sizeof(ActT) == 2, "the 8-bit cache is bf16-only");
    using CacheT = std::conditional_t<KV8, uint8_t, ActT>;
    const int n_heads = nH + 2 * nKV, wpt = (n_heads + HPW - 1) / HPW;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (w >= tokens * wpt) return;                        // (whole waves: every lane of a running wave reaches the butterfly)
    const int t = w / wpt, lane = threadIdx.x & 63;
    const int h = (w - t * wpt) * HPW + lane / LPH, d0 = 4 * (lane % LPH);
    const bool live = h < n_heads, normed = h < nH + nKV;
    const int pos = tok_pos[t];
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
    if (live) {
        const float* src = qkv + (int64_t)t * qkv_stride + (int64_t)h * HD + d0;
        a = *(const f32x4*)src; b = *(const f32x4*)(src + HALF);
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) ss = __builtin_fmaf(a[e], a[e], ss);
#pragma unroll
    for (int e = 0; e < 4; e++) ss = __builtin_fmaf(b[e], b[e], ss);
    ss = qk_head_sum<LPH>(ss);
    if (!live) return;
    if (normed) {
        const float* wn = (h < nH ? q_norm_w : k_norm_w) + d0;
        const float r = qk_norm_scale<HD>(ss, eps);
        a = (a * r) * *(const f32x4*)wn;
        b = (b * r) * *(const f32x4*)(wn + HALF);
        if (cos_t) {                                      // rope.go:196-202; the table's halves are duplicates (gemm.h, attn.h)
            const f32x4 c = *(const f32x4*)(cos_t + (int64_t)pos * HD + d0), s = *(const f32x4*)(sin_t + (int64_t)pos * HD + d0);
            f32x4 lo, hi;
#pragma unroll
            for (int e = 0; e < 4; e++) {                 // the rounding order of attn.h rope_math8: every route rounds alike
                lo[e] = __builtin_fmaf(a[e], c[e], -(b[e] * s[e]));
                hi[e] = __builtin_fmaf(b[e], c[e], a[e] * s[e]);
            }
            a = lo; b = hi;
        }
    }
    if (h < nH) {
        ActT* d = q_out + (int64_t)t * q_stride + (int64_t)h * HD + d0;
        qk_store4(d, a); qk_store4(d + HALF, b);
        return;
    }
    int slot, row;
    kv_locate(blk_table, tok_tbl[t], pos, Tmax, slot, row);
    const bool is_k = h < nH + nKV;
    const int kvh = is_k ? h - nH : h - nH - nKV;
    CacheT* d = (CacheT*)(is_k ? kcache : vcache) + (int64_t)slot * slot_stride + ((int64_t)kvh * Tmax + row) * HD + d0;
    if constexpr (KV8) {
        const float sc = is_k ? ksc : vsc;
        *(uint32_t*)d = kv8_quant4(a, sc);
        *(uint32_t*)(d + HALF) = kv8_quant4(b, sc);
    } else {
        qk_store4(d, a); qk_store4(d + HALF, b);
    }
}

}  // namespace nvl
