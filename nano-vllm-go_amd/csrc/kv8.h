// kv8.h — 8-bit (OCP e4m3fn) K/V storage: the one quantizer every K/V writer uses, the read path, and the attention
// kernels that consume an 8-bit cache.
//
// Numerics:
//   store: code = e4m3fn(x / s), round-to-nearest-even, finite values saturated to +-448 in fp32 BEFORE the conversion
//          (so overflow never depends on the converter's clamp mode), NaN -> a NaN code; x is the fp32 value, no bf16 step.
//   read:  code -> bf16 with scale 1 (exact: every e4m3 value is a bf16 value); Q and P stay bf16; k_scale multiplies the
//          fp32 scores (folded into the exp2 pre-scale sl2), v_scale the fp32 output at the final normalisation.
// Attention over an 8-bit cache is therefore bf16 attention over the dequantized cache, up to fp32 summation order.
//
// The kernels here hold only what an 8-bit cache changes — how a K / V tile reaches registers or its bf16 LDS image, and
// the two scales; the tile arithmetic, the decode tail and the prefill tile / epilogue are attn.h's, shared with the bf16 kernels:
//   decode: K fragments straight HBM -> VGPR, 16 bytes per lane = two bf16x8 MFMA fragments (the k index of K and Q is
//           permuted identically: MFMA step ks = 2 ks2 + j covers columns ks2*64 + fg*16 + j*8 .. +8); V as whole rows,
//           16 codes per lane, converted into the bf16 LDS image of attn.h and read back transposed (ds_read_b64_tr_b16).
//           The same number of tiles per round as the bf16 kernel: half the bytes (and half the registers) in flight.
//   prefill: the 8-bit K/V tiles come through registers (16 bytes per lane per tile half), are converted and written
//           into the bf16 LDS images of attn.h; the next tile's loads are in flight during the current tile's MFMAs.
#pragma once
#include "attn.h"

namespace nvl {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// ---- the quantizer: four fp32 values -> four e4m3fn codes (byte i = value i) ----
__device__ __forceinline__ float kv8_prescale(float x, float s) {
    const float y = x / s;                                     // correctly rounded division (no fast-math in this build)
    return y > 448.f ? 448.f : (y < -448.f ? -448.f : y);      // comparisons are false for NaN: NaN passes through
}
__device__ __forceinline__ uint32_t kv8_quant4(f32x4 x, float s) {
    uint32_t w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_prescale(x[0], s), kv8_prescale(x[1], s), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_prescale(x[2], s), kv8_prescale(x[3], s), w, true);
    return w;
}
// ---- the read path: four codes -> four bf16 (scale 1: exact) ----
__device__ __forceinline__ bf16x4 kv8_to_bf16x4(uint32_t w) {
    const bf16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
    const bf16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
    return bf16x4{lo[0], lo[1], hi[0], hi[1]};
}
__device__ __forceinline__ bf16x8 kv8_to_bf16x8(uint32_t w0, uint32_t w1) {
    const bf16x4 a = kv8_to_bf16x4(w0), b = kv8_to_bf16x4(w1);
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// x [n] fp32 -> codes [n] (4 per thread)
__global__ __launch_bounds__(256) void kv8_quant_kernel(const float* __restrict__ x, int64_t n, float s, uint8_t* __restrict__ codes) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        *(uint32_t*)(codes + i) = kv8_quant4(*(const f32x4*)(x + i), s);
        return;
    }
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < 4 && i + e < n; e++) v[e] = x[i + e];
    const uint32_t w = kv8_quant4(v, s);
    for (int e = 0; e < 4 && i + e < n; e++) codes[i + e] = (uint8_t)(w >> (8 * e));
}
// codes [n] -> back [n] = s * bf16(code) in fp32 (the attention kernels' read path, scale applied as they apply it)
__global__ __launch_bounds__(256) void kv8_dequant_kernel(const uint8_t* __restrict__ codes, int64_t n, float s, float* __restrict__ back) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    uint32_t w = 0;
    for (int e = 0; e < 4 && i + e < n; e++) w |= (uint32_t)codes[i + e] << (8 * e);
    const bf16x4 b = kv8_to_bf16x4(w);
    for (int e = 0; e < 4 && i + e < n; e++) back[i + e] = (float)b[e] * s;
}

// host: the value of a code (NaN for 0x7f / 0xff) — read-back of the cache (nvl_get_kv)
inline float e4m3fn_value(uint8_t c) {
    if ((c & 0x7F) == 0x7F) return NAN;
    const int e = (c >> 3) & 15, mt = c & 7;
    const float mag = e == 0 ? std::ldexp((float)mt, -9) : std::ldexp((float)(8 + mt), e - 10);
    return (c & 0x80) ? -mag : mag;
}

// The model's only 8-bit K/V writer: rope_kv_kernel's RoPE + placement (elem.h) with Q stored bf16 (row-major, the
// attention kernels' operand) and K / V stored through the shared quantizer from the fp32 values (K after RoPE).
// grid = (tokens, nH + 2 nKV), block = HD / 2: one thread per rotation pair.
__global__ void rope_kv8_kernel(const float* __restrict__ qkv, int qkv_stride, const int32_t* __restrict__ tok_pos,
                                const int32_t* __restrict__ tok_tbl, const int32_t* __restrict__ blk_table,
                                const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                bf16_t* __restrict__ q_out, int q_stride, uint8_t* __restrict__ kcache, uint8_t* __restrict__ vcache,
                                int64_t slot_stride, int Tmax, int nH, int nKV, int HD, float ksc, float vsc) {
    const int t = blockIdx.x, h = blockIdx.y;
    const int pos = tok_pos[t];
    int slot, row;
    kv_locate(blk_table, tok_tbl[t], pos, Tmax, slot, row);
    const int half = HD >> 1;
    const float* src = qkv + (int64_t)t * qkv_stride + (int64_t)h * HD;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        const float x1 = src[i], x2 = src[i + half];
        float y1 = x1, y2 = x2;
        if (h < nH + nKV && cos_t) {
            const float c1 = cos_t[(int64_t)pos * HD + i], s1 = sin_t[(int64_t)pos * HD + i];
            const float c2 = cos_t[(int64_t)pos * HD + half + i], s2 = sin_t[(int64_t)pos * HD + half + i];
            y1 = x1 * c1 + (-x2) * s1;
            y2 = x2 * c2 + x1 * s2;
        }
        if (h < nH) {
            bf16_t* d = q_out + (int64_t)t * q_stride + (int64_t)h * HD;
            d[i] = (bf16_t)y1;
            d[i + half] = (bf16_t)y2;
        } else {
            const bool is_k = h < nH + nKV;
            const int kvh = is_k ? h - nH : h - nH - nKV;
            uint8_t* d = (is_k ? kcache : vcache) + (int64_t)slot * slot_stride + ((int64_t)kvh * Tmax + row) * HD;
            const uint32_t w = kv8_quant4(f32x4{y1, y2, 0.f, 0.f}, is_k ? ksc : vsc);
            d[i] = (uint8_t)w;
            d[i + half] = (uint8_t)(w >> 8);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 8-bit decode kernel: attn_decode_bf16_kernel's non-fused form over an 8-bit cache (see the header comment).
// ------------------------------------------------------------------------------------------
template <int HD, int NW>
__global__ __launch_bounds__(NW * 64) void attn_decode_kv8_kernel(const int32_t* __restrict__ a_seq_pos, const int32_t* __restrict__ a_blk_table,
                                                                  int a_tbl_stride, int a_bs_shift, int a_Tmax, int a_group, AttnArgs p,
                                                                  float ksc, float vsc) {
    constexpr int KS = HD / 32, DT = HD / 16;
    constexpr int CPR8 = HD / 16, KPI8 = 64 / CPR8, NVL8 = 64 / KPI8;     // 16-code chunks per row, rows per load, loads per tile
    constexpr int NT2 = HD <= 64 ? 2 : 1;
    constexpr int TILE_BYTES = 64 * HD * 2;                               // the bf16 LDS image
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red_m[NW][16];
    __shared__ float red_l[NW][16];
    const int QT = (a_group + 15) >> 4;
    const int seq = blockIdx.y, kvh = blockIdx.x / QT, qt = blockIdx.x - kvh * QT;
    const int32_t* tbl = a_blk_table + (int64_t)seq * a_tbl_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = seq, pos0 = a_seq_pos[seq];
    const int fq = lane & 15, fg = lane >> 4;
    const int dch8 = lane % CPR8, ksub8 = lane / CPR8;
    const bool row_ok = qt * 16 + fq < p.group;
    const int head = kvh * p.group + (row_ok ? qt * 16 + fq : 0);
    char* vimg = smem + wave * TILE_BYTES;
    const int n_kt = pos0 / 64 + 1;
    const int vw = blockIdx.z * NW + wave, nvw = NW * gridDim.z;
    f32x4 o[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float sl2 = p.scale * ksc * 1.4426950408889634f;
    int v_off[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) v_off[d] = attn_v_off<HD>(fq, fg, d);
    // Q in the permuted k order of the 16-byte K loads
    bf16x8 qf[KS];
    {
        const bf16_t* qp = (const bf16_t*)p.q + (int64_t)tok * p.q_stride + head * HD;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) qf[ks] = *(const bf16x8*)(qp + (ks >> 1) * 64 + fg * 16 + (ks & 1) * 8);
    }
    u32x4 kraw[NT2][4][KS / 2];
    u32x4 vraw[NT2][NVL8];
    auto issue_round_t = [&](int kt0, auto nt_tag) {
        constexpr bool NT = decltype(nt_tag)::value;
#pragma unroll
        for (int h = 0; h < NT2; h++) {
            const int kt = kt0 + h * nvw;
            if (kt >= n_kt) continue;
            const int bi = kv_block_index(p, kt * 64), krow0 = kt * 64 - bi * p.Tmax;
            const int blk = tbl[bi];
            const int64_t blk_off = (int64_t)blk * p.slot_stride + ((int64_t)kvh * p.Tmax + krow0) * HD;   // (bytes = elements)
            const uint8_t* kbase = (const uint8_t*)p.kcache + blk_off;
            const uint8_t* vbase = (const uint8_t*)p.vcache + blk_off;
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int k2 = 0; k2 < KS / 2; k2++) {
                    const u32x4* src = (const u32x4*)(kbase + (int64_t)(t * 16 + fq) * HD + k2 * 64 + fg * 16);
                    if constexpr (NT) kraw[h][t][k2] = __builtin_nontemporal_load(src); else kraw[h][t][k2] = *src;
                }
#pragma unroll
            for (int i = 0; i < NVL8; i++) {                                                   // 1 KiB, contiguous
                const u32x4* src = (const u32x4*)(vbase + (int64_t)lane * 16 + i * 1024);
                if constexpr (NT) vraw[h][i] = __builtin_nontemporal_load(src); else vraw[h][i] = *src;
            }
        }
    };
    auto issue_round = [&](int kt0) {
        if (p.kv_nt) issue_round_t(kt0, std::true_type{}); else issue_round_t(kt0, std::false_type{});
    };
    auto do_round = [&](int kt0) __attribute__((always_inline)) {
        f32x4 s[NT2][4];
        float tmax = -INFINITY;
#pragma unroll
        for (int h = 0; h < NT2; h++) {
            const int kt = kt0 + h * nvw;
            if (kt >= n_kt) {
#pragma unroll
                for (int t = 0; t < 4; t++) s[h][t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                continue;
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k2 = 0; k2 < KS / 2; k2++) {
                    const u32x4 w = kraw[h][t][k2];
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kv8_to_bf16x8(w[0], w[1]), qf[2 * k2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kv8_to_bf16x8(w[2], w[3]), qf[2 * k2 + 1], acc, 0, 0, 0);
                }
                const int lim = pos0 - kt * 64 - fg * 4;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[r] * sl2;
                    v = (t * 16 + r <= lim) ? v : -INFINITY;
                    acc[r] = v;
                    tmax = fmaxf(tmax, v);
                }
                s[h][t] = acc;
            }
        }
        attn_decode_softmax<HD, NT2>(s, tmax, m_run, l_run, o);
#pragma unroll
        for (int h = 0; h < NT2; h++) {
            if (kt0 + h * nvw >= n_kt) continue;
#pragma unroll
            for (int i = 0; i < NVL8; i++) {          // 16 codes of row i*KPI8 + ksub8 -> bf16 chunks 2 dch8, 2 dch8 + 1
                const int row = i * KPI8 + ksub8;
                const u32x4 w = vraw[h][i];
                *(bf16x8*)(vimg + 16 * kv_img_chunk<HD>(row, 2 * dch8)) = kv8_to_bf16x8(w[0], w[1]);
                *(bf16x8*)(vimg + 16 * kv_img_chunk<HD>(row, 2 * dch8 + 1)) = kv8_to_bf16x8(w[2], w[3]);
            }
            attn_pv_tile<HD, 1, false>(vimg, v_off, &s[h], &o, nullptr);
        }
    };
    for (int kt0 = vw; kt0 < n_kt; kt0 += NT2 * nvw) {
        issue_round(kt0);
        do_round(kt0);
    }
    NvlStampsT<false> stamps(nullptr, 0);
    attn_decode_finish<HD, NW>(p, smem, vimg, red_m, red_l, o, m_run, l_run, seq, tok, head, row_ok, wave, lane, fq, fg, vsc, stamps);
}

// ------------------------------------------------------------------------------------------
// 8-bit prefill kernel: attn_prefill_bf16_kernel's tiling (8 waves, 256 query rows, two 16-row sub-tiles per wave) over
// an 8-bit cache.  A K+V tile pair is 2 * 64 * HD codes = HD / 64 16-byte pieces per thread; they are loaded into
// registers one tile ahead, converted, and written into ONE bf16 [K image | V image] (two barriers per tile).
// ------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(512, HD == 64 ? 4 : 2) void attn_prefill_kv8_kernel(AttnArgs p, float ksc, float vsc) {
    constexpr int KS = HD / 32, DT = HD / 16, CPR8 = HD / 16, TQ = PF_TQ, QROWS = PF_QROWS;
    constexpr int TILE_BYTES = 64 * HD * 2, CH = 64 * CPR8, NCH = 2 * CH / 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [K image | V image] (bf16)
    const int seq = blockIdx.y, kvh = blockIdx.x, qt = gridDim.z - 1 - blockIdx.z;
    const int S = p.seq_len[seq];
    const int R = S * p.group;
    if (qt * QROWS >= R) return;
    const int tok0 = p.seq_tok_start[seq], pos0 = p.seq_pos[seq];
    const int32_t* tbl = p.blk_table + (int64_t)seq * p.tbl_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fq = lane & 15, fg = lane >> 4;

    const AttnPrefillRows w{qt, wave, fq, fg, R, tok0, pos0, kvh};
    bf16x8 qf[TQ][KS];
    int qpos[TQ];
    attn_prefill_load_q<HD>(p, w, qf, qpos);
    int n_kt, wave_n_kt, wave_first_limit;
    attn_prefill_setup(p, w, n_kt, wave_n_kt, wave_first_limit);

    // this thread's pieces: piece g = tid + j * 512 of the [K pieces | V pieces] list; piece = 16 codes of one row
    int src_off[NCH], dst_off[NCH];
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        const int g = tid + j * 512, idx = g % CH, row = idx / CPR8, c8 = idx % CPR8;
        src_off[j] = row * HD + c8 * 16;
        dst_off[j] = (g >= CH ? TILE_BYTES : 0) + 16 * kv_img_chunk<HD>(row, 2 * c8);
    }
    u32x4 raw[NCH];
    auto load_tile = [&](int kt) {
        const int bi = kv_block_index(p, kt * 64), krow0 = kt * 64 - bi * p.Tmax;
        const int64_t blk_off = (int64_t)tbl[bi] * p.slot_stride + ((int64_t)kvh * p.Tmax + krow0) * HD;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            const uint8_t* base = (const uint8_t*)(tid + j * 512 >= CH ? p.vcache : p.kcache) + blk_off;
            raw[j] = *(const u32x4*)(base + src_off[j]);
        }
    };
    int k_off[KS], v_off[DT];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) k_off[ks] = attn_k_off<HD>(fq, fg, ks);
#pragma unroll
    for (int d = 0; d < DT; d++) v_off[d] = attn_v_off<HD>(fq, fg, d);
    f32x4 o[TQ][DT];
    f32x4 lacc[TQ];
    float m_run[TQ];
#pragma unroll
    for (int qi = 0; qi < TQ; qi++) {       // (as a loop, not "= {}": that form costs the hd-64 kernel 5 registers)
        m_run[qi] = -INFINITY;
        lacc[qi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < DT; d++) o[qi][d] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float sl2 = p.scale * ksc * 1.4426950408889634f;
    const char* kimg = smem;
    const char* vimg = smem + TILE_BYTES;

    load_tile(0);
    for (int kt = 0; kt < n_kt; kt++) {
        __syncthreads();                                 // every wave is done reading the previous tile's images
        // (the row offset of chunk 2 c8 + 1 in the image: kv_img_chunk flips only bit 0 between the pair)
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            *(bf16x8*)(smem + dst_off[j]) = kv8_to_bf16x8(raw[j][0], raw[j][1]);
            *(bf16x8*)(smem + (dst_off[j] ^ 16)) = kv8_to_bf16x8(raw[j][2], raw[j][3]);
        }
        if (kt + 1 < n_kt) load_tile(kt + 1);            // in flight during this tile's MFMAs
        __syncthreads();
        if (kt >= wave_n_kt) continue;
        attn_prefill_tile<HD>(fg, qpos, kt, wave_first_limit, sl2, kimg, vimg, k_off, v_off, qf, o, lacc, m_run);
    }
    attn_prefill_store<HD>(p, w, o, lacc, vsc);
}
template <int HD> constexpr int attn_prefill_kv8_lds_bytes() { return 2 * 64 * HD * 2; }

}  // namespace nvl
