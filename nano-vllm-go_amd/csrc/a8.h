// a8.h — 8-bit (OCP e4m3fn) activations on top of 8-bit weights (nvl_set_act_dtype NVL_ACT_FP8_E4M3, DESIGN.md §3 and
// §9 f-7): the W8A8 form of every projection that w8.h would run as dequantize + tile.
//
// Numerics, per launch that reaches the tile step of launch_gemm_q (wq.h):
//   activation rows: s_a[m] = amax_m / 448 (fp32 division; 1 for an all-zero row), q_a = e4m3fn_rne(a / s_a) through kv8.h's
//       quantizer (fp32 division, saturated to +-448, NaN -> a NaN code; NaN elements do not enter amax_m, an infinite one
//       makes s_a[m] infinite and the row's outputs NaN).  a is the bf16 operand the bf16 GEMM would read, exact in fp32.
//   product: acc = sum_k e4m3(q_a) * e4m3(q_w) in the fp32 accumulator of v_mfma_scale_f32_32x32x64_f8f6f4 with both E8M0
//       block scales fixed at 2^0 (127); y = (acc * s_a[m]) * s_w[n] in fp32, then the unchanged epilogue (bias, residual,
//       SwiGLU, GELU, QKV + RoPE + K/V placement, the fp32 split-K partials: each slice's partial is scaled the same way).
//   The weight operand is the raw codes and fp32 row scales of w8.h, not W~.
// Decode-form launches (the weight-streaming kernels, the 64-row groups, the short-prefill QKV groups) keep bf16 activations
// and W~ (W8A16): a token's projections are W8A8 when it is part of a tile-step launch and W8A16 otherwise.
//
// Layout: the activation codes are written in the weights' fragment-major byte order (fm_index over bytes: 16-row x 32-k
// blocks of 512 B), so one 1-KiB LDS-DMA wave-instruction moves one 16-row tile over 64 k for either operand.  For the
// 32x32x64 MFMA a lane (row r = lane & 31, half h = lane >> 5) takes the four 8-byte pieces of its row in 32-k block h of
// the 64-k stage: byte 8g + j of its fragment is k = 32h + 8g + j.  The permutation is the same for both operands, so the
// sum over k is unchanged.  The odd 16-row tile of every 32-row pair is stored with its 128-byte halves of each 256 B
// swapped (the DMA source address of lane L is unit L ^ 8), which makes the fragment ds_read_b64s conflict-free.
#pragma once
#include "kv8.h"
#include "gemm.h"

namespace nvl {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// bf16 fragment-major operand A (row-tile stride 16 * lda elements) -> codes [M_pad16][K] (fragment-major bytes) + scale
// [M_pad16]; rows M .. M_pad16-1 get codes 0 and scale 1.  One 256-thread workgroup per 16-row tile: lane l of every wave
// holds row l & 15, each wave walks every fourth 32-k block.
__global__ __launch_bounds__(256) void a8_quant_kernel(const bf16_t* __restrict__ A, int64_t lda, int M, int64_t K,
                                                       uint8_t* __restrict__ codes, float* __restrict__ scale) {
    __shared__ float red[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    const int row = (int)(tile * 16) + (lane & 15);
    const bool live = row < M;
    const int nb = (int)(K >> 5);
    const bf16x8* src = (const bf16x8*)(A + tile * 16 * lda) + lane;        // 32-k block kb: + 64 * kb
    u32x2* dst = (u32x2*)(codes + tile * 16 * K) + lane;
    float amax = 0.f;
    if (live) {
#pragma unroll 4
        for (int kb = wave; kb < nb; kb += 4) {
            const bf16x8 v = src[(int64_t)kb * 64];
#pragma unroll
            for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf((float)v[j]));
        }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    if (lane < 16) red[wave][lane] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0][lane & 15], red[1][lane & 15]), fmaxf(red[2][lane & 15], red[3][lane & 15]));
    const float s = amax == 0.f ? 1.0f : amax / 448.f;
    if (wave == 0 && lane < 16) scale[row] = s;
#pragma unroll 4
    for (int kb = wave; kb < nb; kb += 4) {
        bf16x8 v = {};
        if (live) v = src[(int64_t)kb * 64];
        const f32x4 lo = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, hi = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
        dst[(int64_t)kb * 64] = u32x2{kv8_quant4(lo, s), kv8_quant4(hi, s)};
    }
}

// ------------------------------------------------------------------------------------------
// W8A8 GEMM, ping-pong form: the schedule of gemm_bf16_pp_kernel (gemm.h) — two groups of four waves one phase apart, a
// 4-slot LDS ring filled by global_load_lds_dwordx4, one stage per phase — with 64-k stages of e4m3 codes and the scaled
// 32x32x64 MFMA (the fp8 rate: twice the bf16 FLOP per clock).  A stage is one 16-row x 64-k KiB per row tile, exactly the
// bf16 kernel's 32-k stage in bytes, so K % 64 == 0 needs no tail.  Instances:
//   <256, 256, 4>  wave tile 128x64 (a head of 64 per wave), <256, 256, 2> 64x128 (a head of 128): >= 192 tiles;
//   <128, 128, 2>  wave tile 32x64, two workgroups per CU, <128, 256, 2> 32x128 (QKV, head 128): fewer tiles and the K-split
//                  residual form (GemmArgs::sk_part, gridDim.y slices).
// ------------------------------------------------------------------------------------------
#define A8_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

template <int EPI, typename OutT, int BM, int BN, int WAVES_N>
__global__ __launch_bounds__(512, (BM + BN) <= 256 ? 2 : 1) void gemm_w8a8_pp_kernel(GemmArgs p, const float* __restrict__ a_scale,
                                                                                     const float* __restrict__ w_scale) {
    constexpr int STAGES = 4;
    constexpr int WAVES_M = 8 / WAVES_N, TM = BM / WAVES_M / 32, TN = BN / WAVES_N / 32;   // 32x32 accumulator tiles per wave
    constexpr int NA = BM / 16, NB = BN / 16;            // 1-KiB blocks (16 rows x 64 k) per stage
    constexpr int PW = (NA + NB) / 8;                    // blocks per wave per stage: 4, 3 or 2
    constexpr int STAGE_BYTES = (NA + NB) * 1024;
    static_assert(TM >= 1 && TN >= 1 && TM * WAVES_M * 32 == BM && TN * WAVES_N * 32 == BN, "wave tiles of whole 32x32 MFMAs");
    static_assert((NA + NB) % 8 == 0 && PW >= 2 && PW <= 4, "stage blocks must divide over the 8 waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_n = (p.N + BN - 1) / BN;
    int tm, tn;
    tile_coords(xcd_remap(blockIdx.x, gridDim.x), gridDim.x / tiles_n, tiles_n, 4, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int grp = wave >> 2;
    if (m0 >= p.M) return;

    // ---- staging sources: block i of wave w is row tile w*PW+i of the stage's [A tiles | W tiles]; the odd tile of a
    // 32-row pair fetches unit lane ^ 8 (the swizzle of the header comment).  A tiles past the last live one re-read it.
    const uint8_t* src[PW];
    const int last_at = (p.M - 1) >> 4;
#pragma unroll
    for (int i = 0; i < PW; i++) {
        const int blk = wave * PW + i;
        const int unit = (blk & 1) ? (lane ^ 8) : lane;
        if (blk < NA) {
            const int at = min((m0 >> 4) + blk, last_at);
            src[i] = (const uint8_t*)p.A + (int64_t)at * 16 * p.K + unit * 16;
        } else {
            src[i] = (const uint8_t*)p.W + (int64_t)((n0 >> 4) + blk - NA) * 16 * p.K + unit * 16;
        }
    }
    auto stage = [&](int buf, int ks) {
        char* base = smem + buf * STAGE_BYTES + wave * (PW * 1024);
#pragma unroll
        for (int i = 0; i < PW; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + (int64_t)ks * 1024),
                                             (__attribute__((address_space(3))) void*)(base + i * 1024), 16, 0, 0);
    };
    auto wait_younger = [&](int younger) {              // (s_waitcnt needs an immediate)
        if (younger > STAGES - 2) younger = STAGES - 2;
        if (younger >= 2) {
            if (PW == 4) A8_VMCNT(8); else if (PW == 3) A8_VMCNT(6); else A8_VMCNT(4);
        } else if (younger == 1) {
            if (PW == 4) A8_VMCNT(4); else if (PW == 3) A8_VMCNT(3); else A8_VMCNT(2);
        } else {
            A8_VMCNT(0);
        }
    };
    // fragment reads: lane (r = lane & 31, h = lane >> 5) reads piece g of its row at tile_base + 512 h + 8 (r & 15) +
    // 128 (g ^ o), o = r >> 4 (the odd tile's swizzle): even pieces from pe, odd ones from po, + 256 (g >> 1)
    const int r = lane & 31, o = r >> 4;
    const int lb = (lane >> 5) * 512 + (r & 15) * 8 + o * 1024;
    const int pe = lb + 128 * o, po = lb + 128 * (1 - o);
    const int a_off = wm * TM * 2048;
    const int w_off = NA * 1024 + wn * TN * 2048;
    auto frag = [&](const char* t) {
        const u32x2 g0 = *(const u32x2*)(t + pe), g1 = *(const u32x2*)(t + po);
        const u32x2 g2 = *(const u32x2*)(t + pe + 256), g3 = *(const u32x2*)(t + po + 256);
        return i32x8{(int)g0[0], (int)g0[1], (int)g1[0], (int)g1[1], (int)g2[0], (int)g2[1], (int)g3[0], (int)g3[1]};
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

    // K split over gridDim.y (EPI_RESID with sk_part only): slice y takes stages [kt0, kt0 + nt)
    const int nt_all = p.K >> 6;
    int nt = nt_all, kt0 = 0;
    if (EPI == EPI_RESID && p.sk_part) {
        const int per = nt_all / (int)gridDim.y, extra = nt_all - per * (int)gridDim.y;
        kt0 = (int)blockIdx.y * per + ((int)blockIdx.y < extra ? (int)blockIdx.y : extra);
        nt = per + ((int)blockIdx.y < extra ? 1 : 0);
    }
#pragma unroll
    for (int s = 0; s < STAGES - 1; s++)
        if (s < nt) stage(s, kt0 + s);
    wait_younger((nt < STAGES - 1 ? nt : STAGES - 1) - 1);
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();          // the late group: one phase behind from here on
    int buf = 0;
    for (int s = 0; s < nt; s++) {
        // ---- L phase ----
        i32x8 af[TM], wf[TN];
        const char* sbuf = smem + buf * STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < TN; j++) wf[j] = frag(sbuf + w_off + j * 2048);
#pragma unroll
        for (int i = 0; i < TM; i++) af[i] = frag(sbuf + a_off + i * 2048);
        if (s + STAGES - 1 < nt) {
            int nb = buf + STAGES - 1;                    // the slot read in phase s-1
            if (nb >= STAGES) nb -= STAGES;
            stage(nb, kt0 + s + STAGES - 1);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);               // lgkmcnt(0): my fragment reads are retired
        wait_younger(nt - 2 - s);                         // stage s+1 landed
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- C phase ----
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 0, 127, 0, 127);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        buf = buf + 1 == STAGES ? 0 : buf + 1;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();          // pairs with the late group's last barrier

    // ---- epilogue: lane holds column m = lane & 31 of each 32x32 tile, rows n = 8q + 4h + (0..3) in registers 4q..4q+3
    const int h = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; i++) {
        const int m = m0 + wm * (TM * 32) + i * 32 + r;
        const float sa = m < p.M ? a_scale[m] : 1.0f;
        f32x4 v[TN][4];                                   // y = (acc * s_a) * s_w
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int n = n0 + wn * (TN * 32) + j * 32 + 8 * q + 4 * h;
                const f32x4 sw = *(const f32x4*)(w_scale + n);
                f32x4 t = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                t *= sa;
                v[j][q] = t * sw;
            }
        if constexpr (EPI == EPI_QKV) {
            // the wave's TN*32 columns are one head: d = 32 j + 8 q + 4 h + c = 16 (2 j + (q >> 1)) + 4 (2 (q & 1) + h) + c
            const int head = (n0 + wn * (TN * 32)) / (TN * 32);
            if (head * (TN * 32) < p.N) {
#pragma unroll
                for (int ob = 0; ob < 2; ob++) {
                    f32x4 t[2 * TN];
#pragma unroll
                    for (int j = 0; j < TN; j++) { t[2 * j] = v[j][ob]; t[2 * j + 1] = v[j][2 + ob]; }
                    epilogue_qkv_head<2 * TN>(p, m, head, 2 * ob + h, t);
                }
            }
        } else if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
            for (int j = 0; j < TN; j++) {                // rows 0..15 of the 32: gate block, 16..31: up block
                const int nb = n0 + wn * (TN * 32) + j * 32;
#pragma unroll
                for (int q = 0; q < 2; q++) epilogue_swiglu4<OutT>(p, m, (nb >> 5) * 16 + 8 * q + 4 * h, v[j][q], v[j][q + 2]);
            }
        } else if (EPI == EPI_RESID && p.sk_part) {
            GemmArgs qa = p;                              // this slice's partial tile: plain fp32 store, bias with slice 0
            qa.C = p.sk_part + (int64_t)blockIdx.y * p.M * p.N; qa.ldc = p.N; qa.c_row0 = 0;
            if (blockIdx.y != 0) qa.bias = nullptr;
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) epilogue4<EPI_STORE, float>(qa, m, n0 + wn * (TN * 32) + j * 32 + 8 * q + 4 * h, v[j][q]);
        } else {
#pragma unroll
            for (int j = 0; j < TN; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) epilogue4<EPI, OutT>(p, m, n0 + wn * (TN * 32) + j * 32 + 8 * q + 4 * h, v[j][q]);
        }
    }
}
#undef A8_VMCNT

// activation quantize of a bf16 fragment-major operand (row-tile stride 16 * lda) into codes [M_pad16][K] + scale
static inline void a8_quant_rows(hipStream_t st, const void* A, int64_t lda, int M, int64_t K, uint8_t* codes, float* scale) {
    hipLaunchKernelGGL(a8_quant_kernel, dim3((unsigned)cdiv(M, 16)), dim3(256), 0, st, (const bf16_t*)A, lda, M, K, codes, scale);
}

template <int EPI, typename OutT, int BM, int BN, int WAVES_N>
static inline void launch_w8a8_tile(hipStream_t st, const GemmArgs& a, const float* as, const float* ws) {
    constexpr int lds = 4 * (BM + BN) * 64;
    NVL_LDS_ATTR((gemm_w8a8_pp_kernel<EPI, OutT, BM, BN, WAVES_N>), lds);
    hipLaunchKernelGGL((gemm_w8a8_pp_kernel<EPI, OutT, BM, BN, WAVES_N>),
                       dim3(cdiv(a.M, BM) * cdiv(a.N, BN), (EPI == EPI_RESID && a.sk_part) ? a.sk_slices : 1), dim3(512), lds, st,
                       a, as, ws);
}

// The tile step of an 8-bit weight in W8A8 mode: quantize A into the scratch b (b.rows rows of up to b.k columns), then
// the W8A8 kernel.  The form follows the bf16 dispatch: the 256x256 tile once its tiles cover 3/4 of
// the CUs (>= 192), else the 128-row form; a wave always owns a whole head in EPI_QKV.
struct A8Buf {
    uint8_t* codes;      // [rows][k] bytes
    float* scale;        // [rows]
    int64_t rows, k;
};
template <int EPI, typename OutT>
static inline void launch_gemm_w8a8(hipStream_t st, const GemmArgs& a, const float* ws, const A8Buf& b) {
    if (a.K % 64 != 0) throw std::runtime_error("gemm: W8A8 needs K % 64 == 0");
    if (round_up(a.M, 16) > b.rows || a.K > b.k) throw std::runtime_error("gemm: W8A8 activation scratch too small");
    float* scale = b.scale;
    a8_quant_rows(st, a.A, a.K, a.M, a.K, b.codes, scale);    // (the bf16 tile kernels read A with row-tile stride 16 K too)
    GemmArgs c = a;
    c.A = b.codes;
    const int t3 = cdiv(a.M, 256) * cdiv(a.N, 256);
    const bool big = !a.sk_part && t3 >= 192 && cu_fill(t3, 1) >= 0.74;
    if constexpr (EPI == EPI_QKV) {
        if (a.qkv.hd == 128) {
            if (big) launch_w8a8_tile<EPI, OutT, 256, 256, 2>(st, c, scale, ws);
            else launch_w8a8_tile<EPI, OutT, 128, 256, 2>(st, c, scale, ws);
            return;
        }
        if (a.qkv.hd != 64) throw std::runtime_error("gemm: EPI_QKV needs head_dim 64 or 128");
    }
    if (big) launch_w8a8_tile<EPI, OutT, 256, 256, 4>(st, c, scale, ws);
    else launch_w8a8_tile<EPI, OutT, 128, 128, 2>(st, c, scale, ws);
}

}  // namespace nvl
