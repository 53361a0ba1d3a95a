// logprob.h — log-probabilities of token ids under the model's logits, on the device: what a
// perplexity is built from and what a serving stack reports as `logprobs`, so that 4 x (2 + 2 top_k) bytes per row cross
// PCIe instead of the V x 4 bytes of the row (generic_model.go:467-470 computes the rows, :595-604 keeps the last one).
//
// Per row of x[rows][ld] (fp32, V valid columns; columns >= V hold whatever the GEMM left there and are never used),
// with x' = x / logits_scaling (generic_model.go:473-477; 0 = none):
//   lse     = max_j x'_j + log(sum_j exp(x'_j - max))      (no plain exp(x) anywhere: logits of +-90 are fine)
//   logprob = x'_t - lse for the row's target id t; t = -1 ("no target") gives +0.0f
//   argmax  = first strict maximum (cmd/ask/main.go:389-402): the id launch_argmax gives on the same row, bit for bit
//   top_k <= 8 best ids and their log-probabilities, value descending then index ascending; entry 0 is the argmax.
//           A row with fewer than top_k finite-or-+inf logits (V < top_k, -inf / NaN entries) pads with id -1, -inf.
//
// Two launches, like launch_argmax (elem.h), so that a handful of rows still fill the chip:
//   pass 1, grid (chunks, rows), 256 threads: a workgroup holds its LOGPROB_CHUNK columns in registers (16 per thread, 16-byte
//           loads when the row is 16-byte aligned: every logit is read once), finds the chunk's best `top_k` (value, index)
//           pairs by repeated block selection (round 0 is the chunk's maximum), and sums exp(x' - chunk max);
//   pass 2, one workgroup per row: merges the {max, sum} partials by the online-softmax rule (sum_c s_c exp(m_c - M)),
//           selects the row's top_k among the chunks' candidates, gathers the target logit.
// Every sum runs in a fixed tree order (4 in a lane's 16-byte piece, the lane's 4 pieces in order, xor-shuffle butterfly
// over the wave, the 4 waves as (0+1)+(2+3); pass 2: a thread's chunks in index order, butterfly, 4 waves), so two runs
// give the same bits.
#pragma once

#include "common.h"
#include "elem.h"

namespace nvl {

constexpr int LOGPROB_CHUNK = 4096, LOGPROB_MAX_K = 8, LOGPROB_NONE = 0x7fffffff;

struct LogprobArgs {
    const float* x; int64_t ld;           // [rows][ld] logits, read-only
    int V, top_k, chunks;
    float scaling;                        // LogitsScaling divisor still to be applied (0 = none / already applied in place)
    float* pmax; float* psum; int32_t* pidx;     // [rows][chunks] partials of pass 1
    float* cval; int32_t* cidx;           // [rows][chunks][top_k] candidates of pass 1 (top_k > 0)
    const int32_t* targets;               // [rows] or NULL (= no target anywhere)
    float* logprob; int32_t* argmax;      // [rows] each; any output may be NULL
    int32_t* topk_ids; float* topk_lp;    // [rows][top_k]
};

struct LogprobShared { float v[2][4]; int i[2][4]; float s[4]; };

// the workgroup's best (value, index) pair — larger value, then lower index — from every thread's own best; all threads
// return it.  `round` alternates the LDS slot, so that one barrier per call is enough.
__device__ __forceinline__ void logprob_block_best(float& best, int& bi, LogprobShared& sh, int round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_merge(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    const int w = threadIdx.x >> 6, b = round & 1;
    if ((threadIdx.x & 63) == 0) { sh.v[b][w] = best; sh.i[b][w] = bi; }
    __syncthreads();
    best = sh.v[b][0]; bi = sh.i[b][0];
#pragma unroll
    for (int k = 1; k < 4; k++) argmax_merge(best, bi, sh.v[b][k], sh.i[b][k]);
}
__device__ __forceinline__ float logprob_block_sum(float s, LogprobShared& sh) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh.s[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh.s[0] + sh.s[1]) + (sh.s[2] + sh.s[3]);
}
// does (v, j) come after (pv, pj) in the order "value descending, index ascending"?
__device__ __forceinline__ bool logprob_after(float v, int j, float pv, int pj) { return v < pv || (v == pv && j > pj); }

template <bool VEC>
__global__ __launch_bounds__(256) void logprob_partial_kernel(LogprobArgs a) {
    __shared__ LogprobShared sh;
    const int row = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const float* x = a.x + (int64_t)row * a.ld;
    const int c0 = chunk * LOGPROB_CHUNK, c1 = min(a.V, c0 + LOGPROB_CHUNK);
    // thread tid owns columns c0 + (g * 256 + tid) * 4 + e, g < 4, e < 4: ascending in (g, e)
    float v[16];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int j = c0 + (g * 256 + tid) * 4;
        if (VEC && j + 3 < c1) {
            const f32x4 q = *(const f32x4*)(x + j);
#pragma unroll
            for (int e = 0; e < 4; e++) v[g * 4 + e] = q[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) v[g * 4 + e] = j + e < c1 ? x[j + e] : -INFINITY;    // columns >= V are never read
        }
    }
    if (a.scaling != 0.f) {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int j = c0 + ((q >> 2) * 256 + tid) * 4 + (q & 3);
            if (j < c1) v[q] = v[q] / a.scaling;     // the division of scale_rows_kernel / argmax_partial_kernel
        }
    }
    const int64_t slot = (int64_t)row * a.chunks + chunk;
    const int rounds = a.top_k > 0 ? a.top_k : 1;
    float pv = INFINITY, mx = -INFINITY;
    int pj = -1;
    for (int r = 0; r < rounds; r++) {
        float best = -INFINITY;
        int bi = LOGPROB_NONE;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int j = c0 + ((q >> 2) * 256 + tid) * 4 + (q & 3);
            if (logprob_after(v[q], j, pv, pj) && v[q] > best) { best = v[q]; bi = j; }   // strict >, ascending j: first maximum
        }
        logprob_block_best(best, bi, sh, r);
        if (r == 0) mx = best;
        if (tid == 0) {
            if (r == 0) { a.pmax[slot] = best; a.pidx[slot] = bi; }
            if (a.top_k > 0) { a.cval[slot * a.top_k + r] = best; a.cidx[slot * a.top_k + r] = bi; }
        }
        pv = best; pj = bi;
    }
    float s = 0.f;
    if (mx > -INFINITY) {            // (a chunk of -inf / NaN only: no mass)
#pragma unroll
        for (int g = 0; g < 4; g++)
            s += (expf(v[g * 4] - mx) + expf(v[g * 4 + 1] - mx)) + (expf(v[g * 4 + 2] - mx) + expf(v[g * 4 + 3] - mx));
    }
    s = logprob_block_sum(s, sh);
    if (tid == 0) a.psum[slot] = s;
}

__global__ __launch_bounds__(256) void logprob_final_kernel(LogprobArgs a) {
    __shared__ LogprobShared sh;
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* pmax = a.pmax + (int64_t)row * a.chunks;
    const float* psum = a.psum + (int64_t)row * a.chunks;
    const int32_t* pidx = a.pidx + (int64_t)row * a.chunks;
    float M = -INFINITY;
    int am = LOGPROB_NONE;
    for (int c = tid; c < a.chunks; c += 256) argmax_merge(M, am, pmax[c], pidx[c]);
    logprob_block_best(M, am, sh, 0);
    float s = 0.f;
    for (int c = tid; c < a.chunks; c += 256) {
        const float mc = pmax[c];
        if (mc > -INFINITY) s += psum[c] * expf(mc - M);
    }
    const float lse = M + logf(logprob_block_sum(s, sh));
    if (tid == 0) {
        if (a.argmax) a.argmax[row] = am == LOGPROB_NONE ? 0 : am;       // all -inf / NaN: the reference returns index 0
        if (a.logprob) {
            const int t = a.targets ? a.targets[row] : -1;
            float lp = 0.f;
            if (t >= 0) {
                float xt = a.x[(int64_t)row * a.ld + t];
                if (a.scaling != 0.f) xt = xt / a.scaling;
                lp = xt - lse;
            }
            a.logprob[row] = lp;
        }
    }
    if (a.top_k > 0 && (a.topk_ids || a.topk_lp)) {
        const int n = a.chunks * a.top_k;
        const float* cval = a.cval + (int64_t)row * n;
        const int32_t* cidx = a.cidx + (int64_t)row * n;
        float pv = INFINITY;
        int pj = -1;
        for (int r = 0; r < a.top_k; r++) {
            float best = -INFINITY;
            int bi = LOGPROB_NONE;
            for (int c = tid; c < n; c += 256) {
                const float cv = cval[c];
                const int cj = cidx[c];
                if (cj != LOGPROB_NONE && logprob_after(cv, cj, pv, pj)) argmax_merge(best, bi, cv, cj);
            }
            logprob_block_best(best, bi, sh, r + 1);
            if (tid == 0) {
                const bool none = bi == LOGPROB_NONE;
                if (a.topk_ids) a.topk_ids[(int64_t)row * a.top_k + r] = none ? -1 : bi;
                if (a.topk_lp) a.topk_lp[(int64_t)row * a.top_k + r] = none ? -INFINITY : best - lse;
            }
            pv = best; pj = bi;
        }
    }
}

// 4-byte words of pass-1 scratch for `rows` rows
static inline int64_t logprob_part_words(int64_t rows, int V, int top_k) { return rows * cdiv(V, LOGPROB_CHUNK) * (3 + 2 * (int64_t)top_k); }

// both passes for `rows` rows; `part` holds logprob_part_words(rows, V, top_k) words.  The row-indexed members of `a`
// (x, targets and the outputs) point at row 0.
static inline void launch_logprobs(hipStream_t st, LogprobArgs a, int rows, void* part) {
    a.chunks = cdiv(a.V, LOGPROB_CHUNK);
    const int64_t n = (int64_t)rows * a.chunks;
    a.pmax = (float*)part; a.psum = a.pmax + n; a.pidx = (int32_t*)(a.psum + n);
    a.cval = (float*)(a.pidx + n); a.cidx = (int32_t*)(a.cval + n * a.top_k);
    const bool vec = ((uintptr_t)a.x & 15) == 0 && (a.ld & 3) == 0;
    for (int r0 = 0; r0 < rows; r0 += 32768) {          // (grid.y <= 65535)
        const int nr = rows - r0 < 32768 ? rows - r0 : 32768;
        LogprobArgs b = a;
        const int64_t p0 = (int64_t)r0 * a.chunks;
        b.x += (int64_t)r0 * a.ld;
        b.pmax += p0; b.psum += p0; b.pidx += p0; b.cval += p0 * a.top_k; b.cidx += p0 * a.top_k;
        if (b.targets) b.targets += r0;
        if (b.logprob) b.logprob += r0;
        if (b.argmax) b.argmax += r0;
        if (b.topk_ids) b.topk_ids += (int64_t)r0 * a.top_k;
        if (b.topk_lp) b.topk_lp += (int64_t)r0 * a.top_k;
        if (vec) hipLaunchKernelGGL(logprob_partial_kernel<true>, dim3(a.chunks, nr), dim3(256), 0, st, b);
        else hipLaunchKernelGGL(logprob_partial_kernel<false>, dim3(a.chunks, nr), dim3(256), 0, st, b);
        hipLaunchKernelGGL(logprob_final_kernel, dim3(nr), dim3(256), 0, st, b);
    }
}

}  // namespace nvl
