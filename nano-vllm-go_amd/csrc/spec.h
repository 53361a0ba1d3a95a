// spec.h — the rejection rule of speculative sampling with a draft MODEL on the device, so that neither the
// target's nor the draft's V-wide distributions cross PCIe.  One 1024-thread workgroup per sequence, like the sampler
// (sample.h); only ONE row per sequence is scanned over V: the first rejected row's residual max(p - q, 0), or the bonus row
// p_k when every draft was accepted.  Every reduction runs in a fixed order: a call is reproducible bit for bit.
//
// The multinomial scan below is sample_row_kernel's (sample.h, "multinomial"), restated over a loader instead of a row
// pointer: the same segmenting, the same order of additions, the same fallback to V - 1.  On a plain row it therefore
// returns the id sample_row_kernel draws for that row with that uniform.  sample_row_kernel itself is not touched.
#pragma once

#include "sample.h"

namespace nvl {

struct SpecArgs {
    const float* p; int64_t ldp;          // target: the final distribution of row i * (1+k) + j at p + row * ldp (ldp % 4 == 0)
    const float* q; int64_t ldq;          // draft: the kept distribution of (sequence i, step j) at q + (i * q_seq + j * q_step) * ldq
    int64_t q_seq, q_step;
    const int32_t* tokens;                // [n][1+k]: tokens[i][j+1] = d_j, the draft's id of step j
    const float* u;                       // [n][1+k]: the accept draws of rows j < k, the final draw in row k's slot
    int32_t* res;                         // [a: n | out_tokens: n x (1+k)] (verify_accept_kernel's layout)
    float* accept_prob;                   // optional [n][k][2]: {p_j(d_j), q_j(d_j)}
    int k, V;
};

// entries j .. j+3 of a row, zero from j1 on
struct SpecRowLoad {
    const float* w;
    __device__ __forceinline__ f32x4 operator()(int j, int j1) const {
        if (j + 3 < j1) return *(const f32x4*)(w + j);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4; k++) if (j + k < j1) v[k] = w[j + k];
        return v;
    }
};
// the same of the residual max(p - q, 0)
struct SpecResidualLoad {
    const float* p; const float* q;
    __device__ __forceinline__ f32x4 operator()(int j, int j1) const {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j + 3 < j1) {
            const f32x4 a = *(const f32x4*)(p + j), b = *(const f32x4*)(q + j);
            for (int k = 0; k < 4; k++) v[k] = fmaxf(a[k] - b[k], 0.f);
        } else {
            for (int k = 0; k < 4; k++) if (j + k < j1) v[k] = fmaxf(p[j + k] - q[j + k], 0.f);
        }
        return v;
    }
};

// first index whose running sum (index order) reaches u * sum; `grand` receives the sum.  Called by the whole workgroup.
template <typename Load>
__device__ int spec_multinomial(const Load load4, int V, float u, SampleShared& sh, float& grand) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = ((V + SAMPLE_WAVES - 1) / SAMPLE_WAVES + 255) & ~255;
    const int j0 = wave * seg, j1 = min(V, j0 + seg);
    auto lane_scan = [&](f32x4 v, float& lane_total) {    // inclusive prefix inside the lane, then across the wave
        v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
        float t = v[3];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float y = __shfl_up(t, o, 64);
            if (lane >= o) t += y;
        }
        lane_total = t;
        const float excl = t - v[3];
        return f32x4{excl + v[0], excl + v[1], excl + v[2], excl + v[3]};
    };
    float carry = 0.f;
    for (int base = j0; base < j1; base += 256) {
        float t;
        (void)lane_scan(load4(base + lane * 4, j1), t);
        carry += __shfl(t, 63, 64);
    }
    if (lane == 0) sh.seg_sum[wave] = carry;
    if (tid == 0) sh.idx = 0x7fffffff;
    __syncthreads();
    float off = 0.f;
    grand = 0.f;
    for (int k = 0; k < SAMPLE_WAVES; k++) {
        if (k == wave) off = grand;
        grand += sh.seg_sum[k];
    }
    const float r = u * grand;
    carry = off;
    for (int base = j0; base < j1; base += 256) {
        const int j = base + lane * 4;
        float t;
        const f32x4 c = lane_scan(load4(j, j1), t);
        int k = 4;
        for (int q = 3; q >= 0; q--) if (j + q < j1 && carry + c[q] >= r) k = q;
        const unsigned long long hit = __ballot(k < 4);
        if (hit) {
            const int first = (int)__ffsll((long long)hit) - 1;
            if (lane == first) atomicMin(&sh.idx, j + k);
            break;
        }
        carry += __shfl(t, 63, 64);
    }
    __syncthreads();
    const int idx = sh.idx == 0x7fffffff ? V - 1 : sh.idx;
    __syncthreads();                                      // (sh is free for another scan)
    return idx;
}

// Per sequence i: row j is accepted iff  ua[i][j] * q_j(d_j) < p_j(d_j)  in fp32 as written; a = the
// number of leading accepted rows; a < k: e ~ max(p_a - q_a, 0) (or p_a, should rounding leave that sum 0); a == k: e ~ p_k.
__global__ __launch_bounds__(SAMPLE_THREADS) void spec_reject_kernel(SpecArgs a) {
    __shared__ SampleShared sh;
    __shared__ int ok[8];
    const int i = blockIdx.x, tid = threadIdx.x, k = a.k, S = 1 + k, V = a.V;
    const int32_t* t = a.tokens + (int64_t)i * S;
    const float* u = a.u + (int64_t)i * S;
    if (tid < k) {
        const int d = t[tid + 1];
        float pd = 0.f, qd = 0.f;                         // (an id outside the vocabulary is refused by the host: never accepted here)
        if (d >= 0 && d < V) {
            pd = a.p[((int64_t)i * S + tid) * a.ldp + d];
            qd = a.q[((int64_t)i * a.q_seq + (int64_t)tid * a.q_step) * a.ldq + d];
        }
        ok[tid] = __fmul_rn(u[tid], qd) < pd;
        if (a.accept_prob) {
            a.accept_prob[((int64_t)i * k + tid) * 2] = pd;
            a.accept_prob[((int64_t)i * k + tid) * 2 + 1] = qd;
        }
    }
    __syncthreads();
    int acc = 0;
    while (acc < k && ok[acc]) acc++;
    const float* pr = a.p + ((int64_t)i * S + acc) * a.ldp;
    const float uf = u[k];
    float total;
    int e;
    if (acc < k) {
        const float* qr = a.q + ((int64_t)i * a.q_seq + (int64_t)acc * a.q_step) * a.ldq;
        e = spec_multinomial(SpecResidualLoad{pr, qr}, V, uf, sh, total);
        if (!(total > 0.f)) e = spec_multinomial(SpecRowLoad{pr}, V, uf, sh, total);
    } else {
        e = spec_multinomial(SpecRowLoad{pr}, V, uf, sh, total);
    }
    if (tid == 0) a.res[i] = acc;
    if (tid < S) a.res[gridDim.x + (int64_t)i * S + tid] = tid < acc ? t[tid + 1] : (tid == acc ? e : -1);
}

}  // namespace nvl
