// int4_unpack.h — AWQ / GPTQ 4-bit checkpoint tensors -> the canonical (codes, scales, zeros) of nvl_upload_tensor_int4.
// Pure index shuffling on the host, no device code and no HIP dependency (tests/int4_unpack_driver.cpp builds it alone).
// The layouts, as understood here, of a linear with in = K, out = N and groups of g input features:
//   AWQ "GEMM": qweight I32 [K, N/8], nibble i (bits 4i..4i+3) of word (k, j) is output 8j + {0,2,4,6,1,3,5,7}[i];
//               qzeros I32 [K/g, N/8] in the same nibble order; scales F16 [K/g, N]; w = (q - z) * s.
//   GPTQ (v1):  qweight I32 [K/8, N], nibble i of word (k8, n) is input 8 k8 + i; qzeros I32 [K/g, N/8], nibble i of word
//               (gi, j) is output 8j + i and the stored value is z - 1; scales F16 [K/g, N]; g_idx I32 [K], if present,
//               must equal k / g (anything else is act-order, refused); a stored zero of 15 (z = 16) is refused.
// Canonical: codes [N][K/2] (even k in the low nibble), scales [N][K/g] fp16 bits, zeros [N][K/g] 0..15.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace nvl_int4 {

enum { LAYOUT_UNKNOWN = 0, LAYOUT_AWQ = 1, LAYOUT_GPTQ = 2 };

struct Canon {
    int64_t N = 0, K = 0;
    int g = 0;
    std::vector<uint8_t> codes;      // [N][K/2]
    std::vector<uint16_t> scales;    // [N][K/g]
    std::vector<uint8_t> zeros;      // [N][K/g]
};

// The layout and (K, N, g) from the three shapes; "" on success, else why the tensors are refused.
inline std::string detect(const std::vector<int64_t>& qw, const std::vector<int64_t>& qz, const std::vector<int64_t>& sc, int* layout,
                          int64_t* K, int64_t* N, int* g) {
    *layout = LAYOUT_UNKNOWN;
    if (qw.size() != 2 || qz.size() != 2 || sc.size() != 2) return "qweight / qzeros / scales must be 2-D";
    const int64_t n = sc[1], groups = sc[0];
    if (n <= 0 || groups <= 0 || n % 8 != 0) return "scales must be [K/g, N] with N a multiple of 8";
    if (qz[0] != groups || qz[1] * 8 != n) return "qzeros is not [K/g, N/8]: not a 4-bit checkpoint";
    int64_t k;
    if (qw[1] == n) { *layout = LAYOUT_GPTQ; k = qw[0] * 8; }
    else if (qw[1] * 8 == n) { *layout = LAYOUT_AWQ; k = qw[0]; }
    else return "qweight is neither [K, N/8] (AWQ) nor [K/8, N] (GPTQ): not a 4-bit checkpoint";
    if (k <= 0 || k % groups != 0) return "the input width is not a multiple of the number of groups";
    *K = k; *N = n; *g = (int)(k / groups);
    if (*g != 32 && *g != 64 && *g != 128) return "group size " + std::to_string(k / groups) + " is not 32, 64 or 128";
    return "";
}

inline void canon_alloc(Canon* out, int64_t K, int64_t N, int g) {
    out->N = N; out->K = K; out->g = g;
    out->codes.assign((size_t)(N * K / 2), 0);
    out->scales.assign((size_t)(N * (K / g)), 0);
    out->zeros.assign((size_t)(N * (K / g)), 0);
}
inline void put_code(Canon* out, int64_t n, int64_t k, uint32_t q) { out->codes[(size_t)(n * (out->K / 2) + k / 2)] |= (uint8_t)(q << (4 * (k & 1))); }

inline std::string unpack_awq(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, int64_t K, int64_t N, int g, Canon* out) {
    static const int order[8] = {0, 2, 4, 6, 1, 3, 5, 7};
    canon_alloc(out, K, N, g);
    const int64_t G = K / g, N8 = N / 8;
    for (int64_t k = 0; k < K; k++)
        for (int64_t j = 0; j < N8; j++) {
            const uint32_t w = (uint32_t)qweight[k * N8 + j];
            for (int i = 0; i < 8; i++) put_code(out, 8 * j + order[i], k, (w >> (4 * i)) & 15u);
        }
    for (int64_t gi = 0; gi < G; gi++) {
        for (int64_t j = 0; j < N8; j++) {
            const uint32_t w = (uint32_t)qzeros[gi * N8 + j];
            for (int i = 0; i < 8; i++) out->zeros[(size_t)((8 * j + order[i]) * G + gi)] = (uint8_t)((w >> (4 * i)) & 15u);
        }
        for (int64_t n = 0; n < N; n++) out->scales[(size_t)(n * G + gi)] = scales[gi * N + n];
    }
    return "";
}

inline std::string unpack_gptq(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, const int32_t* g_idx, int64_t K, int64_t N,
                               int g, Canon* out) {
    const int64_t G = K / g, N8 = N / 8;
    if (g_idx)
        for (int64_t k = 0; k < K; k++)
            if (g_idx[k] != (int32_t)(k / g)) return "g_idx is not k / group_size: act-order (desc_act) checkpoints are not supported";
    for (int64_t i = 0; i < G * N8; i++) {
        const uint32_t w = (uint32_t)qzeros[i];
        for (int b = 0; b < 8; b++)
            if (((w >> (4 * b)) & 15u) == 15u) return "a stored zero point of 15 (z = 16) does not fit 4 bits";
    }
    canon_alloc(out, K, N, g);
    for (int64_t k8 = 0; k8 < K / 8; k8++)
        for (int64_t n = 0; n < N; n++) {
            const uint32_t w = (uint32_t)qweight[k8 * N + n];     // 8 consecutive inputs of output n: 4 canonical bytes
            for (int b = 0; b < 4; b++) out->codes[(size_t)(n * (K / 2) + k8 * 4 + b)] = (uint8_t)(w >> (8 * b));
        }
    for (int64_t gi = 0; gi < G; gi++) {
        for (int64_t j = 0; j < N8; j++) {
            const uint32_t w = (uint32_t)qzeros[gi * N8 + j];
            for (int i = 0; i < 8; i++) out->zeros[(size_t)((8 * j + i) * G + gi)] = (uint8_t)(((w >> (4 * i)) & 15u) + 1u);
        }
        for (int64_t n = 0; n < N; n++) out->scales[(size_t)(n * G + gi)] = scales[gi * N + n];
    }
    return "";
}

}  // namespace nvl_int4
