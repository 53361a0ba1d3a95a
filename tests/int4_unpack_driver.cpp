// Stand-alone driver of csrc/int4_unpack.h (built by tests/test_int4_weights_host.py with -fsanitize=address,undefined): the AWQ
// and GPTQ unpackers on tensors the test packs with numpy.  Reads cases from stdin as whitespace-separated integers:
//   layout(1 AWQ, 2 GPTQ) qw_rows qw_cols qz_rows qz_cols sc_rows sc_cols has_g_idx
//   then qweight, qzeros (as unsigned 32-bit words), scales (fp16 bits) and, if has_g_idx, K g_idx values;
// until a line "0".  Prints per case either "REFUSED <message>" or
//   "OK <detected layout> <K> <N> <g>" and three lines with the canonical codes, scales and zeros.
// The arrays are heap vectors of exactly the sizes the shapes give, so an index outside them is an AddressSanitizer report.
#include <cstdio>
#include <iostream>

#include "../nano-vllm-go_amd/csrc/int4_unpack.h"

template <typename T>
static std::vector<T> read_n(int64_t n) {
    std::vector<T> v((size_t)n);
    for (auto& x : v) { long long t; std::cin >> t; x = (T)t; }
    return v;
}

int main() {
    for (;;) {
        int want = 0;
        if (!(std::cin >> want) || want == 0) break;
        std::vector<int64_t> qw = read_n<int64_t>(2), qz = read_n<int64_t>(2), sc = read_n<int64_t>(2);
        int has_g = 0;
        std::cin >> has_g;
        const std::vector<int32_t> qweight = read_n<int32_t>(qw[0] * qw[1]), qzeros = read_n<int32_t>(qz[0] * qz[1]);
        const std::vector<uint16_t> scales = read_n<uint16_t>(sc[0] * sc[1]);
        int layout = 0, g = 0;
        int64_t K = 0, N = 0;
        std::string e = nvl_int4::detect(qw, qz, sc, &layout, &K, &N, &g);
        std::vector<int32_t> g_idx;
        if (has_g) g_idx = read_n<int32_t>(e.empty() ? K : has_g);
        nvl_int4::Canon c;
        if (e.empty() && layout != want) e = "detected the other layout";
        if (e.empty())
            e = layout == nvl_int4::LAYOUT_AWQ ? nvl_int4::unpack_awq(qweight.data(), qzeros.data(), scales.data(), K, N, g, &c)
                                               : nvl_int4::unpack_gptq(qweight.data(), qzeros.data(), scales.data(), has_g ? g_idx.data() : nullptr, K, N, g, &c);
        if (!e.empty()) { std::printf("REFUSED %s\n", e.c_str()); continue; }
        std::printf("OK %d %lld %lld %d\n", layout, (long long)K, (long long)N, g);
        for (uint8_t x : c.codes) std::printf("%u ", (unsigned)x);
        std::printf("\n");
        for (uint16_t x : c.scales) std::printf("%u ", (unsigned)x);
        std::printf("\n");
        for (uint8_t x : c.zeros) std::printf("%u ", (unsigned)x);
        std::printf("\n");
    }
    return 0;
}
