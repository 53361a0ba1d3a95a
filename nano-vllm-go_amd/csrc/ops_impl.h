// ops_impl.h — op-level C-ABI entry points (nvl_op_*), included at the end of nvllm.hip.
// Host fp32 in / host fp32 out; every one runs the SAME device kernels as the model path, on
// one op, so tests/ can compare each reference function with the oracle in isolation.
// (Test/diagnostic surface: allocates and frees device memory on every call.)
#pragma once

namespace {

struct OpCtx {   // a model-less nvl_model carrying just a stream and the fields the helpers read
    nvl_model m;
    std::vector<void*> bufs;
    OpCtx(int device, int precision) {
        if (nvl_device_count() <= device) throw std::runtime_error("no HIP device (this library has no CPU fallback)");
        NVL_HIP(hipSetDevice(device));
        m.device = device;
        m.f32 = precision == NVL_PRECISION_F32;
        m.wsize = m.f32 ? 4 : 2;
        NVL_HIP(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    }
    ~OpCtx() {
        if (m.stream) { (void)hipStreamSynchronize(m.stream); (void)hipStreamDestroy(m.stream); }
        for (void* p : bufs) dfree(p);
    }
    void* alloc(int64_t bytes) { void* p = dmalloc_bytes(bytes); bufs.push_back(p); return p; }
    float* up_f32(const float* h, int64_t n) {
        float* d = (float*)alloc(n * 4);
        NVL_HIP(hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
        return d;
    }
    // host fp32 [N][K] (or [K][N] when in_out) -> device [Npad][K] in the kernels' operand layout
    // (bf16: fragment-major, rows padded to whole tiles; f32: row-major).  row_major=true keeps a bf16
    // matrix row-major (attention's q and KV slabs are not GEMM operands).
    void* up_mat(const float* h, int64_t N, int64_t K, bool in_out, int64_t pad_rows_to = 64, bool row_major = false) {
        const bool weight = !row_major;
        float* raw = up_f32(h, N * K);
        const int64_t Np = round_up(N, pad_rows_to);
        void* d = alloc(Np * K * (int64_t)m.wsize);
        NVL_HIP(hipMemsetAsync(d, 0, (size_t)(Np * K) * m.wsize, m.stream));
        dim3 grid((unsigned)cdiv(K, 32), (unsigned)cdiv(N, 32));
        if (m.f32) hipLaunchKernelGGL((convert_2d_kernel<float, false>), grid, dim3(256), 0, m.stream, raw, 0, in_out ? 1 : 0, (float*)d, N, K, Slice2D{N, K, 0, 0, 0});
        else if (weight) hipLaunchKernelGGL((convert_2d_kernel<bf16_t, true>), grid, dim3(256), 0, m.stream, raw, 0, in_out ? 1 : 0, (bf16_t*)d, N, K, Slice2D{N, K, 0, 0, 0});
        else hipLaunchKernelGGL((convert_2d_kernel<bf16_t, false>), grid, dim3(256), 0, m.stream, raw, 0, in_out ? 1 : 0, (bf16_t*)d, N, K, Slice2D{N, K, 0, 0, 0});
        NVL_HIP(hipGetLastError());
        return d;
    }
    void down(float* h, const void* d, int64_t n) {
        NVL_HIP(hipMemcpyAsync(h, d, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
    }
};

int op_fail(const std::string& s, int code = NVL_ERR_INVALID) { g_create_err = s; return code; }

#define OP_TRY try {
#define OP_CATCH                                                                              \
    } catch (const HipError& e) {                                                             \
        return op_fail(std::string("HIP error: ") + hipGetErrorString(e.code) + " (" + e.what + ")", NVL_ERR_HIP); \
    } catch (const std::exception& e) {                                                       \
        const std::string w = e.what();                                                       \
        return op_fail(w, w.find("no HIP device") != std::string::npos ? NVL_ERR_NO_DEVICE : NVL_ERR_INVALID); \
    }

}  // namespace

extern "C" int nvl_op_matmul(int device, int precision, const float* a, const float* b, float* c, int M, int K, int N) {
    if (!a || !b || !c || M <= 0 || K <= 0 || N <= 0) return op_fail("nvl_op_matmul: bad arguments");
    if (K % 64 != 0) return op_fail("nvl_op_matmul: K must be a multiple of 64");
    OP_TRY
    OpCtx cx(device, precision);
    void* A = cx.up_mat(a, M, K, false);
    void* W = cx.up_mat(b, N, K, true, W_ROW_PAD);
    const int ldc = (int)round_up(N, 4);
    float* C = (float*)cx.alloc((int64_t)M * ldc * 4);
    gemm(&cx.m, EPI_STORE, true, mk(A, K, W, C, ldc, nullptr, 1.f, M, N, K));
    std::vector<float> tmp((size_t)M * ldc);
    cx.down(tmp.data(), C, (int64_t)M * ldc);
    for (int i = 0; i < M; i++) memcpy(c + (size_t)i * N, &tmp[(size_t)i * ldc], (size_t)N * 4);
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_layernorm(int device, const float* x, const float* w, const float* bias, float eps, float* y,
                                int rows, int hidden) {
    if (!x || !w || !y || rows <= 0 || hidden <= 0 || hidden % 4) return op_fail("nvl_op_layernorm: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* dx = cx.up_f32(x, (int64_t)rows * hidden);
    float* dw = cx.up_f32(w, hidden);
    float* db = bias ? cx.up_f32(bias, hidden) : nullptr;
    float* dy = (float*)cx.alloc((int64_t)rows * hidden * 4);
    hipLaunchKernelGGL((norm_kernel<float>), dim3(cdiv(rows, 4)), dim3(256), 0, cx.m.stream, dx, (const int32_t*)nullptr, dw,
                       db, eps, dy, rows, hidden);
    NVL_HIP(hipGetLastError());
    cx.down(y, dy, (int64_t)rows * hidden);
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_softmax(int device, const float* x, float* y, int rows, int cols) {
    if (!x || !y || rows <= 0 || cols <= 0) return op_fail("nvl_op_softmax: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* dx = cx.up_f32(x, (int64_t)rows * cols);
    float* dy = (float*)cx.alloc((int64_t)rows * cols * 4);
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, cx.m.stream, dx, dy, rows, cols);
    NVL_HIP(hipGetLastError());
    cx.down(y, dy, (int64_t)rows * cols);
    return NVL_OK;
    OP_CATCH
}

static int op_unary(int device, const float* x, float* y, int64_t n, int which) {
    if (!x || !y || n <= 0) return op_fail("nvl_op_gelu/silu: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* dx = cx.up_f32(x, n);
    float* dy = (float*)cx.alloc(n * 4);
    if (which == 0) hipLaunchKernelGGL(gelu_kernel, dim3(cdiv(n, 256)), dim3(256), 0, cx.m.stream, dx, dy, n);
    else hipLaunchKernelGGL(silu_kernel, dim3(cdiv(n, 256)), dim3(256), 0, cx.m.stream, dx, dy, n);
    NVL_HIP(hipGetLastError());
    cx.down(y, dy, n);
    return NVL_OK;
    OP_CATCH
}
extern "C" int nvl_op_gelu(int device, const float* x, float* y, int64_t n) { return op_unary(device, x, y, n, 0); }
extern "C" int nvl_op_silu(int device, const float* x, float* y, int64_t n) { return op_unary(device, x, y, n, 1); }

// ApplyRoPESingleTensor on t [heads, seq, hd]: runs rope_kv_kernel with every head treated as a
// query head of a one-sequence batch (the K/V branches are exercised by the model-level tests).
extern "C" int nvl_op_rope(int device, float* t, int heads, int seq, int hd, int start_pos, double base, int max_seq) {
    if (!t || heads <= 0 || seq <= 0 || hd <= 0 || hd % 2) return op_fail("nvl_op_rope: bad arguments");
    if (start_pos < 0 || start_pos + seq > max_seq) return op_fail("nvl_op_rope: position exceeds max_seq", NVL_ERR_POSITION);
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    const int half = hd / 2;
    std::vector<float> ct((size_t)max_seq * hd), st((size_t)max_seq * hd);
    for (int pos = 0; pos < max_seq; pos++)
        for (int i = 0; i < half; i++) {
            const double freq = 1.0 / std::pow(base, (double)(2 * i) / (double)hd);
            const double ang = (double)pos * freq;
            ct[(size_t)pos * hd + i] = ct[(size_t)pos * hd + half + i] = (float)std::cos(ang);
            st[(size_t)pos * hd + i] = st[(size_t)pos * hd + half + i] = (float)std::sin(ang);
        }
    // [heads, seq, hd] -> token-major [seq][heads*hd]
    std::vector<float> tm((size_t)heads * seq * hd);
    for (int h = 0; h < heads; h++)
        for (int s = 0; s < seq; s++)
            memcpy(&tm[((size_t)s * heads + h) * hd], t + ((size_t)h * seq + s) * hd, (size_t)hd * 4);
    std::vector<int32_t> pos((size_t)seq), slot((size_t)seq, 0);
    for (int s = 0; s < seq; s++) pos[(size_t)s] = start_pos + s;
    float* dq = cx.up_f32(tm.data(), (int64_t)tm.size());
    float* dc = cx.up_f32(ct.data(), (int64_t)ct.size());
    float* ds = cx.up_f32(st.data(), (int64_t)st.size());
    int32_t* dpos = (int32_t*)cx.alloc((int64_t)seq * 4);
    int32_t* dslot = (int32_t*)cx.alloc((int64_t)seq * 4);
    NVL_HIP(hipMemcpyAsync(dpos, pos.data(), (size_t)seq * 4, hipMemcpyHostToDevice, cx.m.stream));
    NVL_HIP(hipMemcpyAsync(dslot, slot.data(), (size_t)seq * 4, hipMemcpyHostToDevice, cx.m.stream));
    float* dout = (float*)cx.alloc((int64_t)tm.size() * 4);
    hipLaunchKernelGGL((rope_kv_kernel<float, false>), dim3(seq, heads), dim3(half), 0, cx.m.stream, dq, heads * hd, dpos, dslot, dslot,
                       dc, ds, dout, heads * hd, (float*)nullptr, (float*)nullptr, (int64_t)0, max_seq, heads, 0, hd);
    NVL_HIP(hipGetLastError());
    cx.down(tm.data(), dout, (int64_t)tm.size());
    for (int h = 0; h < heads; h++)
        for (int s = 0; s < seq; s++)
            memcpy(t + ((size_t)h * seq + s) * hd, &tm[((size_t)s * heads + h) * hd], (size_t)hd * 4);
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_attention(int device, int precision, const float* q, const float* k, const float* v, int nH, int nKV,
                                int S, int T, int hd, float scale, float* out) {
    if (!q || !k || !v || !out || nH <= 0 || nKV <= 0 || nH % nKV || S <= 0 || T < S || (hd != 64 && hd != 128))
        return op_fail("nvl_op_attention: bad arguments");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    const int Tmax = (int)round_up(T, 64);
    if (m.f32 && Tmax > 12000) return op_fail("nvl_op_attention: T too long for the f32 kernel");
    // token-major Q, slab-layout K and V
    std::vector<float> qt((size_t)S * nH * hd), kc((size_t)nKV * Tmax * hd, 0.f), vc((size_t)nKV * Tmax * hd, 0.f);
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(&qt[((size_t)s * nH + h) * hd], q + ((size_t)h * S + s) * hd, (size_t)hd * 4);
    for (int h = 0; h < nKV; h++)
        for (int t = 0; t < T; t++)
            for (int d = 0; d < hd; d++) {
                kc[((size_t)h * Tmax + t) * hd + d] = k[((size_t)h * T + t) * hd + d];
                vc[((size_t)h * Tmax + t) * hd + d] = v[((size_t)h * T + t) * hd + d];
            }
    m.q = cx.up_mat(qt.data(), S, (int64_t)nH * hd, false, 1, true);
    m.kcache = cx.up_mat(kc.data(), 1, (int64_t)kc.size(), false, 1, true);
    m.vcache = cx.up_mat(vc.data(), 1, (int64_t)vc.size(), false, 1, true);
    m.attn_out = cx.alloc(round_up(S, 64) * nH * hd * (int64_t)m.wsize);
    m.nH = nH; m.nKV = nKV; m.group = nH / nKV; m.hd = hd; m.Tmax = Tmax; m.L = 1;
    m.layer_stride = (int64_t)nKV * Tmax * hd; m.slot_stride = m.layer_stride;
    m.attn_scale = scale != 0.f ? scale : 1.0f / std::sqrt((float)hd);
    const int32_t meta[5] = {0, S, T - S, 0, 0};      // one sequence whose block table is the single block 0
    int32_t* dmeta = (int32_t*)cx.alloc(20);
    NVL_HIP(hipMemcpyAsync(dmeta, meta, 20, hipMemcpyHostToDevice, m.stream));
    Meta md{};
    md.seq_tok_start = dmeta; md.seq_len = dmeta + 1; md.seq_pos = dmeta + 2; md.seq_tbl = dmeta + 3; md.blk_table = dmeta + 4;
    m.blocks_per_seq = 1;
    attention(&m, 0, md, 1, S, 0.0);
    // back to fp32 [nH, S, hd]
    std::vector<float> ot((size_t)S * nH * hd);
    if (m.f32) {
        cx.down(ot.data(), m.attn_out, (int64_t)ot.size());
    } else {
        std::vector<uint16_t> ob((size_t)(round_up(S, 64) * nH * hd));
        NVL_HIP(hipMemcpyAsync(ob.data(), m.attn_out, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        const int64_t W = (int64_t)nH * hd;     // the kernel wrote the next GEMM's fragment-major operand
        for (int64_t r = 0; r < S; r++)
            for (int64_t c = 0; c < W; c++) {
                uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, W)]) << 16;
                memcpy(&ot[(size_t)(r * W + c)], &u, 4);
            }
    }
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(out + ((size_t)h * S + s) * hd, &ot[((size_t)s * nH + h) * hd], (size_t)hd * 4);
    m.q = m.kcache = m.vcache = m.attn_out = nullptr;   // owned by cx.bufs
    return NVL_OK;
    OP_CATCH
}

// attn_decode_mq_bf16_kernel alone (whatever nvl_set_tuning key 38 says): nvl_op_attention's conventions, S = 2..8 new positions
extern "C" int nvl_op_attention_mq(int device, const float* q, const float* k, const float* v, int nH, int nKV, int S, int T,
                                   int hd, float scale, float* out) {
    if (!q || !k || !v || !out || nH <= 0 || nKV <= 0 || nH % nKV || S < 2 || S > 8 || T < S || (hd != 64 && hd != 128))
        return op_fail("nvl_op_attention_mq: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    nvl_model& m = cx.m;
    const int Tmax = (int)round_up(T, 64);
    std::vector<float> qt((size_t)S * nH * hd), kc((size_t)nKV * Tmax * hd, 0.f), vc((size_t)nKV * Tmax * hd, 0.f);
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(&qt[((size_t)s * nH + h) * hd], q + ((size_t)h * S + s) * hd, (size_t)hd * 4);
    for (int h = 0; h < nKV; h++)
        for (int t = 0; t < T; t++) {
            memcpy(&kc[((size_t)h * Tmax + t) * hd], k + ((size_t)h * T + t) * hd, (size_t)hd * 4);
            memcpy(&vc[((size_t)h * Tmax + t) * hd], v + ((size_t)h * T + t) * hd, (size_t)hd * 4);
        }
    m.q = cx.up_mat(qt.data(), S, (int64_t)nH * hd, false, 1, true);
    m.kcache = cx.up_mat(kc.data(), 1, (int64_t)kc.size(), false, 1, true);
    m.vcache = cx.up_mat(vc.data(), 1, (int64_t)vc.size(), false, 1, true);
    m.attn_out = cx.alloc(round_up(S, 64) * nH * hd * 2);
    m.nH = nH; m.nKV = nKV; m.group = nH / nKV; m.hd = hd; m.Tmax = Tmax; m.L = 1;
    m.layer_stride = (int64_t)nKV * Tmax * hd; m.slot_stride = m.layer_stride;
    m.attn_scale = scale != 0.f ? scale : 1.0f / std::sqrt((float)hd);
    m.ctx_hint = T;                                   // (the wave ladder follows the context, as in the model path)
    const int32_t meta[5] = {0, S, T - S, 0, 0};      // one sequence whose block table is the single block 0
    int32_t* dmeta = (int32_t*)cx.alloc(20);
    NVL_HIP(hipMemcpyAsync(dmeta, meta, 20, hipMemcpyHostToDevice, m.stream));
    Meta md{};
    md.seq_tok_start = dmeta; md.seq_len = dmeta + 1; md.seq_pos = dmeta + 2; md.seq_tbl = dmeta + 3; md.blk_table = dmeta + 4;
    m.blocks_per_seq = 1;
    attention(&m, 0, md, 1, S, 0.0, false, true);
    std::vector<float> ot((size_t)S * nH * hd);
    std::vector<uint16_t> ob((size_t)(round_up(S, 64) * nH * hd));
    NVL_HIP(hipMemcpyAsync(ob.data(), m.attn_out, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
    NVL_HIP(hipStreamSynchronize(m.stream));
    const int64_t W = (int64_t)nH * hd;     // the kernel wrote the next GEMM's fragment-major operand
    for (int64_t r = 0; r < S; r++)
        for (int64_t c = 0; c < W; c++) {
            uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, W)]) << 16;
            memcpy(&ot[(size_t)(r * W + c)], &u, 4);
        }
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(out + ((size_t)h * S + s) * hd, &ot[((size_t)s * nH + h) * hd], (size_t)hd * 4);
    m.q = m.kcache = m.vcache = m.attn_out = nullptr;   // owned by cx.bufs
    return NVL_OK;
    OP_CATCH
}

// Mamba2Layer.Forward between its two projections (mamba2.go:107-170) through the model's own dispatch (mamba_mixer):
// a ragged batch of n_seqs sequences, token rows back to back in proj, sequence i at position seq_pos[i] in state slot
// seq_slot[i].  Every stage's output comes back: xbc, delta, y before gating, and the gated + normed rows (bf16 mode:
// un-permuted from the fragment-major out_proj operand).  state / tail are read and written in place.
extern "C" int nvl_op_mamba_mixer(int device, int precision, const float* proj, int n_seqs, const int32_t* seq_len,
                                  const int32_t* seq_pos, const int32_t* seq_slot, int n_slots, int nh, int hd, int ss, int ng, int K,
                                  const float* conv_w, const float* conv_b, const float* a_log, const float* D, const float* dt_bias,
                                  const float* norm_w, float* state, float* tail, int chain, float* xbc, float* delta, float* y,
                                  float* normed) {
    if (!proj || !seq_len || !seq_pos || !seq_slot || !conv_w || !state || !xbc || !delta || !y || !normed || n_seqs <= 0 || n_slots <= 0)
        return op_fail("nvl_op_mamba_mixer: bad arguments");
    if (!mamba_geometry_ok(nh, hd, ss, ng, K)) return op_fail("nvl_op_mamba_mixer: head_dim / state_size / groups / conv kernel not supported by the kernels");
    if (chain < 0 || chain > 3 || (chain && ((chain != 3 && n_seqs != 1) || (K > 1 && !tail))))
        return op_fail("nvl_op_mamba_mixer: a chained prefill (chain 1 / 2) is one sequence with a tail; a carried window (chain 3) needs a tail");
    int64_t M64 = 0;
    int max_len = 0;
    std::vector<char> used((size_t)n_slots, 0);
    for (int i = 0; i < n_seqs; i++) {
        if (seq_len[i] <= 0 || seq_pos[i] < 0 || seq_slot[i] < 0 || seq_slot[i] >= n_slots || used[(size_t)seq_slot[i]])
            return op_fail("nvl_op_mamba_mixer: bad sequence length / position / slot");
        used[(size_t)seq_slot[i]] = 1;
        M64 += seq_len[i]; max_len = std::max(max_len, (int)seq_len[i]);
    }
    if (M64 > (1 << 20)) return op_fail("nvl_op_mamba_mixer: too many tokens");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    struct Scratch {      // the chunk-parallel scratch mamba_mixer grows on the model
        nvl_model& m;
        ~Scratch() { (void)hipStreamSynchronize(m.stream); dfree(m.ssd_z); dfree(m.ssd_decay); m.ssd_z = m.ssd_decay = nullptr; }
    } scratch{m};
    const int M = (int)M64, EH = nh * hd, conv_dim = EH + 2 * ng * ss, P = EH + conv_dim + nh;
    std::vector<int32_t> meta((size_t)(4 * n_seqs + 2 * M));
    int32_t *h_start = meta.data(), *h_len = h_start + n_seqs, *h_pos = h_len + n_seqs, *h_slot = h_pos + n_seqs,
            *h_tpos = h_slot + n_seqs, *h_tseq = h_tpos + M;
    for (int i = 0, t = 0; i < n_seqs; i++) {
        h_start[i] = t; h_len[i] = seq_len[i]; h_pos[i] = seq_pos[i]; h_slot[i] = seq_slot[i];
        for (int j = 0; j < seq_len[i]; j++, t++) { h_tpos[t] = seq_pos[i] + j; h_tseq[t] = i; }
    }
    int32_t* dmeta = (int32_t*)cx.alloc((int64_t)meta.size() * 4);
    NVL_HIP(hipMemcpyAsync(dmeta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, m.stream));
    MambaArgs a{};
    a.proj = cx.up_f32(proj, (int64_t)M * P); a.P = P; a.EH = EH; a.conv_dim = conv_dim; a.nh = nh; a.hd = hd; a.ss = ss; a.ng = ng; a.K = K;
    a.conv_w = cx.up_f32(conv_w, (int64_t)conv_dim * K);
    a.conv_b = conv_b ? cx.up_f32(conv_b, conv_dim) : nullptr;
    a.a_log = a_log ? cx.up_f32(a_log, nh) : nullptr;
    a.Dskip = D ? cx.up_f32(D, nh) : nullptr;
    a.dt_bias = dt_bias ? cx.up_f32(dt_bias, nh) : nullptr;
    a.norm_w = norm_w ? cx.up_f32(norm_w, EH) : nullptr;
    a.xbc = (float*)cx.alloc((int64_t)M * conv_dim * 4); a.delta = (float*)cx.alloc((int64_t)M * nh * 4); a.y = (float*)cx.alloc((int64_t)M * EH * 4);
    const int64_t state_floats = (int64_t)nh * hd * ss, tail_floats = (int64_t)(K - 1) * conv_dim;
    a.state = cx.up_f32(state, state_floats * n_slots); a.state_slot_stride = state_floats;
    a.seq_tok_start = dmeta; a.seq_len = dmeta + n_seqs; a.seq_pos = dmeta + 2 * n_seqs; a.seq_slot = dmeta + 3 * n_seqs;
    a.tok_pos = dmeta + 4 * n_seqs; a.tok_seq = a.tok_pos + M;
    const bool have_tail = tail && K > 1;      // (as the model: no tail buffer, no chain)
    a.tail = have_tail ? cx.up_f32(tail, tail_floats * n_slots) : nullptr; a.tail_slot_stride = tail_floats;
    a.chain = have_tail ? chain : 0;
    float* y_pre = (float*)cx.alloc((int64_t)M * EH * 4);
    const int64_t Mp = round_up(M, 64);
    void* out = cx.alloc(Mp * EH * (int64_t)m.wsize);
    NVL_HIP(hipMemsetAsync(out, 0, (size_t)(Mp * EH) * m.wsize, m.stream));
    mamba_mixer(&m, a, M, n_seqs, max_len, out, y_pre);
    cx.down(xbc, a.xbc, (int64_t)M * conv_dim);
    cx.down(delta, a.delta, (int64_t)M * nh);
    cx.down(y, y_pre, (int64_t)M * EH);
    cx.down(state, a.state, state_floats * n_slots);
    if (have_tail) cx.down(tail, a.tail, tail_floats * n_slots);
    if (m.f32) {
        cx.down(normed, out, (int64_t)M * EH);
    } else {
        std::vector<uint16_t> ob((size_t)(Mp * EH));
        NVL_HIP(hipMemcpyAsync(ob.data(), out, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int64_t r = 0; r < M; r++)       // the kernel wrote the out_proj GEMM's fragment-major operand
            for (int64_t c = 0; c < EH; c++) {
                uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, EH)]) << 16;
                memcpy(&normed[(size_t)(r * EH + c)], &u, 4);
            }
    }
    return NVL_OK;
    OP_CATCH
}

// The one-weight model of the quantized matmul ops: W [K][N] ([in, out], as nvl_op_matmul) quantized by the upload quantizer
// of format wf into a tensor registered for gemm(), a tile-path scratch of at most scratch_rows weight rows, then
// C = bf16(A) · W~^T through the model's dispatch into c [M][N]; then the quantizer's codes, scales and (INT4) zero points in
// the ABI packing of the prequantized upload, where asked for.
static void op_matmul_q(OpCtx& cx, int wf, const float* a, const float* w, int M, int N, int K, float* c, int64_t scratch_rows,
                        uint8_t* codes_out = nullptr, void* scales_out = nullptr, uint8_t* zeros_out = nullptr) {
    DevTensor t;
    cx.m.wf = wf;
    void* A = cx.up_mat(a, M, K, false);
    upload_2d_q(&cx.m, &t, wf, w, NVL_DTYPE_F32, N, K, true);
    cx.bufs.push_back(t.p); cx.bufs.push_back(t.qs);
    cx.m.qmap[t.p] = nvl_model::QRef{wf, t.qs, t.rows_pad};
    cx.m.wq_scratch_elems = std::min<int64_t>(t.rows_pad, scratch_rows) * K;
    cx.m.wq_scratch = (bf16_t*)cx.alloc(cx.m.wq_scratch_elems * 2);
    const int ldc = (int)round_up(N, 4);
    float* C = (float*)cx.alloc((int64_t)M * ldc * 4);
    gemm(&cx.m, EPI_STORE, true, mk(A, K, t.p, C, ldc, nullptr, 1.f, M, N, K));
    std::vector<float> tmp((size_t)M * ldc);
    cx.down(tmp.data(), C, (int64_t)M * ldc);
    for (int i = 0; i < M; i++) memcpy(c + (size_t)i * N, &tmp[(size_t)i * ldc], (size_t)N * 4);
    if (codes_out || scales_out || zeros_out) {
        std::vector<uint8_t> codes((size_t)wf_code_bytes(wf, t.rows_pad * K)), sc((size_t)wf_scale_bytes(wf, t.rows_pad, K));
        NVL_HIP(hipMemcpy(codes.data(), t.p, codes.size(), hipMemcpyDeviceToHost));
        NVL_HIP(hipMemcpy(sc.data(), t.qs, sc.size(), hipMemcpyDeviceToHost));
        wf_to_abi(wf, codes.data(), sc.data(), N, K, codes_out, scales_out, zeros_out);
    }
}

// 8-bit weights (w8.h): M <= 64 the fp8-weight decode kernels, larger M the 64-row groups or dequantize + tile; the scratch
// holds at most 2048 weight rows, as an LM head's would, so wide N runs in chunks.
extern "C" int nvl_op_matmul_fp8w(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* codes_out,
                                  float* scales_out) {
    if (!a || !w || !c || M <= 0 || K <= 0 || N <= 0) return op_fail("nvl_op_matmul_fp8w: bad arguments");
    if (K % 64 != 0) return op_fail("nvl_op_matmul_fp8w: K must be a multiple of 64");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    op_matmul_q(cx, WF_FP8, a, w, M, N, K, c, 2048, codes_out, scales_out);
    return NVL_OK;
    OP_CATCH
}

// MXFP4 weights (w4.h): the MXFP4-weight decode kernels, the 64-row groups, dequantize + tile (the scratch holds all of W~)
extern "C" int nvl_op_matmul_mxfp4w(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* codes_out,
                                    uint8_t* scales_out) {
    if (!a || !w || !c || M <= 0 || K <= 0 || N <= 0) return op_fail("nvl_op_matmul_mxfp4w: bad arguments");
    if (K % 64 != 0) return op_fail("nvl_op_matmul_mxfp4w: K must be a multiple of 64");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    op_matmul_q(cx, WF_MXFP4, a, w, M, N, K, c, INT64_MAX, codes_out, scales_out);
    return NVL_OK;
    OP_CATCH
}

// INT4 group-quantized weights (w4g.h): the INT4-weight decode kernels, the 64-row groups, dequantize + tile
extern "C" int nvl_op_matmul_int4w(int device, const float* a, const float* w, int M, int N, int K, int group_size, float* c,
                                   uint8_t* codes_out, uint16_t* scales_out, uint8_t* zeros_out) {
    if (!a || !w || !c || M <= 0 || K <= 0 || N <= 0) return op_fail("nvl_op_matmul_int4w: bad arguments");
    if (group_size != 32 && group_size != 64 && group_size != 128) return op_fail("nvl_op_matmul_int4w: the group size must be 32, 64 or 128");
    if (K % 64 != 0 || K % group_size != 0) return op_fail("nvl_op_matmul_int4w: K must be a multiple of 64 and of the group size");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    op_matmul_q(cx, wf_int4(group_size), a, w, M, N, K, c, INT64_MAX, codes_out, scales_out, zeros_out);
    return NVL_OK;
    OP_CATCH
}

// codes [rows_pad16][K] (fragment-major bytes) + scales on the device -> [M][K] row-major / [M] on the host
static void a8_read_back(OpCtx& cx, const uint8_t* dcodes, const float* dscale, int M, int K, uint8_t* codes_out, float* scales_out) {
    const int64_t rows = round_up(M, 16);
    std::vector<uint8_t> codes((size_t)(rows * K));
    std::vector<float> sc((size_t)rows);
    NVL_HIP(hipStreamSynchronize(cx.m.stream));
    NVL_HIP(hipMemcpy(codes.data(), dcodes, codes.size(), hipMemcpyDeviceToHost));
    NVL_HIP(hipMemcpy(sc.data(), dscale, sc.size() * 4, hipMemcpyDeviceToHost));
    if (scales_out) memcpy(scales_out, sc.data(), (size_t)M * 4);
    if (codes_out)
        for (int64_t r = 0; r < M; r++)
            for (int64_t k = 0; k < K; k++) codes_out[r * K + k] = codes[(size_t)fm_index(r, k, K)];
}

// 8-bit weights and activations (a8.h): nvl_op_matmul_fp8w with the model's dispatch in W8A8 mode
extern "C" int nvl_op_matmul_w8a8(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* a_codes_out,
                                  float* a_scales_out) {
    if (!a || !w || !c || M <= 0 || K <= 0 || N <= 0) return op_fail("nvl_op_matmul_w8a8: bad arguments");
    if (K % 64 != 0) return op_fail("nvl_op_matmul_w8a8: K must be a multiple of 64");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    cx.m.a8 = true;
    cx.m.a8_rows = round_up(M, 16);
    cx.m.a8_k = K;
    cx.m.a8_codes = (uint8_t*)cx.alloc(cx.m.a8_rows * K);
    cx.m.a8_scale = (float*)cx.alloc(cx.m.a8_rows * 4);
    NVL_HIP(hipMemsetAsync(cx.m.a8_codes, 0, (size_t)(cx.m.a8_rows * K), cx.m.stream));
    const std::vector<float> ones((size_t)cx.m.a8_rows, 1.0f);
    NVL_HIP(hipMemcpyAsync(cx.m.a8_scale, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, cx.m.stream));
    NVL_HIP(hipStreamSynchronize(cx.m.stream));     // (pageable source)
    op_matmul_q(cx, WF_FP8, a, w, M, N, K, c, 2048);
    if (a_codes_out || a_scales_out) a8_read_back(cx, cx.m.a8_codes, cx.m.a8_scale, M, K, a_codes_out, a_scales_out);
    cx.m.a8_codes = nullptr; cx.m.a8_scale = nullptr;       // owned by cx.bufs
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_act_quant_fp8(int device, const float* a, int M, int K, int lda, uint8_t* codes, float* scales) {
    if (!a || !codes || !scales || M <= 0 || K <= 0 || K % 64 != 0 || lda < K || lda % 64 != 0)
        return op_fail("nvl_op_act_quant_fp8: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    std::vector<float> ext((size_t)M * lda);
    for (int64_t r = 0; r < M; r++)
        for (int64_t k = 0; k < lda; k++) ext[(size_t)(r * lda + k)] = k < K ? a[r * K + k] : (float)((r + k) % 7);
    void* A = cx.up_mat(ext.data(), M, lda, false, 16);
    const int64_t rows = round_up(M, 16);
    uint8_t* dc = (uint8_t*)cx.alloc(rows * K);
    float* ds = (float*)cx.alloc(rows * 4);
    a8_quant_rows(cx.m.stream, A, lda, M, K, dc, ds);
    NVL_HIP(hipGetLastError());
    a8_read_back(cx, dc, ds, M, K, codes, scales);
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_fp8_kv_roundtrip(int device, const float* x, int64_t n, float scale, uint8_t* codes, float* back) {
    if (!x || !codes || !back || n <= 0 || !(scale > 0.f) || !std::isfinite(scale)) return op_fail("nvl_op_fp8_kv_roundtrip: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    float* dx = cx.up_f32(x, n);
    uint8_t* dc = (uint8_t*)cx.alloc(round_up(n, 4));
    float* db = (float*)cx.alloc(n * 4);
    const unsigned blocks = (unsigned)cdiv(cdiv(n, 4), 256);
    hipLaunchKernelGGL(kv8_quant_kernel, dim3(blocks), dim3(256), 0, cx.m.stream, dx, n, scale, dc);
    hipLaunchKernelGGL(kv8_dequant_kernel, dim3(blocks), dim3(256), 0, cx.m.stream, (const uint8_t*)dc, n, scale, db);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipMemcpyAsync(codes, dc, (size_t)n, hipMemcpyDeviceToHost, cx.m.stream));
    cx.down(back, db, n);
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_attention_kv8(int device, const float* q, const float* k, const float* v, int nH, int nKV, int S, int T,
                                    int hd, float scale, float k_scale, float v_scale, float* out) {
    if (!q || !k || !v || !out || nH <= 0 || nKV <= 0 || nH % nKV || S <= 0 || T < S || (hd != 64 && hd != 128))
        return op_fail("nvl_op_attention_kv8: bad arguments");
    if (!(k_scale > 0.f) || !(v_scale > 0.f) || !std::isfinite(k_scale) || !std::isfinite(v_scale))
        return op_fail("nvl_op_attention_kv8: k_scale / v_scale must be finite and positive");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    nvl_model& m = cx.m;
    const int Tmax = (int)round_up(T, 64);
    std::vector<float> qt((size_t)S * nH * hd), kc((size_t)nKV * Tmax * hd, 0.f), vc((size_t)nKV * Tmax * hd, 0.f);
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(&qt[((size_t)s * nH + h) * hd], q + ((size_t)h * S + s) * hd, (size_t)hd * 4);
    for (int h = 0; h < nKV; h++)
        for (int t = 0; t < T; t++) {
            memcpy(&kc[((size_t)h * Tmax + t) * hd], k + ((size_t)h * T + t) * hd, (size_t)hd * 4);
            memcpy(&vc[((size_t)h * Tmax + t) * hd], v + ((size_t)h * T + t) * hd, (size_t)hd * 4);
        }
    m.q = cx.up_mat(qt.data(), S, (int64_t)nH * hd, false, 1, true);
    // the 8-bit slabs, written by the shared quantizer from the fp32 values (padding rows: code 0)
    const int64_t n_el = (int64_t)kc.size();
    const float* dk = cx.up_f32(kc.data(), n_el);
    const float* dv = cx.up_f32(vc.data(), n_el);
    uint8_t* k8 = (uint8_t*)cx.alloc(n_el);
    uint8_t* v8 = (uint8_t*)cx.alloc(n_el);
    const unsigned qblocks = (unsigned)cdiv(cdiv(n_el, 4), 256);
    hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dk, n_el, k_scale, k8);
    hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dv, n_el, v_scale, v8);
    NVL_HIP(hipGetLastError());
    m.attn_out = cx.alloc(round_up(S, 64) * nH * hd * 2);
    m.nH = nH; m.nKV = nKV; m.group = nH / nKV; m.hd = hd; m.Tmax = Tmax; m.L = 1;
    m.layer_stride = (int64_t)nKV * Tmax * hd; m.slot_stride = m.layer_stride;
    m.attn_scale = scale != 0.f ? scale : 1.0f / std::sqrt((float)hd);
    // the key-split decode form needs its partial-result scratch and the context length (as the model path)
    m.attn_part = (float*)cx.alloc((int64_t)ATTN_SPLIT_MAX_PAIRS * ATTN_SPLIT_MAX * (hd == 64 ? attn_part_floats<64>() : attn_part_floats<128>()) * 4);
    m.attn_part_cnt = (int32_t*)cx.alloc(ATTN_SPLIT_MAX_PAIRS * 4);
    NVL_HIP(hipMemsetAsync(m.attn_part_cnt, 0, ATTN_SPLIT_MAX_PAIRS * 4, m.stream));
    m.ctx_hint = T;
    const int32_t meta[5] = {0, S, T - S, 0, 0};
    int32_t* dmeta = (int32_t*)cx.alloc(20);
    NVL_HIP(hipMemcpyAsync(dmeta, meta, 20, hipMemcpyHostToDevice, m.stream));
    Meta md{};
    md.seq_tok_start = dmeta; md.seq_len = dmeta + 1; md.seq_pos = dmeta + 2; md.seq_tbl = dmeta + 3; md.blk_table = dmeta + 4;
    m.blocks_per_seq = 1;
    attention_kv8(&m, md, 1, S, k8, v8, k_scale, v_scale);
    std::vector<float> ot((size_t)S * nH * hd);
    std::vector<uint16_t> ob((size_t)(round_up(S, 64) * nH * hd));
    NVL_HIP(hipMemcpyAsync(ob.data(), m.attn_out, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
    NVL_HIP(hipStreamSynchronize(m.stream));
    const int64_t W = (int64_t)nH * hd;
    for (int64_t r = 0; r < S; r++)
        for (int64_t c = 0; c < W; c++) {
            uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, W)]) << 16;
            memcpy(&ot[(size_t)(r * W + c)], &u, 4);
        }
    for (int h = 0; h < nH; h++)
        for (int s = 0; s < S; s++)
            memcpy(out + ((size_t)h * S + s) * hd, &ot[((size_t)s * nH + h) * hd], (size_t)hd * 4);
    m.q = m.attn_out = nullptr; m.attn_part = nullptr; m.attn_part_cnt = nullptr;   // owned by cx.bufs
    return NVL_OK;
    OP_CATCH
}

// attention() / attention_kv8() on a batch as plan_paged lays it out, set up as nvl_create sets a model up: Tmax = the block
// size, slot_stride = one block of one layer, blocks_per_seq = the table's stride, ctx_hint as attn_cost computes it, the
// split scratch and its zeroed tickets.  attn_out and attn_part start as 0xFF bytes (NaN in bf16 and fp32): a row nobody
// wrote, or a partial record read before its workgroup wrote it, shows in `out`.  Nothing that could index outside the
// pools reaches a kernel: every table entry is checked, used or not.
extern "C" int nvl_op_attention_batch(int device, int precision, int form, int nH, int nKV, int hd, float scale, int n_seqs,
                                      const int32_t* seq_len, const int32_t* seq_pos, float* k_pool, float* v_pool, int n_blocks,
                                      int block_size, const int32_t* block_table, int tbl_stride, const float* q, double rope_base,
                                      int max_seq, float k_scale, float v_scale, float* out, int32_t* ran, int32_t* part_cnt) {
    const char* who = "nvl_op_attention_batch: ";
    if (!seq_len || !seq_pos || !k_pool || !v_pool || !block_table || !q || !out || !ran || !part_cnt || nH <= 0 || nKV <= 0 ||
        nH % nKV || (hd != 64 && hd != 128) || n_seqs <= 0 || n_seqs > 4096 || n_blocks <= 0 || block_size <= 0 || block_size % 64 ||
        tbl_stride <= 0 || max_seq <= 0 || form < NVL_ATTN_OP_PLAIN || form > NVL_ATTN_OP_KV8 ||
        (precision != NVL_PRECISION_BF16 && precision != NVL_PRECISION_F32) || !(scale >= 0.f) || !std::isfinite(scale))
        return op_fail(std::string(who) + "bad arguments");
    const bool fused = form == NVL_ATTN_OP_FUSED, kv8 = form == NVL_ATTN_OP_KV8, mq = form == NVL_ATTN_OP_MQ;
    if (form != NVL_ATTN_OP_PLAIN && precision != NVL_PRECISION_BF16) return op_fail(std::string(who) + "the fused, mq and kv8 forms are bf16 only");
    if (kv8 && (!(k_scale > 0.f) || !(v_scale > 0.f) || !std::isfinite(k_scale) || !std::isfinite(v_scale)))
        return op_fail(std::string(who) + "k_scale / v_scale must be finite and positive");
    if (fused && (!(rope_base >= 0.0) || !std::isfinite(rope_base))) return op_fail(std::string(who) + "rope_base must be finite and >= 0");
    // plan_paged's refusals, in its order, then the rest of the table
    int64_t tokens = 0;
    int max_len = 0, ctx = 0;
    for (int i = 0; i < n_seqs; i++) {
        if (seq_len[i] <= 0 || seq_len[i] > (1 << 16)) return op_fail(std::string(who) + "sequence without rows (or more than 65536)");
        if (fused && seq_len[i] != 1) return op_fail(std::string(who) + "the fused form is a decode step: one row per sequence");
        if (seq_pos[i] < 0) return op_fail(std::string(who) + "negative position");
        if (seq_pos[i] > max_seq - seq_len[i]) return op_fail(std::string(who) + "position exceeds max_seq", NVL_ERR_POSITION);
        if (tbl_stride < cdiv((int64_t)seq_pos[i] + seq_len[i], block_size))
            return op_fail(std::string(who) + "block table shorter than the positions it must cover");
        tokens += seq_len[i];
        max_len = std::max(max_len, seq_len[i]);
        ctx = std::max(ctx, seq_pos[i] + seq_len[i]);
    }
    if (tokens > (1 << 16)) return op_fail(std::string(who) + "more than 65536 rows");
    for (int64_t i = 0; i < (int64_t)n_seqs * tbl_stride; i++)
        if (block_table[i] < 0 || block_table[i] >= n_blocks) return op_fail(std::string(who) + "block id out of range");
    if (precision == NVL_PRECISION_F32 && (int64_t)tbl_stride * block_size > 12000)
        return op_fail(std::string(who) + "block table too long for the f32 kernel");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    auto nan_fill = [&](int64_t bytes) { void* p = cx.alloc(bytes); NVL_HIP(hipMemsetAsync(p, 0xFF, (size_t)bytes, m.stream)); return p; };
    const int64_t W = (int64_t)nH * hd, n_el = (int64_t)n_blocks * nKV * block_size * hd;
    m.nH = nH; m.nKV = nKV; m.group = nH / nKV; m.hd = hd; m.L = 1;
    m.paged = 1; m.Tmax = block_size; m.num_blocks = n_blocks; m.blocks_per_seq = tbl_stride;
    m.layer_stride = (int64_t)nKV * block_size * hd; m.slot_stride = m.layer_stride;
    m.n_qkv = (nH + 2 * nKV) * hd;
    m.attn_scale = scale != 0.f ? scale : 1.0f / std::sqrt((float)hd);
    m.kv8 = kv8; m.kv_esize = kv8 ? 1 : (int)m.wsize;
    uint8_t *k8 = nullptr, *v8 = nullptr;
    if (kv8) {      // the 8-bit blocks, written by the shared quantizer from the fp32 values
        const float* dk = cx.up_f32(k_pool, n_el);
        const float* dv = cx.up_f32(v_pool, n_el);
        k8 = (uint8_t*)cx.alloc(n_el); v8 = (uint8_t*)cx.alloc(n_el);
        const unsigned qblocks = (unsigned)cdiv(cdiv(n_el, 4), 256);
        hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dk, n_el, k_scale, k8);
        hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dv, n_el, v_scale, v8);
        NVL_HIP(hipGetLastError());
    } else {
        m.kcache = cx.up_mat(k_pool, 1, n_el, false, 1, true);
        m.vcache = cx.up_mat(v_pool, 1, n_el, false, 1, true);
    }
    if (fused) {
        m.qkv = cx.up_f32(q, (int64_t)n_seqs * m.n_qkv);
        if (rope_base > 0.0) {
            std::vector<float> ct, st;
            rope_tables(rope_base, max_seq, hd, ct, st);
            m.rope_cos = cx.up_f32(ct.data(), (int64_t)ct.size());
            m.rope_sin = cx.up_f32(st.data(), (int64_t)st.size());
        }
    } else {
        m.q = cx.up_mat(q, tokens, W, false, 1, true);
    }
    m.attn_out = nan_fill(round_up(tokens, 64) * W * (int64_t)m.wsize);
    if (!m.f32) {       // (nvl_create: the split scratch of every bf16 model with a head size the kernels have)
        m.attn_part = (float*)nan_fill((int64_t)ATTN_SPLIT_MAX_PAIRS * ATTN_SPLIT_MAX * (hd == 64 ? attn_part_floats<64>() : attn_part_floats<128>()) * 4);
        m.attn_part_cnt = (int32_t*)cx.alloc(ATTN_SPLIT_MAX_PAIRS * 4);
        NVL_HIP(hipMemsetAsync(m.attn_part_cnt, 0, ATTN_SPLIT_MAX_PAIRS * 4, m.stream));
    }
    // the pass's metadata as plan_paged / plan_rows leave it: [tok_start | len | pos | tbl | the table, verbatim]
    std::vector<int32_t> meta((size_t)4 * n_seqs + (size_t)n_seqs * tbl_stride);
    for (int i = 0, t = 0; i < n_seqs; t += seq_len[i], i++) {
        meta[(size_t)i] = t; meta[(size_t)n_seqs + i] = seq_len[i]; meta[(size_t)2 * n_seqs + i] = seq_pos[i];
        meta[(size_t)3 * n_seqs + i] = i * tbl_stride;
    }
    memcpy(&meta[(size_t)4 * n_seqs], block_table, (size_t)n_seqs * tbl_stride * 4);
    int32_t* dmeta = (int32_t*)cx.alloc((int64_t)meta.size() * 4);
    NVL_HIP(hipMemcpyAsync(dmeta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, m.stream));
    Meta md{};
    md.seq_tok_start = dmeta; md.seq_len = dmeta + n_seqs; md.seq_pos = dmeta + 2 * n_seqs; md.seq_tbl = dmeta + 3 * n_seqs;
    md.blk_table = dmeta + 4 * n_seqs;
    m.ctx_hint = ctx;                                  // attn_cost: the longest context of the batch
    auto release = [&]() {                             // everything is owned by cx.bufs
        m.q = m.kcache = m.vcache = m.attn_out = nullptr; m.qkv = nullptr; m.rope_cos = m.rope_sin = nullptr;
        m.attn_part = nullptr; m.attn_part_cnt = nullptr;
    };
    try {
        if (kv8) attention_kv8(&m, md, n_seqs, max_len, k8, v8, k_scale, v_scale);
        else attention(&m, 0, md, n_seqs, max_len, 0.0, fused, mq);
    } catch (...) { release(); throw; }
    for (int i = 0; i < 3; i++) ran[i] = m.attn_ran[i];
    // out: token-major [tokens][nH][hd]
    if (m.f32) {
        cx.down(out, m.attn_out, tokens * W);
    } else {
        std::vector<uint16_t> ob((size_t)(round_up(tokens, 64) * W));
        NVL_HIP(hipMemcpyAsync(ob.data(), m.attn_out, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int64_t r = 0; r < tokens; r++)        // the kernel wrote the next GEMM's fragment-major operand
            for (int64_t c = 0; c < W; c++) {
                const uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, W)]) << 16;
                memcpy(&out[(size_t)(r * W + c)], &u, 4);
            }
    }
    std::fill(part_cnt, part_cnt + ATTN_SPLIT_MAX_PAIRS, 0);
    if (m.attn_part_cnt) {
        NVL_HIP(hipMemcpyAsync(part_cnt, m.attn_part_cnt, ATTN_SPLIT_MAX_PAIRS * 4, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
    }
    if (fused) {       // the pools after the append
        std::vector<uint16_t> pb((size_t)n_el);
        for (int which = 0; which < 2; which++) {
            NVL_HIP(hipMemcpyAsync(pb.data(), which ? m.vcache : m.kcache, (size_t)n_el * 2, hipMemcpyDeviceToHost, m.stream));
            NVL_HIP(hipStreamSynchronize(m.stream));
            float* dst = which ? v_pool : k_pool;
            for (int64_t i = 0; i < n_el; i++) {
                const uint32_t u = ((uint32_t)pb[(size_t)i]) << 16;
                memcpy(&dst[i], &u, 4);
            }
        }
    }
    release();
    return NVL_OK;
    OP_CATCH
}

// The front of an attention layer on a paged batch, stage by stage: the forward pass's own embed() and qkv_front() — attention
// norm, QKV projection (+ bias), RoPE, Q into the attention operand buffer, K / V into the cache — under the decisions
// qkv_front() takes (the EPI_QKV tile kernels; the decode-form projection + rope_kv_kernel; rope_kv8_kernel; the fp32
// kernels; a bf16 decode step's bare projection), on a model set up as nvl_create sets a paged one up (Tmax = the block size,
// blocks_per_seq = the table's stride, one layer) and metadata as plan_paged / plan_rows leave it.  Every output and scratch
// buffer starts as 0xFF bytes, the q buffer whole 256-row tiles of them: a padded row m >= M that a tile kernel stored shows.
// THE NON-DEFERRED OPERAND PATH ONLY: the deferred-RMSNorm operand into the QKV projection is held by nvl_op_dense_stages
// (yn with has_next = 1), the fused decode append (what NVL_QKV_FORM_STORE_ONLY leaves to the attention kernel) by
// nvl_op_attention_batch (NVL_ATTN_OP_FUSED).  Nothing that could index outside the pools or the tables reaches a kernel:
// every table entry, used or not, and every token id is checked first.
extern "C" int nvl_op_qkv_stages(int device, int precision, const nvl_qkv_stages* d) {
    const char* who = "nvl_op_qkv_stages: ";
    if (!d || d->struct_bytes != (int32_t)sizeof(nvl_qkv_stages) || (precision != NVL_PRECISION_BF16 && precision != NVL_PRECISION_F32))
        return op_fail(std::string(who) + "bad arguments (struct_bytes = sizeof(nvl_qkv_stages))");
    const int nH = d->nH, nKV = d->nKV, hd = d->hd, H = d->hidden, n_seqs = d->n_seqs, bs = d->block_size, stride = d->tbl_stride;
    const bool kv8 = d->kv8 != 0, embed_stage = d->tokens != nullptr;
    if (!d->seq_len || !d->seq_pos || !d->block_table || !d->w_qkv || !d->k_pool || !d->v_pool || !d->x || !d->op || !d->qkv || !d->q || !d->ran)
        return op_fail(std::string(who) + "null argument");
    if (nH <= 0 || nKV <= 0 || nH % nKV || (hd != 64 && hd != 128) || H <= 0 || H % 64 || n_seqs <= 0 || n_seqs > 4096 || d->n_blocks <= 0 ||
        bs <= 0 || bs % 64 || stride <= 0 || d->max_seq <= 0 || (d->kv8 != 0 && d->kv8 != 1))
        return op_fail(std::string(who) + "bad shape (hd 64 / 128, hidden % 64, block_size % 64)");
    if (kv8 && precision != NVL_PRECISION_BF16) return op_fail(std::string(who) + "the 8-bit cache is bf16 only");
    if (kv8 && (!(d->k_scale > 0.f) || !(d->v_scale > 0.f) || !std::isfinite(d->k_scale) || !std::isfinite(d->v_scale)))
        return op_fail(std::string(who) + "k_scale / v_scale must be finite and positive");
    if (!(d->rope_base >= 0.0) || !std::isfinite(d->rope_base)) return op_fail(std::string(who) + "rope_base must be finite and >= 0");
    if ((d->norm_type != NVL_NORM_RMS && d->norm_type != NVL_NORM_LAYER) || !(d->norm_eps >= 0.f) || !std::isfinite(d->norm_eps))
        return op_fail(std::string(who) + "bad norm_type / norm_eps");
    if (d->norm_w && d->norm_type == NVL_NORM_LAYER && !d->norm_b) return op_fail(std::string(who) + "LayerNorm needs its bias");
    if (d->norm_b && (!d->norm_w || d->norm_type != NVL_NORM_LAYER)) return op_fail(std::string(who) + "norm_b belongs to a LayerNorm");
    if (embed_stage && (!d->tok_pos || !d->emb || d->vocab <= 0 || !d->norm_w || (d->pos_emb && d->pos_rows <= 0) || !std::isfinite(d->embedding_multiplier)))
        return op_fail(std::string(who) + "the embedding stage needs tokens, tok_pos, emb [vocab][hidden] and a norm behind it");
    // plan_paged's refusals, in its order, then the rest of the table and the token rows
    int64_t tokens = 0;
    int max_len = 0;
    for (int i = 0; i < n_seqs; i++) {
        if (d->seq_len[i] <= 0 || d->seq_len[i] > (1 << 16)) return op_fail(std::string(who) + "sequence without rows (or more than 65536)");
        if (d->seq_pos[i] < 0) return op_fail(std::string(who) + "negative position");
        if (d->seq_pos[i] > d->max_seq - d->seq_len[i]) return op_fail(std::string(who) + "position exceeds max_seq", NVL_ERR_POSITION);
        if (stride < cdiv((int64_t)d->seq_pos[i] + d->seq_len[i], bs)) return op_fail(std::string(who) + "block table shorter than the positions it must cover");
        tokens += d->seq_len[i];
        max_len = std::max(max_len, d->seq_len[i]);
    }
    if (tokens > (1 << 16)) return op_fail(std::string(who) + "more than 65536 rows");
    for (int64_t i = 0; i < (int64_t)n_seqs * stride; i++)
        if (d->block_table[i] < 0 || d->block_table[i] >= d->n_blocks) return op_fail(std::string(who) + "block id out of range");
    for (int64_t t = 0; embed_stage && t < tokens; t++) {
        if (d->tokens[t] < 0 || d->tokens[t] >= d->vocab) return op_fail(std::string(who) + "token id out of range");
        if (d->tok_pos[t] < 0) return op_fail(std::string(who) + "negative position");
    }
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    auto nan_fill = [&](int64_t bytes) { void* p = cx.alloc(bytes); NVL_HIP(hipMemsetAsync(p, 0xFF, (size_t)bytes, m.stream)); return p; };
    const int M = (int)tokens;
    const int64_t qw = (int64_t)nH * hd, n_el = (int64_t)d->n_blocks * nKV * bs * hd, Mp = round_up(M, 64), Mq = round_up(M, 256);
    m.H = H; m.nH = nH; m.nKV = nKV; m.group = nH / nKV; m.hd = hd; m.L = 1; m.n_qkv = (nH + 2 * nKV) * hd;
    m.paged = 1; m.Tmax = bs; m.num_blocks = d->n_blocks; m.blocks_per_seq = stride;
    m.layer_stride = (int64_t)nKV * bs * hd; m.slot_stride = m.layer_stride;
    m.kv8 = kv8; m.kv_esize = kv8 ? 1 : (int)m.wsize;
    m.k_scale.assign(1, d->k_scale); m.v_scale.assign(1, d->v_scale);
    m.cfg.norm_type = d->norm_type; m.cfg.norm_eps = d->norm_eps; m.cfg.max_seq_len = d->max_seq;
    m.cfg.position_type = d->pos_emb ? NVL_POS_LEARNED : (d->rope_base > 0.0 ? NVL_POS_ROPE : NVL_POS_NONE);
    m.cfg.embedding_multiplier = d->embedding_multiplier;
    m.keep_hidden = false;
    // workspaces (nvl_create, max_batch_tokens = tokens; q in whole 256-row tiles)
    m.x = embed_stage ? (float*)nan_fill((int64_t)M * H * 4) : cx.up_f32(d->x, (int64_t)M * H);
    m.xn = d->norm_w ? nan_fill(Mp * H * (int64_t)m.wsize) : cx.up_mat(d->x, M, H, false);
    m.qkv = (float*)nan_fill((int64_t)M * m.n_qkv * 4);
    m.q = nan_fill(Mq * qw * (int64_t)m.wsize);
    if (kv8) {      // the 8-bit blocks, written by the shared quantizer from the fp32 values
        const float* dk = cx.up_f32(d->k_pool, n_el);
        const float* dv = cx.up_f32(d->v_pool, n_el);
        m.kcache = cx.alloc(n_el); m.vcache = cx.alloc(n_el);
        const unsigned qblocks = (unsigned)cdiv(cdiv(n_el, 4), 256);
        hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dk, n_el, d->k_scale, (uint8_t*)m.kcache);
        hipLaunchKernelGGL(kv8_quant_kernel, dim3(qblocks), dim3(256), 0, m.stream, dv, n_el, d->v_scale, (uint8_t*)m.vcache);
        NVL_HIP(hipGetLastError());
    } else {
        m.kcache = cx.up_mat(d->k_pool, 1, n_el, false, 1, true);
        m.vcache = cx.up_mat(d->v_pool, 1, n_el, false, 1, true);
    }
    if (d->rope_base > 0.0) {
        std::vector<float> ct, st;
        rope_tables(d->rope_base, d->max_seq, hd, ct, st);
        m.rope_cos = cx.up_f32(ct.data(), (int64_t)ct.size());
        m.rope_sin = cx.up_f32(st.data(), (int64_t)st.size());
    }
    // weights (finalize's forms)
    LayerW l;
    l.w_qkv = cx.up_mat(d->w_qkv, m.n_qkv, H, false, W_ROW_PAD);
    l.n_qkv = m.n_qkv;
    if (d->b_qkv) l.b_qkv = cx.up_f32(d->b_qkv, m.n_qkv);
    if (d->norm_w) l.t[NVL_T_ATTN_NORM_W].p = cx.up_f32(d->norm_w, H);
    if (d->norm_b) l.t[NVL_T_ATTN_NORM_B].p = cx.up_f32(d->norm_b, H);
    if (embed_stage) {
        m.g[NVL_T_TOK_EMB].p = cx.up_mat(d->emb, d->vocab, H, false, W_ROW_PAD);
        if (d->pos_emb) { m.g[NVL_T_POS_EMB].p = cx.up_mat(d->pos_emb, d->pos_rows, H, false, W_ROW_PAD); m.g[NVL_T_POS_EMB].rows = d->pos_rows; }
    }
    // the pass's metadata as plan_paged / plan_rows leave it:
    // [tok_start | len | pos | tbl | the table, verbatim | tokens | tok_pos | tok_tbl | the embedding stage's own tok_pos]
    const size_t S = (size_t)n_seqs, T = (size_t)n_seqs * stride;
    std::vector<int32_t> meta(4 * S + T + 4 * (size_t)M, 0);
    int32_t *h_tok = &meta[4 * S + T], *h_pos = h_tok + M, *h_tbl = h_pos + M, *h_epos = h_tbl + M;
    for (int i = 0, t = 0; i < n_seqs; i++) {
        meta[(size_t)i] = t; meta[S + i] = d->seq_len[i]; meta[2 * S + i] = d->seq_pos[i]; meta[3 * S + i] = i * stride;
        for (int j = 0; j < d->seq_len[i]; j++, t++) {
            h_tok[t] = embed_stage ? d->tokens[t] : 0; h_pos[t] = d->seq_pos[i] + j; h_tbl[t] = i * stride;
            h_epos[t] = embed_stage ? d->tok_pos[t] : h_pos[t];
        }
    }
    memcpy(&meta[4 * S], d->block_table, T * 4);
    int32_t* dmeta = (int32_t*)cx.alloc((int64_t)meta.size() * 4);
    NVL_HIP(hipMemcpyAsync(dmeta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, m.stream));
    Meta md{};
    md.seq_tok_start = dmeta; md.seq_len = dmeta + S; md.seq_pos = dmeta + 2 * S; md.seq_tbl = dmeta + 3 * S; md.blk_table = dmeta + 4 * S;
    md.tokens = md.blk_table + T; md.tok_pos = md.tokens + M; md.tok_tbl = md.tok_pos + M;
    Meta md_embed = md;
    md_embed.tok_pos = md.tok_tbl + M;
    auto release = [&]() {                             // everything is owned by cx.bufs
        m.x = nullptr; m.xn = m.q = m.kcache = m.vcache = nullptr; m.qkv = nullptr; m.rope_cos = m.rope_sin = nullptr;
        for (auto& t : l.t) t.p = nullptr;
        l.w_qkv = nullptr; l.b_qkv = nullptr;
        m.g[NVL_T_TOK_EMB].p = nullptr; m.g[NVL_T_POS_EMB].p = nullptr;
    };
    try {
        std::fill(m.front_ran, m.front_ran + NVL_QKV_RAN_INTS, 0);
        m.phase = max_len > 1 ? 0 : 1;
        if (embed_stage) embed(&m, md_embed, M);
        const bool big_decode = tail_plan(&m, M, n_seqs, max_len, 0).big_decode;
        qkv_front(&m, l, 0, md, M, max_len, big_decode, false, d->norm_w == nullptr);
        // ---- read back
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int i = 0; i < NVL_QKV_RAN_INTS; i++) d->ran[i] = m.front_ran[i];
        if (embed_stage) cx.down(d->x, m.x, (int64_t)M * H);
        auto widen = [&](float* dst, const void* src, int64_t n) {      // n row-major elements of the activation type -> fp32
            if (m.f32) { cx.down(dst, src, n); return; }
            std::vector<uint16_t> b((size_t)n);
            NVL_HIP(hipMemcpyAsync(b.data(), src, (size_t)n * 2, hipMemcpyDeviceToHost, m.stream));
            NVL_HIP(hipStreamSynchronize(m.stream));
            for (int64_t i = 0; i < n; i++) { const uint32_t u = ((uint32_t)b[(size_t)i]) << 16; memcpy(&dst[i], &u, 4); }
        };
        if (m.f32) {
            cx.down(d->op, m.xn, (int64_t)M * H);
        } else {        // the fragment-major operand
            std::vector<uint16_t> ob((size_t)(round_up(M, 16) * H));
            NVL_HIP(hipMemcpyAsync(ob.data(), m.xn, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
            NVL_HIP(hipStreamSynchronize(m.stream));
            for (int64_t r = 0; r < M; r++)
                for (int64_t c = 0; c < H; c++) {
                    const uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, H)]) << 16;
                    memcpy(&d->op[(size_t)(r * H + c)], &u, 4);
                }
        }
        cx.down(d->qkv, m.qkv, (int64_t)M * m.n_qkv);
        widen(d->q, m.q, Mq * qw);
        for (int which = 0; which < 2; which++) {
            float* dst = which ? d->v_pool : d->k_pool;
            const void* src = which ? m.vcache : m.kcache;
            if (!kv8) { widen(dst, src, n_el); continue; }
            std::vector<uint8_t> codes((size_t)n_el);
            NVL_HIP(hipMemcpyAsync(codes.data(), src, (size_t)n_el, hipMemcpyDeviceToHost, m.stream));
            NVL_HIP(hipStreamSynchronize(m.stream));
            const float sc = which ? d->v_scale : d->k_scale;
            for (int64_t i = 0; i < n_el; i++) dst[i] = e4m3fn_value(codes[(size_t)i]) * sc;
            uint8_t* raw = which ? d->v_codes : d->k_codes;
            if (raw) memcpy(raw, codes.data(), (size_t)n_el);
        }
    } catch (...) { release(); throw; }
    release();
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_ffn(int device, int precision, const float* x, const float* w1, const float* b1, const float* w2,
                          const float* b2, int rows, int hidden, int ffn, int swiglu, float* y) {
    if (!x || !w1 || !w2 || !y || rows <= 0 || hidden % 64 || ffn % 64) return op_fail("nvl_op_ffn: bad arguments");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    m.H = hidden; m.F = ffn;
    m.cfg.activation_type = swiglu ? NVL_ACT_SWIGLU : NVL_ACT_GELU;
    m.xn = cx.up_mat(x, rows, hidden, false);
    LayerW l;
    const int n1 = swiglu ? 2 * ffn : ffn;
    void* w1c = cx.up_mat(w1, n1, hidden, true, W_ROW_PAD);   // canonical [n1][H] (gate rows | up rows)
    if (swiglu && !m.f32) {
        auto idx = swiglu_interleave(ffn, 0);
        idx.resize((size_t)round_up(n1, W_ROW_PAD), -1);
        l.w1 = cx.alloc((int64_t)idx.size() * hidden * 2);
        gather_rows(&m, w1c, idx, l.w1, hidden);
    } else {
        l.w1 = w1c;
    }
    if (b1) l.t[NVL_T_B1].p = cx.up_f32(b1, ffn);
    void* w2d = cx.up_mat(w2, hidden, ffn, true, W_ROW_PAD);
    float* b2d = b2 ? cx.up_f32(b2, hidden) : nullptr;
    m.hbuf = cx.alloc(round_up(rows, 64) * ffn * (int64_t)m.wsize);
    if (m.f32 && swiglu) m.h2 = (float*)cx.alloc((int64_t)rows * 2 * ffn * 4);
    ffn_up(&m, l, rows);
    float* yd = (float*)cx.alloc((int64_t)rows * hidden * 4);
    gemm(&m, EPI_STORE, true, mk(m.hbuf, ffn, w2d, yd, hidden, b2d, 1.f, rows, hidden, ffn));
    cx.down(y, yd, (int64_t)rows * hidden);
    l.w1 = nullptr; l.t[NVL_T_B1].p = nullptr;
    m.xn = m.hbuf = nullptr; m.h2 = nullptr;
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_moe(int device, int precision, const float* x, const float* router, const float* w_in,
                          const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter, float* y) {
    if (!x || !router || !w_in || !w_out || !y || rows <= 0 || hidden % 64 || inter % 64 || n_experts > 64 || top_k > n_experts)
        return op_fail("nvl_op_moe: bad arguments");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    m.H = hidden; m.F = inter;
    m.cfg.num_experts = n_experts; m.cfg.num_experts_per_tok = top_k; m.cfg.use_moe = 1; m.cfg.residual_multiplier = 0.f;
    m.xn = cx.up_mat(x, rows, hidden, false);
    LayerW l;
    l.t[NVL_T_ROUTER].p = cx.up_mat(router, n_experts, hidden, true, W_ROW_PAD);
    void* inc = cx.up_mat(w_in, (int64_t)n_experts * 2 * inter, hidden, false, W_ROW_PAD);
    if (!m.f32) {
        std::vector<int32_t> idx;
        for (int e = 0; e < n_experts; e++) {
            auto one = swiglu_interleave(inter, (int64_t)e * 2 * inter);
            idx.insert(idx.end(), one.begin(), one.end());
        }
        l.moe_in = cx.alloc((int64_t)idx.size() * hidden * 2);
        gather_rows(&m, inc, idx, l.moe_in, hidden);
    } else {
        l.moe_in = inc;
    }
    l.t[NVL_T_MOE_OUT].p = cx.up_mat(w_out, (int64_t)n_experts * hidden, inter, false, W_ROW_PAD);
    const int64_t pairs = (int64_t)rows * top_k;
    m.router_logits = (float*)cx.alloc((int64_t)rows * 128 * 4);
    m.expert_ids = (int32_t*)cx.alloc(pairs * 4); m.expert_w = (float*)cx.alloc(pairs * 4);
    m.seg_start = (int32_t*)cx.alloc((n_experts + 1) * 4);
    m.moe_counts = (int32_t*)cx.alloc(n_experts * 4); m.moe_cursor = (int32_t*)cx.alloc(n_experts * 4);
    m.moe_tile_map = (int32_t*)cx.alloc(16 * (cdiv(pairs, 128) + n_experts)); m.moe_n_mtiles = (int32_t*)cx.alloc(16);
    m.perm_token = (int32_t*)cx.alloc(pairs * 4); m.slot_of = (int32_t*)cx.alloc(pairs * 4);
    m.moe_eo = (float*)cx.alloc(pairs * hidden * 4);
    if (!m.f32) m.moe_xg = cx.alloc(round_up(pairs, 64) * hidden * 2);
    m.hbuf = cx.alloc(round_up(pairs, 64) * inter * (int64_t)m.wsize);
    if (m.f32) m.h2 = (float*)cx.alloc(pairs * 2 * inter * 4);
    m.x = (float*)cx.alloc((int64_t)rows * hidden * 4);
    NVL_HIP(hipMemsetAsync(m.x, 0, (size_t)rows * hidden * 4, m.stream));
    m.keep_hidden = true;   // (no norm follows here: keep the stand-alone combine instead of leaving it pending)
    moe(&m, l, rows);    // accumulates into x (zeroed) with multiplier 1
    cx.down(y, m.x, (int64_t)rows * hidden);
    l.moe_in = nullptr; l.t[NVL_T_ROUTER].p = nullptr; l.t[NVL_T_MOE_OUT].p = nullptr;
    m.xn = m.hbuf = nullptr; m.h2 = nullptr; m.x = nullptr; m.router_logits = nullptr; m.expert_ids = nullptr;
    m.expert_w = nullptr; m.seg_start = m.perm_token = m.slot_of = nullptr; m.moe_eo = nullptr; m.moe_xg = nullptr;
    m.moe_counts = m.moe_cursor = m.moe_tile_map = m.moe_n_mtiles = nullptr;
    return NVL_OK;
    OP_CATCH
}

namespace {
// The experts of one MoE layer as a model holds them, for the op entry points that run moe(): finalize's weight forms (the
// interleaved gate|up rows with their zero pad rows, the down matrices side by side along K under finalize's own predicate),
// the decode scratch and the sorted forms' workspaces of nvl_create, every buffer a form owns 0xFF bytes.  Sets m.H, m.F and
// the expert counts; keep_hidden off, so moe_dense_ok() answers as in a model.  router [H][E], w_in [E][2 inter][H],
// w_out [E][H][inter].
// wf: the experts' format (a host format id of wq.h; the router stays bf16).  A quantized format goes the way of a model:
// both tensors through the upload quantizer, then finalize_q_experts() and register_q_experts() — nvl_finalize's own code —,
// so the codes and scales lie where finalize lays them, moe_out_cat = moe_out_q under finalize's predicate, and eq_scratch
// (the grouped forms' W~) starts zeroed as finalize zeroes it.
void moe_op_setup(OpCtx& cx, LayerW& l, const float* router, const float* w_in, const float* w_out, int rows, int H, int E, int k, int inter,
                  int wf = WF_BF16) {
    nvl_model& m = cx.m;
    const int64_t pairs = (int64_t)rows * k, hp = round_up(H, W_ROW_PAD);
    auto nan_fill = [&](int64_t bytes) { void* p = cx.alloc(bytes); NVL_HIP(hipMemsetAsync(p, 0xFF, (size_t)bytes, m.stream)); return p; };
    m.H = H; m.F = inter;
    m.cfg.num_experts = E; m.cfg.num_experts_per_tok = k; m.cfg.use_moe = 1;
    m.keep_hidden = false;
    m.ef = wf;
    // the decode form's scratch (nvl_create) and weight (finalize, under its dense_form predicate)
    m.moe_gate = (float*)nan_fill(64 * (int64_t)E * 4);
    m.moe_hall = nan_fill(64 * (int64_t)E * inter * 2);
    m.moe_part = (float*)nan_fill((int64_t)MOE_DOWN_SLICES * 64 * H * 4);
    const bool dense_form = moe_dense_form(H, E, inter);
    if (dense_form) l.moe_out_cat = wf == WF_BF16 ? cx.alloc(hp * E * inter * 2) : (void*)m.moe_part;   // (quantized: a stand-in for the question below)
    // The grouped GEMMs of the sorted forms stream K in 64-wide tiles (nvl_create refuses ffn_dim % 64 != 0), the decode
    // kernels in 32-wide k-steps: a call that will not take the dense form on inter % 64 == 32 runs on experts padded
    // with 32 zero columns — h = silu(0) * 0 = 0 there, times a zero weight: every sum gains exact zeros.
    const int I = (!moe_dense_ok(&m, l, rows) && inter % 64) ? inter + 32 : inter;
    if (I != inter) { l.moe_out_cat = nullptr; m.F = I; }
    std::vector<float> pin, pout;
    {   // host copies: [E][2I][H] (gate rows, then up rows) and [E][H][I], + 128 zero rows after the last expert's down
        // matrix (the grouped down GEMM stages 128 weight rows of an expert whatever H is)
        pout.assign((size_t)(((int64_t)E * H + 128) * I), 0.f);
        for (int64_t r = 0; r < (int64_t)E * H; r++) memcpy(&pout[(size_t)(r * I)], w_out + r * inter, (size_t)inter * 4);
        if (I != inter) {
            pin.assign((size_t)((int64_t)E * 2 * I * H), 0.f);
            for (int64_t e = 0; e < E; e++)
                for (int half = 0; half < 2; half++)
                    memcpy(&pin[(size_t)((e * 2 * I + (int64_t)half * I) * H)], w_in + (e * 2 * inter + (int64_t)half * inter) * H, (size_t)inter * H * 4);
        }
    }
    l.t[NVL_T_ROUTER].p = cx.up_mat(router, E, H, true, W_ROW_PAD);
    std::vector<int32_t> idx;
    for (int e = 0; e < E; e++) {
        auto one = swiglu_interleave(I, (int64_t)e * 2 * I);
        idx.insert(idx.end(), one.begin(), one.end());
    }
    if (wf != WF_BF16) {
        l.moe_out_cat = nullptr;
        DevTensor &tin = l.t[NVL_T_MOE_IN], &tout = l.t[NVL_T_MOE_OUT];
        try {     // (rows = (expert, output row), as nvl_upload_tensor passes MOE_IN / MOE_OUT)
            upload_2d_q(&m, &tin, wf, I != inter ? pin.data() : w_in, NVL_DTYPE_F32, (int64_t)E * 2 * I, H, false);
            upload_2d_q(&m, &tout, wf, pout.data(), NVL_DTYPE_F32, (int64_t)E * H, I, false);
            finalize_q_experts(&m, l, idx, E, I, dense_form && I == inter);
        } catch (...) {
            for (DevTensor* t : {&tin, &tout}) { dfree(t->p); dfree(t->qs); t->p = t->qs = nullptr; }
            for (void* p : {l.moe_in, l.qs_moe_in, l.moe_out_q, l.qs_moe_out}) dfree(p);
            l.moe_in = l.qs_moe_in = l.moe_out_q = l.qs_moe_out = l.moe_out_cat = nullptr;
            throw;
        }
        for (void* p : {l.moe_in, l.qs_moe_in, l.moe_out_q, l.qs_moe_out}) cx.bufs.push_back(p);
        register_q_experts(&m, &l, 1, E, I);
        cx.bufs.push_back(m.eq_scratch);
    } else {
        void* inc = cx.up_mat(I != inter ? pin.data() : w_in, (int64_t)E * 2 * I, H, false, W_ROW_PAD);
        idx.resize((size_t)round_up((int64_t)E * 2 * I, W_ROW_PAD), -1);      // (+ zero pad rows: the decode kernels read whole tiles)
        l.moe_in = cx.alloc((int64_t)idx.size() * H * 2);
        gather_rows(&m, inc, idx, l.moe_in, H);
        l.t[NVL_T_MOE_OUT].p = cx.up_mat(pout.data(), (int64_t)E * H + 128, I, false, W_ROW_PAD);
        if (l.moe_out_cat) {
            NVL_HIP(hipMemsetAsync(l.moe_out_cat, 0, (size_t)(hp * E * I) * 2, m.stream));
            hipLaunchKernelGGL(moe_cat_down_kernel, dim3((unsigned)(H / 16), (unsigned)E), dim3(256), 0, m.stream,
                               (const bf16_t*)l.t[NVL_T_MOE_OUT].p, (bf16_t*)l.moe_out_cat, H, I, E);
            NVL_HIP(hipGetLastError());
        }
    }
    // the sorted forms' workspaces (nvl_create)
    m.router_logits = (float*)nan_fill((int64_t)rows * 128 * 4);
    m.expert_ids = (int32_t*)cx.alloc(pairs * 4); m.expert_w = (float*)cx.alloc(pairs * 4);
    m.seg_start = (int32_t*)cx.alloc((E + 1) * 4);
    m.moe_counts = (int32_t*)cx.alloc(E * 4); m.moe_cursor = (int32_t*)cx.alloc(E * 4);
    m.moe_tile_map = (int32_t*)cx.alloc(16 * (cdiv(pairs, 128) + E)); m.moe_n_mtiles = (int32_t*)cx.alloc(16);
    m.perm_token = (int32_t*)cx.alloc(pairs * 4); m.slot_of = (int32_t*)cx.alloc(pairs * 4);
    m.moe_eo = (float*)nan_fill(pairs * H * 4);
    m.moe_xg = cx.alloc(round_up(pairs, 64) * H * 2);
    m.hbuf = nan_fill(round_up(pairs, 64) * I * 2);
}
// the fp32 router logits the routing consumed [rows][E] and the dense gate matrix [rows][E] (the sorted forms' expert ids /
// weights scattered on the host); false: the routing chose an expert out of range
bool moe_op_results(OpCtx& cx, int rows, int E, int k, float* router_logits, float* gate) {
    nvl_model& m = cx.m;
    const int64_t pairs = (int64_t)rows * k;
    std::vector<float> lg((size_t)rows * 128);
    cx.down(lg.data(), m.router_logits, (int64_t)rows * 128);
    for (int r = 0; r < rows; r++) memcpy(router_logits + (size_t)r * E, &lg[(size_t)r * 128], (size_t)E * 4);
    if (m.moe_form == NVL_MOE_FORM_DENSE_FUSED || m.moe_form == NVL_MOE_FORM_DENSE) {
        cx.down(gate, m.moe_gate, (int64_t)rows * E);
        return true;
    }
    std::vector<int32_t> ids((size_t)pairs);       // (token, rank) -> dense
    std::vector<float> gw((size_t)pairs);
    NVL_HIP(hipMemcpyAsync(ids.data(), m.expert_ids, (size_t)pairs * 4, hipMemcpyDeviceToHost, m.stream));
    cx.down(gw.data(), m.expert_w, pairs);
    std::fill(gate, gate + (size_t)rows * E, 0.f);
    for (int64_t i = 0; i < pairs; i++) {
        if (ids[(size_t)i] < 0 || ids[(size_t)i] >= E) return false;
        gate[(size_t)((i / k) * E + ids[(size_t)i])] = gw[(size_t)i];
    }
    return true;
}
// the experts' format of the *_q entry points -> the host format id (wfmt.h); -1: what the format's setter would refuse
int moe_op_wf(int expert_format, int group_size, int H, int inter) {
    switch (expert_format) {
        case NVL_OP_EXPERTS_BF16: return WF_BF16;
        case NVL_OP_EXPERTS_FP8: return WF_FP8;
        case NVL_OP_EXPERTS_MXFP4: return WF_MXFP4;
        case NVL_OP_EXPERTS_INT4:
            if ((group_size != 32 && group_size != 64 && group_size != 128) || H % group_size || inter % group_size) return -1;
            return wf_int4(group_size);
        default: return -1;
    }
}
// moe()'s hook: moe_hall between the two projections of the dense-masked form (the sorted forms never call it)
struct MoeHTap {
    nvl_model* m; void* h; int64_t bytes;
    static void call(void* ctx, int which) {
        MoeHTap* t = (MoeHTap*)ctx;
        if (which == TAIL_H && t->h) NVL_HIP(hipMemcpyAsync(t->h, t->m->moe_hall, (size_t)t->bytes, hipMemcpyDeviceToDevice, t->m->stream));
    }
};
inline float bf16_bits_f32(uint16_t b) { const uint32_t u = ((uint32_t)b) << 16; float f; memcpy(&f, &u, 4); return f; }
// the copy of moe_hall (fragment-major [64][E * inter]) -> h [rows][E * inter]; what no launch wrote is NaN
void moe_op_h(OpCtx& cx, const void* hcopy, int rows, int E, int inter, float* h) {
    const int64_t K = (int64_t)E * inter;
    if (cx.m.moe_form != NVL_MOE_FORM_DENSE_FUSED && cx.m.moe_form != NVL_MOE_FORM_DENSE) {      // a sorted form: moe_hall was not touched (and rows may exceed its 64)
        std::fill(h, h + (size_t)rows * K, std::numeric_limits<float>::quiet_NaN());
        return;
    }
    std::vector<uint16_t> hb((size_t)(64 * K));
    NVL_HIP(hipMemcpyAsync(hb.data(), hcopy, hb.size() * 2, hipMemcpyDeviceToHost, cx.m.stream));
    NVL_HIP(hipStreamSynchronize(cx.m.stream));
    for (int64_t r = 0; r < rows; r++)
        for (int64_t c = 0; c < K; c++) h[(size_t)(r * K + c)] = bf16_bits_f32(hb[(size_t)fm_index(r, c, K)]);
}
// W~ of the quantized experts as the device holds them after finalize, read through the grouped forms' own dequantize
// launches (wf_dequant_rows on moe_in / qs_moe_in, dequant_down_experts on moe_out_q / qs_moe_out) into buffers of their
// own and de-interleaved on the host: wt_in [E][2 inter][H] (gate rows, then up rows), wt_out [E][H][inter]
void moe_op_wt(OpCtx& cx, const LayerW& l, int H, int E, int inter, float* wt_in, float* wt_out) {
    nvl_model& m = cx.m;
    const int64_t I = m.F, np = round_up((int64_t)E * 2 * I, W_ROW_PAD);      // (I: inter, or inter + 32 zero columns)
    if (wt_in) {
        bf16_t* d = (bf16_t*)cx.alloc(np * H * 2);
        wf_dequant_rows(m.stream, m.ef, l.moe_in, l.qs_moe_in, H, 0, np, d);
        NVL_HIP(hipGetLastError());
        std::vector<uint16_t> hb((size_t)(np * H));
        NVL_HIP(hipMemcpyAsync(hb.data(), d, hb.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int64_t e = 0; e < E; e++) {
            const auto idx = swiglu_interleave(I, 0);      // device row e * 2I + j holds the expert's canonical row idx[j]
            for (int64_t j = 0; j < 2 * I; j++) {
                const int64_t half = idx[(size_t)j] / I, rr = idx[(size_t)j] % I;
                if (rr >= inter) continue;
                float* dst = wt_in + (size_t)((e * 2 * inter + half * inter + rr) * H);
                for (int64_t c = 0; c < H; c++) dst[c] = bf16_bits_f32(hb[(size_t)fm_index(e * 2 * I + j, c, H)]);
            }
        }
    }
    if (wt_out) {
        bf16_t* d = (bf16_t*)cx.alloc((int64_t)E * H * I * 2);
        dequant_down_experts(&m, l, H, (int)I, E, d);
        std::vector<uint16_t> hb((size_t)((int64_t)E * H * I));
        NVL_HIP(hipMemcpyAsync(hb.data(), d, hb.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int64_t e = 0; e < E; e++)
            for (int64_t r = 0; r < H; r++)
                for (int64_t c = 0; c < inter; c++)
                    wt_out[(size_t)((e * H + r) * inter + c)] = bf16_bits_f32(hb[(size_t)(e * H * I + fm_index(r, c, I))]);
    }
}
void moe_op_release(OpCtx& cx, LayerW& l) {      // (the buffers are the OpCtx's)
    nvl_model& m = cx.m;
    l.qs_moe_in = nullptr; l.moe_out_q = nullptr; l.qs_moe_out = nullptr; m.eq_scratch = nullptr; m.eq_scratch_elems = 0; m.qmap.clear();
    l.moe_in = nullptr; l.moe_out_cat = nullptr; l.t[NVL_T_ROUTER].p = nullptr; l.t[NVL_T_MOE_OUT].p = nullptr;
    m.hbuf = nullptr; m.router_logits = nullptr; m.expert_ids = nullptr;
    m.expert_w = nullptr; m.seg_start = m.perm_token = m.slot_of = nullptr; m.moe_eo = nullptr; m.moe_xg = nullptr;
    m.moe_counts = m.moe_cursor = m.moe_tile_map = m.moe_n_mtiles = nullptr;
    m.moe_gate = nullptr; m.moe_hall = nullptr; m.moe_part = nullptr;
}
}  // namespace

// moe() as a layer of the model runs it, stage by stage: finalize's weight forms (the interleaved gate|up rows with their
// zero pad rows, the down matrices side by side along K under finalize's own predicate), the decode scratch of the
// workspace allocation, keep_hidden off — so moe_dense_ok() answers as it does in a model —, then whatever moe() left for
// the next norm completed by tap_hidden_kernel, as tap_layer does.  Every scratch buffer a form owns starts as 0xFF bytes
// (NaN in bf16 and in fp32): the columns of an expert nobody picked, an unwritten K slice or a stale row show in y.
//
// nvl_op_moe_stages_q: the same with the experts in a quantized format — built as nvl_finalize builds them (moe_op_setup) —,
// W~ read back (moe_op_wt) and moe_hall copied between the dense-masked form's two projections (MoeHTap).
extern "C" int nvl_op_moe_stages_q(int device, int precision, const float* x, const float* router, const float* w_in,
                                   const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter,
                                   int expert_format, int group_size, float* y, float* router_logits, float* gate, int32_t* form,
                                   float* wt_in, float* wt_out, float* h) {
    if (!x || !router || !w_in || !w_out || !y || !router_logits || !gate || !form || precision != NVL_PRECISION_BF16 || rows <= 0 ||
        rows > (1 << 16) || hidden <= 0 || hidden % 64 || inter <= 0 || inter % 32 || n_experts < 1 || n_experts > 64 || top_k < 1 ||
        top_k > n_experts)
        return op_fail("nvl_op_moe_stages: bad arguments (bf16 only; hidden % 64, inter % 32, top_k <= n_experts <= 64)");
    const int wf = moe_op_wf(expert_format, group_size, hidden, inter);
    if (wf < 0) return op_fail("nvl_op_moe_stages_q: unknown expert format, or INT4 experts whose group size is not 32, 64 or 128 or does not divide hidden and inter");
    if (wf == WF_BF16 && (wt_in || wt_out)) return op_fail("nvl_op_moe_stages_q: wt_in / wt_out are the read-back of quantized experts");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    const int E = n_experts, H = hidden, k = top_k;
    m.cfg.residual_multiplier = 0.f; m.resid_alpha = 1.f;      // multiplier 1 both ways (nvl_create's reading of 0)
    LayerW l;
    moe_op_setup(cx, l, router, w_in, w_out, rows, H, E, k, inter, wf);
    m.xn = cx.up_mat(x, rows, H, false);
    m.x = (float*)cx.alloc((int64_t)rows * H * 4);
    NVL_HIP(hipMemsetAsync(m.x, 0, (size_t)rows * H * 4, m.stream));
    MoeHTap tap{&m, nullptr, 64 * (int64_t)E * inter * 2};
    if (h) { tap.h = cx.alloc(tap.bytes); NVL_HIP(hipMemsetAsync(tap.h, 0xFF, (size_t)tap.bytes, m.stream)); }
    const StageHook hook{&MoeHTap::call, &tap};
    moe(&m, l, rows, false, nullptr, h ? &hook : nullptr);
    *form = m.moe_form;
    float* yd = (float*)cx.alloc((int64_t)rows * H * 4);
    if (m.pending_slices == 0) {
        NVL_HIP(hipMemcpyAsync(yd, m.x, (size_t)rows * H * 4, hipMemcpyDeviceToDevice, m.stream));
    } else {       // what the next norm would add on its read of x
        PendingResid pr{m.pending_part, m.pending_slices, m.pending_rows, m.pending_alpha, m.pending_slot_of, m.pending_gate_w};
        hipLaunchKernelGGL(tap_hidden_kernel, dim3(rows), dim3(256), 0, m.stream, m.x, yd, H, pr);
        NVL_HIP(hipGetLastError());
    }
    cx.down(y, yd, (int64_t)rows * H);
    if (!moe_op_results(cx, rows, E, k, router_logits, gate)) return op_fail("nvl_op_moe_stages: the routing chose an expert out of range", NVL_ERR_STATE);
    if (h) moe_op_h(cx, tap.h, rows, E, inter, h);
    if (wf != WF_BF16) moe_op_wt(cx, l, H, E, inter, wt_in, wt_out);
    moe_op_release(cx, l);
    m.xn = nullptr; m.x = nullptr;
    m.pending_part = nullptr; m.pending_slices = 0; m.pending_slot_of = nullptr; m.pending_gate_w = nullptr;
    return NVL_OK;
    OP_CATCH
}
extern "C" int nvl_op_moe_stages(int device, int precision, const float* x, const float* router, const float* w_in,
                                 const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter, float* y,
                                 float* router_logits, float* gate, int32_t* form) {
    return nvl_op_moe_stages_q(device, precision, x, router, w_in, w_out, rows, hidden, n_experts, top_k, inter, NVL_OP_EXPERTS_BF16, 0,
                               y, router_logits, gate, form, nullptr, nullptr, nullptr);
}

// The dense layer tail as a layer of the model runs it — layer_tail() itself, under tail_plan()'s decisions — on host inputs,
// bf16 mode: O projection, FFN norm, FFN-up, FFN-down, the norm after the layer and the projection that reads it (a next
// layer's QKV-shaped projection, or head_proj() on last_rows).  Scratch as nvl_create sizes it (sk_part, rs_part, xn, hbuf,
// xn_last), every scratch buffer and every output 0xFF bytes (NaN as bf16 and as fp32) beforehand.  Between the launches a
// StageHook copies what the next launch will read; a residual add still pending is completed by tap_hidden_kernel into the
// copy, as tap_layer does, and stays pending for the norm that consumes it in the model.
namespace {
struct DenseTap {
    nvl_model* m; int M;
    float *x1, *x2, *rs1; void *op1, *h; int rs1_tiles = 0; int64_t op_bytes, h_bytes, rs_bytes;
    const void* h_src = nullptr;      // (the MoE chain: moe_hall, where moe() raises TAIL_H; else hbuf)
    void take_x(float* dst) {
        if (m->pending_slices == 0) { NVL_HIP(hipMemcpyAsync(dst, m->x, (size_t)M * m->H * 4, hipMemcpyDeviceToDevice, m->stream)); return; }
        PendingResid pr{m->pending_part, m->pending_slices, m->pending_rows, m->pending_alpha, m->pending_slot_of, m->pending_gate_w};
        hipLaunchKernelGGL(tap_hidden_kernel, dim3(M), dim3(256), 0, m->stream, m->x, dst, m->H, pr);
        NVL_HIP(hipGetLastError());
    }
    void stage(int which) {
        if (which == TAIL_X1) take_x(x1);
        else if (which == TAIL_X2) take_x(x2);
        else if (which == TAIL_H) { if (h) NVL_HIP(hipMemcpyAsync(h, h_src ? h_src : m->hbuf, (size_t)h_bytes, hipMemcpyDeviceToDevice, m->stream)); }
        else {
            NVL_HIP(hipMemcpyAsync(op1, m->xn, (size_t)op_bytes, hipMemcpyDeviceToDevice, m->stream));
            NVL_HIP(hipMemcpyAsync(rs1, m->rs_part, (size_t)rs_bytes, hipMemcpyDeviceToDevice, m->stream));
            rs1_tiles = m->dense_ran[NVL_DENSE_RAN_PRODUCER] ? (defer_half(m, M) ? m->H / 8 : m->H / 16) : 0;
        }
    }
    static void call(void* ctx, int which) { ((DenseTap*)ctx)->stage(which); }
};
}  // namespace

extern "C" int nvl_op_dense_stages(int device, int precision, const nvl_dense_stages* d) {
    if (!d || precision != NVL_PRECISION_BF16 || d->struct_bytes != (int32_t)sizeof(nvl_dense_stages))
        return op_fail("nvl_op_dense_stages: bad arguments (bf16 only; struct_bytes = sizeof(nvl_dense_stages))");
    const int M = d->rows, H = d->hidden, qw = d->q_width, F = d->ffn, Nn = d->n_next, nl = d->n_last_rows;
    const bool swiglu = d->activation_type == NVL_ACT_SWIGLU, last = !d->has_next;
    if (!d->x || !d->attn_out || !d->wo || !d->norm_w || !d->w1 || !d->w2 || !d->next_norm_w || !d->wn || !d->x1 || !d->op1 || !d->rs1 ||
        !d->h || !d->x2 || !d->op2 || !d->rs2 || !d->yn || !d->x_end || !d->ran)
        return op_fail("nvl_op_dense_stages: null argument");
    // what nvl_create refuses
    if (M <= 0 || M > SK_TILE_MAX_M || H <= 0 || F <= 0 || qw <= 0 || Nn <= 0 || d->max_len <= 0)
        return op_fail("nvl_op_dense_stages: non-positive dimension (rows <= 2048)");
    if (H % 64 != 0 || F % 64 != 0 || qw % 64 != 0) return op_fail("nvl_op_dense_stages: hidden, ffn and q_width must be multiples of 64");
    if (d->attention_multiplier < 0.f) return op_fail("nvl_op_dense_stages: attention_multiplier must not be negative");
    if ((d->norm_type != NVL_NORM_RMS && d->norm_type != NVL_NORM_LAYER) || (d->activation_type != NVL_ACT_SWIGLU && d->activation_type != NVL_ACT_GELU) ||
        (d->block_style != NVL_BLOCK_SEQUENTIAL && d->block_style != NVL_BLOCK_PARALLEL))
        return op_fail("nvl_op_dense_stages: bad norm_type / activation_type / block_style");
    if (d->norm_type == NVL_NORM_LAYER && (!d->norm_b || !d->next_norm_b)) return op_fail("nvl_op_dense_stages: LayerNorm needs its biases");
    if (last && (!d->last_rows || nl <= 0 || nl > M)) return op_fail("nvl_op_dense_stages: the last layer needs last_rows (1..rows of them)");
    if (!last && (d->last_rows || nl != 0)) return op_fail("nvl_op_dense_stages: last_rows belong to the last layer");
    for (int i = 0; last && i < nl; i++)
        if (d->last_rows[i] < 0 || d->last_rows[i] >= M) return op_fail("nvl_op_dense_stages: last_rows out of range", NVL_ERR_POSITION);
    if (d->max_len == 1 && last && nl != M) return op_fail("nvl_op_dense_stages: a decode pass keeps every row (n_last_rows = rows)");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    auto nan_fill = [&](int64_t bytes) { void* p = cx.alloc(bytes); NVL_HIP(hipMemsetAsync(p, 0xFF, (size_t)bytes, m.stream)); return p; };
    m.H = H; m.F = F; m.hd = 64; m.nH = qw / 64; m.L = last ? 1 : 2;
    m.cfg.norm_type = d->norm_type; m.cfg.activation_type = d->activation_type; m.cfg.block_style = d->block_style;
    m.cfg.norm_eps = d->norm_eps; m.cfg.attention_multiplier = d->attention_multiplier; m.cfg.residual_multiplier = d->residual_multiplier;
    m.cfg.use_moe = 0;
    m.resid_alpha = d->residual_multiplier != 0.f ? d->residual_multiplier : 1.0f;      // (nvl_create)
    m.keep_hidden = false;
    const int64_t Mp = round_up(M, 64), rows_out = last ? nl : M;
    // workspaces (nvl_create, max_batch_tokens = rows)
    m.x = cx.up_f32(d->x, (int64_t)M * H);
    m.attn_out = cx.up_mat(d->attn_out, M, qw, false);
    m.xn = nan_fill(Mp * H * 2);
    m.hbuf = nan_fill(Mp * F * 2);
    m.xn_last = nan_fill(round_up(rows_out, 64) * H * 2);
    m.sk_rows = (int)std::min<int64_t>(std::max<int64_t>(M, 64), SK_TILE_MAX_M);
    const int64_t sk_floats = (int64_t)std::max(m.sk_max_slices, SK_TILE_MAX_SLICES) * m.sk_rows * H;
    m.sk_part = (float*)nan_fill(sk_floats * 4);
    const int64_t rs_floats = (int64_t)cdiv(H, 8) * DEFER_MAX_M;
    m.rs_part = (float*)nan_fill(rs_floats * 4);
    // weights (finalize's forms)
    LayerW l;
    l.t[NVL_T_WO].p = cx.up_mat(d->wo, H, qw, false, W_ROW_PAD);
    if (d->bo) l.t[NVL_T_BO].p = cx.up_f32(d->bo, H);
    l.t[NVL_T_FFN_NORM_W].p = cx.up_f32(d->norm_w, H);
    if (d->norm_b) l.t[NVL_T_FFN_NORM_B].p = cx.up_f32(d->norm_b, H);
    const int n1 = swiglu ? 2 * F : F;
    void* w1c = cx.up_mat(d->w1, n1, H, false, W_ROW_PAD);       // canonical [n1][H] (gate rows | up rows)
    if (swiglu) {
        auto idx = swiglu_interleave(F, 0);
        idx.resize((size_t)round_up(n1, W_ROW_PAD), -1);
        l.w1 = cx.alloc((int64_t)idx.size() * H * 2);
        gather_rows(&m, w1c, idx, l.w1, H);
    } else {
        l.w1 = w1c;
    }
    if (d->b1) l.t[NVL_T_B1].p = cx.up_f32(d->b1, F);
    l.t[NVL_T_W2].p = cx.up_mat(d->w2, H, F, false, W_ROW_PAD);
    if (d->b2) l.t[NVL_T_B2].p = cx.up_f32(d->b2, H);
    m.g[NVL_T_FINAL_NORM_W].p = cx.up_f32(d->next_norm_w, H);     // (the norm after the layer, whichever it is)
    if (d->next_norm_b) m.g[NVL_T_FINAL_NORM_B].p = cx.up_f32(d->next_norm_b, H);
    void* wn = cx.up_mat(d->wn, Nn, H, false, W_ROW_PAD);
    const int ldn = (int)round_up(Nn, 128);
    float* yn = (float*)nan_fill(round_up(rows_out, 64) * (int64_t)ldn * 4);
    int32_t* rows_idx = nullptr;
    if (last) {
        rows_idx = (int32_t*)cx.alloc((int64_t)nl * 4);
        NVL_HIP(hipMemcpyAsync(rows_idx, d->last_rows, (size_t)nl * 4, hipMemcpyHostToDevice, m.stream));
    }
    DenseTap tap{&m, M};
    tap.op_bytes = Mp * H * 2; tap.h_bytes = Mp * F * 2; tap.rs_bytes = rs_floats * 4;
    tap.x1 = (float*)nan_fill((int64_t)M * H * 4); tap.x2 = (float*)nan_fill((int64_t)M * H * 4);
    tap.op1 = nan_fill(tap.op_bytes); tap.h = nan_fill(tap.h_bytes); tap.rs1 = (float*)nan_fill(tap.rs_bytes);
    const StageHook hook{&DenseTap::call, &tap};
    std::fill(m.dense_ran, m.dense_ran + NVL_DENSE_RAN_INTS, 0);
    m.pending_slices = 0;
    m.phase = d->max_len > 1 ? 0 : 1;
    const TailPlan plan = tail_plan(&m, M, last ? nl : (d->max_len == 1 ? M : 1), d->max_len, 0);
    if (d->block_style == NVL_BLOCK_PARALLEL) {      // both branches read the block's one norm, which precedes the attention
        norm(&m, m.x, nullptr, l.t[NVL_T_FFN_NORM_W], l.t[NVL_T_FFN_NORM_B], m.xn, M);
        tap.stage(TAIL_OPERAND);
    }
    const bool xn_deferred = layer_tail(&m, l, 0, M, plan, &m.g[NVL_T_FINAL_NORM_W], &m.g[NVL_T_FINAL_NORM_B], !last, &hook);
    const void* op2_src = m.xn;
    if (!last) {      // the next layer's front: its attention norm unless the operand is deferred, then its projection
        if (!xn_deferred) norm(&m, m.x, nullptr, m.g[NVL_T_FINAL_NORM_W], m.g[NVL_T_FINAL_NORM_B], m.xn, M);
        GemmArgs aq = mk(m.xn, H, wn, yn, ldn, nullptr, 1.f, M, Nn, H);
        if (xn_deferred) set_deferred_in(&m, aq);
        m.site = KS_QKV;
        gemm(&m, EPI_STORE, true, aq);
    } else {
        head_proj(&m, xn_deferred, rows_idx, (int)rows_out, wn, yn, ldn, Nn);
        if (!xn_deferred) op2_src = m.xn_last;
    }
    if (m.pending_slices != 0) throw std::runtime_error("nvl_op_dense_stages: a split-K residual was left unconsumed");
    const int rs2_tiles = xn_deferred ? (defer_half(&m, M) ? H / 8 : H / 16) : 0;
    // ---- read back
    NVL_HIP(hipStreamSynchronize(m.stream));
    cx.down(d->x1, tap.x1, (int64_t)M * H);
    cx.down(d->x2, tap.x2, (int64_t)M * H);
    cx.down(d->x_end, m.x, (int64_t)M * H);
    auto unfrag = [&](float* dst, const void* src, int64_t rows, int64_t K) {
        std::vector<uint16_t> ob((size_t)(round_up(rows, 16) * K));
        NVL_HIP(hipMemcpyAsync(ob.data(), src, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
        NVL_HIP(hipStreamSynchronize(m.stream));
        for (int64_t r = 0; r < rows; r++)
            for (int64_t c = 0; c < K; c++) {
                const uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, K)]) << 16;
                memcpy(&dst[(size_t)(r * K + c)], &u, 4);
            }
    };
    auto partials = [&](float* dst, const float* src, int tiles, int64_t rows) {      // [rows][tiles] of [rows][hidden / 8]
        std::vector<float> rs((size_t)rs_floats);
        cx.down(rs.data(), src, rs_floats);
        for (int64_t r = 0; r < rows; r++)
            for (int t = 0; t < H / 8; t++) dst[(size_t)(r * (H / 8) + t)] = t < tiles ? rs[(size_t)(r * tiles + t)] : 0.f;
    };
    unfrag(d->op1, tap.op1, M, H);
    partials(d->rs1, tap.rs1, tap.rs1_tiles, M);
    unfrag(d->h, tap.h, M, F);
    unfrag(d->op2, op2_src, xn_deferred ? M : rows_out, H);
    partials(d->rs2, m.rs_part, rs2_tiles, M);
    {
        std::vector<float> y((size_t)(rows_out * ldn));
        cx.down(y.data(), yn, rows_out * ldn);
        for (int64_t r = 0; r < rows_out; r++) memcpy(d->yn + (size_t)(r * Nn), &y[(size_t)(r * ldn)], (size_t)Nn * 4);
    }
    for (int i = 0; i < NVL_DENSE_RAN_INTS; i++) d->ran[i] = m.dense_ran[i];
    d->ran[NVL_DENSE_RAN_RS1_TILES] = tap.rs1_tiles; d->ran[NVL_DENSE_RAN_RS2_TILES] = rs2_tiles;
    for (auto& t : l.t) t.p = nullptr;
    l.w1 = nullptr;
    m.g[NVL_T_FINAL_NORM_W].p = nullptr; m.g[NVL_T_FINAL_NORM_B].p = nullptr;
    m.x = nullptr; m.attn_out = m.xn = m.hbuf = m.xn_last = nullptr; m.sk_part = m.rs_part = nullptr;
    m.pending_part = nullptr; m.pending_slices = 0;
    return NVL_OK;
    OP_CATCH
}

// The same tail with a MoE block between the projections, decode only (rows <= 64): the O projection as the deferred-RMSNorm
// producer of the FFN norm, then moe(m, l, M, deferred_norm = true) — the router (in either routing form) and the expert up
// projection scale their accumulators by rstd from the x^2 partials —, whose down projection leaves K slices in moe_part
// pending for the next norm.  layer_tail() again, under tail_plan(); experts and scratch from moe_op_setup().
// nvl_op_dense_moe_stages_q: the experts in a quantized format (moe_op_setup), the O projection and the router bf16; W~ read
// back and moe_hall copied between the two expert projections, as nvl_op_moe_stages_q does.
extern "C" int nvl_op_dense_moe_stages_q(int device, int precision, const float* x, const float* attn_out, const float* wo,
                                         const float* bo, const float* norm_w, const float* router, const float* w_in,
                                         const float* w_out, const float* next_norm_w, int rows, int hidden, int q_width,
                                         int n_experts, int top_k, int inter, float residual_multiplier, float norm_eps,
                                         int expert_format, int group_size, float* x1, float* op1, float* rs1, float* router_logits,
                                         float* gate, float* y, int32_t* form, int32_t* ran, float* wt_in, float* wt_out, float* h) {
    if (!x || !attn_out || !wo || !norm_w || !router || !w_in || !w_out || !next_norm_w || !x1 || !op1 || !rs1 || !router_logits ||
        !gate || !y || !form || !ran || precision != NVL_PRECISION_BF16 || rows <= 0 || rows > 64 || hidden <= 0 || hidden % 64 ||
        q_width <= 0 || q_width % 64 || inter <= 0 || inter % 64 || n_experts < 1 || n_experts > 64 || top_k < 1 || top_k > n_experts)
        return op_fail("nvl_op_dense_moe_stages: bad arguments (bf16 only; rows <= 64; hidden, q_width, inter % 64; top_k <= n_experts <= 64)");
    const int wf = moe_op_wf(expert_format, group_size, hidden, inter);
    if (wf < 0) return op_fail("nvl_op_dense_moe_stages_q: unknown expert format, or INT4 experts whose group size is not 32, 64 or 128 or does not divide hidden and inter");
    if (wf == WF_BF16 && (wt_in || wt_out)) return op_fail("nvl_op_dense_moe_stages_q: wt_in / wt_out are the read-back of quantized experts");
    OP_TRY
    OpCtx cx(device, precision);
    nvl_model& m = cx.m;
    const int M = rows, H = hidden, E = n_experts;
    auto nan_fill = [&](int64_t bytes) { void* p = cx.alloc(bytes); NVL_HIP(hipMemsetAsync(p, 0xFF, (size_t)bytes, m.stream)); return p; };
    m.hd = 64; m.nH = q_width / 64; m.L = 2;
    m.cfg.norm_type = NVL_NORM_RMS; m.cfg.activation_type = NVL_ACT_SWIGLU; m.cfg.block_style = NVL_BLOCK_SEQUENTIAL;
    m.cfg.norm_eps = norm_eps; m.cfg.residual_multiplier = residual_multiplier;
    m.resid_alpha = residual_multiplier != 0.f ? residual_multiplier : 1.0f;      // (nvl_create)
    LayerW l;
    moe_op_setup(cx, l, router, w_in, w_out, M, H, E, top_k, inter, wf);
    const int64_t Mp = round_up(M, 64);
    m.x = cx.up_f32(x, (int64_t)M * H);
    m.attn_out = cx.up_mat(attn_out, M, q_width, false);
    m.xn = nan_fill(Mp * H * 2);
    m.sk_rows = 64;
    m.sk_part = (float*)nan_fill((int64_t)std::max(m.sk_max_slices, SK_TILE_MAX_SLICES) * m.sk_rows * H * 4);
    const int64_t rs_floats = (int64_t)cdiv(H, 8) * DEFER_MAX_M;
    m.rs_part = (float*)nan_fill(rs_floats * 4);
    l.t[NVL_T_WO].p = cx.up_mat(wo, H, q_width, false, W_ROW_PAD);
    if (bo) l.t[NVL_T_BO].p = cx.up_f32(bo, H);
    l.t[NVL_T_FFN_NORM_W].p = cx.up_f32(norm_w, H);
    m.g[NVL_T_FINAL_NORM_W].p = cx.up_f32(next_norm_w, H);
    DenseTap tap{&m, M};
    tap.op_bytes = Mp * H * 2; tap.h_bytes = 0; tap.rs_bytes = rs_floats * 4;
    tap.x1 = (float*)nan_fill((int64_t)M * H * 4); tap.x2 = (float*)nan_fill((int64_t)M * H * 4);
    tap.op1 = nan_fill(tap.op_bytes); tap.h = nullptr; tap.rs1 = (float*)nan_fill(tap.rs_bytes);
    if (h) { tap.h_bytes = 64 * (int64_t)E * inter * 2; tap.h = nan_fill(tap.h_bytes); tap.h_src = m.moe_hall; }      // (TAIL_H comes from moe() here)
    const StageHook hook{&DenseTap::call, &tap};
    std::fill(m.dense_ran, m.dense_ran + NVL_DENSE_RAN_INTS, 0);
    m.pending_slices = 0;
    m.phase = 1;
    const TailPlan plan = tail_plan(&m, M, M, 1, 0);
    const bool xn_deferred = layer_tail(&m, l, 0, M, plan, &m.g[NVL_T_FINAL_NORM_W], &m.g[NVL_T_FINAL_NORM_B], true, &hook);
    *form = m.moe_form;
    NVL_HIP(hipStreamSynchronize(m.stream));
    cx.down(x1, tap.x1, (int64_t)M * H);
    cx.down(y, tap.x2, (int64_t)M * H);
    {
        std::vector<uint16_t> ob((size_t)(round_up(M, 16) * H));
        NVL_HIP(hipMemcpyAsync(ob.data(), tap.op1, ob.size() * 2, hipMemcpyDeviceToHost, m.stream));
        std::vector<float> rs((size_t)rs_floats);
        cx.down(rs.data(), tap.rs1, rs_floats);
        for (int64_t r = 0; r < M; r++) {
            for (int64_t c = 0; c < H; c++) {
                const uint32_t u = ((uint32_t)ob[(size_t)fm_index(r, c, H)]) << 16;
                memcpy(&op1[(size_t)(r * H + c)], &u, 4);
            }
            for (int t = 0; t < H / 8; t++) rs1[(size_t)(r * (H / 8) + t)] = t < tap.rs1_tiles ? rs[(size_t)(r * tap.rs1_tiles + t)] : 0.f;
        }
    }
    if (!moe_op_results(cx, M, E, top_k, router_logits, gate)) return op_fail("nvl_op_dense_moe_stages: the routing chose an expert out of range", NVL_ERR_STATE);
    for (int i = 0; i < NVL_DENSE_RAN_INTS; i++) ran[i] = m.dense_ran[i];
    ran[NVL_DENSE_RAN_SLICES + 4] = m.pending_slices;      // (what moe() left for the next norm: its down projection is no resid_gemm)
    ran[NVL_DENSE_RAN_RS1_TILES] = tap.rs1_tiles; ran[NVL_DENSE_RAN_RS2_TILES] = xn_deferred ? 1 : 0;
    if (h) moe_op_h(cx, tap.h, M, E, inter, h);
    if (wf != WF_BF16) moe_op_wt(cx, l, H, E, inter, wt_in, wt_out);
    moe_op_release(cx, l);
    for (auto& t : l.t) t.p = nullptr;
    m.g[NVL_T_FINAL_NORM_W].p = nullptr;
    m.x = nullptr; m.attn_out = m.xn = nullptr; m.sk_part = m.rs_part = nullptr;
    m.pending_part = nullptr; m.pending_slices = 0; m.pending_slot_of = nullptr; m.pending_gate_w = nullptr;
    return NVL_OK;
    OP_CATCH
}
extern "C" int nvl_op_dense_moe_stages(int device, int precision, const float* x, const float* attn_out, const float* wo,
                                       const float* bo, const float* norm_w, const float* router, const float* w_in,
                                       const float* w_out, const float* next_norm_w, int rows, int hidden, int q_width,
                                       int n_experts, int top_k, int inter, float residual_multiplier, float norm_eps,
                                       float* x1, float* op1, float* rs1, float* router_logits, float* gate, float* y,
                                       int32_t* form, int32_t* ran) {
    return nvl_op_dense_moe_stages_q(device, precision, x, attn_out, wo, bo, norm_w, router, w_in, w_out, next_norm_w, rows, hidden, q_width,
                                     n_experts, top_k, inter, residual_multiplier, norm_eps, NVL_OP_EXPERTS_BF16, 0, x1, op1, rs1,
                                     router_logits, gate, y, form, ran, nullptr, nullptr, nullptr);
}

extern "C" int nvl_op_argmax(int device, const float* x, int rows, int cols, int32_t* out) {
    if (!x || !out || rows <= 0 || cols <= 0) return op_fail("nvl_op_argmax: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* dx = cx.up_f32(x, (int64_t)rows * cols);
    int32_t* d = (int32_t*)cx.alloc((int64_t)rows * 4);
    const int chunks = cdiv(cols, ARGMAX_CHUNK);
    float* pv = (float*)cx.alloc((int64_t)rows * chunks * 4);
    int32_t* pi = (int32_t*)cx.alloc((int64_t)rows * chunks * 4);
    launch_argmax(cx.m.stream, dx, cols, cols, rows, 0.f, pv, pi, d);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipMemcpyAsync(out, d, (size_t)rows * 4, hipMemcpyDeviceToHost, cx.m.stream));
    NVL_HIP(hipStreamSynchronize(cx.m.stream));
    return NVL_OK;
    OP_CATCH
}


// Tuning/measurement entry: time one projection GEMM shape on the device with HIP events.
// epi: 0 STORE(fp32 out) 1 RESID 2 SWIGLU 3 GELU; force_bnt/force_ksplit = 0 -> automatic.
extern "C" int nvl_op_sample(int device, const float* logits, int rows, int V, const nvl_sampling_params* params,
                             const int32_t* const* history_ptrs, const int32_t* history_lens, const float* uniforms,
                             int32_t* out_tokens, float* probs_out) {
    if (!logits || rows <= 0 || V <= 0) return op_fail("nvl_op_sample: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* L = cx.up_f32(logits, (int64_t)rows * V);
    SampleBufs b;
    std::string err;
    int rc;
    try { rc = sample_rows(cx.m.stream, b, L, V, rows, V, params, history_ptrs, history_lens, uniforms, out_tokens, probs_out, err); }
    catch (...) { free_sample_bufs(b); throw; }
    free_sample_bufs(b);
    return rc ? op_fail("nvl_op_sample: " + err, rc) : NVL_OK;
    OP_CATCH
}

// The sampler of a sampled verify pass (sample_row_kernel<true>, histories in the offset form) and its accept kernel on
// host logits [n_seqs * (1+k)][V].
extern "C" int nvl_op_sample_drafts(int device, const float* logits, int n_seqs, int k, int V, const nvl_sampling_params* params,
                                    const int32_t* tokens, const int32_t* const* history_ptrs, const int32_t* history_lens,
                                    const float* uniforms, int32_t* sampled_out, int32_t* n_accepted_out, int32_t* out_tokens,
                                    float* probs_out) {
    if (!logits || n_seqs <= 0 || k < 0 || k > 7 || V <= 0 || !params || !tokens || !history_ptrs || !history_lens || !uniforms || !sampled_out)
        return op_fail("nvl_op_sample_drafts: bad arguments");
    const int S = 1 + k, M = n_seqs * S;
    const SampledReq rq{params, history_ptrs, history_lens, uniforms};
    if (const char* why = sampled_check(rq, n_seqs, tokens, S, 0, INT64_MAX, (int64_t)M)) return op_fail(std::string("nvl_op_sample_drafts: ") + why);
    for (int r = 0; r < M; r++) if (tokens[r] < 0) return op_fail("nvl_op_sample_drafts: negative token id");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    std::vector<int32_t> off((size_t)n_seqs + 1, 0), hist;
    for (int i = 0; i < n_seqs; i++) {
        hist.insert(hist.end(), history_ptrs[i], history_ptrs[i] + history_lens[i]);
        off[(size_t)i + 1] = (int32_t)hist.size();
    }
    const int64_t Vp = round_up(V, 4);
    auto up_i32 = [&](const void* h, int64_t n) {
        void* d = cx.alloc(n * 4);
        NVL_HIP(hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, cx.m.stream));
        return d;
    };
    SampleArgs a{};
    a.logits = cx.up_f32(logits, (int64_t)M * V); a.ld = V;
    a.work = (float*)cx.alloc((int64_t)M * Vp * 4);
    a.cnt = (int32_t*)cx.alloc((int64_t)M * V * 4);
    NVL_HIP(hipMemsetAsync(a.cnt, 0, (size_t)M * V * 4, cx.m.stream));
    a.hist = (const int32_t*)up_i32(hist.data(), (int64_t)hist.size()); a.hist_off = (const int32_t*)up_i32(off.data(), (int64_t)off.size());
    a.uniforms = (const float*)up_i32(uniforms, M);
    a.out = (int32_t*)cx.alloc((int64_t)M * 4);
    a.probs_out = probs_out ? (float*)cx.alloc((int64_t)M * V * 4) : nullptr; a.ldp = V;
    a.V = V; a.top_k = params->top_k; a.temperature = params->temperature; a.top_p = params->top_p; a.rep_penalty = params->repetition_penalty;
    a.ext = (const int32_t*)up_i32(tokens, M); a.ext_S = S; a.hist_row = nullptr; a.params = nullptr;
    int32_t* res = (int32_t*)cx.alloc((int64_t)(n_seqs + M) * 4);
    hipLaunchKernelGGL(sample_row_kernel<true>, dim3(M), dim3(SAMPLE_THREADS), 0, cx.m.stream, a);
    NVL_HIP(hipGetLastError());
    hipLaunchKernelGGL(verify_accept_sampled_kernel, dim3(cdiv(n_seqs, 64)), dim3(64), 0, cx.m.stream, (const int32_t*)a.out, a.ext, k, n_seqs,
                       res, (int32_t*)nullptr, (int64_t)0, (int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipMemcpyAsync(sampled_out, a.out, (size_t)M * 4, hipMemcpyDeviceToHost, cx.m.stream));
    if (n_accepted_out) NVL_HIP(hipMemcpyAsync(n_accepted_out, res, (size_t)n_seqs * 4, hipMemcpyDeviceToHost, cx.m.stream));
    if (out_tokens) NVL_HIP(hipMemcpyAsync(out_tokens, res + n_seqs, (size_t)M * 4, hipMemcpyDeviceToHost, cx.m.stream));
    if (probs_out) NVL_HIP(hipMemcpyAsync(probs_out, a.probs_out, (size_t)M * V * 4, hipMemcpyDeviceToHost, cx.m.stream));
    NVL_HIP(hipStreamSynchronize(cx.m.stream));   // (also keeps the host vectors alive until the copies are done)
    return NVL_OK;
    OP_CATCH
}

// spec_reject_kernel (spec.h) on host distributions: p [n_seqs][1+k][V] (the target's rows), q [n_seqs][k][V]
// (the draft's steps), rows padded to round_up(V, 4) floats on upload as the model path keeps them.
extern "C" int nvl_op_spec_reject(int device, const float* p, const float* q, const int32_t* tokens, int n_seqs, int k, int V,
                                  const float* accept_uniforms, const float* final_uniforms, int32_t* n_accepted_out,
                                  int32_t* out_tokens, float* accept_prob_out) {
    if (!p || !q || !tokens || n_seqs <= 0 || k < 1 || k > 7 || V <= 0 || !accept_uniforms || !final_uniforms || !n_accepted_out || !out_tokens)
        return op_fail("nvl_op_spec_reject: bad arguments");
    const int S = 1 + k, M = n_seqs * S;
    for (int i = 0; i < n_seqs; i++)
        for (int j = 1; j < S; j++)
            if (tokens[i * S + j] < 0 || tokens[i * S + j] >= V) return op_fail("nvl_op_spec_reject: draft id outside the vocabulary");
    for (int i = 0; i < n_seqs * k; i++) if (!(accept_uniforms[i] >= 0.f && accept_uniforms[i] <= 1.f)) return op_fail("nvl_op_spec_reject: uniform draw outside [0, 1]");
    for (int i = 0; i < n_seqs; i++) if (!(final_uniforms[i] >= 0.f && final_uniforms[i] <= 1.f)) return op_fail("nvl_op_spec_reject: uniform draw outside [0, 1]");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    const int64_t Vp = round_up(V, 4);
    auto up_rows = [&](const float* h, int64_t rows) {
        float* d = (float*)cx.alloc(rows * Vp * 4);
        NVL_HIP(hipMemsetAsync(d, 0, (size_t)(rows * Vp) * 4, cx.m.stream));
        NVL_HIP(hipMemcpy2DAsync(d, (size_t)Vp * 4, h, (size_t)V * 4, (size_t)V * 4, (size_t)rows, hipMemcpyHostToDevice, cx.m.stream));
        return d;
    };
    auto up_words = [&](const void* h, int64_t n) {
        void* d = cx.alloc(n * 4);
        NVL_HIP(hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, cx.m.stream));
        return d;
    };
    std::vector<float> u((size_t)M);
    for (int i = 0; i < n_seqs; i++) {
        for (int j = 0; j < k; j++) u[(size_t)i * S + j] = accept_uniforms[(size_t)i * k + j];
        u[(size_t)i * S + k] = final_uniforms[i];
    }
    SpecArgs a{};
    a.p = up_rows(p, M); a.ldp = Vp;
    a.q = up_rows(q, (int64_t)n_seqs * k); a.ldq = Vp; a.q_seq = k; a.q_step = 1;
    a.tokens = (const int32_t*)up_words(tokens, M);
    a.u = (const float*)up_words(u.data(), M);
    a.res = (int32_t*)cx.alloc((int64_t)(n_seqs + M) * 4);
    a.accept_prob = (float*)cx.alloc((int64_t)n_seqs * k * 2 * 4);
    a.k = k; a.V = V;
    hipLaunchKernelGGL(spec_reject_kernel, dim3(n_seqs), dim3(SAMPLE_THREADS), 0, cx.m.stream, a);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipMemcpyAsync(n_accepted_out, a.res, (size_t)n_seqs * 4, hipMemcpyDeviceToHost, cx.m.stream));
    NVL_HIP(hipMemcpyAsync(out_tokens, a.res + n_seqs, (size_t)M * 4, hipMemcpyDeviceToHost, cx.m.stream));
    if (accept_prob_out) NVL_HIP(hipMemcpyAsync(accept_prob_out, a.accept_prob, (size_t)n_seqs * k * 2 * 4, hipMemcpyDeviceToHost, cx.m.stream));
    NVL_HIP(hipStreamSynchronize(cx.m.stream));   // (also keeps the host vector alive until the copies are done)
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_op_logprobs(int device, const float* logits, int rows, int V, int ld, float logits_scaling,
                               const int32_t* targets, int top_k, float* logprob_out, int32_t* argmax_out,
                               int32_t* topk_ids_out, float* topk_logprob_out) {
    if (!logits || rows <= 0 || V <= 0 || ld < V) return op_fail("nvl_op_logprobs: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_F32);
    float* L = cx.up_f32(logits, (int64_t)rows * ld);
    LogprobBufs b;
    std::string err;
    int rc;
    try { rc = logprob_rows(cx.m.stream, b, L, ld, rows, V, logits_scaling, targets, top_k, logprob_out, argmax_out, topk_ids_out, topk_logprob_out, err); }
    catch (...) { free_logprob_bufs(b); throw; }
    free_logprob_bufs(b);
    return rc ? op_fail("nvl_op_logprobs: " + err, rc) : NVL_OK;
    OP_CATCH
}

extern "C" int nvl_bench_gemm(int device, int M, int N, int K, int epi, int force_bnt, int force_ksplit, int iters,
                              float* avg_us) {
    if (!avg_us || M <= 0 || N <= 0 || K % 64 || iters <= 0) return op_fail("nvl_bench_gemm: bad arguments");
    OP_TRY
    OpCtx cx(device, NVL_PRECISION_BF16);
    const int64_t Np = round_up(N, W_ROW_PAD);
    std::vector<uint16_t> ha((size_t)round_up(M, 64) * K), hw((size_t)Np * K);
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (uint16_t)(0x3c00u + ((s >> 9) & 0x3ffu) - ((s >> 20) & 1u) * 0x8000u * 0); };
    for (auto& v : ha) { v = rnd(); if (s & 0x80000000u) v |= 0x8000u; }
    for (auto& v : hw) { v = rnd(); if (s & 0x80000000u) v |= 0x8000u; }
    void* A = cx.alloc((int64_t)ha.size() * 2);
    NVL_HIP(hipMemcpy(A, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    // decode shapes (M <= 64) are weight-streaming: rotate through enough copies of W (> 512 MiB in all) that every
    // launch reads its weights cold from HBM, as in the model, not from the 256 MiB Infinity Cache
    const int64_t wbytes = (int64_t)hw.size() * 2;
    const int copies = M <= 64 ? (int)std::min<int64_t>(64, std::max<int64_t>(1, (640ll << 20) / wbytes + 1)) : 1;
    std::vector<void*> Ws((size_t)copies);
    for (int cidx = 0; cidx < copies; cidx++) {
        Ws[(size_t)cidx] = cx.alloc(wbytes);
        if (cidx == 0) NVL_HIP(hipMemcpy(Ws[0], hw.data(), (size_t)wbytes, hipMemcpyHostToDevice));
        else NVL_HIP(hipMemcpy(Ws[(size_t)cidx], Ws[0], (size_t)wbytes, hipMemcpyDeviceToDevice));
    }
    const int ldc = epi == EPI_SWIGLU ? N / 2 : (int)round_up(N, 4);
    void* C = cx.alloc(round_up(M, 64) * ldc * 4);
    NVL_HIP(hipMemsetAsync(C, 0, (size_t)round_up(M, 64) * ldc * 4, cx.m.stream));
    float* bias = nullptr;
    if (epi == EPI_GELU) { bias = (float*)cx.alloc((int64_t)N * 4); NVL_HIP(hipMemsetAsync(bias, 0, (size_t)N * 4, cx.m.stream)); }
    GemmArgs a = mk(A, K, Ws[0], C, ldc, bias, 1e-3f, M, N, K);
    g_force_ntw = force_bnt; g_force_ksplit = force_ksplit;
    if (M > 64) { g_force_tile = force_bnt; g_force_ntw = 0; }   // prefill shapes: force_bnt selects the tile kernel (1/2)
    for (int i = 0; i < 3; i++) gemm(&cx.m, epi, epi == EPI_STORE, a);
    hipEvent_t e0, e1;
    NVL_HIP(hipEventCreate(&e0)); NVL_HIP(hipEventCreate(&e1));
    NVL_HIP(hipEventRecord(e0, cx.m.stream));
    for (int i = 0; i < iters; i++) { a.W = Ws[(size_t)(i % copies)]; gemm(&cx.m, epi, epi == EPI_STORE, a); }
    NVL_HIP(hipEventRecord(e1, cx.m.stream));
    NVL_HIP(hipEventSynchronize(e1));
    g_force_ntw = 0; g_force_ksplit = 0; g_force_tile = 0;
    float ms = 0.f;
    NVL_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = ms * 1e3f / (float)iters;
    return NVL_OK;
    OP_CATCH
}

extern "C" int nvl_set_tuning(int key, int value) {
    g_tune_epoch++;        // captured decode graphs bake the tuning in: a new epoch makes them miss
    if (key == 21) { const int old = g_use_graphs; g_use_graphs = value; return old; }
    if (key == 22) { const int old = g_moe_dense; g_moe_dense = value; return old; }
    if (key == 26) { const int old = g_sk_tile; g_sk_tile = value; return old; }
    if (key == 25) { const int old = g_attn_split; g_attn_split = value; return old; }
    if (key == 24) { const int old = g_x_mask; g_x_mask = value; return old; }
    if (key == 23) { const int old = g_p2p_oneshot_rows; g_p2p_oneshot_rows = value; return old; }
    if (key == 0) { const int old = g_force_tile; g_force_tile = value; return old; }
    if (key == 1) { const int old = g_sk_slices; g_sk_slices = value; return old; }
    if (key == 19) { const int old = g_moe_deep; g_moe_deep = value; return old; }
    if (key == 18) { const int old = g_qkv_store_max_m; g_qkv_store_max_m = value; return old; }
    if (key == 17) { const int old = g_moe_bm; g_moe_bm = value; return old; }
    if (key == 16) { const int old = g_moe_gather; g_moe_gather = value; return old; }
    if (key == 15) { const int old = g_attn_nw; g_attn_nw = value; return old; }
    if (key == 14) { const int old = g_chunk_all_m; g_chunk_all_m = value; return old; }
    if (key == 13) { const int old = g_pass_interleave; g_pass_interleave = value; return old; }
    if (key == 12) { const int old = g_chunk_min_tiles; g_chunk_min_tiles = value; return old; }
    if (key == 11) { const int old = g_chunk_max_m; g_chunk_max_m = value; return old; }
    if (key == 10) { const int old = g_attn_tq2; g_attn_tq2 = value; return old; }
    if (key == 9) { const int old = g_norm_t16; g_norm_t16 = value; return old; }
    if (key == 8) { const int old = g_moe_small; g_moe_small = value; return old; }
    if (key == 7) { const int old = g_decode_seam; g_decode_seam = value; return old; }
    if (key == 6) { const int old = g_msplit_ks; g_msplit_ks = value; return old; }
    if (key == 5) { const int old = g_narrow_waves; g_narrow_waves = value; return old; }
    if (key == 4) { const int old = g_wide_ksplit; g_wide_ksplit = value; return old; }
    if (key == 3) { const int old = g_defer_norm; g_defer_norm = value; return old; }
    if (key == 2) { const int old = g_force_ntw; g_force_ntw = value; return old; }
    if (key == 27) { const int old = g_half_tiles; g_half_tiles = value; return old; }
    if (key == 29) { const int old = g_p2p_spin_ms; g_p2p_spin_ms = value; return old; }
    if (key == 30) { const int old = g_mamba_ssd; g_mamba_ssd = value; return old; }
    if (key == 31) { const int old = g_moe_fused_route; g_moe_fused_route = value; return old; }
    if (key == 33) { const int old = g_moe_defer_down; g_moe_defer_down = value; return old; }
    if (key == 35) { const int old = g_attn_kv_nt; g_attn_kv_nt = value; return old; }
    if (key == 36) { const int old = g_wide_ntb; g_wide_ntb = value; return old; }
    if (key == 38) { const int old = g_verify_mq; g_verify_mq = value; return old; }
    if (key == 39) { const int old = g_mamba_conv_step; g_mamba_conv_step = value; return old; }
    if (key == 37) { const int old = g_score_rows; g_score_rows = value < 16 ? 16 : (value + 15) / 16 * 16; return old; }
    return -1;
}
