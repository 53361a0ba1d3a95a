// nvllm.hip — the C ABI of include/nvllm.h: model lifecycle, weight upload into kernel layouts,
// KV slot management, and the batched prefill/decode forward that replaces
// TransformerModel.ForwardWithCache (purego/tensor/generic_model.go:276-480).
//
// There is NO CPU fallback in this library: every entry point that computes needs a gfx950
// device and fails with NVL_ERR_NO_DEVICE / NVL_ERR_HIP otherwise.
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstring>
#include <new>

#include <rccl/rccl.h>

#include "model.h"
#include "spec_loop.h"

using namespace nvl;

static thread_local std::string g_create_err;
constexpr int ATTN_SPLIT_MAX_PAIRS = 32, ATTN_SPLIT_MAX = 8;     // split decode attention: (sequence, kv head) pairs a launch may have; most workgroups per pair
constexpr int SK_TILE_MAX_M = 2048, SK_TILE_MAX_SLICES = 8;      // split-K of the tile kernel for mid-size residual projections (resid_gemm)
static int g_sk_tile = 1;            // nvl_set_tuning key 26: that split (0 = off)
constexpr int MOE_DOWN_SLICES = 4;    // at most this many K slices (workgroups per column tile) in the dense-masked MoE down projection
static inline int moe_down_slices(int E) { int s = MOE_DOWN_SLICES; while (s > 1 && E % s) s--; return s; }   // a whole number of experts per slice

namespace {

int fail(nvl_model* m, int code, const std::string& msg) {
    if (m) m->err = msg; else g_create_err = msg;
    return code;
}

// a member of an in-process tensor-parallel group (nvl_tp_attach_local) that fails must not leave its peers waiting in
// tp_allreduce forever: the failure poisons the group and wakes them
void note_failure(nvl_model* m) {
    if (!m || !m->tp_local) return;
    { std::lock_guard<std::mutex> lk(m->tp_local->mu); m->tp_local->aborted = true; }
    m->tp_local->cv.notify_all();
}

#define NVL_TRY(m) try {
#define NVL_CATCH(m)                                                                     \
    } catch (const HipError& e) {                                                        \
        note_failure(m);                                                                 \
        char buf[512];                                                                   \
        snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e.code,         \
                 hipGetErrorString(e.code), e.file, e.line, e.what);                     \
        return fail(m, e.code == hipErrorOutOfMemory ? NVL_ERR_OOM : NVL_ERR_HIP, buf);  \
    } catch (const std::bad_alloc&) {                                                    \
        note_failure(m);                                                                 \
        return fail(m, NVL_ERR_OOM, "out of host memory");                               \
    } catch (const std::exception& e) {                                                  \
        note_failure(m);                                                                 \
        return fail(m, NVL_ERR_INVALID, e.what());                                       \
    }

template <typename T>
T* dmalloc(int64_t n) {
    void* p = nullptr;
    if (n <= 0) n = 1;
    NVL_HIP(hipMalloc(&p, (size_t)n * sizeof(T)));
    return (T*)p;
}
void* dmalloc_bytes(int64_t n) {
    void* p = nullptr;
    if (n <= 0) n = 16;
    NVL_HIP(hipMalloc(&p, (size_t)n));
    return p;
}
void dfree(void* p) { if (p) (void)hipFree(p); }
// Captured decode passes (replay_or_capture).  A graph exec may still be executing on the stream (the fused decode loop
// enqueues its steps without a host sync), so nothing is destroyed while work can be in flight: retire_graphs() only moves
// the execs aside, reap_graphs() destroys them and is called right after a hipStreamSynchronize of the model's stream.
void reap_graphs(nvl_model* m) {
    for (auto ge : m->graphs_retired) (void)hipGraphExecDestroy(ge);
    m->graphs_retired.clear();
}
void retire_graphs(nvl_model* m) {
    for (auto& kv : m->graphs) m->graphs_retired.push_back(kv.second);
    m->graphs.clear();
    m->graph_seen.clear();
}
// every captured pass bakes in the addresses of the buffers it was captured with: call before any of them is re-allocated
void clear_graphs(nvl_model* m) {
    retire_graphs(m);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    reap_graphs(m);
}
void free_sample_bufs(SampleBufs& b) {
    dfree(b.work); dfree(b.cnt); dfree(b.hist); dfree(b.off); dfree(b.out); dfree(b.u); dfree(b.probs);
    b = SampleBufs{};
}

void free_logprob_bufs(LogprobBufs& b) {
    dfree(b.part); dfree(b.io);
    b = LogprobBufs{};
}
// room for one launch over `launch_rows` rows and for the per-row inputs / outputs of `io_rows` rows
void reserve_logprob_bufs(LogprobBufs& b, int64_t launch_rows, int64_t io_rows, int V) {
    const int64_t words = logprob_part_words(launch_rows, V, LOGPROB_MAX_K);
    if (words > b.part_words) { dfree(b.part); b.part = nullptr; b.part_words = 0; b.part = dmalloc<int32_t>(words); b.part_words = words; }
    if (io_rows > b.io_rows) {
        dfree(b.io); b.io = nullptr; b.io_rows = 0;
        const int64_t cap = round_up(io_rows, 64);
        b.io = dmalloc<int32_t>(cap * (3 + 2 * LOGPROB_MAX_K)); b.io_rows = cap;
    }
}

bool is_1d(int kind) {
    switch (kind) {
        case NVL_T_FINAL_NORM_W: case NVL_T_FINAL_NORM_B: case NVL_T_ATTN_NORM_W: case NVL_T_ATTN_NORM_B:
        case NVL_T_FFN_NORM_W: case NVL_T_FFN_NORM_B: case NVL_T_BQ: case NVL_T_BK: case NVL_T_BV:
        case NVL_T_BO: case NVL_T_B1: case NVL_T_B2:
        case NVL_T_MAMBA_CONV_W: case NVL_T_MAMBA_CONV_B: case NVL_T_MAMBA_A_LOG: case NVL_T_MAMBA_D: case NVL_T_MAMBA_DT_BIAS:
        case NVL_T_MAMBA_NORM: return true;
        default: return false;
    }
}
bool is_global(int kind) { return kind < NVL_T_ATTN_NORM_W; }

DevTensor* tensor_slot(nvl_model* m, int kind, int layer) {
    if (kind < 0 || kind >= NVL_T_COUNT) return nullptr;
    if (is_global(kind)) return &m->g[kind];
    if (layer < 0 || layer >= m->L) return nullptr;
    return &m->layers[layer].t[kind];
}

// ---- profiling helpers --------------------------------------------------------------------
hipEvent_t get_event(nvl_model* m) {
    if (!m->ev_pool.empty()) { hipEvent_t e = m->ev_pool.back(); m->ev_pool.pop_back(); return e; }
    hipEvent_t e; NVL_HIP(hipEventCreate(&e)); return e;
}
struct KScope {   // brackets ONE kernel launch with HIP events on the model's stream
    nvl_model* m; int cls; double flops; hipEvent_t a = nullptr, b = nullptr;
    int site, phase; double bytes;
    KScope(nvl_model* m_, int cls_, double flops_ = 0, int site_ = -1, double bytes_ = -1) : m(m_), cls(cls_), flops(flops_) {
        // the launch site and its algorithmic bytes: set by the caller (m->site / m->site_bytes) or passed here
        site = site_ >= 0 ? site_ : m->site; bytes = bytes_ >= 0 ? bytes_ : m->site_bytes; phase = m->phase;
        m->site = KS_OTHER; m->site_bytes = 0;
        if (m->profile) { a = get_event(m); b = get_event(m); NVL_HIP(hipEventRecord(a, m->stream)); }
    }
    ~KScope() {
        if (m->profile && a) { (void)hipEventRecord(b, m->stream); m->prof.push_back({a, b, cls, flops, site, phase, bytes}); }
    }
};
void drain_profile(nvl_model* m) {
    for (auto& r : m->prof) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        if (r.cls == KC_GEMM) { m->stats.gemm_ms += ms; m->stats.gemm_flops += r.flops; m->stats.gemm_launches++; }
        else if (r.cls == KC_ATTN) { m->stats.attn_ms += ms; m->stats.attn_flops += r.flops; m->stats.attn_launches++; }
        else { m->stats.other_ms += ms; m->stats.other_launches++; }
        SiteStat& ss = m->site_stats[r.phase & 1][r.site >= 0 && r.site < KS_COUNT ? r.site : 0];
        ss.ms += ms; ss.flops += r.flops; ss.bytes += r.bytes; ss.launches++;
        m->ev_pool.push_back(r.a); m->ev_pool.push_back(r.b);
    }
    m->prof.clear();
}

// ---- GEMM dispatch ---------------------------------------------------------------------------
// out_f32: output element type of STORE (fp32 vs activation type)
// diagnostic runs (nvl_set_debug mode 4): the stamp slab of the next launch, or NULL
unsigned long long* next_stamps(nvl_model* m, int site, int nwg) {
    if (!m->stamping || !m->stamp_buf || m->stamp_launches >= STAMP_MAX_LAUNCH || nwg > STAMP_MAX_WG) return nullptr;
    m->stamp_recs.push_back({site, m->phase, nwg});
    return m->stamp_buf + (size_t)(m->stamp_launches++) * STAMP_MAX_WG * 8;
}
// the epilogue switch of a quantized weight of format WF
template <int WF>
void gemm_q(nvl_model* m, int epi, bool out_f32, const GemmArgs& a, const nvl_model::QRef& q) {
    const A8Buf a8buf{m->a8_codes, m->a8_scale, m->a8_rows, m->a8_k};
    const A8Buf* a8 = m->a8 ? &a8buf : nullptr;     // 8-bit activations at the tile step (a8.h; fp8 weights only)
#define NVL_GQ(EPIv, OutTv) launch_gemm_q<EPIv, OutTv, WF>(m->stream, a, q.scales, q.rows_pad, m->wq_scratch, m->wq_scratch_elems, a8, wf_group(q.wf))
    switch (epi) {
        case EPI_STORE:  if (out_f32) NVL_GQ(EPI_STORE, float); else NVL_GQ(EPI_STORE, bf16_t); break;
        case EPI_RESID:  NVL_GQ(EPI_RESID, float); break;
        case EPI_SWIGLU: NVL_GQ(EPI_SWIGLU, bf16_t); break;
        case EPI_GELU:   NVL_GQ(EPI_GELU, bf16_t); break;
        case EPI_QKV:    NVL_GQ(EPI_QKV, bf16_t); break;
        default: throw std::runtime_error("gemm: bad epilogue");
    }
#undef NVL_GQ
}
void gemm(nvl_model* m, int epi, bool out_f32, GemmArgs a, double flops = -1.0) {
    a.stamps = (m->stamping && !m->f32 && a.M <= 64 && !a.tile_map) ? next_stamps(m, m->site, STAMP_MAX_WG) : nullptr;
    // algorithmic bytes of a projection: every weight byte once + the activation operand + the output rows
    const auto qi = m->qmap.find(a.W);     // a quantized weight: its codes + scales (wq.h: 1 byte + 4 bytes per row, or 0.5 + 1/32 bytes)
    const nvl_model::QRef* q = qi != m->qmap.end() ? &qi->second : nullptr;
    const double wbytes = q ? (double)(wf_code_bytes(q->wf, (int64_t)a.N * a.K) + wf_scale_bytes(q->wf, a.N, a.K)) : (double)a.N * a.K * (double)m->wsize;
    const double gbytes = m->site_bytes > 0 ? m->site_bytes
        : wbytes + (double)a.M * a.K * (double)m->wsize + (double)a.M * a.N * (out_f32 || epi == EPI_RESID ? 4.0 : (double)m->wsize);
    KScope ks(m, KC_GEMM, flops >= 0 ? flops : 2.0 * (double)a.M * (double)a.N * (double)a.K, -1, gbytes);
    hipStream_t st = m->stream;
    m->gemm_ran = NVL_GEMM_RAN_NONE;      // (the instance of a bf16 projection, for nvl_op_qkv_stages: launch_gemm_bf16 names it)
    if (q) {     // the same dispatch on the kernels of the weight's format / dequantize + tile (wq.h)
        if (q->wf == WF_FP8) gemm_q<WF_FP8>(m, epi, out_f32, a, *q);
        else if (wf_base(q->wf) == WF_INT4) gemm_q<WF_INT4>(m, epi, out_f32, a, *q);
        else gemm_q<WF_MXFP4>(m, epi, out_f32, a, *q);
        NVL_HIP(hipGetLastError());
        return;
    }
    if (m->f32) {
        switch (epi) {
            case EPI_STORE: launch_gemm_f32<EPI_STORE, float>(st, a); break;
            case EPI_RESID: launch_gemm_f32<EPI_RESID, float>(st, a); break;
            case EPI_GELU:  launch_gemm_f32<EPI_GELU, float>(st, a); break;
            default: throw std::runtime_error("gemm: epilogue not available in f32 mode");
        }
    } else {
        switch (epi) {
            case EPI_STORE:
                if (out_f32) launch_gemm_bf16<EPI_STORE, float>(st, a);
                else launch_gemm_bf16<EPI_STORE, bf16_t>(st, a);
                break;
            case EPI_RESID:  launch_gemm_bf16<EPI_RESID, float>(st, a); break;
            case EPI_SWIGLU: launch_gemm_bf16<EPI_SWIGLU, bf16_t>(st, a); break;
            case EPI_GELU:   launch_gemm_bf16<EPI_GELU, bf16_t>(st, a); break;
            case EPI_QKV:    launch_gemm_bf16<EPI_QKV, bf16_t>(st, a); break;
            default: throw std::runtime_error("gemm: bad epilogue");
        }
        m->gemm_ran = t_gemm_ran;
    }
    NVL_HIP(hipGetLastError());
}

}  // namespace

// =================================================================================================
// lifecycle
// =================================================================================================
extern "C" int nvl_abi_version(void) { return NVL_ABI_VERSION; }

extern "C" int nvl_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(nvl_model_config);
        case 1: return (int)sizeof(nvl_runtime_opts);
        case 2: return (int)sizeof(nvl_stats);
        case 3: return (int)sizeof(nvl_sampling_params);
        default: return -1;
    }
}

extern "C" int nvl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char* nvl_last_error(const nvl_model* m) { return m ? m->err.c_str() : g_create_err.c_str(); }

// The RoPE tables [max_seq][hd] in fp64 on the host, exactly as NewRoPECache (rope.go:18-50): both halves of a row hold
// the same hd/2 values (nvl_create's tables; nvl_op_attention_batch builds its own with the same function)
static void rope_tables(double base, int max_seq, int hd, std::vector<float>& ct, std::vector<float>& st) {
    const int half = hd / 2;
    ct.resize((size_t)max_seq * hd); st.resize((size_t)max_seq * hd);
    for (int pos = 0; pos < max_seq; pos++)
        for (int i = 0; i < half; i++) {
            const double freq = 1.0 / std::pow(base, (double)(2 * i) / (double)hd);
            const double ang = (double)pos * freq;
            const float cv = (float)std::cos(ang), sv = (float)std::sin(ang);
            ct[(size_t)pos * hd + i] = cv; ct[(size_t)pos * hd + half + i] = cv;
            st[(size_t)pos * hd + i] = sv; st[(size_t)pos * hd + half + i] = sv;
        }
}

extern "C" int nvl_create(const nvl_model_config* cfg, const nvl_runtime_opts* opts, nvl_model** out) {
    if (!cfg || !opts || !out) return fail(nullptr, NVL_ERR_INVALID, "nvl_create: null argument");
    *out = nullptr;
    const nvl_model_config& c = *cfg;
    if (c.hidden <= 0 || c.num_layers <= 0 || c.num_heads <= 0 || c.head_dim <= 0 || c.vocab_size <= 0 ||
        c.max_seq_len <= 0)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: non-positive model dimension");
    if (c.head_dim != 64 && c.head_dim != 128)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: head_dim must be 64 or 128");
    if (c.attention_multiplier < 0.f)      // the kernels take the row maximum before scaling
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: attention_multiplier must not be negative");
    if (c.hidden % 64 != 0 || (c.ffn_dim % 64) != 0)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: hidden and ffn_dim must be multiples of 64");
    // runtime options are validated BEFORE any size is derived from them (a zero-valued host struct must not turn into
    // a 0-block KV cache): max_seqs >= 1 is required, max_batch_tokens 0 selects max_seq_len
    if (opts->max_seqs <= 0)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: max_seqs must be >= 1 (KV slots / sequences per call)");
    if (opts->max_batch_tokens < 0 || opts->kv_num_blocks < 0 || opts->kv_block_size < 0)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: negative max_batch_tokens / kv_num_blocks / kv_block_size");
    if (opts->kv_cache_dtype != NVL_KV_AUTO && opts->kv_cache_dtype != NVL_KV_FP8_E4M3)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: kv_cache_dtype must be NVL_KV_AUTO (0) or NVL_KV_FP8_E4M3 (1)");
    if (opts->kv_cache_dtype == NVL_KV_FP8_E4M3 && opts->precision == NVL_PRECISION_F32)
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: the fp8 KV cache needs NVL_PRECISION_BF16");
    if (opts->kv_cache_dtype == NVL_KV_FP8_E4M3 && ((opts->tp_size > 1) || opts->tp_force_single == 1))
        return fail(nullptr, NVL_ERR_INVALID, "nvl_create: the fp8 KV cache does not cover tensor parallelism");
    const int tp = opts->tp_size > 1 ? opts->tp_size : 1;
    if (tp > 1) {
        const int nkv_full = c.attention_type == NVL_ATTN_MHA ? c.num_heads : c.num_kv_heads;
        if (opts->tp_rank < 0 || opts->tp_rank >= tp || tp > 8)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: tp_rank/tp_size out of range (tp_size <= 8)");
        if (c.attention_type == NVL_ATTN_MQA || c.use_moe)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: tensor parallelism covers MHA/GQA dense models (MQA has one KV head; MoE shards by expert)");
        if (c.num_heads % tp || nkv_full % tp || c.ffn_dim % (tp * 64))
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: heads, kv heads and ffn_dim/64 must divide by tp_size");
    }
    if (opts->device < 0 || nvl_device_count() <= opts->device)
        return fail(nullptr, NVL_ERR_NO_DEVICE,
                    "nvl_create: no HIP device (this library has no CPU fallback)");
    const bool any_mamba = (c.mamba_layer_mask[0] | c.mamba_layer_mask[1]) != 0;
    if (any_mamba) {
        const int eh = c.mamba_expand * c.hidden;
        const int mhd = c.mamba_head_dim > 0 ? c.mamba_head_dim : (c.mamba_num_heads > 0 ? eh / c.mamba_num_heads : 0);
        if (c.num_layers > 128 || c.mamba_expand <= 0 || c.mamba_state_size <= 0 || c.mamba_num_heads <= 0 || c.mamba_n_groups <= 0 ||
            c.mamba_conv_kernel <= 0 || c.mamba_conv_kernel > 8 || mhd <= 0 || mhd * c.mamba_num_heads != eh)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: bad Mamba2 dimensions (heads x head_dim must equal expand x hidden)");
        // the scan kernel keeps state_size / (256 / head_dim) states per thread: head_dim | 256, at most 32 states per thread
        if (!mamba_geometry_ok(c.mamba_num_heads, mhd, c.mamba_state_size, c.mamba_n_groups, c.mamba_conv_kernel))
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: Mamba2 head_dim / state_size not supported by the scan kernel");
        if (tp > 1) return fail(nullptr, NVL_ERR_INVALID, "nvl_create: tensor parallelism does not cover Mamba2 layers");
        if (opts->kv_num_blocks > 0)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: Mamba2 layers keep per-sequence state in KV slots: not available in paged-KV mode");
        if (c.use_moe || c.block_style != NVL_BLOCK_SEQUENTIAL)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_create: hybrid (Mamba2) models are sequential blocks with a dense MLP");
    }
    nvl_model* m = new (std::nothrow) nvl_model();
    if (!m) return fail(nullptr, NVL_ERR_OOM, "nvl_create: out of host memory");
    NVL_TRY(m)
    m->cfg = c; m->opts = *opts;
    m->f32 = (opts->precision == NVL_PRECISION_F32);
    m->wsize = m->f32 ? 4 : 2;
    m->kv8 = opts->kv_cache_dtype == NVL_KV_FP8_E4M3;
    m->kv_esize = m->kv8 ? 1 : m->wsize;
    m->k_scale.assign((size_t)std::max(c.num_layers, 1), 1.0f);
    m->v_scale.assign((size_t)std::max(c.num_layers, 1), 1.0f);
    m->device = opts->device;
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    NVL_HIP(hipEventCreate(&m->ev0));
    NVL_HIP(hipEventCreate(&m->ev1));
    m->H = c.hidden; m->nH = c.num_heads; m->hd = c.head_dim; m->F = c.ffn_dim; m->V = c.vocab_size;
    m->L = c.num_layers;
    m->nKV = c.attention_type == NVL_ATTN_MHA ? c.num_heads : (c.attention_type == NVL_ATTN_MQA ? 1 : c.num_kv_heads);
    if (m->nKV <= 0 || m->nH % m->nKV != 0) throw std::runtime_error("num_heads must be a multiple of num_kv_heads");
    // tensor parallel shard: this rank owns nH/tp query heads, nKV/tp kv heads and F/tp FFN
    // columns; from here on nH / nKV / F are the LOCAL sizes (hidden H, vocab V stay full: residual stream,
    // norms, embeddings and the LM head are replicated)
    m->tp = tp; m->tp_rank = tp > 1 ? opts->tp_rank : 0;
    m->tp_force = tp == 1 && opts->tp_force_single == 1;   // diagnostics: run the row-parallel path + all-reduce with one rank
    m->nH_full = m->nH; m->nKV_full = m->nKV; m->F_full = m->F;
    m->nH /= tp; m->nKV /= tp; m->F /= tp;
    m->group = m->nH / m->nKV;
    m->Vpad = (int)round_up(m->V, 128);
    m->n_qkv = (m->nH + 2 * m->nKV) * m->hd;
    m->Tmax = (int)round_up(c.max_seq_len, 64);
    if (opts->kv_num_blocks > 0) {            // paged KV: the host's block manager names the blocks
        const int bs = opts->kv_block_size > 0 ? opts->kv_block_size : 256;
        if (bs % 64 != 0) throw std::runtime_error("kv_block_size must be a multiple of 64");
        m->paged = 1; m->Tmax = bs; m->num_blocks = opts->kv_num_blocks;
        m->blocks_per_seq = cdiv(c.max_seq_len, bs);
    } else {
        m->num_blocks = opts->max_seqs;
    }
    m->table_cap = opts->max_seqs * m->blocks_per_seq;
    // score scale: GQA uses AttentionMultiplier when set (attention.go:361-364); MHA/MQA 1/sqrt(hd)
    if (c.attention_type == NVL_ATTN_GQA && c.attention_multiplier != 0.f) m->attn_scale = c.attention_multiplier;
    else m->attn_scale = 1.0f / std::sqrt((float)m->hd);
    m->resid_alpha = c.residual_multiplier != 0.f ? c.residual_multiplier : 1.0f;
    m->layers.resize(m->L);
    for (int li = 0; li < m->L && li < 128; li++)
        if ((c.mamba_layer_mask[li >> 6] >> (li & 63)) & 1) { m->layers[li].mamba = true; m->layers[li].mamba_idx = m->n_mamba++; }
    if (m->n_mamba) {
        m->mEH = c.mamba_expand * c.hidden; m->m_nh = c.mamba_num_heads; m->m_ss = c.mamba_state_size; m->m_ng = c.mamba_n_groups;
        m->m_K = c.mamba_conv_kernel; m->m_hd = c.mamba_head_dim > 0 ? c.mamba_head_dim : m->mEH / m->m_nh;
        m->mConv = m->mEH + 2 * m->m_ng * m->m_ss; m->mP = m->mEH + m->mConv + m->m_nh;
    }
    if (m->opts.max_batch_tokens <= 0) m->opts.max_batch_tokens = c.max_seq_len;
    *out = m;
    return NVL_OK;
    } catch (const HipError& e) {
        std::string s = std::string("nvl_create: HIP error: ") + hipGetErrorString(e.code);
        delete m;
        return fail(nullptr, NVL_ERR_HIP, s);
    } catch (const std::exception& e) {
        std::string s = e.what();
        delete m;
        return fail(nullptr, NVL_ERR_INVALID, s);
    }
}

extern "C" void nvl_destroy(nvl_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (int k = 0; k < NVL_T_COUNT; k++) { dfree(m->g[k].p); dfree(m->g[k].qs); }
    for (auto& l : m->layers) {
        for (int k = 0; k < NVL_T_COUNT; k++) { dfree(l.t[k].p); dfree(l.t[k].qs); }
        dfree(l.w_qkv); dfree(l.b_qkv); dfree(l.w1); dfree(l.moe_in); dfree(l.moe_out_cat);
        dfree(l.qs_qkv); dfree(l.qs1);
        if (l.moe_out_cat != l.moe_out_q) dfree(l.moe_out_q);
        dfree(l.qs_moe_in); dfree(l.qs_moe_out);
    }
    dfree(m->wq_scratch); dfree(m->eq_scratch); dfree(m->a8_codes); dfree(m->a8_scale);
    if (m->lm_head && m->lm_head != m->g[NVL_T_TOK_EMB].p && m->lm_head != m->g[NVL_T_LM_HEAD].p) dfree(m->lm_head);
    dfree(m->rope_cos); dfree(m->rope_sin); dfree(m->kcache); dfree(m->vcache);
    dfree(m->x); dfree(m->xn); dfree(m->qkv); dfree(m->q); dfree(m->attn_out); dfree(m->attn_part); dfree(m->attn_part_cnt); dfree(m->hbuf); dfree(m->h2);
    dfree(m->xn_last); dfree(m->logits); dfree(m->argmax_dev); dfree(m->argmax_pval); dfree(m->argmax_pidx); dfree(m->router_logits); dfree(m->expert_ids);
    dfree(m->expert_w); dfree(m->seg_start); dfree(m->moe_counts); dfree(m->moe_cursor); dfree(m->moe_tile_map); dfree(m->moe_n_mtiles); dfree(m->perm_token); dfree(m->slot_of); dfree(m->moe_eo); dfree(m->moe_xg);
    dfree(m->meta_dev); dfree(m->hidden); dfree(m->sk_part); dfree(m->tp_part); dfree(m->ring); dfree(m->rs_part);
    for (int r = 0; r < 8; r++) if (m->p2p_peer[r] && m->p2p_peer[r] != m->p2p_buf) (void)hipIpcCloseMemHandle(m->p2p_peer[r]);
    dfree(m->p2p_buf);
    dfree(m->moe_gate); dfree(m->moe_hall); dfree(m->moe_part);
    clear_graphs(m);
    if (m->am_host) (void)hipHostFree(m->am_host);
    if (m->verify_host) (void)hipHostFree(m->verify_host);
    dfree(m->verify_dev);
    if (m->vs_host) (void)hipHostFree(m->vs_host);
    dfree(m->vs_dev);
    dfree(m->ring_pos0);
    dfree(m->conv_tail); dfree(m->stamp_buf); dfree(m->ssd_z); dfree(m->ssd_decay);
    dfree(m->ssm_state); dfree(m->mproj); dfree(m->mxbc); dfree(m->mdelta); dfree(m->my); dfree(m->myn);
    free_sample_bufs(m->samp);
    free_logprob_bufs(m->lpb);
    dfree(m->samp_hist); dfree(m->samp_hist_len); dfree(m->samp_u_steps);
    dfree(m->draft_q); dfree(m->spec_ap);
    if (m->tp_comm) (void)ncclCommDestroy((ncclComm_t)m->tp_comm);
    if (m->tp_local) {
        bool last;
        { std::lock_guard<std::mutex> lk(m->tp_local->mu); last = --m->tp_local->refs == 0; }
        if (last) { dfree(m->tp_local->scratch); delete m->tp_local; }
    }
    if (m->meta_host) (void)hipHostFree(m->meta_host);
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

// =================================================================================================
// weights
// =================================================================================================
namespace {

// canonical device copy: 2-D -> [rows_pad(W_ROW_PAD)][K] in weight dtype; 1-D -> fp32.
// `sl` selects the sub-block of the uploaded tensor that lands in rows [dn0, dn0+N) (the whole tensor for
// replicated kinds, this rank's shard for tensor-parallel kinds); total_rows sizes the destination.
// the quantized format this 2-D kind is stored in (wq.h wf_covers), or WF_BF16
int q_kind(const nvl_model* m, int kind) { return wf_covers(m->wf, m->ef, m->hf, kind, m->cfg.tied_embedding != 0) ? m->wf : WF_BF16; }

// the scales of `rows` rows of K inputs, every one the pad value of the format (wq.h wf_fill_pad_scales)
void* q_alloc_scales(nvl_model* m, int wf, int64_t rows, int64_t K) {
    void* qs = dmalloc_bytes(wf_scale_bytes(wf, rows, K));
    wf_fill_pad_scales(m->stream, wf, qs, rows, K);
    return qs;
}

// codes of [Npad][K] zeroed, scales at their pad value, and the tensor's shape
void q_alloc(nvl_model* m, DevTensor* t, int wf, int64_t N, int64_t K) {
    const int64_t Npad = round_up(N, W_ROW_PAD);
    dfree(t->p); dfree(t->qs);
    t->p = dmalloc_bytes(wf_code_bytes(wf, Npad * K));
    NVL_HIP(hipMemsetAsync(t->p, 0, (size_t)wf_code_bytes(wf, Npad * K), m->stream));
    t->qs = q_alloc_scales(m, wf, Npad, K);
    t->wf = wf; t->rows = N; t->cols = K; t->rows_pad = Npad;
}
double q_bytes(const DevTensor& t) { return (double)wf_code_bytes(t.wf, t.rows_pad * t.cols) + (double)wf_scale_bytes(t.wf, t.rows_pad, t.cols); }

// quantized weight (tensor parallelism is refused in these modes: the tensor is always whole, one piece): fp32 [N][K] on the
// device, then the format's quantizer -> codes + scales in its device layout (w8.h / w4.h)
void upload_2d_q(nvl_model* m, DevTensor* t, int wf, const void* data, int dtype, int64_t N, int64_t K, bool src_is_in_out) {
    if (K % 32 != 0) throw std::runtime_error(std::string(wf_name(wf)) + " weights: the input width must be a multiple of 32");
    if (K % wf_in_multiple(wf) != 0) throw std::runtime_error(std::string(wf_name(wf)) + " weights: the input width must be a multiple of the group size");
    const size_t esz = dtype == NVL_DTYPE_F32 ? 4 : 2;
    void* raw = dmalloc_bytes(N * K * (int64_t)esz);
    NVL_HIP(hipMemcpyAsync(raw, data, (size_t)(N * K) * esz, hipMemcpyDefault, m->stream));
    float* f = dmalloc<float>(N * K);
    hipLaunchKernelGGL((convert_2d_kernel<float, false>), dim3((unsigned)cdiv(K, 32), (unsigned)cdiv(N, 32)), dim3(256), 0,
                       m->stream, raw, dtype, src_is_in_out ? 1 : 0, f, N, K, Slice2D{N, K, 0, 0, 0});
    NVL_HIP(hipGetLastError());
    q_alloc(m, t, wf, N, K);
    int* bad = dmalloc<int>(1);
    NVL_HIP(hipMemsetAsync(bad, 0, 4, m->stream));
    wf_quant_rows(m->stream, wf, f, N, K, t->p, t->qs, bad);
    NVL_HIP(hipGetLastError());
    int h_bad = 0;
    NVL_HIP(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, m->stream));
    NVL_HIP(hipStreamSynchronize(m->stream));
    dfree(bad); dfree(f); dfree(raw);
    if (h_bad) {
        dfree(t->p); dfree(t->qs); t->p = t->qs = nullptr;
        throw std::runtime_error(std::string("nvl_upload_tensor: a weight is not finite (") + wf_name(wf) + " weights refuse " + wf_quant_refuses(wf) + ")");
    }
    m->stats.weight_bytes += q_bytes(*t);
}

void upload_2d(nvl_model* m, DevTensor* t, const void* data, int dtype, int64_t N, int64_t K, bool src_is_in_out,
               Slice2D sl, int64_t total_rows, bool first_piece) {
    const size_t esz = dtype == NVL_DTYPE_F32 ? 4 : 2;
    const int64_t src_elems = sl.SN * sl.SK;
    void* raw = dmalloc_bytes(src_elems * (int64_t)esz);
    NVL_HIP(hipMemcpyAsync(raw, data, (size_t)src_elems * esz, hipMemcpyDefault, m->stream));
    const int64_t Npad = round_up(total_rows, W_ROW_PAD);
    if (first_piece) {
        dfree(t->p);
        t->p = dmalloc_bytes(Npad * K * (int64_t)m->wsize);
        NVL_HIP(hipMemsetAsync(t->p, 0, (size_t)(Npad * K) * m->wsize, m->stream));
        m->stats.weight_bytes += (double)Npad * K * m->wsize;
    }
    dim3 grid((unsigned)cdiv(K, 32), (unsigned)cdiv(N, 32));
    if (m->f32)
        hipLaunchKernelGGL((convert_2d_kernel<float, false>), grid, dim3(256), 0, m->stream, raw, dtype,
                           src_is_in_out ? 1 : 0, (float*)t->p, N, K, sl);
    else   // bf16 weights (and the embedding tables) live in the fragment-major layout
        hipLaunchKernelGGL((convert_2d_kernel<bf16_t, true>), grid, dim3(256), 0, m->stream, raw, dtype,
                           src_is_in_out ? 1 : 0, (bf16_t*)t->p, N, K, sl);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    dfree(raw);
    t->rows = total_rows; t->cols = K; t->rows_pad = Npad;
}

void upload_1d(nvl_model* m, DevTensor* t, const void* data, int dtype, int64_t n_src, int64_t off, int64_t n) {
    const size_t esz = dtype == NVL_DTYPE_F32 ? 4 : 2;
    void* raw = dmalloc_bytes(n_src * (int64_t)esz);
    NVL_HIP(hipMemcpyAsync(raw, data, (size_t)n_src * esz, hipMemcpyDefault, m->stream));
    dfree(t->p);
    t->p = dmalloc<float>(n);
    hipLaunchKernelGGL(convert_1d_kernel, dim3(cdiv(n, 256)), dim3(256), 0, m->stream, raw, dtype, (float*)t->p, n, off);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    dfree(raw);
    t->rows = n; t->cols = 1; t->rows_pad = n;
    m->stats.weight_bytes += (double)n * 4;
}

// FULL (unsharded) logical sizes of a 2-D weight kind, as the host holds it
int64_t full_out(const nvl_model* m, int kind) {
    switch (kind) {
        case NVL_T_LM_HEAD: return m->V;
        case NVL_T_WQ: return (int64_t)m->nH_full * m->hd;
        case NVL_T_WK: case NVL_T_WV: return (int64_t)m->nKV_full * m->hd;
        case NVL_T_WKV: return 2 * m->hd;
        case NVL_T_WO: return m->H;
        case NVL_T_W1: return m->cfg.activation_type == NVL_ACT_SWIGLU ? 2 * (int64_t)m->F_full : m->F_full;
        case NVL_T_W2: return m->H;
        case NVL_T_ROUTER: return m->cfg.num_experts;
        case NVL_T_MAMBA_IN_PROJ: return m->mP;
        case NVL_T_MAMBA_OUT_PROJ: return m->H;
        default: return -1;
    }
}
int64_t full_in(const nvl_model* m, int kind) {
    switch (kind) {
        case NVL_T_WO: return (int64_t)m->nH_full * m->hd;
        case NVL_T_W2: return m->F_full;
        case NVL_T_MAMBA_OUT_PROJ: return m->mEH;
        default: return m->H;
    }
}
// the shape [out][in] an upload of a 2-D kind must have, whole (unsharded): the token embedding [V][H]; the experts of a layer
// [E * out][in], gate | up rows [2F][H] or down rows [H][F] per expert (per_expert: one expert's out); a weight its
// full_out x full_in (out < 0: not a 2-D weight kind)
void expected_2d_shape(const nvl_model* m, int kind, int64_t* out, int64_t* in, int64_t* per_expert = nullptr) {
    if (kind == NVL_T_MOE_IN || kind == NVL_T_MOE_OUT) {
        const int64_t one = kind == NVL_T_MOE_IN ? 2 * (int64_t)m->F : m->H;
        if (per_expert) *per_expert = one;
        *out = m->cfg.num_experts * one;
        *in = kind == NVL_T_MOE_IN ? m->H : m->F;
    } else if (kind == NVL_T_TOK_EMB) { *out = m->V; *in = m->H; }
    else { *out = full_out(m, kind); *in = full_in(m, kind); }
}
// one whole 2-D tensor in the format its kind is stored in (the setters refuse tensor parallelism for the quantized ones)
void upload_2d_whole(nvl_model* m, DevTensor* t, int kind, const void* data, int dtype, int64_t N, int64_t K, bool src_is_in_out) {
    if (q_kind(m, kind)) upload_2d_q(m, t, q_kind(m, kind), data, dtype, N, K, src_is_in_out);
    else upload_2d(m, t, data, dtype, N, K, src_is_in_out, Slice2D{N, K, 0, 0, 0}, N, true);
}

}  // namespace

extern "C" int nvl_upload_tensor(nvl_model* m, int kind, int layer, const void* data, int dtype,
                                 int64_t rows, int64_t cols, int layout) {
    if (!m || !data) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: null argument");
    if (m->finalized) return fail(m, NVL_ERR_STATE, "nvl_upload_tensor: model already finalized");
    if (dtype < 0 || dtype > 2) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: unsupported dtype");
    DevTensor* t = tensor_slot(m, kind, layer);
    if (!t) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: bad kind or layer");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    char buf[256];
    const int r = m->tp_rank;
    if (is_1d(kind)) {
        const int64_t n = rows * (cols > 0 ? cols : 1);
        int64_t off = 0, cnt = n;
        {   // the kernels read exactly this many elements: a short norm / bias tensor would be an out-of-bounds read
            int64_t want = m->H;
            if (kind == NVL_T_BQ) want = (int64_t)m->nH_full * m->hd;
            else if (kind == NVL_T_BK || kind == NVL_T_BV) want = (int64_t)m->nKV_full * m->hd;
            else if (kind == NVL_T_B1) want = m->F_full;
            else if (kind == NVL_T_MAMBA_CONV_W) want = (int64_t)m->mConv * m->m_K;
            else if (kind == NVL_T_MAMBA_CONV_B) want = m->mConv;
            else if (kind == NVL_T_MAMBA_A_LOG || kind == NVL_T_MAMBA_D || kind == NVL_T_MAMBA_DT_BIAS) want = m->m_nh;
            else if (kind == NVL_T_MAMBA_NORM) want = m->mEH;
            if (kind >= NVL_T_MAMBA_IN_PROJ && !m->n_mamba) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: the model has no Mamba2 layers");
            if (rows <= 0 || n != want) {
                snprintf(buf, sizeof buf, "1-D tensor kind %d has %lld elements, the model needs %lld", kind, (long long)n,
                         (long long)want);
                return fail(m, NVL_ERR_INVALID, buf);
            }
        }
        if (m->tp > 1) {   // column-parallel biases follow their projection's shard; row-parallel biases stay on rank 0
            if (kind == NVL_T_BQ) { cnt = (int64_t)m->nH * m->hd; off = r * cnt; }
            else if (kind == NVL_T_BK || kind == NVL_T_BV) { cnt = (int64_t)m->nKV * m->hd; off = r * cnt; }
            else if (kind == NVL_T_B1) { cnt = m->F; off = r * cnt; }
            else if ((kind == NVL_T_BO || kind == NVL_T_B2) && r != 0) return NVL_OK;
            if (off + cnt > n) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: bias shorter than the full (unsharded) size");
        }
        upload_1d(m, t, data, dtype, n, off, cnt);
        return NVL_OK;
    }
    if (kind == NVL_T_TOK_EMB || kind == NVL_T_POS_EMB) {
        const int64_t want_rows = kind == NVL_T_TOK_EMB ? m->V : rows;
        if (cols != m->H || rows != want_rows) {
            snprintf(buf, sizeof buf, "embedding shape [%lld,%lld] does not match [%lld,%d]", (long long)rows,
                     (long long)cols, (long long)want_rows, m->H);
            return fail(m, NVL_ERR_INVALID, buf);
        }
        m->w2d_uploaded = true;
        upload_2d_whole(m, t, kind, data, dtype, rows, cols, false);
        return NVL_OK;
    }
    if (kind == NVL_T_MOE_IN || kind == NVL_T_MOE_OUT) {
        int64_t out, in, one;
        expected_2d_shape(m, kind, &out, &in, &one);
        if (rows != out || cols != in) {
            snprintf(buf, sizeof buf, "MoE tensor shape [%lld,%lld] does not match [E*%lld,%lld]", (long long)rows,
                     (long long)cols, (long long)one, (long long)in);
            return fail(m, NVL_ERR_INVALID, buf);
        }
        m->w2d_uploaded = true;
        m->expert_uploaded = true;
        upload_2d_whole(m, t, kind, data, dtype, rows, cols, false);     // (quantized: scales per (expert, output row))
        return NVL_OK;
    }
    if (kind >= NVL_T_MAMBA_IN_PROJ && !m->n_mamba) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: the model has no Mamba2 layers");
    const int64_t SN = full_out(m, kind), SK = full_in(m, kind);
    if (SN < 0) return fail(m, NVL_ERR_INVALID, "nvl_upload_tensor: kind is not a 2-D weight");
    const int64_t got_in = layout == NVL_LAYOUT_IN_OUT ? rows : cols;
    const int64_t got_out = layout == NVL_LAYOUT_IN_OUT ? cols : rows;
    if (got_in != SK || got_out != SN) {   // reference: panic "incompatible shapes" tensor.go:67
        snprintf(buf, sizeof buf, "weight kind %d: got [in=%lld,out=%lld], model needs [in=%lld,out=%lld]", kind,
                 (long long)got_in, (long long)got_out, (long long)SK, (long long)SN);
        return fail(m, NVL_ERR_INVALID, buf);
    }
    const bool io = layout == NVL_LAYOUT_IN_OUT;
    m->w2d_uploaded = true;
    if (q_kind(m, kind) || m->tp == 1) {     // (a quantized kind: tp == 1, the weight dtype setters refuse tensor parallelism)
        upload_2d_whole(m, t, kind, data, dtype, SN, SK, io);
        return NVL_OK;
    }
    // ---- tensor-parallel shard of the uploaded FULL tensor ----
    const int64_t hd = m->hd;
    switch (kind) {
        case NVL_T_WQ: { const int64_t nl = m->nH * hd;     // column parallel: this rank's query heads
            upload_2d(m, t, data, dtype, nl, SK, io, Slice2D{SN, SK, r * nl, 0, 0}, nl, true); break; }
        case NVL_T_WK: case NVL_T_WV: { const int64_t nl = m->nKV * hd;
            upload_2d(m, t, data, dtype, nl, SK, io, Slice2D{SN, SK, r * nl, 0, 0}, nl, true); break; }
        case NVL_T_WO: { const int64_t kl = m->nH * hd;     // row parallel: K slice = this rank's heads
            upload_2d(m, t, data, dtype, SN, kl, io, Slice2D{SN, SK, 0, r * kl, 0}, SN, true); break; }
        case NVL_T_W1: { const int64_t fl = m->F;
            if (m->cfg.activation_type == NVL_ACT_SWIGLU) {   // [gate F | up F] -> [gate_loc | up_loc]
                upload_2d(m, t, data, dtype, fl, SK, io, Slice2D{SN, SK, r * fl, 0, 0}, 2 * fl, true);
                upload_2d(m, t, data, dtype, fl, SK, io, Slice2D{SN, SK, m->F_full + r * fl, 0, fl}, 2 * fl, false);
            } else {
                upload_2d(m, t, data, dtype, fl, SK, io, Slice2D{SN, SK, r * fl, 0, 0}, fl, true);
            }
            break; }
        case NVL_T_W2: { const int64_t kl = m->F;           // row parallel
            upload_2d(m, t, data, dtype, SN, kl, io, Slice2D{SN, SK, 0, r * kl, 0}, SN, true); break; }
        default:                                            // LM head etc.: replicated
            upload_2d(m, t, data, dtype, SN, SK, io, Slice2D{SN, SK, 0, 0, 0}, SN, true);
    }
    return NVL_OK;
    NVL_CATCH(m)
}

// The pre-quantized uploads: codes [rows][cols] in the ABI packing of the format family `base` ([out, in], as in the checkpoint),
// their scales and (INT4) zero points, taken as they are.  The format itself is the model's (INT4: with its group size).
// fn / setter: the entry point's name and its mode's setter, for the messages.
static int upload_prequant(nvl_model* m, int base, const char* fn, const char* setter, int kind, int layer, const uint8_t* codes,
                           const void* scales, const uint8_t* zeros, int64_t rows, int64_t cols, int layout) {
    char buf[200];
    auto bad = [&](int code, const char* fmt, auto... args) { snprintf(buf, sizeof buf, fmt, fn, args...); return fail(m, code, buf); };
    if (!m || !codes || !scales || (base == WF_INT4 && !zeros)) return bad(NVL_ERR_INVALID, "%s: null argument");
    if (m->finalized) return bad(NVL_ERR_STATE, "%s: model already finalized");
    const int wf = q_kind(m, kind);
    if (wf_base(wf) != base) return bad(NVL_ERR_INVALID, "%s: not an %s weight kind of this model (%s)", wf_name(base), setter);
    if (layout != NVL_LAYOUT_OUT_IN) return bad(NVL_ERR_INVALID, "%s: codes must be [out, in] (NVL_LAYOUT_OUT_IN)");
    DevTensor* t = tensor_slot(m, kind, layer);
    if (!t) return bad(NVL_ERR_INVALID, "%s: bad kind or layer");
    int64_t SN, SK;
    expected_2d_shape(m, kind, &SN, &SK);
    if (rows != SN || cols != SK || SK % wf_in_multiple(wf) != 0)
        return bad(NVL_ERR_INVALID, "%s: kind %d: got [out=%lld,in=%lld], model needs [out=%lld,in=%lld]%s", kind, (long long)rows,
                   (long long)cols, (long long)SN, (long long)SK, wf_in_multiple_hint(wf));
    if (const char* why = wf_check_prequant(wf, codes, scales, zeros, rows, cols)) return bad(NVL_ERR_INVALID, why);
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    m->w2d_uploaded = true;
    if (kind == NVL_T_MOE_IN || kind == NVL_T_MOE_OUT) m->expert_uploaded = true;
    q_alloc(m, t, wf, rows, cols);
    const int64_t bytes[3] = {wf_code_bytes(wf, rows * cols), wf_abi_scale_bytes(wf, rows, cols), wf_abi_zero_bytes(wf, rows, cols)};
    const void* host[3] = {codes, scales, zeros};
    void* raw[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; i++) {
        if (!bytes[i]) continue;
        raw[i] = dmalloc_bytes(bytes[i]);
        NVL_HIP(hipMemcpy(raw[i], host[i], (size_t)bytes[i], hipMemcpyHostToDevice));
    }
    wf_place(m->stream, wf, (const uint8_t*)raw[0], raw[1], (const uint8_t*)raw[2], rows, cols, t->p, t->qs);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    for (void* r : raw) dfree(r);
    m->stats.weight_bytes += q_bytes(*t);
    return NVL_OK;
    NVL_CATCH(m)
}
extern "C" int nvl_upload_tensor_fp8(nvl_model* m, int kind, int layer, const uint8_t* codes, const float* scales,
                                     int64_t rows, int64_t cols, int layout) {
    return upload_prequant(m, WF_FP8, "nvl_upload_tensor_fp8", "nvl_set_weight_dtype", kind, layer, codes, scales, nullptr, rows, cols, layout);
}
// MXFP4: codes [rows][cols/2] (even k in the low nibble), e8m0 scales [rows][cols/32]
extern "C" int nvl_upload_tensor_mxfp4(nvl_model* m, int kind, int layer, const uint8_t* codes, const uint8_t* scales,
                                       int64_t rows, int64_t cols, int layout) {
    return upload_prequant(m, WF_MXFP4, "nvl_upload_tensor_mxfp4", "nvl_set_mx_weight_dtype", kind, layer, codes, scales, nullptr, rows, cols, layout);
}
// INT4 (w4g.h): codes [rows][cols/2] (even k in the low nibble), fp16 scales and zero points [rows][cols/g].
// With nvl_set_gq_expert_dtype also MOE_IN / MOE_OUT, as [E * out][in] (q_kind covers them only then)
extern "C" int nvl_upload_tensor_int4(nvl_model* m, int kind, int layer, const uint8_t* codes, const uint16_t* scales, const uint8_t* zeros,
                                      int64_t rows, int64_t cols, int layout) {
    return upload_prequant(m, WF_INT4, "nvl_upload_tensor_int4", "nvl_set_gq_weight_dtype", kind, layer, codes, scales, zeros, rows, cols, layout);
}

// splitGPT2QKV (generic_loader.go:674-702): c_attn [H, 3H] is [in,out]; columns split Q|K|V.
extern "C" int nvl_upload_gpt2_qkv(nvl_model* m, int layer, const float* w, const float* b) {
    if (!m || !w) return fail(m, NVL_ERR_INVALID, "nvl_upload_gpt2_qkv: null argument");
    NVL_TRY(m)
    const int64_t H = m->H;
    std::vector<float> part((size_t)H * H);
    const int kinds[3] = {NVL_T_WQ, NVL_T_WK, NVL_T_WV};
    const int bk[3] = {NVL_T_BQ, NVL_T_BK, NVL_T_BV};
    for (int s = 0; s < 3; s++) {
        for (int64_t r = 0; r < H; r++)
            memcpy(&part[(size_t)(r * H)], w + r * 3 * H + s * H, (size_t)H * sizeof(float));
        int rc = nvl_upload_tensor(m, kinds[s], layer, part.data(), NVL_DTYPE_F32, H, H, NVL_LAYOUT_IN_OUT);
        if (rc) return rc;
        if (b) {   // generic_loader.go:418-427
            rc = nvl_upload_tensor(m, bk[s], layer, b + s * H, NVL_DTYPE_F32, H, 1, 0);
            if (rc) return rc;
        }
    }
    return NVL_OK;
    NVL_CATCH(m)
}

// splitFalconQKV + combineMQAKV (generic_loader.go:705-765): rows of [H, (nH+2)*hd] hold
// [Q_0 .. Q_{nH-1} | K | V] chunks of hd.
extern "C" int nvl_upload_falcon_qkv(nvl_model* m, int layer, const float* qkv) {
    if (!m || !qkv) return fail(m, NVL_ERR_INVALID, "nvl_upload_falcon_qkv: null argument");
    NVL_TRY(m)
    const int64_t H = m->H, nH = m->nH, hd = m->hd, roww = (nH + 2) * hd;
    std::vector<float> q((size_t)(H * nH * hd)), kv((size_t)(H * 2 * hd));
    for (int64_t r = 0; r < H; r++) {
        memcpy(&q[(size_t)(r * nH * hd)], qkv + r * roww, (size_t)(nH * hd) * sizeof(float));
        memcpy(&kv[(size_t)(r * 2 * hd)], qkv + r * roww + nH * hd, (size_t)(2 * hd) * sizeof(float));
    }
    int rc = nvl_upload_tensor(m, NVL_T_WQ, layer, q.data(), NVL_DTYPE_F32, H, nH * hd, NVL_LAYOUT_IN_OUT);
    if (rc) return rc;
    return nvl_upload_tensor(m, NVL_T_WKV, layer, kv.data(), NVL_DTYPE_F32, H, 2 * hd, NVL_LAYOUT_IN_OUT);
    NVL_CATCH(m)
}

namespace {

// a row permutation in 16-row tiles (the fragment-major layouts move whole tiles): the source tile of every destination
// tile, -1 for a pad tile
std::vector<int32_t> gather_tiles(const std::vector<int32_t>& idx) {
    if (idx.size() % 16) throw std::runtime_error("gather_rows: row count must be a multiple of 16");
    std::vector<int32_t> use(idx.size() / 16);
    for (size_t t = 0; t < use.size(); t++) {
        const int32_t r0 = idx[t * 16];
        for (int c = 1; c < 16; c++)
            if ((r0 < 0) != (idx[t * 16 + c] < 0) || (r0 >= 0 && (idx[t * 16 + c] != r0 + c || (r0 & 15))))
                throw std::runtime_error("gather_rows: permutation does not preserve 16-row tiles");
        use[t] = r0 < 0 ? -1 : r0 / 16;
    }
    return use;
}
// dst row r = src row idx[r] (or zeros).  idx must move whole 16-row groups together (it does: the
// SwiGLU interleave works in blocks of 16), because in the fragment-major bf16 layout the unit that
// can be relocated is a 16-row n-tile (16*K contiguous elements).
void gather_rows(nvl_model* m, const void* src, const std::vector<int32_t>& idx, void* dst, int64_t K) {
    std::vector<int32_t> use = idx;
    int64_t unit = K;
    if (!m->f32) {
        use = gather_tiles(idx);
        unit = 16 * K;
    }
    int32_t* didx = dmalloc<int32_t>((int64_t)use.size());
    NVL_HIP(hipMemcpyAsync(didx, use.data(), use.size() * 4, hipMemcpyHostToDevice, m->stream));
    if (m->f32)
        hipLaunchKernelGGL((gather_rows_kernel<float>), dim3((unsigned)use.size()), dim3(256), 0, m->stream,
                           (const float*)src, didx, (float*)dst, unit);
    else
        hipLaunchKernelGGL((gather_rows_kernel<bf16_t>), dim3((unsigned)use.size()), dim3(256), 0, m->stream,
                           (const bf16_t*)src, didx, (bf16_t*)dst, unit);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    dfree(didx);
}

// interleave [gate F rows | up F rows] into blocks of 16: [g0..15 | u0..15 | g16..31 | ...]
std::vector<int32_t> swiglu_interleave(int64_t F, int64_t src_base) {
    std::vector<int32_t> idx((size_t)(2 * F));
    for (int64_t b = 0; b < F / 16; b++)
        for (int c = 0; c < 16; c++) {
            idx[(size_t)(32 * b + c)] = (int32_t)(src_base + 16 * b + c);
            idx[(size_t)(32 * b + 16 + c)] = (int32_t)(src_base + F + 16 * b + c);
        }
    return idx;
}

// gather_rows for a quantized weight: the codes move as 16-row tiles and the scales with them (wq.h wf_gather_scales; pad
// rows, idx < 0, get codes 0)
void gather_rows_q(nvl_model* m, const DevTensor& src, const std::vector<int32_t>& idx, void* dst, void* dst_qs, int64_t K) {
    const std::vector<int32_t> use = gather_tiles(idx);
    int32_t* didx = dmalloc<int32_t>((int64_t)use.size());
    NVL_HIP(hipMemcpyAsync(didx, use.data(), use.size() * 4, hipMemcpyHostToDevice, m->stream));
    wf_gather_scales(m->stream, src.wf, src.qs, src.rows_pad, idx, didx, dst_qs, K);
    hipLaunchKernelGGL((gather_rows_kernel<uint8_t>), dim3((unsigned)use.size()), dim3(256), 0, m->stream,
                       (const uint8_t*)src.p, didx, (uint8_t*)dst, wf_code_bytes(src.wf, 16 * K));
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    dfree(didx);
}
// the fused FFN-up weight of a layer (SwiGLU: gate|up rows interleaved in blocks of 16)
void fuse_w1(nvl_model* m, LayerW& l, bool swiglu) {
    const int64_t H = m->H;
    if (swiglu && !m->f32) {
        auto idx = swiglu_interleave(m->F, 0);
        const int64_t np = round_up(l.n1, W_ROW_PAD);
        idx.resize((size_t)np, -1);
        DevTensor& t = l.t[NVL_T_W1];
        if (t.qs) {
            l.w1 = dmalloc_bytes(wf_code_bytes(t.wf, np * H));
            l.qs1 = dmalloc_bytes(wf_scale_bytes(t.wf, np, H));
            gather_rows_q(m, t, idx, l.w1, l.qs1, H);
            dfree(t.qs); t.qs = nullptr;
        } else {
            l.w1 = dmalloc_bytes(np * H * (int64_t)m->wsize);
            gather_rows(m, t.p, idx, l.w1, H);
        }
        dfree(t.p); t.p = nullptr;
    } else {
        l.w1 = l.t[NVL_T_W1].p; l.t[NVL_T_W1].p = nullptr;
        l.qs1 = l.t[NVL_T_W1].qs; l.t[NVL_T_W1].qs = nullptr;
    }
}

// does finalize build the decode (dense-masked) form of a MoE layer's down matrices?  (nvl_finalize; ops_impl.h moe_op_setup)
inline bool moe_dense_form(int64_t H, int64_t E, int64_t I) {
    return I % 32 == 0 && H % 16 == 0 && E <= 64 && E / moe_down_slices((int)E) <= 16;
}

// The quantized experts of one MoE layer from their uploaded tensors (l.t[NVL_T_MOE_IN] [E*2I][H], l.t[NVL_T_MOE_OUT]
// [E*H][I]: codes + scales of the upload quantizer), as nvl_finalize leaves them — and as ops_impl.h moe_op_setup builds
// them, through this one function.  idx: the SwiGLU interleave of all experts' gate|up rows.  Frees the uploaded tensors.
void finalize_q_experts(nvl_model* m, LayerW& l, std::vector<int32_t>& idx, int64_t E, int64_t I, bool dense_form) {
    const int64_t H = m->H;
    const int wf = l.t[NVL_T_MOE_IN].wf;
    const int64_t np = round_up(E * 2 * I, W_ROW_PAD), hp = round_up(H, W_ROW_PAD);
    idx.resize((size_t)np, -1);
    l.moe_in = dmalloc_bytes(wf_code_bytes(wf, np * H));
    l.qs_moe_in = dmalloc_bytes(wf_scale_bytes(wf, np, H));
    gather_rows_q(m, l.t[NVL_T_MOE_IN], idx, l.moe_in, l.qs_moe_in, H);
    // down: codes over K = E*I, [H_pad][E*I] (the decode form's layout; the tile path dequantizes from it)
    const DevTensor& d = l.t[NVL_T_MOE_OUT];
    l.moe_out_q = dmalloc_bytes(wf_code_bytes(wf, hp * E * I));
    NVL_HIP(hipMemsetAsync(l.moe_out_q, 0, (size_t)wf_code_bytes(wf, hp * E * I), m->stream));
    int64_t s_rows, s_K;     // where the down scales live (wq.h)
    wf_down_scale_dims(wf, hp, E, I, &s_rows, &s_K);
    l.qs_moe_out = q_alloc_scales(m, wf, s_rows, s_K);
    wf_cat_down(m->stream, wf, d.p, d.qs, d.rows_pad, l.moe_out_q, l.qs_moe_out, H, I, E);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipStreamSynchronize(m->stream));
    if (dense_form) l.moe_out_cat = l.moe_out_q;
    for (int k : {NVL_T_MOE_IN, NVL_T_MOE_OUT}) { dfree(l.t[k].p); l.t[k].p = nullptr; dfree(l.t[k].qs); l.t[k].qs = nullptr; }
}

// quantized experts after finalize_q_experts: the codes by pointer (decode dispatch), and the scratch of one layer's W~ (up,
// then down) for the grouped GEMMs, zeroed
void register_q_experts(nvl_model* m, const LayerW* layers, size_t n_layers, int64_t E, int64_t I) {
    const int64_t H = m->H, hp = round_up(H, W_ROW_PAD);
    for (size_t i = 0; i < n_layers; i++) {
        const LayerW& l = layers[i];
        if (!l.qs_moe_in) continue;
        m->qmap[l.moe_in] = nvl_model::QRef{m->ef, l.qs_moe_in, round_up(E * 2 * I, W_ROW_PAD)};
        if (l.moe_out_cat) m->qmap[l.moe_out_cat] = nvl_model::QRef{m->ef, l.qs_moe_out, hp};
    }
    // (down: the grouped GEMMs read whole 256-row tiles of the last expert past its H rows)
    m->eq_scratch_elems = std::max(round_up(E * 2 * I, W_ROW_PAD) * H, (E * H + 2 * W_ROW_PAD) * I);
    m->eq_scratch = dmalloc<bf16_t>(m->eq_scratch_elems);
    NVL_HIP(hipMemsetAsync(m->eq_scratch, 0, (size_t)m->eq_scratch_elems * 2, m->stream));
}

}  // namespace

extern "C" int nvl_set_kv_scales(nvl_model* m, const float* k_scale, const float* v_scale) {
    if (!m) return fail(nullptr, NVL_ERR_INVALID, "nvl_set_kv_scales: no model");
    if (!m->kv8) return fail(m, NVL_ERR_STATE, "nvl_set_kv_scales: the model's KV cache is not 8-bit (kv_cache_dtype)");
    if (m->kv_written) return fail(m, NVL_ERR_STATE, "nvl_set_kv_scales: the cache has been written (first forward done)");
    if (!k_scale || !v_scale) return fail(m, NVL_ERR_INVALID, "nvl_set_kv_scales: NULL scales");
    const bool any_mamba = (m->cfg.mamba_layer_mask[0] | m->cfg.mamba_layer_mask[1]) != 0;
    for (int l = 0; l < m->L; l++) {
        if (any_mamba && ((m->cfg.mamba_layer_mask[l >> 6] >> (l & 63)) & 1)) continue;     // Mamba2 layers: ignored
        if (!(k_scale[l] > 0.f) || !(v_scale[l] > 0.f) || !std::isfinite(k_scale[l]) || !std::isfinite(v_scale[l]))
            return fail(m, NVL_ERR_INVALID, "nvl_set_kv_scales: scales must be finite and positive");
    }
    for (int l = 0; l < m->L; l++) { m->k_scale[(size_t)l] = k_scale[l]; m->v_scale[(size_t)l] = v_scale[l]; }
    for (int l = 0; l < m->L; l++)        // (Mamba2 entries are not used; keep them valid)
        if (!(m->k_scale[(size_t)l] > 0.f) || !(m->v_scale[(size_t)l] > 0.f) || !std::isfinite(m->k_scale[(size_t)l]) || !std::isfinite(m->v_scale[(size_t)l]))
            m->k_scale[(size_t)l] = m->v_scale[(size_t)l] = 1.0f;
    return NVL_OK;
}

// The weight-format setters: every rule is wfmt.h's wf_decide(); an entry point names what it sets and through which family.
static int set_dtype(nvl_model* m, int target, int family, int value, int group, const char* fn) {
    if (!m) return fail(nullptr, NVL_ERR_INVALID, std::string(fn) + ": no model");
    const WfFacts facts{m->f32, m->tp > 1 || m->tp_force, m->cfg.use_moe && m->cfg.num_experts > 0, m->H, m->F,
                        m->finalized, m->w2d_uploaded, m->expert_uploaded};
    const WfDecision d = wf_decide(WfState{m->wf, m->ef, m->hf, m->a8}, facts, WfRequest{target, family, value, group, fn});
    if (d.code != NVL_OK) return fail(m, d.code, d.msg);
    m->wf = d.state.wf; m->ef = d.state.ef; m->hf = d.state.hf; m->a8 = d.state.a8;
    return NVL_OK;
}
extern "C" int nvl_set_weight_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_PROJ, WFAM_FP8, dtype, 0, "nvl_set_weight_dtype"); }
extern "C" int nvl_set_mx_weight_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_PROJ, WFAM_MX, dtype, 0, "nvl_set_mx_weight_dtype"); }
extern "C" int nvl_set_gq_weight_dtype(nvl_model* m, int dtype, int group_size) {
    return set_dtype(m, WT_PROJ, WFAM_GQ, dtype, group_size, "nvl_set_gq_weight_dtype");
}
extern "C" int nvl_set_expert_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_EXPERT, WFAM_FP8, dtype, 0, "nvl_set_expert_dtype"); }
extern "C" int nvl_set_mx_expert_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_EXPERT, WFAM_MX, dtype, 0, "nvl_set_mx_expert_dtype"); }
extern "C" int nvl_set_gq_expert_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_EXPERT, WFAM_GQ, dtype, 0, "nvl_set_gq_expert_dtype"); }
extern "C" int nvl_set_mx_head_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_HEAD, WFAM_MX, dtype, 0, "nvl_set_mx_head_dtype"); }
extern "C" int nvl_set_act_dtype(nvl_model* m, int dtype) { return set_dtype(m, WT_ACT, WFAM_FP8, dtype, 0, "nvl_set_act_dtype"); }

extern "C" int nvl_set_mamba_conv_state(nvl_model* m, int mode) {
    if (!m) return fail(nullptr, NVL_ERR_INVALID, "nvl_set_mamba_conv_state: no model");
    if (m->finalized) return fail(m, NVL_ERR_STATE, "nvl_set_mamba_conv_state: call it before nvl_finalize");
    if (mode != NVL_MAMBA_CONV_PER_CALL && mode != NVL_MAMBA_CONV_CARRIED)
        return fail(m, NVL_ERR_INVALID, "nvl_set_mamba_conv_state: unknown mode");
    if (!m->n_mamba) return fail(m, NVL_ERR_INVALID, "nvl_set_mamba_conv_state: the model has no Mamba2 layers");
    m->conv_carried = mode == NVL_MAMBA_CONV_CARRIED;      // (K == 1: no tail, nothing to carry — accepted, changes nothing)
    return NVL_OK;
}

extern "C" int nvl_finalize(nvl_model* m) {
    if (!m) return NVL_ERR_INVALID;
    if (m->finalized) return fail(m, NVL_ERR_STATE, "nvl_finalize: already finalized");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    const nvl_model_config& c = m->cfg;
    const int64_t H = m->H, hd = m->hd;
    auto need = [&](bool ok, const char* what) { if (!ok) throw std::runtime_error(std::string("nvl_finalize: missing tensor: ") + what); };
    need(m->g[NVL_T_TOK_EMB].present(), "token embedding");
    need(m->g[NVL_T_FINAL_NORM_W].present(), "final norm weight");
    if (c.norm_type == NVL_NORM_LAYER) need(m->g[NVL_T_FINAL_NORM_B].present(), "final norm bias (LayerNorm)");

    for (int li = 0; li < m->L; li++) {
        LayerW& l = m->layers[li];
        need(l.t[NVL_T_ATTN_NORM_W].present(), "attention/input norm weight");
        if (l.mamba) {       // Mamba2 block: in/out projections + SSM parameters, then the shared MLP (loadMamba2 + loadFFN)
            need(l.t[NVL_T_MAMBA_IN_PROJ].present() && l.t[NVL_T_MAMBA_OUT_PROJ].present() && l.t[NVL_T_MAMBA_CONV_W].present(),
                 "Mamba2 in_proj / out_proj / conv1d weight");
            need(l.t[NVL_T_FFN_NORM_W].present() && l.t[NVL_T_W1].present() && l.t[NVL_T_W2].present(), "Mamba2 block: FFN norm / shared MLP");
            const bool swiglu = c.activation_type == NVL_ACT_SWIGLU;
            l.n1 = swiglu ? 2 * m->F : m->F;
            fuse_w1(m, l, swiglu);
            continue;
        }
        need(l.t[NVL_T_WQ].present() && l.t[NVL_T_WO].present(), "attention Q/O projection");
        const bool mqa = c.attention_type == NVL_ATTN_MQA;
        if (mqa) need(l.t[NVL_T_WKV].present(), "MQA fused KV projection");
        else need(l.t[NVL_T_WK].present() && l.t[NVL_T_WV].present(), "K/V projection");
        if (c.block_style == NVL_BLOCK_SEQUENTIAL) need(l.t[NVL_T_FFN_NORM_W].present(), "FFN norm weight");
        // ---- fused QKV [n_qkv_pad][H]: rows Q | K | V (canonical rows are contiguous: plain copies)
        const int64_t nq = (int64_t)m->nH * hd, nkv = (int64_t)m->nKV * hd;
        const int64_t npad = round_up(m->n_qkv, W_ROW_PAD);
        // quantized weights: the codes move like bf16 rows and the scales beside them (row counts are multiples of 16: whole
        // tiles of both); cat copies the parts Q | K | V (or Q | KV) of `bytes`-per-row data into dst
        const int wf = l.t[NVL_T_WQ].wf;
        const size_t rowb = wf != WF_BF16 ? (size_t)wf_code_bytes(wf, H) : (size_t)H * m->wsize;
        auto cat = [&](void* dst, size_t bytes, void* DevTensor::*part) {
            char* d = (char*)dst;
            NVL_HIP(hipMemcpyAsync(d, l.t[NVL_T_WQ].*part, nq * bytes, hipMemcpyDeviceToDevice, m->stream));
            if (mqa) {
                NVL_HIP(hipMemcpyAsync(d + nq * bytes, l.t[NVL_T_WKV].*part, 2 * hd * bytes, hipMemcpyDeviceToDevice, m->stream));
            } else {
                NVL_HIP(hipMemcpyAsync(d + nq * bytes, l.t[NVL_T_WK].*part, nkv * bytes, hipMemcpyDeviceToDevice, m->stream));
                NVL_HIP(hipMemcpyAsync(d + (nq + nkv) * bytes, l.t[NVL_T_WV].*part, nkv * bytes, hipMemcpyDeviceToDevice, m->stream));
            }
        };
        l.w_qkv = dmalloc_bytes(npad * (int64_t)rowb);
        NVL_HIP(hipMemsetAsync(l.w_qkv, 0, (size_t)npad * rowb, m->stream));
        cat(l.w_qkv, rowb, &DevTensor::p);
        if (wf != WF_BF16) {
            l.qs_qkv = q_alloc_scales(m, wf, npad, H);
            cat(l.qs_qkv, (size_t)wf_scale_bytes(wf, 1, H), &DevTensor::qs);
        }
        l.n_qkv = m->n_qkv;
        if (l.t[NVL_T_BQ].present() || l.t[NVL_T_BK].present() || l.t[NVL_T_BV].present()) {
            l.b_qkv = dmalloc<float>(m->n_qkv);
            NVL_HIP(hipMemsetAsync(l.b_qkv, 0, (size_t)m->n_qkv * 4, m->stream));
            if (l.t[NVL_T_BQ].present()) NVL_HIP(hipMemcpyAsync(l.b_qkv, l.t[NVL_T_BQ].p, nq * 4, hipMemcpyDeviceToDevice, m->stream));
            if (l.t[NVL_T_BK].present()) NVL_HIP(hipMemcpyAsync(l.b_qkv + nq, l.t[NVL_T_BK].p, nkv * 4, hipMemcpyDeviceToDevice, m->stream));
            if (l.t[NVL_T_BV].present()) NVL_HIP(hipMemcpyAsync(l.b_qkv + nq + nkv, l.t[NVL_T_BV].p, nkv * 4, hipMemcpyDeviceToDevice, m->stream));
        }
        NVL_HIP(hipStreamSynchronize(m->stream));
        for (int k : {NVL_T_WQ, NVL_T_WK, NVL_T_WV, NVL_T_WKV}) { dfree(l.t[k].p); l.t[k].p = nullptr; dfree(l.t[k].qs); l.t[k].qs = nullptr; }

        // ---- FFN / MoE
        if (c.use_moe) {
            need(l.t[NVL_T_ROUTER].present() && l.t[NVL_T_MOE_IN].present() && l.t[NVL_T_MOE_OUT].present(), "MoE tensors");
            if (!m->f32) {   // interleave gate/up rows per expert for the fused SwiGLU epilogue
                const int64_t E = c.num_experts, I = m->F;
                std::vector<int32_t> idx;
                idx.reserve((size_t)(E * 2 * I));
                for (int64_t e = 0; e < E; e++) {
                    auto one = swiglu_interleave(I, e * 2 * I);
                    idx.insert(idx.end(), one.begin(), one.end());
                }
                const bool dense_form = moe_dense_form(H, E, I);
                if (l.t[NVL_T_MOE_IN].qs) {     // quantized experts: codes + scales follow the interleave
                    finalize_q_experts(m, l, idx, E, I, dense_form);
                    continue;
                }
                l.moe_in = dmalloc_bytes(round_up(E * 2 * I, W_ROW_PAD) * H * (int64_t)m->wsize);   // (+ zero pad rows: the decode kernels read whole tiles)
                NVL_HIP(hipMemsetAsync(l.moe_in, 0, (size_t)(round_up(E * 2 * I, W_ROW_PAD) * H) * m->wsize, m->stream));
                gather_rows(m, l.t[NVL_T_MOE_IN].p, idx, l.moe_in, H);
                dfree(l.t[NVL_T_MOE_IN].p); l.t[NVL_T_MOE_IN].p = nullptr;
                if (dense_form) {
                    // decode form: the experts' down matrices side by side along K
                    const int64_t hp = round_up(H, W_ROW_PAD);
                    l.moe_out_cat = dmalloc_bytes(hp * E * I * 2);
                    NVL_HIP(hipMemsetAsync(l.moe_out_cat, 0, (size_t)(hp * E * I) * 2, m->stream));
                    hipLaunchKernelGGL(moe_cat_down_kernel, dim3((unsigned)(H / 16), (unsigned)E), dim3(256), 0, m->stream,
                                       (const bf16_t*)l.t[NVL_T_MOE_OUT].p, (bf16_t*)l.moe_out_cat, (int)H, (int)I, (int)E);
                    NVL_HIP(hipGetLastError());
                    NVL_HIP(hipStreamSynchronize(m->stream));
                }
            } else {
                l.moe_in = l.t[NVL_T_MOE_IN].p; l.t[NVL_T_MOE_IN].p = nullptr;
            }
        } else {
            need(l.t[NVL_T_W1].present() && l.t[NVL_T_W2].present(), "FFN weights");
            const bool swiglu = c.activation_type == NVL_ACT_SWIGLU;
            l.n1 = swiglu ? 2 * m->F : m->F;
            fuse_w1(m, l, swiglu);
        }
    }
    // ---- LM head: tied (or absent) => the token embedding itself, already [Vpad][H] K-contiguous
    const DevTensor& head = (!c.tied_embedding && m->g[NVL_T_LM_HEAD].present()) ? m->g[NVL_T_LM_HEAD] : m->g[NVL_T_TOK_EMB];   // generic_loader.go:255-259
    m->lm_head = head.p;
    if (m->wf != WF_BF16) {   // the quantized weights by code pointer (gemm() dispatch) and the dequantize scratch of the tile path
        int64_t big = 0;
        auto reg = [&](const void* p, const void* qs, int64_t rows, int64_t K) {
            if (!p || !qs) return;
            m->qmap[p] = nvl_model::QRef{m->wf, qs, round_up(rows, W_ROW_PAD)};
            big = std::max(big, round_up(rows, W_ROW_PAD) * K);
        };
        for (auto& l : m->layers) {
            reg(l.w_qkv, l.qs_qkv, l.n_qkv, H); reg(l.w1, l.qs1, l.n1, H);
            reg(l.t[NVL_T_WO].p, l.t[NVL_T_WO].qs, H, l.t[NVL_T_WO].cols); reg(l.t[NVL_T_W2].p, l.t[NVL_T_W2].qs, H, l.t[NVL_T_W2].cols);
        }
        if (head.qs) {   // (fp8, or MXFP4 with nvl_set_mx_head_dtype; at least one row tile of the LM head: it runs in chunks)
            m->qmap[head.p] = nvl_model::QRef{m->wf, head.qs, round_up(m->V, W_ROW_PAD)};
            big = std::max(big, W_ROW_PAD * H);
        }
        m->wq_scratch_elems = big;
        if (big) m->wq_scratch = dmalloc<bf16_t>(big);
        // quantized experts: the codes by pointer (decode dispatch), and the scratch of one layer's W~ (up, then down)
        if (m->ef != WF_BF16) register_q_experts(m, m->layers.data(), m->layers.size(), c.num_experts, m->F);
        if (m->a8) {   // the activation codes + row scales of the W8A8 tile step: every row of a batch, the widest K
            int64_t kmax = H;
            for (auto& l : m->layers) {
                if (l.t[NVL_T_WO].qs) kmax = std::max(kmax, l.t[NVL_T_WO].cols);
                if (l.t[NVL_T_W2].qs) kmax = std::max(kmax, l.t[NVL_T_W2].cols);
            }
            m->a8_rows = round_up(m->opts.max_batch_tokens, 16);
            m->a8_k = kmax;
            m->a8_codes = (uint8_t*)dmalloc_bytes(m->a8_rows * kmax);
            m->a8_scale = dmalloc<float>(m->a8_rows);
        }
    }

    // ---- RoPE tables in fp64 on the host, exactly as NewRoPECache (rope.go:18-50)
    bool rope = false; double base = c.rope_base;
    if (c.attention_type == NVL_ATTN_MQA) { rope = true; base = 10000.0; }           // mqa.go:35
    else if (c.attention_type == NVL_ATTN_GQA && c.position_type == NVL_POS_ROPE) rope = true;
    if (rope) {
        std::vector<float> ct, stt;
        rope_tables(base, c.max_seq_len, (int)hd, ct, stt);
        m->rope_cos = dmalloc<float>((int64_t)ct.size());
        m->rope_sin = dmalloc<float>((int64_t)stt.size());
        NVL_HIP(hipMemcpy(m->rope_cos, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
        NVL_HIP(hipMemcpy(m->rope_sin, stt.data(), stt.size() * 4, hipMemcpyHostToDevice));
    }

    // ---- KV slabs: [slot][layer][kv head][Tmax][hd]; zero-filled so stale tiles hold finite values
    m->layer_stride = (int64_t)m->nKV * m->Tmax * hd;
    m->slot_stride = m->layer_stride * m->L;
    const int64_t kv_elems = m->slot_stride * m->num_blocks;
    m->kcache = dmalloc_bytes(kv_elems * (int64_t)m->kv_esize);
    m->vcache = dmalloc_bytes(kv_elems * (int64_t)m->kv_esize);
    NVL_HIP(hipMemsetAsync(m->kcache, 0, (size_t)kv_elems * m->kv_esize, m->stream));
    NVL_HIP(hipMemsetAsync(m->vcache, 0, (size_t)kv_elems * m->kv_esize, m->stream));
    m->slot_len.assign((size_t)m->opts.max_seqs, 0);
    m->slot_tick.assign((size_t)m->opts.max_seqs, 0);
    m->slot_pin.assign((size_t)m->opts.max_seqs, 0);
    m->free_slots.clear();
    for (int s = m->opts.max_seqs - 1; s >= 0; s--) m->free_slots.push_back(s);

    // ---- workspaces
    const int64_t Mmax = m->opts.max_batch_tokens, S = m->opts.max_seqs;
    const int64_t Mp = round_up(Mmax, 64);   // GEMM operands are whole 16-row tiles; decode reads up to 64 rows
    const int64_t qw = (int64_t)m->nH * hd;
    m->x = dmalloc<float>(Mmax * H);
    m->xn = dmalloc_bytes(Mp * H * (int64_t)m->wsize);
    m->qkv = dmalloc<float>(Mmax * m->n_qkv);
    m->q = dmalloc_bytes(Mmax * qw * (int64_t)m->wsize);
    m->attn_out = dmalloc_bytes(Mp * qw * (int64_t)m->wsize);
    if (!m->f32 && (m->hd == 64 || m->hd == 128)) {     // partial results of a split decode attention (attn.h)
        m->attn_part = dmalloc<float>((int64_t)ATTN_SPLIT_MAX_PAIRS * ATTN_SPLIT_MAX * (m->hd == 64 ? attn_part_floats<64>() : attn_part_floats<128>()));
        m->attn_part_cnt = dmalloc<int32_t>(ATTN_SPLIT_MAX_PAIRS);
        NVL_HIP(hipMemset(m->attn_part_cnt, 0, ATTN_SPLIT_MAX_PAIRS * sizeof(int32_t)));
    }
    const int64_t k = c.use_moe ? c.num_experts_per_tok : 1;
    m->hbuf = dmalloc_bytes(round_up(Mmax * k, 64) * m->F * (int64_t)m->wsize);
    NVL_HIP(hipMemsetAsync(m->xn, 0, (size_t)(Mp * H) * m->wsize, m->stream));
    NVL_HIP(hipMemsetAsync(m->attn_out, 0, (size_t)(Mp * qw) * m->wsize, m->stream));
    NVL_HIP(hipMemsetAsync(m->hbuf, 0, (size_t)(round_up(Mmax * k, 64) * m->F) * m->wsize, m->stream));
    if (m->f32 && (c.activation_type == NVL_ACT_SWIGLU || c.use_moe)) m->h2 = dmalloc<float>(Mmax * k * 2 * m->F);
    m->xn_last = dmalloc_bytes(round_up(S, 64) * H * (int64_t)m->wsize);
    NVL_HIP(hipMemsetAsync(m->xn_last, 0, (size_t)(round_up(S, 64) * H) * m->wsize, m->stream));
    m->logit_rows = S;
    m->logits = dmalloc<float>(S * (int64_t)m->Vpad);
    m->argmax_dev = dmalloc<int32_t>(std::max<int64_t>(S, Mmax));
    m->argmax_pval = dmalloc<float>(std::max<int64_t>(S, Mmax) * cdiv(m->V, ARGMAX_CHUNK));
    m->argmax_pidx = dmalloc<int32_t>(std::max<int64_t>(S, Mmax) * cdiv(m->V, ARGMAX_CHUNK));
    if (c.use_moe) {
        m->router_logits = dmalloc<float>(Mmax * 128);
        m->expert_ids = dmalloc<int32_t>(Mmax * k);
        m->expert_w = dmalloc<float>(Mmax * k);
        m->seg_start = dmalloc<int32_t>(c.num_experts + 1);
        m->moe_counts = dmalloc<int32_t>(c.num_experts);
        m->moe_cursor = dmalloc<int32_t>(c.num_experts);
        m->moe_tile_map = dmalloc<int32_t>(4 * (cdiv(Mmax * k, 128) + c.num_experts));
        m->moe_n_mtiles = dmalloc<int32_t>(4);
        m->perm_token = dmalloc<int32_t>(Mmax * k);
        m->slot_of = dmalloc<int32_t>(Mmax * k);
        m->moe_eo = dmalloc<float>(Mmax * k * H);
        if (!m->f32) m->moe_xg = dmalloc_bytes(round_up(Mmax * k, 64) * H * 2);
        if (!m->f32) {
            m->moe_gate = dmalloc<float>(64 * (int64_t)c.num_experts);
            m->moe_hall = dmalloc_bytes(64 * (int64_t)c.num_experts * m->F * 2);
            NVL_HIP(hipMemsetAsync(m->moe_hall, 0, (size_t)(64 * (int64_t)c.num_experts * m->F) * 2, m->stream));
            m->moe_part = dmalloc<float>((int64_t)MOE_DOWN_SLICES * 64 * H);
        }
    }
    if (m->n_mamba) {
        m->ssm_layer_stride = (int64_t)m->m_nh * m->m_hd * m->m_ss;
        m->ssm_slot_stride = m->ssm_layer_stride * m->n_mamba;
        m->ssm_state = dmalloc<float>(m->ssm_slot_stride * S);
        NVL_HIP(hipMemsetAsync(m->ssm_state, 0, (size_t)(m->ssm_slot_stride * S) * 4, m->stream));
        if (m->m_K > 1) {     // raw xBC rows of a chunked prefill's last K-1 tokens, per (slot, Mamba2 layer)
            m->conv_tail_layer_stride = (int64_t)(m->m_K - 1) * m->mConv;
            m->conv_tail_slot_stride = m->conv_tail_layer_stride * m->n_mamba;
            m->conv_tail = dmalloc<float>(m->conv_tail_slot_stride * S);
            NVL_HIP(hipMemsetAsync(m->conv_tail, 0, (size_t)(m->conv_tail_slot_stride * S) * 4, m->stream));
        }
        m->mproj = dmalloc<float>(Mmax * m->mP);
        m->mxbc = dmalloc<float>(Mmax * m->mConv);
        m->mdelta = dmalloc<float>(Mmax * m->m_nh);
        m->my = dmalloc<float>(Mmax * m->mEH);
        m->myn = dmalloc_bytes(Mp * m->mEH * (int64_t)m->wsize);
        NVL_HIP(hipMemsetAsync(m->myn, 0, (size_t)(Mp * m->mEH) * m->wsize, m->stream));
    }
    // split-K partial slices of the residual projections: decode (<= 64 rows) and mid-size batches (<= SK_TILE_MAX_M rows)
    m->sk_rows = (int)std::min<int64_t>(std::max<int64_t>(Mmax, 64), SK_TILE_MAX_M);
    if (!m->f32) m->sk_part = dmalloc<float>((int64_t)std::max(m->sk_max_slices, SK_TILE_MAX_SLICES) * m->sk_rows * H);
    if (!m->f32) m->rs_part = dmalloc<float>((int64_t)cdiv(H, 8) * DEFER_MAX_M);      // x^2 partials per 16 (half tiles: 8) columns
    if (m->tp > 1 || m->tp_force) m->tp_part = dmalloc<float>(Mmax * H);
    m->meta_ints = 3 * Mmax + 5 * S + m->table_cap + 16;
    NVL_HIP(hipHostMalloc((void**)&m->meta_host, (size_t)m->meta_ints * 4, hipHostMallocDefault));
    m->meta_dev = dmalloc<int32_t>(m->meta_ints);
    NVL_HIP(hipHostMalloc((void**)&m->am_host, (size_t)std::max<int64_t>(S, Mmax) * 4, hipHostMallocDefault));
    NVL_HIP(hipHostMalloc((void**)&m->verify_host, (size_t)(S + Mmax) * 4, hipHostMallocDefault));    // a verify pass: [accepted S | ids Mmax]
    m->verify_dev = dmalloc<int32_t>(S + Mmax);
    NVL_HIP(hipHostMalloc((void**)&m->vs_host, (size_t)(4 + 3 * S + Mmax) * 4, hipHostMallocDefault));   // a sampled verify pass (bind_vs) + S history lengths to upload
    m->vs_dev = dmalloc<int32_t>(4 + 2 * S + Mmax);
    m->ring_pos0 = dmalloc<int32_t>(S);
    NVL_HIP(hipStreamSynchronize(m->stream));   // every memset/copy above ran on the model's own (non-blocking) stream
    m->finalized = true;
    return NVL_OK;
    NVL_CATCH(m)
}

// =================================================================================================
// tensor parallel group
// =================================================================================================
extern "C" int nvl_tp_get_unique_id(void* id_out, int bytes) {
    if (!id_out || bytes < (int)sizeof(ncclUniqueId)) return fail(nullptr, NVL_ERR_INVALID, "nvl_tp_get_unique_id: need a 128-byte buffer");
    ncclUniqueId id;
    const ncclResult_t rc = ncclGetUniqueId(&id);
    if (rc != ncclSuccess) return fail(nullptr, NVL_ERR_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(rc));
    memcpy(id_out, &id, sizeof id);
    return NVL_OK;
}
extern "C" int nvl_tp_init(nvl_model* m, const void* id_in, int bytes) {
    if (!m || !id_in || bytes < (int)sizeof(ncclUniqueId)) return fail(m, NVL_ERR_INVALID, "nvl_tp_init: bad arguments");
    if (m->tp_comm || m->tp_local) return fail(m, NVL_ERR_STATE, "nvl_tp_init: a group is already attached");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof id);
    ncclComm_t comm;
    const ncclResult_t rc = ncclCommInitRank(&comm, m->tp, id, m->tp_rank);
    if (rc != ncclSuccess) return fail(m, NVL_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(rc));
    m->tp_comm = comm;
    return NVL_OK;
    NVL_CATCH(m)
}
namespace {
constexpr int P2P_ONESHOT_CAP_ROWS = 64;
void p2p_alloc(nvl_model* m) {
    if (m->p2p_buf) return;
    const int64_t esz = m->f32 ? 4 : 2, T = m->tp;
    const int64_t cap = (int64_t)m->opts.max_batch_tokens * m->H;
    m->p2p_in1_stride = (int64_t)P2P_ONESHOT_CAP_ROWS * m->H;
    m->p2p_in2_stride = round_up(cdiv(cap, T), 8);       // (16-byte peer stores: 8 bf16)
    m->p2p_res_stride = round_up(cap, 8);
    m->p2p_off_in1 = 1024;
    m->p2p_off_in2 = round_up(m->p2p_off_in1 + 2 * T * m->p2p_in1_stride * esz, 256);
    m->p2p_off_res = round_up(m->p2p_off_in2 + 2 * T * m->p2p_in2_stride * esz, 256);
    m->p2p_bytes = (size_t)round_up(m->p2p_off_res + 2 * m->p2p_res_stride * esz, 256);
    void* p = nullptr;
    NVL_HIP(hipExtMallocWithFlags(&p, m->p2p_bytes, hipDeviceMallocUncached));     // coherent across GPUs: peers write it, we poll it
    m->p2p_buf = (char*)p;
    NVL_HIP(hipMemset(m->p2p_buf, 0, m->p2p_bytes));
}
}  // namespace
extern "C" int nvl_tp_p2p_export(nvl_model* m, void* handle_out, int bytes) {
    if (!m || !handle_out || bytes < (int)sizeof(hipIpcMemHandle_t)) return fail(m, NVL_ERR_INVALID, "nvl_tp_p2p_export: need a 64-byte buffer");
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_tp_p2p_export: finalize the model first");
    if (m->tp < 2) return fail(m, NVL_ERR_STATE, "nvl_tp_p2p_export: the model is not tensor-parallel");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    p2p_alloc(m);
    hipIpcMemHandle_t h;
    NVL_HIP(hipIpcGetMemHandle(&h, m->p2p_buf));
    memcpy(handle_out, &h, sizeof h);
    return NVL_OK;
    NVL_CATCH(m)
}
extern "C" int nvl_tp_p2p_attach(nvl_model* m, const void* handles, int bytes_per_handle) {
    if (!m || !handles || bytes_per_handle < (int)sizeof(hipIpcMemHandle_t)) return fail(m, NVL_ERR_INVALID, "nvl_tp_p2p_attach: bad arguments");
    if (!m->p2p_buf) return fail(m, NVL_ERR_STATE, "nvl_tp_p2p_attach: call nvl_tp_p2p_export first");
    if (m->p2p_ready) return fail(m, NVL_ERR_STATE, "nvl_tp_p2p_attach: already attached");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    for (int r = 0; r < m->tp; r++) {
        if (r == m->tp_rank) { m->p2p_peer[r] = m->p2p_buf; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, (const char*)handles + (size_t)r * bytes_per_handle, sizeof h);
        void* p = nullptr;
        NVL_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        m->p2p_peer[r] = (char*)p;
    }
    m->p2p_ready = true;
    return NVL_OK;
    NVL_CATCH(m)
}

// After a timed-out all-reduce (nvl_forward failed with "timed out waiting for a peer rank") the group's arrival counters are
// out of step.  Every rank calls this while NO rank is inside a forward call (e.g. behind a host barrier): it zeroes the
// rank's own header — arrival counters, call counters, error word — and drops the captured graphs.
extern "C" int nvl_tp_p2p_rearm(nvl_model* m) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->p2p_buf) return fail(m, NVL_ERR_STATE, "nvl_tp_p2p_rearm: no P2P group (nvl_tp_p2p_export / _attach first)");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamSynchronize(m->stream));
    NVL_HIP(hipMemset(m->p2p_buf, 0, 1024));
    NVL_HIP(hipDeviceSynchronize());
    return NVL_OK;
    NVL_CATCH(m)
}

extern "C" int nvl_tp_attach_local(nvl_model** models, int n) {
    if (!models || n < 1 || n > 8) return fail(nullptr, NVL_ERR_INVALID, "nvl_tp_attach_local: bad arguments");
    bool seen[8] = {false};
    int64_t need = 0;
    for (int i = 0; i < n; i++) {
        nvl_model* m = models[i];
        if (!m || m->tp != n || m->tp_rank < 0 || m->tp_rank >= n || seen[m->tp_rank] || m->tp_comm || m->tp_local ||
            m->device != models[0]->device)
            return fail(nullptr, NVL_ERR_INVALID, "nvl_tp_attach_local: members must be the n distinct ranks of one tp_size = n group on one device");
        seen[m->tp_rank] = true;
        need = std::max<int64_t>(need, (int64_t)m->opts.max_batch_tokens * m->H);
    }
    try {
        nvl_local_group* g = new nvl_local_group();
        g->n = n; g->refs = n;
        NVL_HIP(hipSetDevice(models[0]->device));
        g->scratch = dmalloc<float>(need);
        g->scratch_floats = need;
        for (int i = 0; i < n; i++) models[i]->tp_local = g;
        return NVL_OK;
    } catch (const HipError& e) {
        return fail(nullptr, NVL_ERR_HIP, hipGetErrorString(e.code));
    }
}

// =================================================================================================
// sequences
// =================================================================================================
namespace {
// Open a KV slot for seq_id.  evict: when every slot is taken, drop the least-recently-forwarded sequence that is not
// pinned (= not part of the forward call being assembled) and reuse its slot.  The reference keeps map[int64]*KVCache
// forever and the engine never calls ClearCache (tensor_model_runner.go:11-18,59-68; llm_engine.go:35-37), so the runner
// entry points evict; a later decode of an evicted sequence finds no slot and is re-prefilled from its full TokenIDs
// (runner_impl), which is what makes eviction safe.  The explicit nvl_seq_open keeps its NVL_ERR_NO_SLOT contract.
int seq_open_impl(nvl_model* m, int64_t seq_id, bool evict) {
    if (!m || !m->finalized) return fail(m, NVL_ERR_STATE, "nvl_seq_open: model not finalized");
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_seq_open: the model is in paged-KV mode (the host's block manager owns the cache)");
    auto it = m->seq_slot.find(seq_id);
    if (it != m->seq_slot.end()) { m->slot_tick[(size_t)it->second] = ++m->tick; return NVL_OK; }
    if (m->free_slots.empty()) {
        if (!evict) return fail(m, NVL_ERR_NO_SLOT, "nvl_seq_open: all KV slots in use");
        auto victim = m->seq_slot.end();
        for (auto jt = m->seq_slot.begin(); jt != m->seq_slot.end(); ++jt) {
            if (m->slot_pin[(size_t)jt->second]) continue;
            if (victim == m->seq_slot.end() || m->slot_tick[(size_t)jt->second] < m->slot_tick[(size_t)victim->second]) victim = jt;
        }
        if (victim == m->seq_slot.end()) return fail(m, NVL_ERR_NO_SLOT, "nvl_runner_run: every KV slot belongs to the batch being assembled");
        m->free_slots.push_back(victim->second);
        m->seq_slot.erase(victim);
        m->stats.evictions++;
    }
    const int s = m->free_slots.back(); m->free_slots.pop_back();
    m->seq_slot[seq_id] = s; m->slot_len[(size_t)s] = 0; m->slot_tick[(size_t)s] = ++m->tick; m->slot_pin[(size_t)s] = 0;
    return NVL_OK;
}
}  // namespace
extern "C" int nvl_seq_open(nvl_model* m, int64_t seq_id) {
    NVL_TRY(m)
    return seq_open_impl(m, seq_id, false);
    NVL_CATCH(m)
}
extern "C" int nvl_seq_reset(nvl_model* m, int64_t seq_id) {
    const int rc = nvl_seq_open(m, seq_id);
    if (rc) return rc;
    m->slot_len[(size_t)m->seq_slot[seq_id]] = 0;
    return NVL_OK;
}
extern "C" int nvl_seq_close(nvl_model* m, int64_t seq_id) {
    if (!m) return NVL_ERR_INVALID;
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return NVL_OK;   // delete() of a missing key is a no-op in Go
    m->free_slots.push_back(it->second);
    m->seq_slot.erase(it);
    return NVL_OK;
}
extern "C" int nvl_seq_close_all(nvl_model* m) {
    if (!m) return NVL_ERR_INVALID;
    for (auto& kv : m->seq_slot) m->free_slots.push_back(kv.second);
    m->seq_slot.clear();
    return NVL_OK;
}
extern "C" int nvl_seq_len(nvl_model* m, int64_t seq_id) {
    if (!m) return NVL_ERR_INVALID;
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return NVL_ERR_UNKNOWN_SEQ;
    return m->slot_len[(size_t)it->second];
}

// =================================================================================================
// forward
// =================================================================================================
namespace {

struct Meta {   // device pointers into meta_dev
    int32_t *tokens, *tok_pos, *tok_tbl, *seq_tok_start, *seq_len, *seq_pos, *seq_tbl, *last_rows, *blk_table;
};
// layout of meta_host / meta_dev for a call carrying M tokens:
//   [seq_tok_start S | seq_len S | seq_pos S | seq_tbl S | last_rows S | blk_table table_cap | tokens M | tok_pos M | tok_tbl M]
Meta bind_meta(const nvl_model* m, int32_t* base, int M) {
    const int64_t S = m->opts.max_seqs;
    Meta md;
    md.seq_tok_start = base; md.seq_len = base + S; md.seq_pos = base + 2 * S; md.seq_tbl = base + 3 * S;
    md.last_rows = base + 4 * S; md.blk_table = base + 5 * S;
    md.tokens = md.blk_table + m->table_cap; md.tok_pos = md.tokens + M; md.tok_tbl = md.tok_pos + M;
    return md;
}
size_t meta_bytes(const nvl_model* m, int M) { return (size_t)(5 * (int64_t)m->opts.max_seqs + m->table_cap + 3 * (int64_t)M) * 4; }

static int g_norm_t16 = 1;     // nvl_set_tuning key 9: norm_tile16_kernel for prefill-sized bf16 norms (0 = norm_kernel)
template <typename ActT>
void launch_norm(nvl_model* m, float* x, const int32_t* rows_idx, const float* w, const float* b,
                 void* y, int rows) {
    KScope ks(m, KC_OTHER, 0, KS_NORM, (double)rows * m->H * (4.0 + (double)m->wsize));
    PendingResid pr{nullptr, 0, 0, 0.f, nullptr, nullptr};
    m->dense_ran[NVL_DENSE_RAN_NORMS]++;    // (what ran, for nvl_op_dense_stages; below: the kernel that completes a projection's pending add)
    int* consumed = m->pending_slices > 0 && !m->pending_slot_of ? &m->dense_ran[NVL_DENSE_RAN_CONSUMER + m->pending_from] : nullptr;
    if (m->pending_slices > 0) {            // complete the residual add the previous decode GEMM left as split-K slices
        pr.part = m->pending_part; pr.slices = m->pending_slices; pr.rows_total = m->pending_rows; pr.alpha = m->pending_alpha;
        pr.slot_of = m->pending_slot_of; pr.gate_w = m->pending_gate_w;
        m->pending_slices = 0; m->pending_slot_of = nullptr; m->pending_gate_w = nullptr;
        const bool row_kernel = rows <= 512 && m->H <= 1024 * NORM_ROW_MAXCH;
        const bool tile_kernel = sizeof(ActT) == 2 && m->H % 32 == 0 && m->H <= 2048 && g_norm_t16 && !pr.slot_of;   // (the 16-chunk instance would spill)
        if (!row_kernel && !tile_kernel) throw std::runtime_error("norm: no kernel for this pending residual");
    }
    if (rows <= 512 && m->H <= 1024 * NORM_ROW_MAXCH) {
        m->norm_ran = rows_idx ? NVL_NORM_RAN_ROW_IDX : NVL_NORM_RAN_ROW;
        if (consumed) *consumed = rows_idx ? NVL_NORM_RAN_ROW_IDX : NVL_NORM_RAN_ROW;
        hipLaunchKernelGGL((norm_row_kernel<ActT>), dim3(rows), dim3(256), 0, m->stream, x, rows_idx, w, b,
                           m->cfg.norm_eps, (ActT*)y, m->H, pr);
    } else if (sizeof(ActT) == 2 && m->H % 32 == 0 && m->H <= 4096 && g_norm_t16) {   // (wider rows would spill: norm_kernel)
        // 16 rows x H bf16 of LDS (up to 160 KiB); the row sits in registers: instance by chunks per lane
#define NVL_NT16(CH, PEND)                                                                                             \
        do {                                                                                                           \
            NVL_LDS_ATTR((norm_tile16_kernel<CH, PEND>), 160 * 1024);                                                  \
            hipLaunchKernelGGL((norm_tile16_kernel<CH, PEND>), dim3(cdiv(rows, 16)), dim3(1024), (size_t)16 * m->H * 2, m->stream, x, \
                               rows_idx, w, b, m->cfg.norm_eps, (bf16_t*)y, rows, m->H, pr);                            \
        } while (0)
        m->norm_ran = NVL_NORM_RAN_TILE16;
        if (consumed) *consumed = NVL_NORM_RAN_TILE16;
        if (pr.part) NVL_NT16(8, true);        // (H <= 2048: checked above)
        else { if (m->H <= 2048) NVL_NT16(8, false); else NVL_NT16(16, false); }
#undef NVL_NT16
    } else {
        m->norm_ran = NVL_NORM_RAN_WAVE;
        hipLaunchKernelGGL((norm_kernel<ActT>), dim3(cdiv(rows, 4)), dim3(256), 0, m->stream, x, rows_idx, w, b,
                           m->cfg.norm_eps, (ActT*)y, rows, m->H);
    }
}
void norm(nvl_model* m, float* x, const int32_t* rows_idx, const DevTensor& w, const DevTensor& b, void* y, int rows) {
    if (m->f32) launch_norm<float>(m, x, rows_idx, (const float*)w.p, (const float*)b.p, y, rows);
    else launch_norm<bf16_t>(m, x, rows_idx, (const float*)w.p, (const float*)b.p, y, rows);
    NVL_HIP(hipGetLastError());
}

static int g_p2p_oneshot_rows = 64;   // nvl_set_tuning key 23: payloads of up to this many rows take the one-shot all-reduce
static int g_use_graphs = 1;   // nvl_set_tuning key 21: hipGraph replay of decode passes (0 = every launch eager)
static int g_tune_epoch = 0;   // bumped by every nvl_set_tuning: captured graphs bake the tuning in (part of their key)
static int g_attn_nw = 0;      // nvl_set_tuning key 15: waves per decode-attention workgroup (0 = from the context length, 2, 4, 8)
static int g_attn_tq2 = 1;     // nvl_set_tuning key 10: unused since round 2 (the prefill kernel always keeps two sub-tiles per wave)
static int g_attn_kv_nt = 1;   // nvl_set_tuning key 35: non-temporal K/V loads in the decode attention (0 never, 1 automatic, 2 always)
static int g_attn_split = 1;   // nvl_set_tuning key 25: split a decode attention's keys over up to 8 workgroups per (sequence, kv head) (0 = never)
static int g_verify_mq = 1;    // nvl_set_tuning key 38: verify passes (nvl_verify_greedy*) run the multi-position decode attention (0 = rope_kv + the prefill kernel)
// Launch shape of the decode attention for the batch being enqueued (also part of a captured graph's key): waves per
// workgroup | workgroups per (sequence, kv head) << 8.
// Split: a workgroup pulls all K/V of its (sequence, kv head) through ONE CU; with a few sequences and a long context
// (B = 1 at 2048 keys: 8 workgroups x 512 KB) that, not HBM, is the time.  Then the key tiles are dealt over up to 8
// workgroups of 2 waves each; the last of them to finish combines the partial results (attn.h).  Every workgroup of a
// split launch pays a device-scope release fence, so the launch stays within 128 workgroups.  Measured (decode ms/step,
// Llama-3.2-1B, 2048 / 1024 keys): B=1 0.891 -> 0.811 / 0.808 -> 0.780, B=2 0.893 -> 0.834 / 0.869 -> 0.792, B=4 (4
// workgroups per pair) 0.924 -> 0.883 / 0.812 -> 0.817 (hence from 2048 keys on above 16 pairs); B=8 loses either way
// (2 workgroups per pair 0.96 -> 0.99, 8 per pair -> 1.13).
// mq_S > 0: the multi-position kernel with mq_S positions per sequence — its grid, and never a key split.
int decode_attn_cfg(const nvl_model* m, int n_seqs, int mq_S = 0) {
    const int n_kt = m->ctx_hint > 0 ? (m->ctx_hint - 1) / 64 + 1 : 1 << 20;
    const int per_wave = m->hd == 64 ? 2 : 1;
    const int wgs = m->nKV * cdiv(m->group * std::max(mq_S, 1), 16) * n_seqs;
    if (!mq_S && g_attn_split && !g_attn_nw && m->attn_part && m->ctx_hint > 0 && wgs <= ATTN_SPLIT_MAX_PAIRS && n_kt >= 16) {
        const int want = cdiv(n_kt, 2 * per_wave);                       // workgroups of 2 waves that get a full round each
        const int ns = (wgs > 16 && n_kt < 32) ? 1 : std::min(std::min(want, ATTN_SPLIT_MAX), 128 / wgs);
        if (ns >= 2) return 2 | (ns << 8);
    }
    const int cap = wgs >= 512 ? 2 : (wgs >= 320 ? 4 : 8);
    const int nw = n_kt <= 2 * per_wave ? 2 : (n_kt <= 4 * per_wave ? 4 : 8);
    return (g_attn_nw ? g_attn_nw : std::min(nw, cap)) | (1 << 8);
}
int decode_attn_waves(const nvl_model* m, int n_seqs) { return decode_attn_cfg(m, n_seqs); }   // (graph keys: the whole shape)
// The decode launch ladder: 2 / 4 / 8 waves per workgroup, K2 / K4 / K8 the kernel's instantiations for them; `rest` are
// the kernel's arguments after the AttnArgs (the scales of an 8-bit cache).
template <auto K2, auto K4, auto K8, typename... Rest>
static void launch_decode_attn(nvl_model* m, dim3 grid, int nw, int tile_bytes, const AttnArgs& a, Rest... rest) {
#define NVL_DEC_LEAD a.seq_pos, a.blk_table, a.tbl_stride, a.bs_shift, a.Tmax, a.group      /* the preloaded leading arguments (attn.h) */
    if (nw == 2) hipLaunchKernelGGL(K2, grid, dim3(128), 2 * tile_bytes, m->stream, NVL_DEC_LEAD, a, rest...);
    else if (nw == 4) hipLaunchKernelGGL(K4, grid, dim3(256), 4 * tile_bytes, m->stream, NVL_DEC_LEAD, a, rest...);
    else {
        NVL_LDS_ATTR(K8, 8 * tile_bytes);
        hipLaunchKernelGGL(K8, grid, dim3(512), 8 * tile_bytes, m->stream, NVL_DEC_LEAD, a, rest...);
    }
#undef NVL_DEC_LEAD
}
// Every attention launch.  kc / vc: the layer's K / V slabs; kv8: {k_scale, v_scale} of an 8-bit (e4m3fn) cache — the slabs
// are then the layer's code slabs (same element layout, one byte per element; kv8.h) — else NULL.  The 8-bit kernels have
// no fused (RoPE + append) and no stamped form, and their prefill kernel reads the block table from global memory (no
// 128-block limit); grids, wave choices and the K/V load policy are the same.
// mq: the caller is a verify pass (or nvl_op_attention_mq): 2..8 positions per sequence on attn_decode_mq_bf16_kernel.
static bool attention_mq_ok(const nvl_model* m, int max_len) { return !m->f32 && !m->kv8 && max_len >= 2 && max_len <= 8; }
static void attention_launch(nvl_model* m, const Meta& md, int n_seqs, int max_len, const void* kc, const void* vc,
                             double flops, double abytes, bool fused_qkv, const float* kv8, bool mq = false) {
    AttnArgs a{};
    a.q = m->q; a.q_stride = m->nH * m->hd;
    a.out = m->attn_out; a.out_stride = m->nH * m->hd;
    a.kcache = kc; a.vcache = vc;
    a.slot_stride = m->slot_stride; a.Tmax = m->Tmax;
    a.seq_tok_start = md.seq_tok_start; a.seq_len = md.seq_len; a.seq_pos = md.seq_pos; a.blk_table = md.blk_table; a.tbl_stride = m->blocks_per_seq;
    a.bs_shift = (m->Tmax & (m->Tmax - 1)) == 0 ? __builtin_ctz((unsigned)m->Tmax) : -1;
    a.nH = m->nH; a.nKV = m->nKV; a.group = m->group; a.scale = m->attn_scale;
    KScope ks(m, KC_ATTN, flops, KS_ATTN, abytes);
    if (m->f32) {
        // one score per key a row can see: up to blocks_per_seq blocks of Tmax keys (slab mode: the one block)
        const size_t lds = (size_t)m->Tmax * m->blocks_per_seq * 4;
        if (lds > 64 * 1024) NVL_LDS_ATTR(attn_f32_kernel, 160 * 1024 - 64);
        hipLaunchKernelGGL(attn_f32_kernel, dim3(max_len, m->nH, n_seqs), dim3(256), lds, m->stream, a, m->hd);
        m->attn_ran[0] = NVL_ATTN_RAN_F32; m->attn_ran[1] = 4; m->attn_ran[2] = 1;
    } else if (mq && !kv8 && attention_mq_ok(m, max_len)) {
        const int nw = decode_attn_cfg(m, n_seqs, max_len) & 255;
        dim3 grid(m->nKV * cdiv(m->group * max_len, 16), n_seqs, 1);     // (kv head x 16-row query tile, sequence); no key split
        // K/V read once per step by its only workgroup: the one-position launch's policy, with this grid
        a.kv_nt = g_attn_kv_nt == 2 || (g_attn_kv_nt == 1 && cdiv(m->group * max_len, 16) == 1 && (m->nKV * n_seqs >= 160 || n_seqs == 1));
#define NVL_DEC_MQ(HDv, NWv) attn_decode_mq_bf16_kernel<HDv, NWv>
        if (m->hd == 64) launch_decode_attn<NVL_DEC_MQ(64, 2), NVL_DEC_MQ(64, 4), NVL_DEC_MQ(64, 8)>(m, grid, nw, 64 * 64 * 2, a, max_len);
        else launch_decode_attn<NVL_DEC_MQ(128, 2), NVL_DEC_MQ(128, 4), NVL_DEC_MQ(128, 8)>(m, grid, nw, 64 * 128 * 2, a, max_len);
#undef NVL_DEC_MQ
        m->attn_ran[0] = NVL_ATTN_RAN_DECODE_MQ; m->attn_ran[1] = nw; m->attn_ran[2] = 1;
    } else if (max_len == 1) {
        const int cfg = decode_attn_cfg(m, n_seqs), nsplit = cfg >> 8;
        dim3 grid(m->nKV * cdiv(m->group, 16), n_seqs, nsplit);      // (kv head x 16-head query tile, sequence, key split)
        a.part = m->attn_part; a.part_cnt = m->attn_part_cnt;
        // waves per workgroup: each wave takes NT2 key tiles per round trip (2 for hd 64, 1 for hd 128).  Short contexts
        // need fewer than 8 waves (idle waves still cost LDS and a slot in the final merge), and once the grid alone
        // fills the chip (>= 2 workgroups per CU) fewer, longer-running waves stream better than many short ones
        // (profiles/r01g_decode_attention_waves.txt).  ctx_hint = the batch's longest context when the caller knows it.
        const int nw = cfg & 255;
        // non-temporal K/V loads when one workgroup serves a (sequence, kv head)'s whole group (the K/V are then read once) and
        // the launch fills the chip — by batch size on Llama-3.2-1B (8 kv heads, 520 keys; profiles/r03_kv_nontemporal.txt):
        // B = 1 +1.7 %, 2 +-0, 4 -2.3 %, 8 -2.4 %, 16 +-0, 24 +2.7 %, 32 +5 %, 48 +1 %; GPT-2 B = 128 (1536 workgroups) +3.2 %
        a.kv_nt = g_attn_kv_nt == 2 || (g_attn_kv_nt == 1 && cdiv(m->group, 16) == 1 && (m->nKV * n_seqs >= 160 || n_seqs == 1));
        a.stamps = (fused_qkv && m->hd == 64) ? next_stamps(m, KS_ATTN, (int)(grid.x * grid.y * grid.z)) : nullptr;
        if (fused_qkv) {   // RoPE + KV append + attention in one launch, straight from the QKV projection's fp32 output
            a.qkv = m->qkv; a.qkv_stride = m->n_qkv; a.cos_t = m->rope_cos; a.sin_t = m->rope_sin;
        }
#define NVL_DEC(HDv, KERN, ...) launch_decode_attn<KERN(HDv, 2), KERN(HDv, 4), KERN(HDv, 8)>(m, grid, nw, 64 * HDv * 2, a, ##__VA_ARGS__)
#define NVL_DEC_KV8(HDv, NWv) attn_decode_kv8_kernel<HDv, NWv>
#define NVL_DEC_PLAIN(HDv, NWv) attn_decode_bf16_kernel<HDv, NWv, false>
#define NVL_DEC_FUSED(HDv, NWv) attn_decode_bf16_kernel<HDv, NWv, true>
#define NVL_DEC_STAMP(HDv, NWv) attn_decode_bf16_kernel<HDv, NWv, true, true>     /* diagnostic: the in-kernel stamps compiled in */
        if (kv8) { if (m->hd == 64) NVL_DEC(64, NVL_DEC_KV8, kv8[0], kv8[1]); else NVL_DEC(128, NVL_DEC_KV8, kv8[0], kv8[1]); }
        else if (a.stamps) NVL_DEC(64, NVL_DEC_STAMP);
        else if (fused_qkv) { if (m->hd == 64) NVL_DEC(64, NVL_DEC_FUSED); else NVL_DEC(128, NVL_DEC_FUSED); }
        else { if (m->hd == 64) NVL_DEC(64, NVL_DEC_PLAIN); else NVL_DEC(128, NVL_DEC_PLAIN); }
        m->attn_ran[0] = kv8 ? NVL_ATTN_RAN_DECODE_KV8 : (a.stamps ? NVL_ATTN_RAN_DECODE_STAMPED : (fused_qkv ? NVL_ATTN_RAN_DECODE_FUSED : NVL_ATTN_RAN_DECODE));
        m->attn_ran[1] = nw; m->attn_ran[2] = nsplit;
#undef NVL_DEC_STAMP
#undef NVL_DEC_FUSED
#undef NVL_DEC_PLAIN
#undef NVL_DEC_KV8
#undef NVL_DEC
    } else {
        // 256 query rows (position x head-in-group, position-major) per workgroup of 8 waves
        const int64_t qrows = (int64_t)max_len * m->group;
        dim3 grid(m->nKV, n_seqs, cdiv(qrows, 256));      // (kv head fastest, query tile slowest: attn.h)
        m->attn_ran[0] = kv8 ? NVL_ATTN_RAN_PREFILL_KV8 : NVL_ATTN_RAN_PREFILL; m->attn_ran[1] = 8; m->attn_ran[2] = 1;
        if (kv8) {     // K/V tiles through registers into one bf16 image pair
            if (m->hd == 64) {
                hipLaunchKernelGGL((attn_prefill_kv8_kernel<64>), grid, dim3(512), attn_prefill_kv8_lds_bytes<64>(), m->stream, a, kv8[0], kv8[1]);
            } else {
                NVL_LDS_ATTR(attn_prefill_kv8_kernel<128>, attn_prefill_kv8_lds_bytes<128>());
                hipLaunchKernelGGL((attn_prefill_kv8_kernel<128>), grid, dim3(512), attn_prefill_kv8_lds_bytes<128>(), m->stream, a, kv8[0], kv8[1]);
            }
        } else {       // K/V tiles by LDS-DMA; the kernel keeps the sequence's block table in LDS
            if (m->blocks_per_seq > 128) throw std::runtime_error("attention: more than 128 KV blocks per sequence");
            if (m->hd == 64) {
                hipLaunchKernelGGL((attn_prefill_bf16_kernel<64>), grid, dim3(512), attn_prefill_lds_bytes<64>(), m->stream, a);
            } else {
                NVL_LDS_ATTR(attn_prefill_bf16_kernel<128>, attn_prefill_lds_bytes<128>());
                hipLaunchKernelGGL((attn_prefill_bf16_kernel<128>), grid, dim3(512), attn_prefill_lds_bytes<128>(), m->stream, a);
            }
        }
    }
    NVL_HIP(hipGetLastError());
}
// algorithmic bytes: every cached key/value of the batch once + Q in + O out (+ the fp32 QKV row of a fused decode step)
void attention(nvl_model* m, int li, const Meta& md, int n_seqs, int max_len, double flops, bool fused_qkv = false, bool mq = false) {
    attention_launch(m, md, n_seqs, max_len, (char*)m->kcache + (size_t)li * m->layer_stride * m->wsize,
                     (char*)m->vcache + (size_t)li * m->layer_stride * m->wsize, flops, m->kv_tok * 2.0 * m->nKV * m->hd * (double)m->wsize, fused_qkv, nullptr, mq);
}
// attention over an 8-bit cache: kc / vc the layer's code slabs, k_scale / v_scale the layer's scales.  bf16 only.
void attention_kv8(nvl_model* m, const Meta& md, int n_seqs, int max_len, const void* kc, const void* vc, float ksc, float vsc) {
    if (m->f32) throw std::runtime_error("attention_kv8: the 8-bit KV cache is bf16-only");
    const float scales[2] = {ksc, vsc};
    attention_launch(m, md, n_seqs, max_len, kc, vc, 0.0, m->kv_tok * 2.0 * m->nKV * m->hd, false, scales);
}

void rope_kv(nvl_model* m, int li, const Meta& md, int M) {
    KScope ks(m, KC_OTHER, 0, KS_ROPE, (double)M * m->n_qkv * (4.0 + (double)m->wsize));
    dim3 grid(M, m->nH + 2 * m->nKV);
    const int thr = m->hd / 2;
    void* kc = (char*)m->kcache + (size_t)li * m->layer_stride * m->kv_esize;
    void* vc = (char*)m->vcache + (size_t)li * m->layer_stride * m->kv_esize;
    if (m->kv8)
        hipLaunchKernelGGL(rope_kv8_kernel, grid, dim3(thr), 0, m->stream, m->qkv, m->n_qkv,
                           md.tok_pos, md.tok_tbl, md.blk_table, m->rope_cos, m->rope_sin, (bf16_t*)m->q, m->nH * m->hd,
                           (uint8_t*)kc, (uint8_t*)vc, m->slot_stride, m->Tmax, m->nH, m->nKV, m->hd, m->k_scale[li], m->v_scale[li]);
    else if (m->f32)
        hipLaunchKernelGGL((rope_kv_kernel<float, false>), grid, dim3(thr), 0, m->stream, m->qkv, m->n_qkv,
                           md.tok_pos, md.tok_tbl, md.blk_table, m->rope_cos, m->rope_sin, (float*)m->q, m->nH * m->hd,
                           (float*)kc, (float*)vc, m->slot_stride, m->Tmax, m->nH, m->nKV, m->hd);
    else
        hipLaunchKernelGGL((rope_kv_kernel<bf16_t, false>), grid, dim3(thr), 0, m->stream, m->qkv, m->n_qkv,
                           md.tok_pos, md.tok_tbl, md.blk_table, m->rope_cos, m->rope_sin, (bf16_t*)m->q, m->nH * m->hd,
                           (bf16_t*)kc, (bf16_t*)vc, m->slot_stride, m->Tmax, m->nH, m->nKV, m->hd);
    NVL_HIP(hipGetLastError());
}

void launch_argmax(hipStream_t st, float* logits, int ld, int V, int rows, float scaling, float* pval, int32_t* pidx,
                   int32_t* out) {
    const int chunks = cdiv(V, ARGMAX_CHUNK);
    hipLaunchKernelGGL(argmax_partial_kernel, dim3(chunks, rows), dim3(256), 0, st, logits, ld, V, scaling, pval, pidx);
    if (out) hipLaunchKernelGGL(argmax_final_kernel, dim3(rows), dim3(64), 0, st, pval, pidx, chunks, out);
}

GemmArgs mk(const void* A, int lda, const void* W, void* C, int ldc, const float* bias, float alpha, int M, int N, int K) {
    GemmArgs a{};
    a.A = A; a.lda = lda; a.a_rows = nullptr; a.W = W; a.C = C; a.ldc = ldc; a.bias = bias; a.alpha = alpha;
    a.M = M; a.N = N; a.K = K; a.seg = nullptr; a.c_row0 = 0;
    a.qkv = QkvEpi{};
    a.tile_map = nullptr; a.n_mtiles = nullptr; a.w_expert_stride = 0;
    a.sk_part = nullptr; a.sk_slices = 1; a.m_split = 0; a.rs_half = 0; a.grid_y = 1; a.nrm_w = nullptr; a.nrm_xn = nullptr; a.rs_out = nullptr; a.rs_in = nullptr; a.rs_tiles = 0; a.rs_inv_h = 0.f; a.rs_eps = 0.f;
    return a;
}

// ---- tensor-parallel all-reduce (sum) of a row-parallel projection's fp32 partial -----------------------
// Real runs: one process per GPU, RCCL over xGMI (nvl_tp_init).  Tests on one GPU: the shard models of a
// process form a local group (nvl_tp_attach_local) and are driven from one host thread each; the last
// thread to arrive sums every member's buffer on the device and hands the result back to all of them.
void tp_allreduce(nvl_model* m, float* buf, int64_t count) {
    KScope ks(m, KC_OTHER, 0, KS_ALLREDUCE, (double)count * 4.0);
    if (m->tp_comm) {
        const ncclResult_t rc = ncclAllReduce(buf, buf, (size_t)count, ncclFloat, ncclSum, (ncclComm_t)m->tp_comm, m->stream);
        if (rc != ncclSuccess) throw std::runtime_error(std::string("ncclAllReduce: ") + ncclGetErrorString(rc));
        return;
    }
    nvl_local_group* g = m->tp_local;
    if (!g) throw std::runtime_error("tp_size > 1 but no communicator: call nvl_tp_init (RCCL) or nvl_tp_attach_local first");
    NVL_HIP(hipStreamSynchronize(m->stream));                 // this rank's partial is complete
    std::unique_lock<std::mutex> lk(g->mu);
    if (g->aborted) throw std::runtime_error("tp local group: another member failed (group aborted)");
    if (count > g->scratch_floats) throw std::runtime_error("tp local group: scratch too small");
    g->bufs[m->tp_rank] = buf;
    const uint64_t my_gen = g->gen;
    if (++g->arrived == g->n) {
        PtrList8 pl{};
        for (int r = 0; r < g->n; r++) pl.p[r] = g->bufs[r];
        hipLaunchKernelGGL(sum_bufs_kernel, dim3(cdiv(count, 1024)), dim3(256), 0, m->stream, g->scratch, pl, g->n, count);
        for (int r = 0; r < g->n; r++)
            NVL_HIP(hipMemcpyAsync(g->bufs[r], g->scratch, (size_t)count * 4, hipMemcpyDeviceToDevice, m->stream));
        NVL_HIP(hipStreamSynchronize(m->stream));
        g->arrived = 0;
        g->gen++;
        g->cv.notify_all();
    } else {
        // a peer that fails sets `aborted` (note_failure); the timeout covers a peer that never calls at all
        const bool ok = g->cv.wait_for(lk, std::chrono::seconds(120), [&] { return g->gen != my_gen || g->aborted; });
        if (!ok || g->gen == my_gen) {
            g->aborted = true;
            g->cv.notify_all();
            throw std::runtime_error(ok ? "tp local group: another member failed (group aborted)"
                                        : "tp local group: timed out waiting for the other members");
        }
    }
}

static int g_half_tiles = 1;   // nvl_set_tuning key 27: deferred-norm residual projections of <= 16 rows on 8-row half tiles (gemm.h HALF)
// (producer and consumer agree through M alone: every projection of a pass has the same row count)
// (only while the 16-row tiles leave CUs idle: at H = 4096 — 256 tiles — the halves doubled the x^2 partials every consumer
// sums and the workgroups that each fetch the activations: Llama-3-8B B = 16 FFN-down 23.7 -> 34.2 us, O 9.3 -> 12.4 us)
static int g_defer_norm = 1;   // nvl_set_tuning key 3: deferred RMSNorm between O-proj and FFN-up in decode (0 = off)
// (keys 3 = 2 / 3: the producer runs without m_split, and only the m_split form has half tiles — it writes H / 16 partials
//  per row, so the consumers must not look for H / 8: they summed the next rows' partials into rows 1..15)
bool defer_half(const nvl_model* m, int M) { return g_half_tiles && g_defer_norm < 2 && M <= 16 && m->H % 128 == 0 && m->H / 16 < 256; }
// after a forward's stream sync: did a P2P wait give up?  (a peer died or never called: the residual stream is garbage)
void p2p_check(nvl_model* m) {
    if (!m->p2p_ready) return;
    int err = 0;
    NVL_HIP(hipMemcpy(&err, m->p2p_buf + P2P_OFF_ERR, 4, hipMemcpyDeviceToHost));
    if (err) throw std::runtime_error("tensor-parallel all-reduce: timed out waiting for a peer rank (nvl_tp_p2p_rearm on every rank clears the group)");
}
static int g_p2p_spin_ms = 30000;     // nvl_set_tuning key 29: how long a rank waits for its peers inside an all-reduce before it gives up
// x += alpha * sum over the tensor-parallel ranks of `part` [M][N], by direct peer stores over the xGMI mesh (tp_p2p.h): ONE
// launch.  nrm_w != NULL (decode, RMSNorm + SwiGLU): the same launch emits the deferred-RMSNorm operand of the next projection.
void tp_p2p_allreduce_resid(nvl_model* m, const float* part, int M, int N, float alpha, const float* nrm_w = nullptr) {
    const int64_t count = (int64_t)M * N;
    if (count % 8 || N % 16) throw std::runtime_error("tp p2p: the row length must be a multiple of 16");
    P2PArgs a{};
    a.T = m->tp; a.rank = m->tp_rank;
    a.count = count; a.part = part; a.x = m->x; a.alpha = alpha;
    for (int r = 0; r < m->tp; r++) a.peer[r] = m->p2p_peer[r];
    a.off_in1 = m->p2p_off_in1; a.off_in2 = m->p2p_off_in2; a.off_res = m->p2p_off_res;
    a.in1_stride = m->p2p_in1_stride; a.in2_stride = m->p2p_in2_stride; a.res_stride = m->p2p_res_stride;
    a.spin_limit = (int)std::min<int64_t>((int64_t)g_p2p_spin_ms * 1000, 2000000000);      // x ~1 us of s_sleep per poll
    a.oneshot = (M <= g_p2p_oneshot_rows && M <= P2P_ONESHOT_CAP_ROWS) ? 1 : 0;
    if (!a.oneshot) a.chunk = round_up(cdiv(count, a.T), 8);
    if (nrm_w) {
        if (!a.oneshot) throw std::runtime_error("tp p2p: the fused norm rides on the one-shot form");
        a.H = N; a.nrm_w = nrm_w; a.nrm_xn = (bf16_t*)m->xn; a.rs_out = m->rs_part; a.rs_cols = defer_half(m, M) ? 8 : 16;
    }
    const int nwg = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(count, 256 * 8), 512));    // all resident: the kernel spins
    KScope ks(m, KC_OTHER, 0, KS_ALLREDUCE, (double)count * (m->f32 ? 4.0 : 2.0) * 2.0);
    if (m->f32) hipLaunchKernelGGL((p2p_allreduce_kernel<float, false>), dim3(nwg), dim3(256), 0, m->stream, a);
    else if (nrm_w) hipLaunchKernelGGL((p2p_allreduce_kernel<bf16_t, true>), dim3(nwg), dim3(256), 0, m->stream, a);
    else hipLaunchKernelGGL((p2p_allreduce_kernel<bf16_t, false>), dim3(nwg), dim3(256), 0, m->stream, a);
    NVL_HIP(hipGetLastError());
}

// Residual projection (O projection / W2): x += alpha * (A·W^T + bias)   (generic_model.go:320-326,383-389).
// Prefill and the fp32 mode fuse the add into the GEMM epilogue.  Decode-sized batches split K over
// `slices` workgroups per column block so that all 256 CUs stream weights (a 2048-column projection has
// only 128 column blocks), and leave the add to the norm kernel that always follows (PendingResid).
static int g_qkv_store_max_m = 256;   // nvl_set_tuning key 18: largest prefill batch whose QKV projection runs as decode-form groups + rope_kv_kernel
static int g_moe_dense = 1;    // nvl_set_tuning key 22: decode MoE as two dense-masked projections (gemm.h moe_gate); 0 = sort + grouped GEMMs
static int g_moe_deep = 1;     // nvl_set_tuning key 19: four-stage grouped GEMM for decode-sized MoE batches (0 = two stages)
static int g_moe_bm = 0;       // nvl_set_tuning key 17: prefill MoE grouped GEMMs: 0 = 256-row tiles on the ping-pong kernel, 128 / 256 = the lock-step tile kernels
static int g_moe_gather = 1;   // nvl_set_tuning key 16: prefill MoE gathers the token rows into expert order before the grouped GEMM (0 = per-lane gather inside it)
static int g_moe_defer_down = 0;    // nvl_set_tuning key 33: MoE decode: the down projection carries the next norm (deferred RMSNorm producer: all of
                                    // K in one workgroup, one launch less per layer) instead of K slices + a norm launch.  Off: with 128 workgroups of
                                    // 16 waves each wave walks 8 blocks (two experts) instead of 4 — Granite-1B B=8 down projection 8.9 -> 14.5 us, more
                                    // than the norm launch it saves: 6.48 K -> 6.26 K decode tok/s (profiles/r03_moe_decode_experiments.txt)
static int g_moe_fused_route = 1;   // nvl_set_tuning key 31: MoE decode routing (router GEMM + softmax / top-k / gate matrix) as one launch (0 = two)
static int g_moe_small = 1;    // nvl_set_tuning key 8: fused MoE planning launch + combine folded into the next norm (0 = off)
static int g_mamba_ssd = 1;    // nvl_set_tuning key 30: chunked (SSD) Mamba2 scan on MFMA for prefill-sized bf16 calls (0 = the sequential scan,
                               // 2 = chunk after chunk only, never the chunk-parallel three-launch form)
static int g_mamba_conv_step = 1;   // nvl_set_tuning key 39: decode passes of a carried model (NVL_MAMBA_CONV_CARRIED) run mamba_conv_step_kernel
                                    // (0 = mamba_conv_kernel + mamba_tail_kernel)
static int g_decode_seam = 1;  // nvl_set_tuning key 7: decode_seam_kernel in nvl_decode_greedy (0 = separate kernels)
static int g_sk_slices = 0;    // tuning override (nvl_set_tuning key 1): 0 automatic, 1 = never split
// consumer side of the deferred RMSNorm: the projection reads xn_raw and scales its accumulators (gemm.h)
void set_deferred_in(nvl_model* m, GemmArgs& a) {
    a.rs_in = m->rs_part; a.rs_tiles = defer_half(m, a.M) ? m->H / 8 : m->H / 16; a.rs_inv_h = 1.0f / (float)m->H; a.rs_eps = m->cfg.norm_eps;
}
void resid_gemm(nvl_model* m, const void* A, int lda, const void* W, const float* bias, float alpha, int M, int N, int K,
                const float* defer_norm_w = nullptr) {
    if (m->tp > 1 || m->tp_force) {
        // row-parallel projection: this rank holds a K slice -> fp32 partial [M][N] (the bias lives on rank 0 only),
        // all-reduce over the tensor-parallel group, then the residual add (folded into the next norm for decode)
        gemm(m, EPI_STORE, true, mk(A, lda, W, m->tp_part, N, bias, 1.f, M, N, K));
        if (m->p2p_ready) { tp_p2p_allreduce_resid(m, m->tp_part, M, N, alpha, defer_norm_w); return; }     // sum + residual add (+ the deferred norm) in one go
        if (defer_norm_w) throw std::runtime_error("resid_gemm: the deferred norm of a tensor-parallel projection needs the P2P all-reduce");
        tp_allreduce(m, m->tp_part, (int64_t)M * N);
        if (!m->f32 && M <= 64 && !m->keep_hidden && m->pending_slices == 0) {
            m->pending_part = m->tp_part; m->pending_slices = 1; m->pending_rows = M; m->pending_alpha = alpha;
        } else {
            KScope ks(m, KC_OTHER);
            hipLaunchKernelGGL(axpy_rows_kernel, dim3(cdiv((int64_t)M * N / 4, 256)), dim3(256), 0, m->stream, m->x,
                               m->tp_part, (const float*)nullptr, alpha, (int64_t)M, N);
            NVL_HIP(hipGetLastError());
        }
        return;
    }
    GemmArgs a = mk(A, lda, W, m->x, N, bias, alpha, M, N, K);
    // what this projection ran, for nvl_op_dense_stages (nvl_model::dense_ran): the O projection's record, or FFN-down's
    const int which = m->site == KS_FFN_DOWN ? 1 : 0;
    int* ran = m->dense_ran + 4 * which;
    t_skinny_form = 0; t_skinny_half = 0;
    auto record = [&](int producer, int slices) {
        ran[NVL_DENSE_RAN_PRODUCER] = producer; ran[NVL_DENSE_RAN_HALF] = t_skinny_half; ran[NVL_DENSE_RAN_FORM] = t_skinny_form; ran[NVL_DENSE_RAN_SLICES] = slices;
    };
    if (defer_norm_w) {     // deferred RMSNorm: x complete in this launch (no K split over workgroups) + xn_raw + x^2 partials
        a.nrm_w = defer_norm_w; a.nrm_xn = (bf16_t*)m->xn; a.rs_out = m->rs_part; a.m_split = g_defer_norm >= 2 ? 0 : 1;
        a.rs_half = a.m_split && N == m->H && defer_half(m, M) ? 1 : 0;
        gemm(m, EPI_RESID, true, a);
        record(1, 0);
        return;
    }
    int slices = 1;
    if (!m->f32 && M <= 64 && !m->keep_hidden && m->sk_part && m->pending_slices == 0 && N % 16 == 0) {
        const int nblocks = N / 16;
        if (g_sk_slices > 0) slices = g_sk_slices;
        else while (slices < m->sk_max_slices && nblocks * slices < 256 && (K >> 5) / (slices * 2) >= 8) slices *= 2;
    }
    // 65..512 rows (a short prompt, a few hundred decode rows that do not take the decode form): N / 128 x M / 128 tiles of the
    // lock-step kernel are a handful of workgroups (FFN-down of Llama-1B at 512 rows: 64), and the 64-row groups of the decode
    // form pull every activation row through every CU (1.3 GB of ingest for that projection: 85 us).  K split over
    // gridDim.y workgroups per tile instead, the slices summed by the norm that follows (which must be the row kernel).
    const bool norm_ok = (M <= 512 && m->H <= 1024 * NORM_ROW_MAXCH) || (m->H % 32 == 0 && m->H <= 2048 && g_norm_t16);   // launch_norm
    if (g_sk_tile && !m->f32 && M > 64 && M <= m->sk_rows && !m->keep_hidden && m->sk_part && m->pending_slices == 0 &&
        N % 128 == 0 && K % 64 == 0 && norm_ok && N == m->H && g_force_tile == 0 && m->n_mamba == 0) {
        const int tiles = cdiv(M, 128) * (N / 128);
        while (slices < SK_TILE_MAX_SLICES && tiles * slices < 512 && K / (slices * 2) >= 512) slices *= 2;
        // (fewer than 64 workgroups even so — GPT-2's 768 columns below 512 rows —: the decode form's 64-row groups stream
        // better, profiles/r03_gpt2_large_decode_batches.txt: B = 128 147.5 K -> 159.0 K, B = 256 224.8 K -> 237.2 K tok/s)
        if (tiles * slices < 64) slices = 1;
    }
    if (slices > 1) {
        a.sk_part = m->sk_part; a.sk_slices = slices;
        gemm(m, EPI_RESID, true, a);
        m->pending_part = m->sk_part; m->pending_slices = slices; m->pending_rows = M; m->pending_alpha = alpha;
        m->pending_from = which;
        record(0, slices);
    } else {
        gemm(m, EPI_RESID, true, a);
        record(0, 0);
    }
}

// FeedForward.Forward (transformer.go:40-96) up to (not including) the W2 projection:
// leaves act(x·W1) in m->hbuf [M][F]
void ffn_up(nvl_model* m, const LayerW& l, int M, bool deferred_norm = false) {
    const bool swiglu = m->cfg.activation_type == NVL_ACT_SWIGLU;
    const float* b1 = (const float*)l.t[NVL_T_B1].p;
    if (swiglu) {
        if (m->f32) {
            m->site = KS_FFN_UP;
            gemm(m, EPI_STORE, true, mk(m->xn, m->H, l.w1, m->h2, 2 * m->F, nullptr, 1.f, M, 2 * m->F, m->H));
            KScope ks(m, KC_OTHER);
            const int64_t n = (int64_t)M * m->F;
            hipLaunchKernelGGL((swiglu_kernel<float>), dim3(cdiv(n, 256)), dim3(256), 0, m->stream, m->h2,
                               (float*)m->hbuf, (int64_t)M, m->F);
            NVL_HIP(hipGetLastError());
        } else {
            GemmArgs a = mk(m->xn, m->H, l.w1, m->hbuf, m->F, nullptr, 1.f, M, 2 * m->F, m->H);
            if (deferred_norm) set_deferred_in(m, a);
            m->site = KS_FFN_UP;
            gemm(m, EPI_SWIGLU, false, a);
        }
    } else {
        m->site = KS_FFN_UP;
        gemm(m, EPI_GELU, false, mk(m->xn, m->H, l.w1, m->hbuf, m->F, b1, 1.f, M, m->F, m->H));
    }
}

// MoELayer.Forward (moe.go:43-128): router GEMM -> route (softmax, top-k, renormalise) -> counting sort of
// the (token, rank) pairs by expert -> ONE grouped gate/up GEMM and ONE grouped down GEMM over all experts
// (m-tiles mapped to (expert, row segment) by a device table; token rows gathered by per-lane source address)
// -> combine in rank order into x (with the residual multiplier).  The fp32 parity mode launches per expert.
// the op entry points look at the buffers between the launches of layer_tail and of moe (a model passes no hook)
enum { TAIL_X1 = 0, TAIL_OPERAND, TAIL_H, TAIL_X2 };     // after the O projection | FFN-up's operand in place | after FFN-up | after FFN-down
struct StageHook { void (*fn)(void* ctx, int stage); void* ctx; };

// can this call take the decode ("dense-masked") MoE form?  (also decides whether the O projection may carry the FFN norm)
// (the down form's per-wave live-block mask is 32 bits wide: an expert of more than 32 blocks of U k-steps — U = 4 up to 32
// rows, 2 above — would lose the blocks past 32, so such widths take the grouped form: I > 4096, or I > 2048 above 32 rows)
bool moe_dense_ok(const nvl_model* m, const LayerW& l, int M) {
    // (the last condition: an expert's k-steps in blocks of U fit the down form's 32-bit live-block mask; U = 4 up to 32 rows,
    //  then 2, and 1 for INT4 experts, whose 64-row kernels run one k-step per register set: gemm.h launch_skinny_wf)
    const int u_down = M <= 32 ? 4 : (wf_base(m->ef) == WF_INT4 ? 1 : 2);
    return !m->f32 && M <= 64 && g_moe_dense && l.moe_out_cat && m->moe_part && !m->keep_hidden && m->H % 4 == 0 &&
           m->H <= 1024 * NORM_ROW_MAXCH && g_force_tile == 0 && (m->F >> 5) / u_down <= 32;
}
// quantized experts, the grouped forms: W~ of the layer's down matrices from the stored [H_pad][E*I] codes into dst, [E][H][I]
// fragment-major per expert (ops_impl.h reads the experts back through it too)
void dequant_down_experts(nvl_model* m, const LayerW& l, int H, int I, int E, bf16_t* dst) {
    wf_dequant_down(m->stream, m->ef, l.moe_out_q, l.qs_moe_out, H, I, E, dst);
    NVL_HIP(hipGetLastError());
}
// deferred_norm: m->xn holds xn_raw = bf16(x * w_norm) and m->rs_part the x^2 partials (the O projection carried the FFN
// norm): the router and the expert-up projection scale their accumulators by rstd[m] instead of reading a normed operand
// next_norm_w (decode, dense-masked form only): the down projection carries the NEXT norm (the following layer's attention
// norm / the final norm) as the deferred-RMSNorm producer — all of K in one workgroup per (weight half-tile, row tile), no
// slices left for a norm launch to sum; returns true when it did (m->xn / m->rs_part then hold that norm's operand).
// hook (the op entry points only): called with TAIL_H between the dense-masked form's two projections, moe_hall written
bool moe(nvl_model* m, const LayerW& l, int M, bool deferred_norm = false, const float* next_norm_w = nullptr, const StageHook* hook = nullptr) {
    const nvl_model_config& c = m->cfg;
    const int E = c.num_experts, k = c.num_experts_per_tok, I = m->F, H = m->H;
    const int pairs = M * k;
    // algorithmic weight bytes of the expert GEMMs: the experts a batch of `pairs` (token, rank) pairs can touch, once
    const double e_touch = (double)std::min(E, pairs);
    const double eb = m->ef != WF_BF16 ? wf_stored_bytes(m->ef) : (double)m->wsize;     // bytes per expert weight
    m->site = KS_MOE_ROUTER;
    const bool dense = moe_dense_ok(m, l, M) && m->pending_slices == 0;
    // decode: router logits, softmax, top-k and the dense gate matrix in one launch (gemm.h moe_router_gate_kernel)
    const bool fused_route = dense && g_moe_fused_route && E <= 64 && H % 32 == 0;
    m->moe_form = dense ? (fused_route ? NVL_MOE_FORM_DENSE_FUSED : NVL_MOE_FORM_DENSE) : 0;      // (the sorted forms: below)
    {
        GemmArgs ar = mk(m->xn, H, l.t[NVL_T_ROUTER].p, m->router_logits, 128, nullptr, 1.f, M, E, H);
        if (deferred_norm) set_deferred_in(m, ar);
        if (fused_route) {
            KScope ks(m, KC_GEMM, 2.0 * (double)M * E * H, -1, ((double)E * H + (double)M * H) * (double)m->wsize + (double)M * E * 8.0);
            hipLaunchKernelGGL(moe_router_gate_kernel, dim3(cdiv(M, 16)), dim3(1024), 0, m->stream, ar, k, m->moe_gate, m->router_logits, 128);
            NVL_HIP(hipGetLastError());
        } else {
            gemm(m, EPI_STORE, true, ar);
        }
    }
    // Decode: the dense-masked form (gemm.h GemmArgs::moe_gate).  Routing weights as a dense [M][E] matrix, then all experts
    // as ONE weight-streaming projection each way; untouched experts are skipped inside the kernels, the gate weight in the up
    // epilogue turns the down projection's K reduction into the weighted combine, its K slices are summed by the next norm.
    if (deferred_norm && !dense)
        throw std::runtime_error("moe: a deferred FFN norm needs the dense-masked decode form");
    if (dense) {
        if (!fused_route) {
            KScope ks(m, KC_OTHER, 0, KS_MOE_PLAN, (double)M * (128 + E) * 4.0);
            hipLaunchKernelGGL(moe_gate_kernel, dim3(cdiv(M, 4)), dim3(256), 0, m->stream, m->router_logits, 128, M, E, k, m->moe_gate);
            NVL_HIP(hipGetLastError());
        }
        GemmArgs a = mk(m->xn, H, l.moe_in, m->moe_hall, E * I, nullptr, 1.f, M, E * 2 * I, H);
        a.moe_gate = m->moe_gate; a.moe_E = E; a.moe_I = I;
        if (deferred_norm) set_deferred_in(m, a);
        m->site = KS_MOE_UP; m->site_bytes = e_touch * 2 * I * H * eb + ((double)M * H + e_touch * M * I) * (double)m->wsize;
        gemm(m, EPI_SWIGLU, false, a, 2.0 * pairs * 2 * I * H);
        if (hook) hook->fn(hook->ctx, TAIL_H);
        const int nks = (E * I) >> 5, spe = I >> 5;
        // (8-bit experts: no producer form — a wave's live blocks cross experts, the scale would change with the block;
        //  MXFP4 and INT4 experts: no instance of it either — key 33 is off by default and was measured slower)
        if (next_norm_w && g_moe_defer_down && m->ef == WF_BF16 && nks % 64 == 0 && spe % 4 == 0 && nks / 16 <= 4 * spe && nks / 64 <= 32) {
            // (the launcher's conditions: 16 waves, whole blocks of 4 k-steps inside one expert, <= 4 experts per wave)
            GemmArgs d = mk(m->moe_hall, E * I, l.moe_out_cat, m->x, H, nullptr, m->resid_alpha, M, H, E * I);
            d.moe_gate = m->moe_gate; d.moe_E = E; d.moe_I = I;
            d.nrm_w = next_norm_w; d.nrm_xn = (bf16_t*)m->xn; d.rs_out = m->rs_part; d.m_split = 1;
            d.rs_half = defer_half(m, M) ? 1 : 0;
            m->site = KS_MOE_DOWN; m->site_bytes = (e_touch * H * I + e_touch * M * I) * (double)m->wsize + (double)M * H * 10.0;
            gemm(m, EPI_RESID, true, d, 2.0 * pairs * H * I);
            return true;
        }
        // One slice (a prime E above MOE_DOWN_SLICES: 5, 7, 11, 13) is no K split: the kernel's single workgroup per column
        // tile adds alpha x its sum into x itself and writes no partial, so nothing is left pending.  (This branch used to
        // announce one pending slice all the same: the next norm then added the unwritten moe_part rows on top.)
        const int nsl = moe_down_slices(E);
        GemmArgs d = mk(m->moe_hall, E * I, l.moe_out_cat, m->x, H, nullptr, nsl > 1 ? 1.f : m->resid_alpha, M, H, E * I);
        d.moe_gate = m->moe_gate; d.moe_E = E; d.moe_I = I;
        if (nsl > 1) { d.sk_part = m->moe_part; d.sk_slices = nsl; }
        m->site = KS_MOE_DOWN; m->site_bytes = e_touch * H * I * eb + e_touch * M * I * (double)m->wsize + (double)nsl * M * H * 4.0;
        gemm(m, EPI_RESID, true, d, 2.0 * pairs * H * I);
        if (nsl > 1) { m->pending_part = m->moe_part; m->pending_slices = nsl; m->pending_rows = M; m->pending_alpha = m->resid_alpha; }
        return false;
    }
    // decode-sized batches: one planning launch, and the weighted combine rides on the norm that follows
    const bool small = !m->f32 && M <= 64 && pairs <= MOE_PLAN_MAX_PAIRS && E <= MOE_PLAN_MAX_E && g_moe_small;
    // m-tile height of the grouped GEMMs: 128 rows; the 256x128 three-stage instance stays a tuning option (Granite-1B,
    // 4096 rows per expert: 441 K vs 450 K prefill tok/s)
    // prefill default: 256-row m-tiles on the ping-pong kernel (needs the rows copied into expert order and K >= 160)
    const bool pp = !m->f32 && !small && g_moe_bm == 0 && m->moe_xg && g_moe_gather && H >= 160 && I >= 160 && (2 * I) % 256 == 0 && H % 256 == 0;
    const int BM = pp ? 256 : ((!m->f32 && !small && g_moe_bm == 256) ? 256 : 128);
    m->moe_form = small ? NVL_MOE_FORM_PLAN : NVL_MOE_FORM_GROUPED;
    if (small) {
        KScope ks(m, KC_OTHER, 0, KS_MOE_PLAN);
        hipLaunchKernelGGL(moe_plan_kernel, dim3(1), dim3(M <= 4 ? 256 : (M <= 8 ? 512 : 1024)), 0, m->stream, m->router_logits, 128, M, E, k, 128, m->expert_ids,
                           m->expert_w, m->seg_start, m->moe_tile_map, m->moe_n_mtiles, m->perm_token, m->slot_of);
        NVL_HIP(hipGetLastError());
    } else {
        KScope ks(m, KC_OTHER, 0, KS_MOE_PLAN);
        NVL_HIP(hipMemsetAsync(m->moe_counts, 0, (size_t)E * 4, m->stream));
        hipLaunchKernelGGL(moe_route_kernel, dim3(cdiv(M, 4)), dim3(256), 0, m->stream, m->router_logits, 128, M, E, k,
                           m->expert_ids, m->expert_w);
        hipLaunchKernelGGL(moe_hist_kernel, dim3(cdiv(pairs, MOE_PAIRS_PER_WG)), dim3(256), 0, m->stream, m->expert_ids, pairs, m->moe_counts);
        hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(64), 0, m->stream, m->moe_counts, E, BM, m->seg_start, m->moe_cursor,
                           m->moe_tile_map, m->moe_n_mtiles);
        hipLaunchKernelGGL(moe_scatter_kernel, dim3(cdiv(pairs, MOE_PAIRS_PER_WG)), dim3(256), 0, m->stream, m->expert_ids, pairs, k,
                           m->moe_cursor, m->perm_token, m->slot_of);
        NVL_HIP(hipGetLastError());
    }
    const int max_mtiles = cdiv(pairs, BM) + E;      // every expert may end on a partial tile
    if (m->f32) {
        for (int e = 0; e < E; e++) {   // grid bounded by M: a token picks an expert at most once; surplus blocks exit
            const char* win = (const char*)l.moe_in + (size_t)e * 2 * I * H * m->wsize;
            GemmArgs a = mk(m->xn, H, win, m->h2, 2 * I, nullptr, 1.f, M, 2 * I, H);
            a.a_rows = m->perm_token; a.seg = m->seg_start + e;
            gemm(m, EPI_STORE, true, a);
        }
        {
            KScope ks(m, KC_OTHER);
            const int64_t n = (int64_t)pairs * I;
            hipLaunchKernelGGL((swiglu_kernel<float>), dim3(cdiv(n, 256)), dim3(256), 0, m->stream, m->h2, (float*)m->hbuf,
                               (int64_t)pairs, I);
            NVL_HIP(hipGetLastError());
        }
        for (int e = 0; e < E; e++) {
            const char* wout = (const char*)l.t[NVL_T_MOE_OUT].p + (size_t)e * H * I * m->wsize;
            GemmArgs a = mk(m->hbuf, I, wout, m->moe_eo, H, nullptr, 1.f, M, H, I);
            a.seg = m->seg_start + e;
            gemm(m, EPI_STORE, true, a);
        }
    } else {
        GemmArgs a = mk(m->xn, H, l.moe_in, m->hbuf, I, nullptr, 1.f, max_mtiles, 2 * I, H);
        a.a_rows = m->perm_token; a.tile_map = m->moe_tile_map; a.n_mtiles = m->moe_n_mtiles;
        if (!small && m->moe_xg && g_moe_gather) {
            // prefill: every m-tile's rows would be re-gathered 16 bytes at a time by each of its 2I/128 column tiles
            // (64 cache lines per load instruction); copy them into expert order once, then the GEMM streams whole
            // 1-KiB operand blocks (Granite-1B, 16384 tokens: expert-up 1119 -> ? us per layer)
            KScope ks(m, KC_OTHER);
            hipLaunchKernelGGL(moe_gather_fm_kernel, dim3(cdiv(pairs, 16)), dim3(256), 0, m->stream, (const bf16_t*)m->xn,
                               m->perm_token, (bf16_t*)m->moe_xg, pairs, H);
            NVL_HIP(hipGetLastError());
            a.A = m->moe_xg; a.a_rows = nullptr;
        }
        a.w_expert_stride = (int64_t)2 * I * H; a.grp_bm = pp ? 512 : BM; a.grp_deep = small && g_moe_deep;
        // quantized experts: the grouped GEMMs run on this layer's W~, dequantized into one scratch buffer — up first, then down
        // over it, in stream order (the down dequantize starts after the up GEMM has read the scratch).
        const void* w_down = l.t[NVL_T_MOE_OUT].p;
        const double dq_bytes = wf_dequant_bytes(m->ef);     // algorithmic bytes of a dequantize, per element
        if (m->ef != WF_BF16) {
            KScope ks(m, KC_OTHER, 0, KS_MOE_UP, (double)round_up(E * 2 * I, W_ROW_PAD) * H * dq_bytes);
            wf_dequant_rows(m->stream, m->ef, l.moe_in, l.qs_moe_in, H, 0, round_up(E * 2 * I, W_ROW_PAD), m->eq_scratch);
            NVL_HIP(hipGetLastError());
            a.W = m->eq_scratch;
        }
        m->site = KS_MOE_UP; m->site_bytes = (e_touch * 2 * I * H + (double)pairs * H + (double)pairs * I) * (double)m->wsize;
        gemm(m, EPI_SWIGLU, false, a, 2.0 * pairs * 2 * I * H);
        if (m->ef != WF_BF16) {
            KScope ks(m, KC_OTHER, 0, KS_MOE_DOWN, (double)E * H * I * dq_bytes);
            dequant_down_experts(m, l, H, I, E, m->eq_scratch);
            w_down = m->eq_scratch;
        }
        GemmArgs d = mk(m->hbuf, I, w_down, m->moe_eo, H, nullptr, 1.f, max_mtiles, H, I);
        d.tile_map = m->moe_tile_map; d.n_mtiles = m->moe_n_mtiles; d.w_expert_stride = (int64_t)H * I; d.grp_bm = pp ? 512 : BM; d.grp_deep = small && g_moe_deep;
        m->site = KS_MOE_DOWN; m->site_bytes = (e_touch * H * I + (double)pairs * I) * (double)m->wsize + (double)pairs * H * 4.0;
        gemm(m, EPI_STORE, true, d, 2.0 * pairs * H * I);
    }
    if (small && !m->keep_hidden && m->pending_slices == 0 && H % 4 == 0 && H <= 1024 * NORM_ROW_MAXCH) {
        // x += rm * sum_k w[t][k] * eo[slot[t][k]] is completed by the next norm's read of x (PendingResid)
        m->pending_part = m->moe_eo; m->pending_slices = k; m->pending_rows = M; m->pending_alpha = c.residual_multiplier;
        m->pending_slot_of = m->slot_of; m->pending_gate_w = m->expert_w;
    } else {
        KScope ks(m, KC_OTHER, 0, KS_MOE_COMBINE, (double)pairs * H * 4.0 + (double)M * H * 8.0);
        hipLaunchKernelGGL(moe_combine_kernel, dim3(M), dim3(256), 0, m->stream, m->moe_eo, m->slot_of, m->expert_w, k,
                           c.residual_multiplier, m->x, H, 1);
        NVL_HIP(hipGetLastError());
    }
    return false;
}

}  // namespace

namespace {
// ---- hipGraph replay of decode passes ----------------------------------------------------------------------------------
// A decode pass is ~85 dependent launches of a few microseconds each.  A pass whose launch configuration (the key) has been
// seen before is captured once from the model's stream and replayed with hipGraphLaunch: the arguments of every launch are
// device buffers whose CONTENTS change (token ids, positions, block tables, KV slabs), never their addresses.  First sight
// of a key runs eagerly (it also sets the per-function attributes, which must not happen during capture).
template <typename F>
bool replay_or_capture(nvl_model* m, const std::array<int, 5>& key, F&& enqueue) {
    m->draft_valid = false;      // a replayed pass never reaches enqueue_forward: the kept proposals of nvl_draft_sampled end here too
    // (tensor parallel: only with the P2P all-reduce, whose call state lives on the device; RCCL / the in-process emulation
    //  are host-driven)
    if (!g_use_graphs || !m->graphs_ok || m->profile || m->keep_hidden || m->tap || m->stamping || ((m->tp > 1 || m->tp_force) && !m->p2p_ready)) return false;
    auto it = m->graphs.find(key);
    if (it != m->graphs.end()) { NVL_HIP(hipGraphLaunch(it->second, m->stream)); m->stats.graph_replays++; return true; }
    if (!m->graph_seen.count(key)) { m->graph_seen.insert(key); return false; }
    if (m->graphs.size() >= 64) retire_graphs(m);        // (keys come and go with the context length: keep the table small;
                                                         //  earlier steps' replays may still be running: destroyed at the next sync)
    if (hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); m->graphs_ok = false; return false; }
    hipGraph_t g = nullptr;
    try {
        enqueue();
    } catch (...) {
        (void)hipStreamEndCapture(m->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        m->graphs_ok = false;
        throw;
    }
    if (hipStreamEndCapture(m->stream, &g) != hipSuccess || !g) { (void)hipGetLastError(); m->graphs_ok = false; enqueue(); return true; }
    hipGraphExec_t ge = nullptr;
    const hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess || !ge) { (void)hipGetLastError(); m->graphs_ok = false; enqueue(); return true; }
    m->graphs[key] = ge;
    NVL_HIP(hipGraphLaunch(ge, m->stream));
    m->stats.graph_replays++;
    return true;
}

// debug taps: the residual stream after layer li.  Mode 1 (keep_hidden) runs every residual add to completion in its own
// launch, so x is the layer's output; mode 2 (tap) leaves the product path alone and adds what is still pending.
void tap_layer(nvl_model* m, int li, int M) {
    if (!m->keep_hidden && !m->tap) return;
    float* dst = m->hidden + (int64_t)li * M * m->H;
    if (m->pending_slices == 0) { NVL_HIP(hipMemcpyAsync(dst, m->x, (size_t)M * m->H * 4, hipMemcpyDeviceToDevice, m->stream)); return; }
    PendingResid pr{m->pending_part, m->pending_slices, m->pending_rows, m->pending_alpha, m->pending_slot_of, m->pending_gate_w};
    hipLaunchKernelGGL(tap_hidden_kernel, dim3(M), dim3(256), 0, m->stream, m->x, dst, m->H, pr);
    NVL_HIP(hipGetLastError());
}

// ---- embed (generic_model.go:295-302): tokens -> the residual stream m->x, by the kernel of the table's format ----
void embed(nvl_model* m, const Meta& md, int M) {
    const nvl_model_config& c = m->cfg;
    const int H = m->H;
    KScope ks(m, KC_OTHER, 0, KS_EMBED, (double)M * H * (4.0 + (double)m->wsize));
    const void* pe = (c.position_type == NVL_POS_LEARNED) ? m->g[NVL_T_POS_EMB].p : nullptr;
    const int pe_rows = pe ? (int)std::min<int64_t>(m->g[NVL_T_POS_EMB].rows, c.max_seq_len) : 0;
    if (m->f32) {
        m->front_ran[NVL_QKV_RAN_EMBED] = NVL_EMBED_RAN_F32;
        hipLaunchKernelGGL((embed_kernel<float, false>), dim3(M), dim3(256), 0, m->stream, md.tokens, md.tok_pos,
                           (const float*)m->g[NVL_T_TOK_EMB].p, (const float*)pe, pe_rows, c.embedding_multiplier, m->x, H);
    } else if (m->g[NVL_T_TOK_EMB].wf == WF_MXFP4) {     // MXFP4 tied table (w4.h)
        m->front_ran[NVL_QKV_RAN_EMBED] = NVL_EMBED_RAN_W4;
        hipLaunchKernelGGL(embed_w4_kernel, dim3(M), dim3(256), 0, m->stream, md.tokens, md.tok_pos,
                           (const uint8_t*)m->g[NVL_T_TOK_EMB].p, (const uint8_t*)m->g[NVL_T_TOK_EMB].qs, (const bf16_t*)pe, pe_rows,
                           c.embedding_multiplier, m->x, H);
    } else if (m->g[NVL_T_TOK_EMB].qs) {     // 8-bit tied table (w8.h)
        m->front_ran[NVL_QKV_RAN_EMBED] = NVL_EMBED_RAN_W8;
        hipLaunchKernelGGL(embed_w8_kernel, dim3(M), dim3(256), 0, m->stream, md.tokens, md.tok_pos,
                           (const uint8_t*)m->g[NVL_T_TOK_EMB].p, (const float*)m->g[NVL_T_TOK_EMB].qs, (const bf16_t*)pe, pe_rows,
                           c.embedding_multiplier, m->x, H);
    } else {
        m->front_ran[NVL_QKV_RAN_EMBED] = NVL_EMBED_RAN_BF16;
        hipLaunchKernelGGL((embed_kernel<bf16_t, true>), dim3(M), dim3(256), 0, m->stream, md.tokens, md.tok_pos,
                           (const bf16_t*)m->g[NVL_T_TOK_EMB].p, (const bf16_t*)pe, pe_rows, c.embedding_multiplier, m->x, H);
    }
    NVL_HIP(hipGetLastError());
}

// ---- the front of an attention layer: attention norm -> QKV projection (+ bias) -> RoPE -> Q into m->q, K / V into the
// cache (enqueue_forward; nvl_op_qkv_stages).  m->xn holds the projection's operand already, and no norm runs, when the
// layer before deferred it (qkv_deferred: xn_raw + the x^2 partials) or the decode seam left it (seam_operand).  Returns fused_dec: the
// projection only stored its fp32 rows, RoPE and the K / V append are left to the decode attention kernel.
// What ran goes to m->front_ran (NVL_QKV_RAN_*).
bool qkv_front(nvl_model* m, const LayerW& l, int li, const Meta& md, int M, int max_len, bool big_decode, bool qkv_deferred,
               bool seam_operand) {
    const int H = m->H;
    m->front_ran[NVL_QKV_RAN_NORM] = 0;
    if (!qkv_deferred && !seam_operand) {
        norm(m, m->x, nullptr, l.t[NVL_T_ATTN_NORM_W], l.t[NVL_T_ATTN_NORM_B], m->xn, M);
        m->front_ran[NVL_QKV_RAN_NORM] = m->norm_ran;
    }
    bool fused_dec = false;
    // a decode batch of 64 < M <= g_chunk_max_m rows keeps the decode form (64-row passes, gemm.h) and the fused
    // decode attention
    // short prefill batches (65..g_qkv_store_max_m tokens): the fused-epilogue tile kernel would run on M/128 * 24
    // workgroups; the decode form + rope_kv_kernel is faster there
    const bool short_prefill = max_len > 1 && M <= g_qkv_store_max_m && M <= g_chunk_max_m && g_force_tile == 0;
    if (!m->f32 && !m->kv8 && M > 64 && !big_decode && !short_prefill) {
        // prefill: RoPE + Q/K/V placement fused into the projection's epilogue (no fp32 qkv round trip)
        GemmArgs a = mk(m->xn, H, l.w_qkv, nullptr, 0, l.b_qkv, 1.f, M, m->n_qkv, H);
        a.qkv.tok_pos = md.tok_pos; a.qkv.tok_tbl = md.tok_tbl; a.qkv.blk_table = md.blk_table; a.qkv.cos_t = m->rope_cos; a.qkv.sin_t = m->rope_sin;
        a.qkv.q_out = (bf16_t*)m->q;
        a.qkv.kcache = (bf16_t*)m->kcache + (int64_t)li * m->layer_stride;
        a.qkv.vcache = (bf16_t*)m->vcache + (int64_t)li * m->layer_stride;
        a.qkv.slot_stride = m->slot_stride; a.qkv.Tmax = m->Tmax; a.qkv.nH = m->nH; a.qkv.nKV = m->nKV; a.qkv.hd = m->hd;
        m->site = KS_QKV;
        gemm(m, EPI_QKV, false, a);
        m->front_ran[NVL_QKV_RAN_FORM] = NVL_QKV_FORM_EPILOGUE;
    } else {
        GemmArgs aq = mk(m->xn, H, l.w_qkv, m->qkv, m->n_qkv, l.b_qkv, 1.f, M, m->n_qkv, H);
        if (qkv_deferred) set_deferred_in(m, aq);
        m->site = KS_QKV;
        gemm(m, EPI_STORE, true, aq);
        fused_dec = !m->f32 && !m->kv8 && max_len == 1;     // decode: RoPE + KV append live in the attention kernel
        if (!fused_dec) rope_kv(m, li, md, M);     // (8-bit mode: always here — rope_kv8_kernel is its only K/V writer)
        m->front_ran[NVL_QKV_RAN_FORM] = fused_dec ? NVL_QKV_FORM_STORE_ONLY : m->kv8 ? NVL_QKV_FORM_STORE_ROPE_KV8
            : m->f32 ? NVL_QKV_FORM_F32_STORE_ROPE
            : m->gemm_ran == NVL_GEMM_RAN_GROUPS ? NVL_QKV_FORM_GROUPS_STORE_ROPE : NVL_QKV_FORM_DECODE_STORE_ROPE;
    }
    m->front_ran[NVL_QKV_RAN_GEMM] = m->gemm_ran;
    return fused_dec;
}

// What a pass decides once, for all of its layers, about the dense layer tail (enqueue_forward; nvl_op_dense_stages).
// decode, RMSNorm + SwiGLU, sequential block: every residual projection carries the norm that follows it (deferred
// RMSNorm, gemm.h), so a step keeps ONE norm launch (layer 0's, after the embedding) instead of 2L + 1
struct TailPlan { bool big_decode, defer_ok, defer_moe_ok, all_rows; int n_seqs; };
TailPlan tail_plan(const nvl_model* m, int M, int n_seqs, int max_len, uint32_t flags) {
    const nvl_model_config& c = m->cfg;
    const int H = m->H;
    const bool big_decode = max_len == 1 && M <= g_chunk_max_m && g_force_tile == 0;
    // (tensor parallel: the all-reduce launch carries the norm — one-shot payloads only, i.e. M <= 64 — when the P2P group is attached)
    const bool tp_on = m->tp > 1 || m->tp_force;
    const bool tp_defer = tp_on && m->p2p_ready && M <= g_p2p_oneshot_rows && M <= 64;
    TailPlan t{};
    t.big_decode = big_decode;      // (a decode batch that keeps the decode form above 64 rows: the QKV dispatch asks too)
    t.defer_ok = g_defer_norm && !m->f32 && (M <= 64 || (M <= DEFER_MAX_M && big_decode && g_defer_norm == 1 && !tp_on)) && !c.use_moe && (!tp_on || tp_defer) && !m->keep_hidden &&
                 c.block_style == NVL_BLOCK_SEQUENTIAL && c.norm_type == NVL_NORM_RMS &&
                 c.activation_type == NVL_ACT_SWIGLU && H % 256 == 0 && m->rs_part && m->n_mamba == 0;
    // MoE layers (decode form): only the O projection carries a norm (the FFN norm); the expert-down projection leaves
    // K-slice partials that the next attention norm sums
    t.defer_moe_ok = g_defer_norm && c.use_moe && M <= 64 && m->tp == 1 && !m->tp_force && c.block_style == NVL_BLOCK_SEQUENTIAL &&
                     c.norm_type == NVL_NORM_RMS && H % 256 == 0 && m->rs_part && m->n_mamba == 0;
    t.all_rows = (flags & NVL_FWD_ALL_LOGITS) != 0;
    t.n_seqs = n_seqs;
    return t;
}

// One attention layer from its O projection to the end: both residual projections, the FFN (or MoE) between them, the
// norms they do not carry.  Returns whether m->xn / m->rs_part hold the deferred operand of the norm (nxt_w, nxt_b) that
// follows the layer (has_next: a layer's attention norm; else the final norm).
bool layer_tail(nvl_model* m, const LayerW& l, int li, int M, const TailPlan& tp, const DevTensor* nxt_w, const DevTensor* nxt_b,
                bool has_next, const StageHook* hook = nullptr) {
    const nvl_model_config& c = m->cfg;
    const int H = m->H, qw = m->nH * m->hd;
    const bool defer_ok = tp.defer_ok, defer_moe_ok = tp.defer_moe_ok, all_rows = tp.all_rows;
    const int n_seqs = tp.n_seqs;
    bool xn_deferred = false;
    auto at = [&](int stage) { if (hook) hook->fn(hook->ctx, stage); };
    const float* bo = (const float*)l.t[NVL_T_BO].p;
    if (c.block_style == NVL_BLOCK_PARALLEL) {
        // generic_model.go:395-418: r + [am*]attn + [rm*]ffn, both branches read the same normed x
        const bool mults = c.attention_multiplier != 0.f && c.residual_multiplier != 0.f;
        ffn_up(m, l, M);
        at(TAIL_H);
        m->site = KS_OPROJ;
        resid_gemm(m, m->attn_out, qw, l.t[NVL_T_WO].p, bo, mults ? c.attention_multiplier : 1.f, M, H, qw);
        at(TAIL_X1);
        m->site = KS_FFN_DOWN;
        resid_gemm(m, m->hbuf, m->F, l.t[NVL_T_W2].p, (const float*)l.t[NVL_T_B2].p, mults ? c.residual_multiplier : 1.f,
                   M, H, m->F);   // (only one of the two may be pending: the second one adds into x directly)
        at(TAIL_X2);
    } else {
        // decode, RMSNorm + SwiGLU: the O-projection carries the FFN norm (deferred RMSNorm, gemm.h) — one launch less
        const bool defer = (defer_ok || (defer_moe_ok && moe_dense_ok(m, l, M))) && m->pending_slices == 0 && !l.t[NVL_T_FFN_NORM_B].present();
        m->site = KS_OPROJ;
        if (defer) {
            resid_gemm(m, m->attn_out, qw, l.t[NVL_T_WO].p, bo, m->resid_alpha, M, H, qw, (const float*)l.t[NVL_T_FFN_NORM_W].p);
            at(TAIL_X1);
        } else {
            resid_gemm(m, m->attn_out, qw, l.t[NVL_T_WO].p, bo, m->resid_alpha, M, H, qw);
            at(TAIL_X1);
            norm(m, m->x, nullptr, l.t[NVL_T_FFN_NORM_W], l.t[NVL_T_FFN_NORM_B], m->xn, M);
        }
        at(TAIL_OPERAND);
        // the FFN-down projection carries the NEXT layer's attention norm, or the final norm when every row is
        // a last row (decode)
        if (c.use_moe) {
            const bool defer2 = defer && defer_moe_ok && g_defer_norm != 3 && !nxt_b->present() &&
                                (has_next || (!all_rows && M == n_seqs && M <= 64));
            xn_deferred = moe(m, l, M, defer, defer2 ? (const float*)nxt_w->p : nullptr, hook);
        } else {
            ffn_up(m, l, M, defer);
            at(TAIL_H);
            const bool defer2 = defer_ok && g_defer_norm != 3 && m->pending_slices == 0 && !nxt_b->present() &&
                                (has_next || (!all_rows && M == n_seqs && M <= 64));   // (the LM head of a larger batch runs on the tile kernels)
            m->site = KS_FFN_DOWN;
            resid_gemm(m, m->hbuf, m->F, l.t[NVL_T_W2].p, (const float*)l.t[NVL_T_B2].p, m->resid_alpha, M, H, m->F,
                       defer2 ? (const float*)nxt_w->p : nullptr);
            xn_deferred = defer2;
        }
        at(TAIL_X2);
    }
    tap_layer(m, li, M);
    return xn_deferred;
}

// The norm after the last layer and the projection that reads it: the LM head of a model (W = lm_head, out = logits).
// xn_deferred: the last FFN-down projection already produced the final norm's operand for every row.
void head_proj(nvl_model* m, bool xn_deferred, const int32_t* rows_idx, int rows, const void* W, float* out, int ld, int N) {
    const int H = m->H;
    if (xn_deferred) {
        GemmArgs al = mk(m->xn, H, W, out, ld, nullptr, 1.f, rows, N, H);
        set_deferred_in(m, al);
        m->site = KS_LM_HEAD;
        gemm(m, EPI_STORE, true, al);
    } else {
        norm(m, m->x, rows_idx, m->g[NVL_T_FINAL_NORM_W], m->g[NVL_T_FINAL_NORM_B], m->xn_last, rows);
        if (m->pending_slices != 0) throw std::runtime_error("forward: a split-K residual was left unconsumed");
        m->site = KS_LM_HEAD;
        gemm(m, EPI_STORE, true, mk(m->xn_last, H, W, out, ld, nullptr, 1.f, rows, N, H));
    }
}

// Mamba2Layer.Forward between its two projections (mamba2.go:107-170) for the batch `a` describes: conv + softplus (and
// the tail of a chained prefill), the scan in the form the batch calls for, gate + RMS norm into `out` (the out_proj
// operand, ActT).  `a` arrives without the chunk-parallel scratch, which is the model's and grows here.  y_pre != NULL
// (nvl_op_mamba_mixer) receives the scan's y before the gate kernel overwrites it in place.
void mamba_mixer(nvl_model* m, MambaArgs a, int M, int n_seqs, int max_len, void* out, float* y_pre = nullptr) {
    const int64_t state_floats = (int64_t)a.nh * a.hd * a.ss;
    const double tail_bytes = a.chain ? 2.0 * n_seqs * (double)(a.K - 1) * a.conv_dim * 4.0 : 0.0;
    if (a.chain == 3 && max_len == 1 && g_mamba_conv_step) {
        // a decode pass of a carried model: conv, tail shift and softplus in one launch (mamba.h mamba_conv_step_kernel)
        KScope ks(m, KC_OTHER, 0, KS_MAMBA_CONV, (double)M * (a.P + a.conv_dim + a.nh) * 4.0 + tail_bytes);
        const dim3 grid(cdiv(a.conv_dim / 4 + a.nh, 64), n_seqs);
        switch (a.K) {     // (K == 1 has no tail and so no chain)
            case 2: hipLaunchKernelGGL(mamba_conv_step_kernel<2>, grid, dim3(64), 0, m->stream, a); break;
            case 3: hipLaunchKernelGGL(mamba_conv_step_kernel<3>, grid, dim3(64), 0, m->stream, a); break;
            case 4: hipLaunchKernelGGL(mamba_conv_step_kernel<4>, grid, dim3(64), 0, m->stream, a); break;
            case 5: hipLaunchKernelGGL(mamba_conv_step_kernel<5>, grid, dim3(64), 0, m->stream, a); break;
            case 6: hipLaunchKernelGGL(mamba_conv_step_kernel<6>, grid, dim3(64), 0, m->stream, a); break;
            case 7: hipLaunchKernelGGL(mamba_conv_step_kernel<7>, grid, dim3(64), 0, m->stream, a); break;
            case 8: hipLaunchKernelGGL(mamba_conv_step_kernel<8>, grid, dim3(64), 0, m->stream, a); break;
            default: throw std::runtime_error("mamba_mixer: a carried conv window needs 2 <= K <= 8");
        }
        NVL_HIP(hipGetLastError());
    } else {
        {
            KScope ks(m, KC_OTHER, 0, KS_MAMBA_CONV, (double)M * (a.P + a.conv_dim + a.nh) * 4.0);
            hipLaunchKernelGGL(mamba_conv_kernel, dim3(M), dim3(256), 0, m->stream, a);
            NVL_HIP(hipGetLastError());
        }
        if (a.chain) {     // (a launch of its own in the per-site profile)
            KScope ks(m, KC_OTHER, 0, KS_MAMBA_CONV, tail_bytes);
            hipLaunchKernelGGL(mamba_tail_kernel, dim3(n_seqs), dim3(256), 0, m->stream, a);
            NVL_HIP(hipGetLastError());
        }
    }
    {
        KScope ks(m, KC_OTHER, 2.0 * 3.0 * (double)M * a.EH * a.ss, KS_MAMBA_SCAN,
                  (double)M * (a.conv_dim + a.nh + a.EH) * 4.0 + 2.0 * n_seqs * (double)state_floats * 4.0);
        const int per = a.ss / (256 / a.hd);
        dim3 grid(a.nh, n_seqs);
        // prefill-sized calls, bf16 mode: the chunked (SSD) form on MFMA — 64 tokens per step instead of one
        const bool ssd = g_mamba_ssd && !m->f32 && max_len >= 16 && (a.hd == 32 || a.hd == 64) &&
                         (a.ss == 32 || a.ss == 64 || a.ss == 128) && a.conv_dim % 4 == 0 && a.EH % 4 == 0;
        // (sequence, head) pairs for fewer than half the CUs and several chunks: the chunks of a sequence in parallel (state
        // contributions, a short recurrence over the chunks, outputs: three launches; 1 x 2048: 318 -> 90 us per layer) —
        // with a workgroup per CU already (8 x 512) the extra state traffic loses (86 -> 174 us); scratch capped at 256 MB
        const int max_chunks = cdiv(max_len, 64);
        const int64_t z_floats = (int64_t)n_seqs * max_chunks * state_floats;
        const bool par = ssd && g_mamba_ssd >= 1 && g_mamba_ssd != 2 && max_chunks >= 4 && a.nh * n_seqs < 128 && z_floats * 4 <= (256ll << 20);
        if (par && z_floats > m->ssd_z_floats) {
            NVL_HIP(hipStreamSynchronize(m->stream));
            dfree(m->ssd_z); dfree(m->ssd_decay);
            m->ssd_z = dmalloc<float>(z_floats); m->ssd_z_floats = z_floats;
            m->ssd_decay = dmalloc<float>((int64_t)n_seqs * max_chunks * a.nh + 1024);
            m->ssd_decay_floats = (int64_t)n_seqs * max_chunks * a.nh + 1024;
        }
        if (par && (int64_t)n_seqs * max_chunks * a.nh > m->ssd_decay_floats) {
            NVL_HIP(hipStreamSynchronize(m->stream));
            dfree(m->ssd_decay);
            m->ssd_decay_floats = (int64_t)n_seqs * max_chunks * a.nh + 1024;
            m->ssd_decay = dmalloc<float>(m->ssd_decay_floats);
        }
        a.ssd_z = m->ssd_z; a.ssd_decay = m->ssd_decay;
#define NVL_SSD(HDv, SSv)                                                                                              \
        do {                                                                                                   \
            constexpr int lds_ = mamba_ssd_lds_bytes<HDv, SSv>();                                              \
            if (par) {                                                                                         \
                dim3 g3(a.nh, n_seqs, max_chunks);                                                             \
                NVL_LDS_ATTR((mamba_ssd_kernel<HDv, SSv, 1>), lds_);                                           \
                NVL_LDS_ATTR((mamba_ssd_kernel<HDv, SSv, 2>), lds_);                                           \
                hipLaunchKernelGGL((mamba_ssd_kernel<HDv, SSv, 1>), g3, dim3(256), lds_, m->stream, a);        \
                hipLaunchKernelGGL(mamba_ssd_prefix_kernel, dim3(a.nh, n_seqs, cdiv(HDv * SSv, 1024)), dim3(256), 0, m->stream, a, max_chunks, HDv * SSv); \
                hipLaunchKernelGGL((mamba_ssd_kernel<HDv, SSv, 2>), g3, dim3(256), lds_, m->stream, a);        \
            } else {                                                                                           \
                NVL_LDS_ATTR((mamba_ssd_kernel<HDv, SSv, 0>), lds_);                                           \
                hipLaunchKernelGGL((mamba_ssd_kernel<HDv, SSv, 0>), grid, dim3(256), lds_, m->stream, a);      \
            }                                                                                                  \
        } while (0)
        if (ssd) {
            if (a.hd == 64) { if (a.ss == 128) NVL_SSD(64, 128); else if (a.ss == 64) NVL_SSD(64, 64); else NVL_SSD(64, 32); }
            else { if (a.ss == 128) NVL_SSD(32, 128); else if (a.ss == 64) NVL_SSD(32, 64); else NVL_SSD(32, 32); }
        } else
#undef NVL_SSD
        if (per <= 4) hipLaunchKernelGGL(mamba_scan_kernel<4>, grid, dim3(256), 0, m->stream, a);
        else if (per <= 8) hipLaunchKernelGGL(mamba_scan_kernel<8>, grid, dim3(256), 0, m->stream, a);
        else if (per <= 16) hipLaunchKernelGGL(mamba_scan_kernel<16>, grid, dim3(256), 0, m->stream, a);
        else hipLaunchKernelGGL(mamba_scan_kernel<32>, grid, dim3(256), 0, m->stream, a);
        NVL_HIP(hipGetLastError());
    }
    if (y_pre) NVL_HIP(hipMemcpyAsync(y_pre, a.y, (size_t)M * a.EH * 4, hipMemcpyDeviceToDevice, m->stream));
    {
        KScope ks(m, KC_OTHER, 0, KS_MAMBA_GATE, (double)M * a.EH * (8.0 + (double)m->wsize));
        if (m->f32) hipLaunchKernelGGL((mamba_gate_norm_kernel<float>), dim3(M), dim3(256), 0, m->stream, a, (float*)out);
        else hipLaunchKernelGGL((mamba_gate_norm_kernel<bf16_t>), dim3(M), dim3(256), 0, m->stream, a, (bf16_t*)out);
        NVL_HIP(hipGetLastError());
    }
}

// Enqueue ONE forward pass (embedding ... argmax) on the model's stream for the batch described by the device
// metadata `md` — no host synchronisation.  Returns the number of logits rows produced.
// seam: 0 = whole pass; bit 0 = x and layer 0's normed operand are already in place (skip embed + first norm);
// bit 1 = stop after the argmax partials (the caller's decode_seam_kernel finishes the step); bit 2 = no argmax at
// all (the caller samples from the logits); bit 3 = a verify pass (nvl_verify_greedy*): its 2..8 positions per sequence
// take the multi-position decode attention instead of the prefill kernel (attention_mq_ok)
// Either tail leaves LogitsScaling APPLIED IN PLACE in m->logits (argmax_partial_kernel writes the divided value back,
// scale_rows_kernel is the division itself): nvl_sample and nvl_logprobs read final logits and never divide again.
// `sc` != NULL (nvl_score; flags carry NVL_FWD_ALL_LOGITS): the tail is final norm over every row, then LM head +
// logprob kernels over chunks of at most g_score_rows rows; no logits rows are left (last_rows = 0).
struct ScoreReq { int top_k; bool want_topk; };
static int g_score_rows = 1024;   // nvl_set_tuning key 37: rows per LM-head + logprob chunk of nvl_score (a multiple of 16)
int enqueue_forward(nvl_model* m, const Meta& md, int n_seqs, int M, int max_len, double attn_flops, uint32_t flags,
                    int seam = 0, const ScoreReq* sc = nullptr) {
    const nvl_model_config& c = m->cfg;
    const int H = m->H;
    m->kv_written = true;                  // (nvl_set_kv_scales is refused from here on)
    m->draft_valid = false;                // (the kept proposals of nvl_draft_sampled describe the pass before this one)
    m->pending_slices = 0;
    std::fill(m->dense_ran, m->dense_ran + NVL_DENSE_RAN_INTS, 0);
    m->phase = max_len > 1 ? 0 : 1;         // per-site profile: prefill / decode
    if ((m->keep_hidden || m->tap) && m->hidden_tokens < M) {
        dfree(m->hidden);
        m->hidden = dmalloc<float>((int64_t)m->L * M * H);
        m->hidden_tokens = M;
    }
    m->hidden_last_M = M;

    if (!(seam & 1)) embed(m, md, M);

    const TailPlan tp_ = tail_plan(m, M, n_seqs, max_len, flags);
    const bool big_decode = tp_.big_decode;
    bool xn_deferred = false;       // m->xn holds xn_raw of the upcoming norm, m->rs_part its x^2 partials
    for (int li = 0; li < m->L; li++) {
        const LayerW& l = m->layers[li];
        if (l.mamba) {
            // forwardMamba2 (generic_model.go:160-202): norm, Mamba2Layer.Forward (mamba2.go:74-181), residual; norm, shared MLP, residual
            norm(m, m->x, nullptr, l.t[NVL_T_ATTN_NORM_W], l.t[NVL_T_ATTN_NORM_B], m->xn, M);
            m->site = KS_MAMBA_IN;
            gemm(m, EPI_STORE, true, mk(m->xn, H, l.t[NVL_T_MAMBA_IN_PROJ].p, m->mproj, m->mP, nullptr, 1.f, M, m->mP, H));
            MambaArgs a{};
            a.proj = m->mproj; a.P = m->mP; a.EH = m->mEH; a.conv_dim = m->mConv; a.nh = m->m_nh; a.hd = m->m_hd; a.ss = m->m_ss;
            a.ng = m->m_ng; a.K = m->m_K;
            a.conv_w = (const float*)l.t[NVL_T_MAMBA_CONV_W].p; a.conv_b = (const float*)l.t[NVL_T_MAMBA_CONV_B].p;
            a.a_log = (const float*)l.t[NVL_T_MAMBA_A_LOG].p; a.Dskip = (const float*)l.t[NVL_T_MAMBA_D].p;
            a.dt_bias = (const float*)l.t[NVL_T_MAMBA_DT_BIAS].p; a.norm_w = (const float*)l.t[NVL_T_MAMBA_NORM].p;
            a.xbc = m->mxbc; a.delta = m->mdelta; a.y = m->my;
            a.state = m->ssm_state + (int64_t)l.mamba_idx * m->ssm_layer_stride; a.state_slot_stride = m->ssm_slot_stride;
            a.tok_pos = md.tok_pos; a.tok_seq = md.tok_tbl; a.seq_tok_start = md.seq_tok_start; a.seq_len = md.seq_len;
            a.seq_pos = md.seq_pos; a.seq_slot = md.blk_table;     // slab mode: token -> sequence index i, blk_table[i] = slot
            // a carried model runs every pass as chain 3; the runner's chunk loop (conv_chain 1 / 2) is then a special case of it
            a.chain = m->conv_tail ? (m->conv_carried ? 3 : m->conv_chain) : 0;
            a.tail = m->conv_tail ? m->conv_tail + (int64_t)l.mamba_idx * m->conv_tail_layer_stride : nullptr;
            a.tail_slot_stride = m->conv_tail_slot_stride;
            mamba_mixer(m, a, M, n_seqs, max_len, m->myn);
            m->site = KS_MAMBA_OUT;
            resid_gemm(m, m->myn, m->mEH, l.t[NVL_T_MAMBA_OUT_PROJ].p, nullptr, m->resid_alpha, M, H, m->mEH);
            norm(m, m->x, nullptr, l.t[NVL_T_FFN_NORM_W], l.t[NVL_T_FFN_NORM_B], m->xn, M);
            ffn_up(m, l, M);
            m->site = KS_FFN_DOWN;
            resid_gemm(m, m->hbuf, m->F, l.t[NVL_T_W2].p, (const float*)l.t[NVL_T_B2].p, m->resid_alpha, M, H, m->F);
            tap_layer(m, li, M);
            continue;
        }
        const bool fused_dec = qkv_front(m, l, li, md, M, max_len, big_decode, xn_deferred, li == 0 && (seam & 1));
        xn_deferred = false;
        if (m->kv8)
            attention_kv8(m, md, n_seqs, max_len, (char*)m->kcache + (size_t)li * m->layer_stride,
                          (char*)m->vcache + (size_t)li * m->layer_stride, m->k_scale[li], m->v_scale[li]);
        else
            attention(m, li, md, n_seqs, max_len, attn_flops, fused_dec, (seam & 8) != 0);
        const DevTensor* nxt_w = li + 1 < m->L ? &m->layers[li + 1].t[NVL_T_ATTN_NORM_W] : &m->g[NVL_T_FINAL_NORM_W];
        const DevTensor* nxt_b = li + 1 < m->L ? &m->layers[li + 1].t[NVL_T_ATTN_NORM_B] : &m->g[NVL_T_FINAL_NORM_B];
        xn_deferred = layer_tail(m, l, li, M, tp_, nxt_w, nxt_b, li + 1 < m->L);
    }

    // ---- final norm + LM head on the rows the caller keeps (generic_model.go:464-477, :595-604) ----
    const bool all = (flags & NVL_FWD_ALL_LOGITS) != 0;
    const int rows = sc ? std::min(M, g_score_rows) : (all ? M : n_seqs);      // rows of m->logits this pass needs
    if (rows > m->logit_rows) {
        clear_graphs(m);               // (captured passes hold the old addresses)
        dfree(m->logits); dfree(m->xn_last);
        m->logits = dmalloc<float>((int64_t)rows * m->Vpad);
        m->xn_last = dmalloc_bytes(round_up(rows, 64) * H * (int64_t)m->wsize);
        NVL_HIP(hipMemsetAsync(m->xn_last, 0, (size_t)(round_up(rows, 64) * H) * m->wsize, m->stream));
        m->logit_rows = rows;
    }
    if (sc) {
        // ONE final norm over all M rows (the launch an all-logits pass makes: it also completes a pending split-K
        // residual) into m->xn, free by now; then per chunk of `rows` rows: its normed rows -> xn_last (whole 16-row
        // tiles of the fragment-major operand are contiguous: chunk starts are multiples of 16), LM head, logprob kernels.
        if (xn_deferred) throw std::runtime_error("score: deferred final norm on the all-rows path");
        norm(m, m->x, nullptr, m->g[NVL_T_FINAL_NORM_W], m->g[NVL_T_FINAL_NORM_B], m->xn, M);
        if (m->pending_slices != 0) throw std::runtime_error("forward: a split-K residual was left unconsumed");
        const LogprobBufs& b = m->lpb;
        for (int r0 = 0; r0 < M; r0 += rows) {
            const int n = std::min(rows, M - r0);
            const size_t row_bytes = (size_t)H * m->wsize;
            NVL_HIP(hipMemcpyAsync(m->xn_last, (const char*)m->xn + (size_t)r0 * row_bytes,
                                   (size_t)(m->f32 ? n : round_up(n, 16)) * row_bytes, hipMemcpyDeviceToDevice, m->stream));
            m->site = KS_LM_HEAD;
            gemm(m, EPI_STORE, true, mk(m->xn_last, H, m->lm_head, m->logits, m->Vpad, nullptr, 1.f, n, m->V, H));
            KScope ks(m, KC_OTHER, 0, KS_LOGPROBS, (double)n * m->V * 4.0);
            LogprobArgs a{};
            a.x = m->logits; a.ld = m->Vpad; a.V = m->V; a.top_k = sc->want_topk ? sc->top_k : 0; a.scaling = c.logits_scaling;
            a.targets = b.targets() + r0; a.logprob = b.logprob() + r0; a.argmax = b.argmax() + r0;
            a.topk_ids = b.topk_ids() + (int64_t)r0 * a.top_k; a.topk_lp = b.topk_lp() + (int64_t)r0 * a.top_k;
            launch_logprobs(m->stream, a, n, b.part);
            NVL_HIP(hipGetLastError());
        }
        m->last_rows = 0;
        m->ctx_hint = 0;
        return M;
    }
    head_proj(m, xn_deferred, all ? nullptr : md.last_rows, rows, m->lm_head, m->logits, m->Vpad, m->V);
    if (seam & 4) {      // sampling reads the logits: apply LogitsScaling here (argmax_partial_kernel does it otherwise)
        if (c.logits_scaling != 0.f) {
            KScope ks(m, KC_OTHER);
            hipLaunchKernelGGL(scale_rows_kernel, dim3(cdiv(m->V, 256), rows), dim3(256), 0, m->stream, m->logits, m->Vpad, m->V,
                               c.logits_scaling);
            NVL_HIP(hipGetLastError());
        }
    } else {
        KScope ks(m, KC_OTHER, 0, KS_ARGMAX, (double)rows * m->V * 4.0);
        launch_argmax(m->stream, m->logits, m->Vpad, m->V, rows, c.logits_scaling, m->argmax_pval, m->argmax_pidx,
                      (seam & 2) ? nullptr : m->argmax_dev);
        NVL_HIP(hipGetLastError());
    }
    m->last_rows = rows;
    m->ctx_hint = 0;
    return rows;
}

// after a decode step: feed the greedy tokens back as the next step's inputs and advance every position by one
// (cmd/ask/main.go:315-320: allTokens = append(allTokens, nextToken); ForwardWithCache([last], kv, len-1))
__global__ void advance_decode_kernel(const int32_t* __restrict__ argmax, int32_t* __restrict__ tokens,
                                      int32_t* __restrict__ tok_pos, int32_t* __restrict__ seq_pos,
                                      int32_t* __restrict__ out_step, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = argmax[i];
    out_step[i] = t;
    tokens[i] = t;
    tok_pos[i] += 1;
    seq_pos[i] += 1;
}
}  // namespace

namespace {
// what nvl_score / nvl_score_paged return instead of logits: host pointers, [sum(seq_lens)] rows (any may be NULL)
struct ScoreOut { const int32_t* targets; int top_k; float* logprob; int32_t* argmax; int32_t* topk_ids; float* topk_lp; };
// before the pass: refusals, device room, targets upload.  Returns NVL_OK or the refusal (m->err set).
int score_prepare(nvl_model* m, const ScoreOut& so, int M, const char* who) {
    if (m->tp > 1 || m->tp_force) return fail(m, NVL_ERR_STATE, std::string(who) + ": tensor-parallel models are not supported");
    if (so.top_k < 0 || so.top_k > LOGPROB_MAX_K) return fail(m, NVL_ERR_INVALID, std::string(who) + ": top_k outside [0, 8]");
    if (!so.targets) return fail(m, NVL_ERR_INVALID, std::string(who) + ": null targets");
    for (int i = 0; i < M; i++)
        if (so.targets[i] < -1 || so.targets[i] >= m->V) return fail(m, NVL_ERR_INVALID, std::string(who) + ": target id outside [-1, V)");
    reserve_logprob_bufs(m->lpb, std::min(M, g_score_rows), M, m->V);
    NVL_HIP(hipMemcpyAsync(m->lpb.targets(), so.targets, (size_t)M * 4, hipMemcpyHostToDevice, m->stream));
    return NVL_OK;
}
// after the pass is enqueued: the per-row results to the host (the caller synchronises the stream)
void score_download(nvl_model* m, const ScoreOut& so, int M) {
    const LogprobBufs& b = m->lpb;
    if (so.logprob) NVL_HIP(hipMemcpyAsync(so.logprob, b.logprob(), (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
    if (so.argmax) NVL_HIP(hipMemcpyAsync(so.argmax, b.argmax(), (size_t)M * 4, hipMemcpyDeviceToHost, m->stream));
    if (so.top_k > 0 && so.topk_ids) NVL_HIP(hipMemcpyAsync(so.topk_ids, b.topk_ids(), (size_t)M * so.top_k * 4, hipMemcpyDeviceToHost, m->stream));
    if (so.top_k > 0 && so.topk_lp) NVL_HIP(hipMemcpyAsync(so.topk_lp, b.topk_lp(), (size_t)M * so.top_k * 4, hipMemcpyDeviceToHost, m->stream));
}

// ---- the batch planner: every entry point validates its batch and fills meta_host here ----------------------------------
// A batch is n_seqs sequences whose token rows lie back to back in `tokens` (M rows in all): lens[i] rows each, or S rows
// each when lens == NULL.  `need` more positions must fit every sequence (lens[i] when lens != NULL).
// ORDER OF THE CHECKS (the one place that states it).  Paged mode first refuses table_offsets[0] < 0.  Then sequence by
// sequence, i ascending, the first defect of the first defective sequence is reported:
//   slab:   unknown sequence -> duplicate of an earlier sequence -> pos_offset != cached length (nvl_forward only)
//   paged:  negative position
//   both:   position + need beyond max_seq_len
//   paged:  table_offsets decreasing -> block table too short -> block table too long -> block id out of range
//   both:   token id outside [0, V), row by row
// Nothing but meta_host (scratch of the call) is written: a refused call leaves every length, tick and draft record alone.
struct Batch {
    const char* who; int n_seqs, M; const int32_t* tokens; const int32_t* lens; int S, need;
    static Batch uniform(const char* who, int n_seqs, const int32_t* tokens, int S, int need) { return {who, n_seqs, n_seqs * S, tokens, nullptr, S, need}; }
    static Batch ragged(const char* who, int n_seqs, int M, const int32_t* tokens, const int32_t* lens) { return {who, n_seqs, M, tokens, lens, 0, 0}; }
    int rows(int i) const { return lens ? lens[i] : S; }
    int fit(int i) const { return lens ? lens[i] : need; }
};
int refuse(nvl_model* m, const Batch& b, int code, const char* what) { return fail(m, code, std::string(b.who) + ": " + what); }
// what both front ends end in: sequence i's rows, starting at row t, positions pos .., block-table row at blk_table + tbl
int plan_rows(nvl_model* m, const Batch& b, const Meta& hm, int i, int& t, int pos, int tbl) {
    const int n = b.rows(i);
    hm.seq_tok_start[i] = t; hm.seq_len[i] = n; hm.seq_pos[i] = pos; hm.seq_tbl[i] = tbl;
    for (int j = 0; j < n; j++, t++) {
        const int tok = b.tokens[t];
        if (tok < 0 || tok >= m->V) return refuse(m, b, NVL_ERR_INVALID, "token id out of range");
        hm.tokens[t] = tok; hm.tok_pos[t] = pos + j; hm.tok_tbl[t] = tbl;
    }
    hm.last_rows[i] = t - 1;
    return NVL_OK;
}
// slab front end: seq_ids -> h_slot; positions are the cached lengths, which pos_offsets (nvl_forward, else NULL) must equal.
// `limit`: max_seq_len, or the smaller one of a target / draft pair.  The sequence's block table is the one entry
// blk_table[i] = its slot (blocks_per_seq == 1 here).
int plan_slab(nvl_model* m, const Batch& b, const int64_t* seq_ids, const int32_t* pos_offsets, std::vector<int>& h_slot, int limit) {
    const Meta hm = bind_meta(m, m->meta_host, b.M);
    h_slot.resize((size_t)b.n_seqs);
    for (int i = 0, t = 0; i < b.n_seqs; i++) {
        auto it = m->seq_slot.find(seq_ids[i]);
        if (it == m->seq_slot.end()) return refuse(m, b, NVL_ERR_UNKNOWN_SEQ, "sequence has no KV slot (nvl_seq_open first)");
        for (int j = 0; j < i; j++) if (seq_ids[j] == seq_ids[i]) return refuse(m, b, NVL_ERR_INVALID, "duplicate sequence in batch");
        const int slot = it->second, pos = m->slot_len[(size_t)slot];
        if (pos_offsets && pos_offsets[i] != pos) return refuse(m, b, NVL_ERR_INVALID, "pos_offset does not equal the cached length");
        if (pos > limit - b.fit(i))   // rope.go:84-86 / :176-178 panic
            return refuse(m, b, NVL_ERR_POSITION, "position exceeds max_seq_len");
        h_slot[(size_t)i] = slot; hm.blk_table[i] = slot;
        if (const int rc = plan_rows(m, b, hm, i, t, pos, i)) return rc;
    }
    return NVL_OK;
}
// paged front end: the caller's positions and block tables (table i = block_tables[table_offsets[i] .. table_offsets[i+1])),
// which must cover position + need
int plan_paged(nvl_model* m, const Batch& b, const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets) {
    const Meta hm = bind_meta(m, m->meta_host, b.M);
    if (table_offsets[0] < 0) return refuse(m, b, NVL_ERR_INVALID, "negative table offset");
    for (int i = 0, t = 0; i < b.n_seqs; i++) {
        const int pos = pos_offsets[i];
        if (pos < 0) return refuse(m, b, NVL_ERR_INVALID, "negative position");
        if (pos > m->cfg.max_seq_len - b.fit(i))      // (written so that the sum cannot overflow)
            return refuse(m, b, NVL_ERR_POSITION, "position exceeds max_seq_len");
        if (table_offsets[i + 1] < table_offsets[i]) return refuse(m, b, NVL_ERR_INVALID, "table_offsets must be non-decreasing");
        const int nb = table_offsets[i + 1] - table_offsets[i];
        if (nb < cdiv(pos + b.fit(i), m->Tmax)) return refuse(m, b, NVL_ERR_INVALID, "block table shorter than the positions it must cover");
        if (nb > m->blocks_per_seq) return refuse(m, b, NVL_ERR_INVALID, "block table too long");
        const int tb = i * m->blocks_per_seq;                      // fixed stride: the kernels index blk_table[seq][block]
        for (int j = 0; j < nb; j++) {
            const int blk = block_tables[table_offsets[i] + j];
            if (blk < 0 || blk >= m->num_blocks) return refuse(m, b, NVL_ERR_INVALID, "block id out of range");
            hm.blk_table[tb + j] = blk;
        }
        if (const int rc = plan_rows(m, b, hm, i, t, pos, tb)) return rc;
    }
    return NVL_OK;
}
// A planned pass's attention cost, `step` positions on (decode_loop: step s of one row per sequence): 4*hd FLOPs per (query,
// visible key) pair per head -> returned; cached + new keys of the batch -> kv_tok; the longest context -> ctx_hint.
double attn_cost(nvl_model* m, const Meta& hm, int n_seqs, int step = 0) {
    double attn_flops = 0, kv_tok = 0;
    for (int i = 0; i < n_seqs; i++) {
        const double s = hm.seq_len[i], p0 = hm.seq_pos[i] + step;
        attn_flops += 4.0 * m->hd * m->nH * (s * p0 + s * (s + 1) / 2);
        m->ctx_hint = std::max(m->ctx_hint, hm.seq_pos[i] + step + hm.seq_len[i]);
        kv_tok += p0 + s;
    }
    m->kv_tok = kv_tok;
    return attn_flops;
}
// after a slab pass: sequence i's cache grew by rows(i)
template <typename F>
void advance_slots(nvl_model* m, const std::vector<int>& h_slot, F rows) {
    for (size_t i = 0; i < h_slot.size(); i++) { m->slot_len[(size_t)h_slot[i]] += rows((int)i); m->slot_tick[(size_t)h_slot[i]] = ++m->tick; }
}
// the rows of a ragged batch: NVL_OK and M / the longest sequence / whether any has more than one row, or the refusal
int count_rows(nvl_model* m, const char* who, int n_seqs, const int32_t* seq_lens, int& M, int& max_len, bool& prefill) {
    int64_t M64 = 0;
    max_len = 0; prefill = false;
    for (int i = 0; i < n_seqs; i++) {
        if (seq_lens[i] <= 0) return fail(m, NVL_ERR_INVALID, std::string(who) + ": empty sequence");
        M64 += seq_lens[i]; max_len = std::max(max_len, seq_lens[i]);
        if (seq_lens[i] > 1) prefill = true;
    }
    if (M64 > m->opts.max_batch_tokens) return fail(m, NVL_ERR_INVALID, std::string(who) + ": batch exceeds max_batch_tokens");
    M = (int)M64;
    return NVL_OK;
}

// nvl_forward, and nvl_score when `so` != NULL (the same validation, KV append and state update; flags then carry
// NVL_FWD_ALL_LOGITS and logits_out / argmax_out are NULL)
int forward_slab(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens,
                 const int32_t* seq_lens, const int32_t* pos_offsets, uint32_t flags,
                 float* logits_out, int32_t* argmax_out, const ScoreOut* so) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_forward: model not finalized");
    if (n_seqs <= 0 || !seq_ids || !tokens || !seq_lens || !pos_offsets)
        return fail(m, NVL_ERR_INVALID, "nvl_forward: null/empty arguments");
    if (n_seqs > m->opts.max_seqs) return fail(m, NVL_ERR_INVALID, "nvl_forward: n_seqs exceeds max_seqs");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    // ---- validate + build metadata -------------------------------------------------------
    int M = 0, max_len = 0; bool prefill = false;
    if (const int rc = count_rows(m, "nvl_forward", n_seqs, seq_lens, M, max_len, prefill)) return rc;
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_forward: the model is in paged-KV mode (use nvl_forward_paged)");
    std::vector<int> h_slot;
    if (const int rc = plan_slab(m, Batch::ragged("nvl_forward", n_seqs, M, tokens, seq_lens), seq_ids, pos_offsets, h_slot, m->cfg.max_seq_len)) return rc;
    const Meta hm = bind_meta(m, m->meta_host, M);
    const ScoreReq sreq{so ? so->top_k : 0, so && so->top_k > 0 && (so->topk_ids || so->topk_lp)};
    if (so) { const int rc = score_prepare(m, *so, M, "nvl_score"); if (rc) return rc; }
    const Meta md = bind_meta(m, m->meta_dev, M);
    NVL_HIP(hipEventRecord(m->ev0, m->stream));
    const double attn_flops = attn_cost(m, hm, n_seqs);
    const bool all = (flags & NVL_FWD_ALL_LOGITS) != 0;
    int rows = all ? M : n_seqs;
    std::vector<int32_t> am;
    const int32_t* am_p = nullptr;
    bool replayed = false;
    if (!so && !prefill && rows <= m->logit_rows) {
        // a decode pass (what TensorModelRunner.Run issues every step): metadata upload + all launches + the argmax
        // download as ONE graph launch once this configuration has been seen
        const std::array<int, 5> key{0, n_seqs, decode_attn_waves(m, n_seqs), (int)flags, g_tune_epoch};
        replayed = replay_or_capture(m, key, [&] {
            NVL_HIP(hipMemcpyAsync(m->meta_dev, m->meta_host, meta_bytes(m, M), hipMemcpyHostToDevice, m->stream));
            enqueue_forward(m, md, n_seqs, M, max_len, attn_flops, flags);
            NVL_HIP(hipMemcpyAsync(m->am_host, m->argmax_dev, (size_t)rows * 4, hipMemcpyDeviceToHost, m->stream));
        });
        if (replayed) { am_p = m->am_host; m->ctx_hint = 0; }
    }
    if (!replayed) {
        NVL_HIP(hipMemcpyAsync(m->meta_dev, m->meta_host, meta_bytes(m, M), hipMemcpyHostToDevice, m->stream));
        rows = enqueue_forward(m, md, n_seqs, M, max_len, attn_flops, flags, 0, so ? &sreq : nullptr);
        am.resize((size_t)rows);
        if (!so) NVL_HIP(hipMemcpyAsync(am.data(), m->argmax_dev, (size_t)rows * 4, hipMemcpyDeviceToHost, m->stream));
        am_p = am.data();
    }
    NVL_HIP(hipEventRecord(m->ev1, m->stream));
    if (so) score_download(m, *so, M);
    if (logits_out)
        NVL_HIP(hipMemcpy2DAsync(logits_out, (size_t)m->V * 4, m->logits, (size_t)m->Vpad * 4, (size_t)m->V * 4,
                                 (size_t)rows, hipMemcpyDeviceToHost, m->stream));
    NVL_HIP(hipStreamSynchronize(m->stream));
    reap_graphs(m);
    p2p_check(m);
    m->last_rows = so ? 0 : rows;        // (a scoring pass leaves no logits rows: nvl_sample / nvl_logprobs are refused after it)
    if (argmax_out) {
        if (all) for (int i = 0; i < n_seqs; i++) argmax_out[i] = am_p[(size_t)hm.last_rows[i]];
        else for (int i = 0; i < n_seqs; i++) argmax_out[i] = am_p[(size_t)i];
    }
    advance_slots(m, h_slot, [&](int i) { return seq_lens[i]; });
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, m->ev0, m->ev1);
    m->stats.forward_calls++;
    if (prefill) { m->stats.prefill_tokens += (uint64_t)M; m->stats.prefill_ms += ms; }
    else { m->stats.decode_tokens += (uint64_t)M; m->stats.decode_ms += ms; }
    if (m->profile) drain_profile(m);
    return NVL_OK;
    NVL_CATCH(m)
}
}  // namespace

extern "C" int nvl_forward(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens,
                           const int32_t* seq_lens, const int32_t* pos_offsets, uint32_t flags,
                           float* logits_out, int32_t* argmax_out) {
    return forward_slab(m, n_seqs, seq_ids, tokens, seq_lens, pos_offsets, flags, logits_out, argmax_out, nullptr);
}
// nvl_forward returning per NEW token row its target's log-probability, the greedy id and the top-k instead of logits
// (the checks and their messages are nvl_forward's own)
extern "C" int nvl_score(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, const int32_t* seq_lens,
                         const int32_t* pos_offsets, const int32_t* targets, int top_k, float* logprob_out,
                         int32_t* argmax_out, int32_t* topk_ids_out, float* topk_logprob_out) {
    const ScoreOut so{targets, top_k, logprob_out, argmax_out, topk_ids_out, topk_logprob_out};
    return forward_slab(m, n_seqs, seq_ids, tokens, seq_lens, pos_offsets, NVL_FWD_ALL_LOGITS, nullptr, nullptr, &so);
}

// nvl_forward for a model whose KV cache is the host block manager's pool (block_manager.go:128-263,
// sequence.go:22-23): no per-sequence state here, the block tables say where every position lives.
namespace {
int forward_paged_impl(nvl_model* m, int n_seqs, const int32_t* tokens, const int32_t* seq_lens,
                       const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets,
                       uint32_t flags, float* logits_out, int32_t* argmax_out, const ScoreOut* so) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_forward_paged: model not finalized");
    if (!m->paged) return fail(m, NVL_ERR_STATE, "nvl_forward_paged: the model was created without kv_num_blocks");
    if (n_seqs <= 0 || !tokens || !seq_lens || !pos_offsets || !block_tables || !table_offsets)
        return fail(m, NVL_ERR_INVALID, "nvl_forward_paged: null/empty arguments");
    if (n_seqs > m->opts.max_seqs) return fail(m, NVL_ERR_INVALID, "nvl_forward_paged: n_seqs exceeds max_seqs");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    int M = 0, max_len = 0; bool prefill = false;
    if (const int rc = count_rows(m, "nvl_forward_paged", n_seqs, seq_lens, M, max_len, prefill)) return rc;
    if (const int rc = plan_paged(m, Batch::ragged("nvl_forward_paged", n_seqs, M, tokens, seq_lens), pos_offsets, block_tables, table_offsets)) return rc;
    const Meta hm = bind_meta(m, m->meta_host, M);
    const ScoreReq sreq{so ? so->top_k : 0, so && so->top_k > 0 && (so->topk_ids || so->topk_lp)};
    if (so) { const int rc = score_prepare(m, *so, M, "nvl_score_paged"); if (rc) return rc; }
    const Meta md = bind_meta(m, m->meta_dev, M);
    NVL_HIP(hipEventRecord(m->ev0, m->stream));
    NVL_HIP(hipMemcpyAsync(m->meta_dev, m->meta_host, meta_bytes(m, M), hipMemcpyHostToDevice, m->stream));
    const double attn_flops = attn_cost(m, hm, n_seqs);
    const bool all = (flags & NVL_FWD_ALL_LOGITS) != 0;
    const int rows = enqueue_forward(m, md, n_seqs, M, max_len, attn_flops, flags, 0, so ? &sreq : nullptr);
    NVL_HIP(hipEventRecord(m->ev1, m->stream));
    std::vector<int32_t> am((size_t)rows);
    if (so) score_download(m, *so, M);
    else NVL_HIP(hipMemcpyAsync(am.data(), m->argmax_dev, (size_t)rows * 4, hipMemcpyDeviceToHost, m->stream));
    if (logits_out)
        NVL_HIP(hipMemcpy2DAsync(logits_out, (size_t)m->V * 4, m->logits, (size_t)m->Vpad * 4, (size_t)m->V * 4,
                                 (size_t)rows, hipMemcpyDeviceToHost, m->stream));
    NVL_HIP(hipStreamSynchronize(m->stream));
    if (argmax_out) {
        if (all) for (int i = 0; i < n_seqs; i++) argmax_out[i] = am[(size_t)hm.last_rows[i]];
        else for (int i = 0; i < n_seqs; i++) argmax_out[i] = am[(size_t)i];
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, m->ev0, m->ev1);
    m->stats.forward_calls++;
    if (prefill) { m->stats.prefill_tokens += (uint64_t)M; m->stats.prefill_ms += ms; }
    else { m->stats.decode_tokens += (uint64_t)M; m->stats.decode_ms += ms; }
    if (m->profile) drain_profile(m);
    return NVL_OK;
    NVL_CATCH(m)
}
}  // namespace

extern "C" int nvl_forward_paged(nvl_model* m, int n_seqs, const int32_t* tokens, const int32_t* seq_lens,
                                 const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets,
                                 uint32_t flags, float* logits_out, int32_t* argmax_out) {
    return forward_paged_impl(m, n_seqs, tokens, seq_lens, pos_offsets, block_tables, table_offsets, flags, logits_out, argmax_out, nullptr);
}
extern "C" int nvl_score_paged(nvl_model* m, int n_seqs, const int32_t* tokens, const int32_t* seq_lens,
                               const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets,
                               const int32_t* targets, int top_k, float* logprob_out, int32_t* argmax_out,
                               int32_t* topk_ids_out, float* topk_logprob_out) {
    const ScoreOut so{targets, top_k, logprob_out, argmax_out, topk_ids_out, topk_logprob_out};
    return forward_paged_impl(m, n_seqs, tokens, seq_lens, pos_offsets, block_tables, table_offsets, NVL_FWD_ALL_LOGITS, nullptr, nullptr, &so);
}

// ModelRunner.Run over block tables: what a runner that honours Sequence.BlockTable / NumCachedTokens does
// (the reference's runners ignore both: SURVEY §2 row 17).
extern "C" int nvl_runner_run_paged(nvl_model* m, int n_seqs, const int32_t* const* token_ptrs, const int32_t* token_lens,
                                    const int32_t* num_cached_tokens, const int32_t* const* block_table_ptrs,
                                    const int32_t* block_table_lens, int is_prefill, int32_t* next_tokens,
                                    float* logits_out) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->paged) return fail(m, NVL_ERR_STATE, "nvl_runner_run_paged: the model was created without kv_num_blocks");
    if (n_seqs <= 0 || !token_ptrs || !token_lens || !block_table_ptrs || !block_table_lens || !next_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_runner_run_paged: null/empty arguments");
    NVL_TRY(m)
    const int V = m->V;
    int k = 0;
    while (k < n_seqs) {
        // pack sequences into one forward call while they fit max_seqs / max_batch_tokens
        std::vector<int32_t> toks, lens, pos, tbl, off{0};
        std::vector<int> who;
        int64_t budget = m->opts.max_batch_tokens;
        while (k < n_seqs && (int)who.size() < m->opts.max_seqs) {
            const int len = token_lens[k];
            if (len <= 0) return fail(m, NVL_ERR_INVALID, "nvl_runner_run_paged: sequence without tokens");
            int p0;
            if (is_prefill) {
                p0 = num_cached_tokens ? num_cached_tokens[k] : 0;
                if (p0 < 0 || p0 > len) return fail(m, NVL_ERR_INVALID, "nvl_runner_run_paged: num_cached_tokens outside [0, len]");
                if (p0 == len) p0 = len - 1;                 // whole prompt cached: the last token still has to produce logits
            } else {
                p0 = len - 1;                                // tensor_model_runner.go:78-80
            }
            const int n_new = len - p0;
            if (n_new > m->opts.max_batch_tokens) return fail(m, NVL_ERR_INVALID, "nvl_runner_run_paged: uncached suffix exceeds max_batch_tokens");
            if (n_new > budget) break;
            toks.insert(toks.end(), token_ptrs[k] + p0, token_ptrs[k] + len);
            lens.push_back(n_new); pos.push_back(p0);
            if (block_table_lens[k] < 0) return fail(m, NVL_ERR_INVALID, "nvl_runner_run_paged: negative block table length");
            tbl.insert(tbl.end(), block_table_ptrs[k], block_table_ptrs[k] + block_table_lens[k]);
            off.push_back((int32_t)tbl.size());
            who.push_back(k);
            budget -= n_new;
            k++;
        }
        std::vector<int32_t> out(who.size());
        std::vector<float> lg(logits_out ? who.size() * (size_t)V : 0);
        const int rc = nvl_forward_paged(m, (int)who.size(), toks.data(), lens.data(), pos.data(), tbl.data(), off.data(), 0,
                                         logits_out ? lg.data() : nullptr, out.data());
        if (rc) return rc;
        for (size_t j = 0; j < who.size(); j++) {
            next_tokens[who[j]] = out[j];
            if (logits_out) memcpy(logits_out + (size_t)who[j] * V, &lg[j * (size_t)V], (size_t)V * 4);
        }
    }
    return NVL_OK;
    NVL_CATCH(m)
}

namespace {
// the sampler's arguments over the device-kept histories (rows of m->samp_hist, max_seq_len ids each), drawing from `uniforms`;
// the caller adds what only its form of sample_row_kernel reads
SampleArgs sample_args(const nvl_model* m, const float* uniforms) {
    SampleArgs a{};
    a.logits = m->logits; a.ld = m->Vpad; a.work = m->samp.work; a.cnt = m->samp.cnt; a.hist = m->samp_hist;
    a.hist_off = nullptr; a.hist_stride = m->cfg.max_seq_len; a.hist_len = m->samp_hist_len;
    a.uniforms = uniforms; a.out = m->samp.out; a.probs_out = nullptr; a.ldp = m->V; a.V = m->V;
    return a;
}
// the n_steps decode passes of nvl_decode_greedy[_paged]: metadata for step 0 is in meta_host (one token per sequence),
// every later step's tokens / positions are produced on the device
// `sp` != NULL: every step samples (tensor.SampleWithHistory, sample.h) instead of taking the argmax; the histories live
// on the device (m->samp_hist, one row of max_seq_len ids per sequence) and grow by the sampled token each step;
// `uniforms_dev` is [n_steps][n_seqs]; `keep` (nvl_draft_sampled, or NULL) receives every step's final distribution,
// [n_steps][n_seqs][round_up(V, 4)]
void decode_loop(nvl_model* m, const Meta& hm, int n_seqs, int n_steps, int32_t* out_tokens,
                 const nvl_sampling_params* sp = nullptr, const float* uniforms_dev = nullptr, float* keep = nullptr) {
    const int M = n_seqs;
    const int32_t* h_pos = hm.seq_pos;
    const Meta md = bind_meta(m, m->meta_dev, M);
    if ((int64_t)n_steps * n_seqs > m->ring_ints) {
        clear_graphs(m);      // the fused loop's captured steps hold the old ring address as a kernel argument
        dfree(m->ring);
        m->ring_ints = (int64_t)n_steps * n_seqs;
        m->ring = dmalloc<int32_t>(m->ring_ints);
    }
    NVL_HIP(hipEventRecord(m->ev0, m->stream));
    NVL_HIP(hipMemcpyAsync(m->meta_dev, m->meta_host, meta_bytes(m, M), hipMemcpyHostToDevice, m->stream));
    NVL_HIP(hipMemcpyAsync(m->ring_pos0, h_pos, (size_t)n_seqs * 4, hipMemcpyHostToDevice, m->stream));   // (pinned meta_host)
    const bool dbg = m->keep_hidden, dbg_tap = m->tap;
    m->keep_hidden = false; m->tap = false;      // the per-layer taps belong to single nvl_forward calls
    for (int s = 0; s < n_steps; s++) {
        const double attn_flops = attn_cost(m, hm, n_seqs, s);
        // bf16 path: the step's tail (argmax, token feedback) and the next step's head (embedding gather + layer 0's
        // norm) are one launch (decode_seam_kernel); fp32 parity mode keeps the separate kernels
        const bool seam_ok = (g_decode_seam || sp) && !m->f32 && m->H <= 1024 * NORM_ROW_MAXCH && m->H % 4 == 0;
        if (sp && !seam_ok) throw std::runtime_error("sampled decode loop: bf16 models only");
        auto one_step = [&] {
        enqueue_forward(m, md, n_seqs, M, 1, attn_flops, 0, seam_ok ? ((s > 0 ? 1 : 0) | (sp ? 4 : 2)) : 0);
        if (sp) {
            SampleArgs a = sample_args(m, uniforms_dev + (int64_t)s * n_seqs);
            if (keep) { a.ldp = round_up(m->V, 4); a.probs_out = keep + (int64_t)s * n_seqs * a.ldp; }
            a.top_k = sp->top_k; a.temperature = sp->temperature; a.top_p = sp->top_p; a.rep_penalty = sp->repetition_penalty;
            hipLaunchKernelGGL(sample_row_kernel<false>, dim3(n_seqs), dim3(SAMPLE_THREADS), 0, m->stream, a);
            NVL_HIP(hipGetLastError());
        }
        if (seam_ok) {
            const void* pe = (m->cfg.position_type == NVL_POS_LEARNED) ? m->g[NVL_T_POS_EMB].p : nullptr;
            const int pe_rows = pe ? (int)std::min<int64_t>(m->g[NVL_T_POS_EMB].rows, m->cfg.max_seq_len) : 0;
            const LayerW& l0 = m->layers[0];
            if (m->g[NVL_T_TOK_EMB].wf == WF_MXFP4)     // MXFP4 tied embedding table (w4.h)
                hipLaunchKernelGGL(decode_seam_w4_kernel, dim3(n_seqs), dim3(256), 0, m->stream, m->argmax_pval, m->argmax_pidx,
                                   cdiv(m->V, ARGMAX_CHUNK), sp ? (const int32_t*)m->samp.out : (const int32_t*)nullptr, m->samp_hist,
                                   (int64_t)m->cfg.max_seq_len, m->samp_hist_len, m->argmax_dev, m->ring, (const int32_t*)m->ring_pos0, n_seqs,
                                   md.tokens, md.tok_pos,
                                   md.seq_pos, (const uint8_t*)m->g[NVL_T_TOK_EMB].p, (const uint8_t*)m->g[NVL_T_TOK_EMB].qs, (const bf16_t*)pe, pe_rows,
                                   m->cfg.embedding_multiplier, m->x, (const float*)l0.t[NVL_T_ATTN_NORM_W].p,
                                   (const float*)l0.t[NVL_T_ATTN_NORM_B].p, m->cfg.norm_eps, (bf16_t*)m->xn, m->H);
            else if (m->g[NVL_T_TOK_EMB].qs)     // 8-bit tied embedding table (w8.h)
                hipLaunchKernelGGL(decode_seam_w8_kernel, dim3(n_seqs), dim3(256), 0, m->stream, m->argmax_pval, m->argmax_pidx,
                                   cdiv(m->V, ARGMAX_CHUNK), sp ? (const int32_t*)m->samp.out : (const int32_t*)nullptr, m->samp_hist,
                                   (int64_t)m->cfg.max_seq_len, m->samp_hist_len, m->argmax_dev, m->ring, (const int32_t*)m->ring_pos0, n_seqs,
                                   md.tokens, md.tok_pos,
                                   md.seq_pos, (const uint8_t*)m->g[NVL_T_TOK_EMB].p, (const float*)m->g[NVL_T_TOK_EMB].qs, (const bf16_t*)pe, pe_rows,
                                   m->cfg.embedding_multiplier, m->x, (const float*)l0.t[NVL_T_ATTN_NORM_W].p,
                                   (const float*)l0.t[NVL_T_ATTN_NORM_B].p, m->cfg.norm_eps, (bf16_t*)m->xn, m->H);
            else
                hipLaunchKernelGGL(decode_seam_kernel, dim3(n_seqs), dim3(256), 0, m->stream, m->argmax_pval, m->argmax_pidx,
                                   cdiv(m->V, ARGMAX_CHUNK), sp ? (const int32_t*)m->samp.out : (const int32_t*)nullptr, m->samp_hist,
                                   (int64_t)m->cfg.max_seq_len, m->samp_hist_len, m->argmax_dev, m->ring, (const int32_t*)m->ring_pos0, n_seqs,
                                   md.tokens, md.tok_pos,
                                   md.seq_pos, (const bf16_t*)m->g[NVL_T_TOK_EMB].p, (const bf16_t*)pe, pe_rows,
                                   m->cfg.embedding_multiplier, m->x, (const float*)l0.t[NVL_T_ATTN_NORM_W].p,
                                   (const float*)l0.t[NVL_T_ATTN_NORM_B].p, m->cfg.norm_eps, (bf16_t*)m->xn, m->H);
        } else {
            hipLaunchKernelGGL(advance_decode_kernel, dim3(cdiv(n_seqs, 256)), dim3(256), 0, m->stream, m->argmax_dev, md.tokens,
                               md.tok_pos, md.seq_pos, m->ring + (int64_t)s * n_seqs, n_seqs);
        }
        NVL_HIP(hipGetLastError());
        };
        // steps 1.. of the greedy seam loop launch the SAME kernels with the SAME arguments (the ring row comes from the
        // positions): one captured graph per (batch, attention wave count), replayed
        bool replayed = false;
        if (s > 0 && seam_ok && !sp) {
            const std::array<int, 5> key{1, n_seqs, decode_attn_waves(m, n_seqs), 0, g_tune_epoch};
            replayed = replay_or_capture(m, key, one_step);
            if (replayed) m->ctx_hint = 0;
        }
        if (!replayed) one_step();
    }
    m->keep_hidden = dbg; m->tap = dbg_tap;
    NVL_HIP(hipEventRecord(m->ev1, m->stream));
    NVL_HIP(hipMemcpyAsync(out_tokens, m->ring, (size_t)n_steps * n_seqs * 4, hipMemcpyDeviceToHost, m->stream));
    NVL_HIP(hipStreamSynchronize(m->stream));
    reap_graphs(m);
    p2p_check(m);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, m->ev0, m->ev1);
    m->stats.forward_calls += (uint64_t)n_steps;
    m->stats.decode_tokens += (uint64_t)n_steps * n_seqs; m->stats.decode_ms += ms;
    if (m->profile) drain_profile(m);
}
}  // namespace

// The greedy decode loop of cmd/ask (main.go:315-360, without the EOS stop) as ONE call: `n_steps` forward passes of one
// token per sequence, each step's argmax fed back on the device — no host round trip between steps.  Identical
// arithmetic to calling nvl_forward n_steps times with the returned tokens.
extern "C" int nvl_decode_greedy(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens,
                                 int n_steps, int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_decode_greedy: model not finalized");
    if (n_seqs <= 0 || n_steps <= 0 || !seq_ids || !first_tokens || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy: null/empty arguments");
    if (n_seqs > m->opts.max_seqs || n_seqs > m->opts.max_batch_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy: n_seqs exceeds max_seqs / max_batch_tokens");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_decode_greedy: not available in paged-KV mode");
    std::vector<int> h_slot;
    if (const int rc = plan_slab(m, Batch::uniform("nvl_decode_greedy", n_seqs, first_tokens, 1, n_steps), seq_ids, nullptr, h_slot, m->cfg.max_seq_len)) return rc;
    const Meta hm = bind_meta(m, m->meta_host, n_seqs);
    decode_loop(m, hm, n_seqs, n_steps, out_tokens);
    advance_slots(m, h_slot, [&](int) { return n_steps; });
    return NVL_OK;
    NVL_CATCH(m)
}

// nvl_decode_greedy for a paged-KV model: positions[i] tokens are cached (the sequence length before the first
// generated token is appended); the block tables must already cover positions[i] + n_steps tokens (the host's block
// manager allocates ahead: BlockManager.MayAppend per step, block_manager.go:231-263).
extern "C" int nvl_decode_greedy_paged(nvl_model* m, int n_seqs, const int32_t* first_tokens, const int32_t* positions,
                                       int n_steps, const int32_t* block_tables, const int32_t* table_offsets,
                                       int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_decode_greedy_paged: model not finalized");
    if (!m->paged) return fail(m, NVL_ERR_STATE, "nvl_decode_greedy_paged: the model was created without kv_num_blocks");
    if (n_seqs <= 0 || n_steps <= 0 || !first_tokens || !positions || !block_tables || !table_offsets || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy_paged: null/empty arguments");
    if (n_seqs > m->opts.max_seqs || n_seqs > m->opts.max_batch_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy_paged: n_seqs exceeds max_seqs / max_batch_tokens");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    if (const int rc = plan_paged(m, Batch::uniform("nvl_decode_greedy_paged", n_seqs, first_tokens, 1, n_steps), positions, block_tables, table_offsets)) return rc;
    const Meta hm = bind_meta(m, m->meta_host, n_seqs);
    decode_loop(m, hm, n_seqs, n_steps, out_tokens);
    return NVL_OK;
    NVL_CATCH(m)
}

// =================================================================================================
// greedy speculative decoding: verify 1 + k rows per sequence in one pass, accept on the device, roll the cache back
// =================================================================================================
namespace {
// per sequence i: g = the pass's greedy ids of its 1 + k rows, t = its input rows (t[0] the next input token, t[1..k] the
// draft).  a = the longest prefix with t[j+1] == g[j]; res = [a: n | out_tokens: n x (1+k)], out_tokens[i][0..a] = g, the rest -1.
__global__ void verify_accept_kernel(const int32_t* __restrict__ argmax, const int32_t* __restrict__ tokens, int k, int n,
                                     int32_t* __restrict__ res) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int S = 1 + k;
    const int32_t* g = argmax + (int64_t)i * S;
    const int32_t* t = tokens + (int64_t)i * S;
    int a = 0;
    while (a < k && t[a + 1] == g[a]) a++;
    res[i] = a;
    int32_t* o = res + n + (int64_t)i * S;
    for (int j = 0; j < S; j++) o[j] = j <= a ? g[j] : -1;
}

// The sampled twin: s = the ids sample_row_kernel<true> drew for the pass's rows; same rule, same result
// layout.  hist != NULL (nvl_decode_sampled_lookup): sequence i's history is row hist_row[i] of the device history buffer;
// the kernel appends s[0 .. min(a, keep[i] - 1)], the tokens the loop emits, and advances the length, so the next pass
// finds the history current and uploads only drafts and draws.
__global__ void verify_accept_sampled_kernel(const int32_t* __restrict__ s, const int32_t* __restrict__ tokens, int k, int n,
                                             int32_t* __restrict__ res, int32_t* __restrict__ hist, int64_t hist_stride,
                                             int32_t* __restrict__ hist_len, const int32_t* __restrict__ hist_row,
                                             const int32_t* __restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int S = 1 + k;
    const int32_t* g = s + (int64_t)i * S;
    const int32_t* t = tokens + (int64_t)i * S;
    int a = 0;
    while (a < k && t[a + 1] == g[a]) a++;
    res[i] = a;
    int32_t* o = res + n + (int64_t)i * S;
    for (int j = 0; j < S; j++) o[j] = j <= a ? g[j] : -1;
    if (hist) {
        const int h = hist_row[i], len = hist_len[h];
        const int take = min(min(a + 1, keep[i]), (int)hist_stride - len);
        for (int j = 0; j < take; j++) hist[(int64_t)h * hist_stride + len + j] = g[j];
        hist_len[h] = len + take;
    }
}

// What a sampled verify pass reads besides the metadata, in ONE pinned block mirrored on the device (vs_host / vs_dev):
//   [nvl_sampling_params | keep n_seqs | hist_row n_seqs | uniforms M]
// A captured pass bakes in only addresses inside the block: parameters, draws and history rows are its CONTENTS.
struct VsBlock { nvl_sampling_params* params; int32_t *keep, *hist_row; float* u; };
VsBlock bind_vs(int32_t* base, int n_seqs) {
    return VsBlock{(nvl_sampling_params*)base, base + 4, base + 4 + n_seqs, (float*)(base + 4 + 2 * n_seqs)};
}
static_assert(sizeof(nvl_sampling_params) == 16, "bind_vs layout");
// the sampled calls' arguments (SampleWithHistory per row, sampling.go:33-102)
struct SampledReq { const nvl_sampling_params* params; const int32_t* const* hist_ptrs; const int32_t* hist_lens; const float* uniforms; };
// the draft's kept distributions of a speculative pass (nvl_verify_speculative)
struct SpecReq { const float* q; int64_t ldq, q_seq, q_step; float* accept_prob_out; };
// What a verify pass is, as one value.  The factories are the only way to make one, so every value is a legal pass:
//   greedy       the argmax and verify_accept_kernel
//   sampled      ONE sampled pass (nvl_verify_sampled[_paged]): the caller's histories and draws are checked and staged, then
//                the sampler and verify_accept_sampled_kernel
//   in_loop      a pass of nvl_decode_sampled_lookup: the loop has staged the histories and filled vs_host itself, and the
//                accept kernel also appends the emitted ids to the device histories
//   speculative  `sampled` with the draft's distributions: spec_reject_kernel (spec.h) takes the accept kernel's place
// The histories are rows of m->samp_hist with lengths m->samp_hist_len in every sampled kind.
class VerifyKind {
public:
    enum Tag { GREEDY, SAMPLED, IN_LOOP, SPECULATIVE };
    static VerifyKind greedy() { return VerifyKind(GREEDY, SampledReq{}, SpecReq{}); }
    static VerifyKind sampled(const SampledReq& rq) { return VerifyKind(SAMPLED, rq, SpecReq{}); }
    static VerifyKind in_loop() { return VerifyKind(IN_LOOP, SampledReq{}, SpecReq{}); }
    static VerifyKind speculative(const SampledReq& rq, const SpecReq& spec) { return VerifyKind(SPECULATIVE, rq, spec); }
    const Tag tag; const SampledReq rq; const SpecReq spec;
    bool samples() const { return tag != GREEDY; }
    bool stages() const { return tag == SAMPLED || tag == SPECULATIVE; }      // rq is the caller's, to be checked and staged
private:
    VerifyKind(Tag t, const SampledReq& r, const SpecReq& s) : tag(t), rq(r), spec(s) {}
};

// the sampler's scratch for `rows` rows; a captured sampled pass holds these addresses
void reserve_sample_rows(nvl_model* m, int rows) {
    SampleBufs& b = m->samp;
    const int64_t elems = (int64_t)rows * round_up(m->V, 4);
    if (elems > b.elems || rows > b.rows_cap) clear_graphs(m);
    if (elems > b.elems) {
        dfree(b.work); dfree(b.cnt); b.work = nullptr; b.cnt = nullptr; b.elems = 0;
        b.work = dmalloc<float>(elems); b.cnt = dmalloc<int32_t>(elems); b.elems = elems;
        NVL_HIP(hipMemsetAsync(b.cnt, 0, (size_t)elems * 4, m->stream));
    }
    if (rows > b.rows_cap) {
        dfree(b.off); dfree(b.out); dfree(b.u); b.off = nullptr; b.out = nullptr; b.u = nullptr; b.rows_cap = 0;
        const int cap = (int)round_up(rows, 64);
        b.off = dmalloc<int32_t>(cap + 1); b.out = dmalloc<int32_t>(cap); b.u = dmalloc<float>(cap);
        b.rows_cap = cap;
    }
}
// the device-kept histories: one row of max_seq_len ids per sequence, allocated once (the address never changes)
void reserve_sample_hist(nvl_model* m) {
    if (m->samp_hist) return;
    m->samp_hist_cap = (int64_t)m->opts.max_seqs * m->cfg.max_seq_len;
    m->samp_hist = dmalloc<int32_t>(m->samp_hist_cap); m->samp_hist_len = dmalloc<int32_t>(m->opts.max_seqs);
}

// The pass itself, metadata already in meta_host (n_seqs sequences of 1 + k rows each, positions seq_pos[i] ..): upload,
// launches, accept kernel and result download — captured and replayed like a decode pass when every projection is in
// decode form (<= 64 rows) — then the host copies.  Leaves the n_seqs x (1+k) logits rows as the last forward group.
// A sampled kind finds vs_host filled and the histories on the device.
void verify_pass(nvl_model* m, int n_seqs, int k, int32_t* n_acc_out, int32_t* out_tokens, const VerifyKind& vk) {
    const int S = 1 + k, M = n_seqs * S;
    const Meta md = bind_meta(m, m->meta_dev, M);
    NVL_HIP(hipEventRecord(m->ev0, m->stream));
    const double attn_flops = attn_cost(m, bind_meta(m, m->meta_host, M), n_seqs);
    const bool spec = vk.tag == VerifyKind::SPECULATIVE;
    const bool mq = g_verify_mq && attention_mq_ok(m, S);
    const int nres = n_seqs * (1 + S);
    if (vk.samples()) reserve_sample_rows(m, M);
    auto pass = [&] {
        NVL_HIP(hipMemcpyAsync(m->meta_dev, m->meta_host, meta_bytes(m, M), hipMemcpyHostToDevice, m->stream));
        if (vk.samples()) {
            NVL_HIP(hipMemcpyAsync(m->vs_dev, m->vs_host, (size_t)(4 + 2 * n_seqs + M) * 4, hipMemcpyHostToDevice, m->stream));
            enqueue_forward(m, md, n_seqs, M, S, attn_flops, NVL_FWD_ALL_LOGITS, (mq ? 8 : 0) | 4);
            const VsBlock vs = bind_vs(m->vs_dev, n_seqs);
            SampleArgs a = sample_args(m, vs.u);
            a.ext = md.tokens; a.ext_S = S; a.hist_row = vs.hist_row; a.params = vs.params;
            hipLaunchKernelGGL(sample_row_kernel<true>, dim3(M), dim3(SAMPLE_THREADS), 0, m->stream, a);
            NVL_HIP(hipGetLastError());
            if (spec) {     // the sampler left row r's final distribution in work row r; its ids of the pass are not used
                SpecArgs r{};
                r.p = m->samp.work; r.ldp = round_up(m->V, 4); r.q = vk.spec.q; r.ldq = vk.spec.ldq; r.q_seq = vk.spec.q_seq;
                r.q_step = vk.spec.q_step; r.tokens = md.tokens; r.u = vs.u; r.res = m->verify_dev; r.accept_prob = m->spec_ap;
                r.k = k; r.V = m->V;
                KScope ks(m, KC_OTHER, 0, KS_SPEC_REJECT, (double)n_seqs * m->V * 8.0);
                hipLaunchKernelGGL(spec_reject_kernel, dim3(n_seqs), dim3(SAMPLE_THREADS), 0, m->stream, r);
            } else
            hipLaunchKernelGGL(verify_accept_sampled_kernel, dim3(cdiv(n_seqs, 64)), dim3(64), 0, m->stream, (const int32_t*)m->samp.out,
                               (const int32_t*)md.tokens, k, n_seqs, m->verify_dev, vk.tag == VerifyKind::IN_LOOP ? m->samp_hist : (int32_t*)nullptr,
                               (int64_t)m->cfg.max_seq_len, m->samp_hist_len, (const int32_t*)vs.hist_row, (const int32_t*)vs.keep);
        } else {
            enqueue_forward(m, md, n_seqs, M, S, attn_flops, NVL_FWD_ALL_LOGITS, mq ? 8 : 0);
            hipLaunchKernelGGL(verify_accept_kernel, dim3(cdiv(n_seqs, 64)), dim3(64), 0, m->stream, m->argmax_dev, md.tokens, k, n_seqs, m->verify_dev);
        }
        NVL_HIP(hipGetLastError());
        NVL_HIP(hipMemcpyAsync(m->verify_host, m->verify_dev, (size_t)nres * 4, hipMemcpyDeviceToHost, m->stream));
        if (spec && vk.spec.accept_prob_out)      // (a speculative pass is never captured: the host address is not baked in)
            NVL_HIP(hipMemcpyAsync(vk.spec.accept_prob_out, m->spec_ap, (size_t)n_seqs * k * 2 * 4, hipMemcpyDeviceToHost, m->stream));
    };
    bool replayed = false;
    if (M <= 64 && M <= m->logit_rows && !spec) {      // (a speculative pass runs eagerly: it reads another model's buffer)
        const int acfg = mq ? decode_attn_cfg(m, n_seqs, S) : (S == 1 ? decode_attn_waves(m, n_seqs) : 0);
        const std::array<int, 5> key{vk.samples() ? 4 : 3, n_seqs, acfg, k | (mq ? 256 : 0) | (vk.tag == VerifyKind::IN_LOOP ? 512 : 0), g_tune_epoch};
        replayed = replay_or_capture(m, key, pass);
    }
    if (!replayed) pass();
    m->ctx_hint = 0;
    NVL_HIP(hipEventRecord(m->ev1, m->stream));
    NVL_HIP(hipStreamSynchronize(m->stream));
    reap_graphs(m);
    m->last_rows = M;
    if (n_acc_out) memcpy(n_acc_out, m->verify_host, (size_t)n_seqs * 4);
    if (out_tokens) memcpy(out_tokens, m->verify_host + n_seqs, (size_t)M * 4);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, m->ev0, m->ev1);
    m->stats.forward_calls++;
    m->stats.decode_tokens += (uint64_t)M; m->stats.decode_ms += ms;
    if (m->profile) drain_profile(m);
}

int verify_refusals(nvl_model* m, const char* who, int n_seqs, int k, int k_min) {
    if (!m->finalized) return fail(m, NVL_ERR_STATE, std::string(who) + ": model not finalized");
    if (k < k_min || k > 7) return fail(m, NVL_ERR_INVALID, std::string(who) + ": k outside 1..7");
    if (n_seqs <= 0 || n_seqs > m->opts.max_seqs) return fail(m, NVL_ERR_INVALID, std::string(who) + ": n_seqs outside 1..max_seqs");
    if ((int64_t)n_seqs * (1 + k) > m->opts.max_batch_tokens) return fail(m, NVL_ERR_INVALID, std::string(who) + ": n_seqs x (1 + k) exceeds max_batch_tokens");
    if (m->n_mamba) return fail(m, NVL_ERR_STATE, std::string(who) + ": a Mamba2 state cannot be rolled back");
    if (m->tp > 1 || m->tp_force) return fail(m, NVL_ERR_STATE, std::string(who) + ": tensor-parallel models are not supported");
    return NVL_OK;
}

bool sampling_params_ok(const nvl_sampling_params* sp) {     // the rules of nvl_sample / nvl_decode_sampled
    return sp->repetition_penalty != 0.f && sp->repetition_penalty == sp->repetition_penalty &&
           sp->temperature == sp->temperature && sp->top_p == sp->top_p;
}
// every history present, ending with its sequence's first token of the pass, free of negative ids, and short enough that
// history + `grow` more ids fit `max_len`; `n_u` draws inside [0, 1].  `strict` = false (nvl_decode_sampled, nvl_draft_sampled):
// a history may be empty and need not end with the first token.  Pure validation.
const char* sampled_check(const SampledReq& rq, int n_seqs, const int32_t* first, int first_stride, int grow, int64_t max_len, int64_t n_u,
                          bool strict = true) {
    if (!sampling_params_ok(rq.params)) return "bad sampling parameters (NaN, or repetition_penalty 0)";
    for (int i = 0; i < n_seqs; i++) {
        const int hn = rq.hist_lens[i];
        if (hn < 0 || (hn > 0 && !rq.hist_ptrs[i]) || (strict && hn == 0)) return "a sequence has no history (it must end with the sequence's first token)";
        if ((int64_t)hn + grow > max_len) return "history longer than max_seq_len";
        if (strict && rq.hist_ptrs[i][hn - 1] != first[(int64_t)i * first_stride]) return "a history must end with its first token";
        for (int j = 0; j < hn; j++) if (rq.hist_ptrs[i][j] < 0) return "negative token id in the history";
    }
    for (int64_t i = 0; i < n_u; i++) if (!(rq.uniforms[i] >= 0.f && rq.uniforms[i] <= 1.f)) return "uniform draw outside [0, 1]";
    return nullptr;
}
// histories -> rows 0 .. n_seqs-1 of the device history buffer (the lengths go through the pinned tail of vs_host).  The
// caller's arrays must stay alive until the stream is synchronised.
void sampled_stage_histories(nvl_model* m, int n_seqs, const SampledReq& rq) {
    reserve_sample_hist(m);
    const int64_t T = m->cfg.max_seq_len;
    int32_t* hlen = m->vs_host + 4 + 2 * (int64_t)m->opts.max_seqs + m->opts.max_batch_tokens;
    for (int i = 0; i < n_seqs; i++) {
        hlen[i] = rq.hist_lens[i];
        NVL_HIP(hipMemcpyAsync(m->samp_hist + i * T, rq.hist_ptrs[i], (size_t)rq.hist_lens[i] * 4, hipMemcpyHostToDevice, m->stream));
    }
    NVL_HIP(hipMemcpyAsync(m->samp_hist_len, hlen, (size_t)n_seqs * 4, hipMemcpyHostToDevice, m->stream));
}
// a single sampled pass (nvl_verify_sampled[_paged]): stage the histories and fill the pass's block
void sampled_stage_pass(nvl_model* m, int n_seqs, int k, const SampledReq& rq) {
    sampled_stage_histories(m, n_seqs, rq);
    const int S = 1 + k;
    const VsBlock vs = bind_vs(m->vs_host, n_seqs);
    *vs.params = *rq.params;
    for (int i = 0; i < n_seqs; i++) { vs.keep[i] = S; vs.hist_row[i] = i; }
    memcpy(vs.u, rq.uniforms, (size_t)n_seqs * S * 4);
}

// where a verify pass's sequences live: KV slots of the slab (seq_ids), or the caller's block tables
struct KvRef {
    const int64_t* seq_ids; const int32_t *pos_offsets, *block_tables, *table_offsets;
    static KvRef slab(const int64_t* seq_ids) { return {seq_ids, nullptr, nullptr, nullptr}; }
    static KvRef paged(const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets) { return {nullptr, pos_offsets, block_tables, table_offsets}; }
};
// Every verify call and every pass of the three loops: k_min = 1, or 0 for a loop's last pass of one row per sequence.
// keep[i] (or NULL): at most that many of sequence i's accepted tokens stay in the cache.  A caller's histories and draws
// (vk.stages()) are checked here, after everything else, and staged.
int verify_batch(nvl_model* m, const char* who, int n_seqs, const KvRef& kv, const int32_t* tokens, int k, int k_min,
                 int32_t* n_acc_out, int32_t* out_tokens, const int* keep, const VerifyKind& vk) {
    if (const int rc = verify_refusals(m, who, n_seqs, k, k_min)) return rc;
    const bool slab = kv.seq_ids != nullptr;
    if (slab && m->paged) return fail(m, NVL_ERR_STATE, std::string(who) + ": the model is in paged-KV mode (use the _paged call)");
    if (!slab && !m->paged) return fail(m, NVL_ERR_STATE, std::string(who) + ": the model was created without kv_num_blocks");
    const int S = 1 + k, M = n_seqs * S;
    const Batch b = Batch::uniform(who, n_seqs, tokens, S, S);
    std::vector<int> h_slot;      // (stays empty in paged mode: the caller owns the lengths)
    if (const int rc = slab ? plan_slab(m, b, kv.seq_ids, nullptr, h_slot, m->cfg.max_seq_len)
                            : plan_paged(m, b, kv.pos_offsets, kv.block_tables, kv.table_offsets)) return rc;
    if (vk.stages()) {
        if (const char* why = sampled_check(vk.rq, n_seqs, tokens, S, k, m->cfg.max_seq_len, (int64_t)M)) return fail(m, NVL_ERR_INVALID, std::string(who) + ": " + why);
        if (vk.tag == VerifyKind::SPECULATIVE && !m->spec_ap) m->spec_ap = dmalloc<float>((int64_t)m->opts.max_seqs * 7 * 2);
        sampled_stage_pass(m, n_seqs, k, vk.rq);
    }
    verify_pass(m, n_seqs, k, n_acc_out, out_tokens, vk);
    // slab rollback: the accepted prefix and the row that produced the first unaccepted id stay; the rows behind are dead
    advance_slots(m, h_slot, [&](int i) { const int adv = m->verify_host[i] + 1; return keep ? std::min(adv, keep[i]) : adv; });
    return NVL_OK;
}
}  // namespace

extern "C" int nvl_verify_greedy(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                                 int32_t* n_accepted_out, int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!seq_ids || !tokens || !n_accepted_out || !out_tokens) return fail(m, NVL_ERR_INVALID, "nvl_verify_greedy: null arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    return verify_batch(m, "nvl_verify_greedy", n_seqs, KvRef::slab(seq_ids), tokens, k, 1, n_accepted_out, out_tokens, nullptr, VerifyKind::greedy());
    NVL_CATCH(m)
}

extern "C" int nvl_verify_greedy_paged(nvl_model* m, int n_seqs, const int32_t* tokens, int k, const int32_t* pos_offsets,
                                       const int32_t* block_tables, const int32_t* table_offsets, int32_t* n_accepted_out,
                                       int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!tokens || !pos_offsets || !block_tables || !table_offsets || !n_accepted_out || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_verify_greedy_paged: null arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    return verify_batch(m, "nvl_verify_greedy_paged", n_seqs, KvRef::paged(pos_offsets, block_tables, table_offsets), tokens, k, 1,
                        n_accepted_out, out_tokens, nullptr, VerifyKind::greedy());
    NVL_CATCH(m)
}

// ---- sampled speculative decoding: the verify pass under tensor.SampleWithHistory (sampling.go:33-102),
// the step every TensorModelRunner.Run ends in (tensor_model_runner.go:89-93) ----
extern "C" int nvl_verify_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                                  const nvl_sampling_params* params, const int32_t* const* history_ptrs, const int32_t* history_lens,
                                  const float* uniforms, int32_t* n_accepted_out, int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!seq_ids || !tokens || !params || !history_ptrs || !history_lens || !uniforms || !n_accepted_out || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_verify_sampled: null arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    return verify_batch(m, "nvl_verify_sampled", n_seqs, KvRef::slab(seq_ids), tokens, k, 1, n_accepted_out, out_tokens, nullptr,
                        VerifyKind::sampled({params, history_ptrs, history_lens, uniforms}));
    NVL_CATCH(m)
}

extern "C" int nvl_verify_sampled_paged(nvl_model* m, int n_seqs, const int32_t* tokens, int k, const int32_t* pos_offsets,
                                        const int32_t* block_tables, const int32_t* table_offsets,
                                        const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                        const int32_t* history_lens, const float* uniforms, int32_t* n_accepted_out,
                                        int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!tokens || !pos_offsets || !block_tables || !table_offsets || !params || !history_ptrs || !history_lens || !uniforms ||
        !n_accepted_out || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_verify_sampled_paged: null arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    return verify_batch(m, "nvl_verify_sampled_paged", n_seqs, KvRef::paged(pos_offsets, block_tables, table_offsets), tokens, k, 1,
                        n_accepted_out, out_tokens, nullptr, VerifyKind::sampled({params, history_ptrs, history_lens, uniforms}));
    NVL_CATCH(m)
}

extern "C" int nvl_seq_truncate(nvl_model* m, int64_t seq_id, int new_len) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_seq_truncate: model not finalized");
    if (m->n_mamba) return fail(m, NVL_ERR_STATE, "nvl_seq_truncate: a Mamba2 state cannot be rolled back");
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_seq_truncate: paged-KV mode keeps no lengths (the caller owns them)");
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return fail(m, NVL_ERR_UNKNOWN_SEQ, "nvl_seq_truncate: sequence has no KV slot");
    if (new_len < 0 || new_len > m->slot_len[(size_t)it->second]) return fail(m, NVL_ERR_INVALID, "nvl_seq_truncate: new_len outside [0, cached length]");
    m->slot_len[(size_t)it->second] = new_len;
    return NVL_OK;
}

// prompt-lookup drafting: pure host code, no device
extern "C" int nvl_lookup_draft(const int32_t* history, int n, int k, int ngram, int32_t* draft_out) {
    return (!history || !draft_out || n < 1 || k < 1) ? NVL_ERR_INVALID : lookup_draft(history, n, k, ngram, draft_out);
}

namespace {
// how many rows beyond the first a pass may still append to the sequence in `slot` (the lookup loops' room rule)
int cache_room(const nvl_model* m, int slot) { return m->cfg.max_seq_len - m->slot_len[(size_t)slot] - 1; }
// drafts are taken from the history and fed to the model(s): every id must be inside the vocabulary
bool history_in_vocab(const nvl_model* m, int n_seqs, const int32_t* const* history_ptrs, const int32_t* history_lens) {
    for (int i = 0; i < n_seqs; i++)
        if (history_ptrs[i])
            for (int j = 0; j < history_lens[i]; j++) if (history_ptrs[i][j] >= m->V) return false;
    return true;
}
}  // namespace

extern "C" int nvl_decode_greedy_lookup(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                                        int k, int ngram, const int32_t* const* history_ptrs, const int32_t* history_lens,
                                        int32_t* out_tokens, int32_t* passes_out) {
    if (!m) return NVL_ERR_INVALID;
    if (!seq_ids || !first_tokens || !out_tokens || n_steps <= 0 || ngram < 1 || (history_ptrs && !history_lens))
        return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy_lookup: null/empty arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    int rc = verify_refusals(m, "nvl_decode_greedy_lookup", n_seqs, k, 1);
    if (rc) return rc;
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_decode_greedy_lookup: not available in paged-KV mode");
    std::vector<int> h_slot;
    if ((rc = plan_slab(m, Batch::uniform("nvl_decode_greedy_lookup", n_seqs, first_tokens, 1, n_steps), seq_ids, nullptr, h_slot, m->cfg.max_seq_len))) return rc;
    SpecLoop loop(n_seqs, n_steps);
    for (int i = 0; i < n_seqs; i++) {
        std::vector<int32_t>& h = loop.hist[(size_t)i];
        if (history_ptrs && history_ptrs[i] && history_lens[i] > 0) {
            h.assign(history_ptrs[i], history_ptrs[i] + history_lens[i]);
            if (h.back() != first_tokens[i]) return fail(m, NVL_ERR_INVALID, "nvl_decode_greedy_lookup: a history must end with its first token");
        } else
            h.push_back(first_tokens[i]);
    }
    while (loop.plan(k, seq_ids, [&](int i) { return cache_room(m, h_slot[(size_t)i]); })) {
        loop.draft_by_lookup(ngram);
        rc = verify_batch(m, "nvl_decode_greedy_lookup", loop.na, KvRef::slab(loop.ids.data()), loop.toks.data(), loop.k_pass, 0, loop.acc.data(),
                          loop.got.data(), loop.keep.data(), VerifyKind::greedy());
        if (rc) return rc;
        loop.emit(out_tokens);
    }
    if (passes_out) *passes_out = loop.passes;
    return NVL_OK;
    NVL_CATCH(m)
}

// nvl_decode_sampled's contract from prompt-lookup drafts + sampled verify passes: nvl_decode_greedy_lookup's loop with
// the histories kept on the device (uploaded once; verify_accept_sampled_kernel appends what each pass emits) and the draw
// of decode step t of sequence i fixed to uniforms[t][i] however the passes group the steps.
extern "C" int nvl_decode_sampled_lookup(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                                         int k, int ngram, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                         const int32_t* history_lens, const float* uniforms, int32_t* out_tokens, int32_t* passes_out) {
    if (!m) return NVL_ERR_INVALID;
    if (!seq_ids || !first_tokens || !params || !history_ptrs || !history_lens || !uniforms || !out_tokens || n_steps <= 0 || ngram < 1)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_sampled_lookup: null/empty arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    int rc = verify_refusals(m, "nvl_decode_sampled_lookup", n_seqs, k, 1);
    if (rc) return rc;
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_decode_sampled_lookup: not available in paged-KV mode");
    std::vector<int> h_slot;
    if ((rc = plan_slab(m, Batch::uniform("nvl_decode_sampled_lookup", n_seqs, first_tokens, 1, n_steps), seq_ids, nullptr, h_slot, m->cfg.max_seq_len))) return rc;
    if (!history_in_vocab(m, n_seqs, history_ptrs, history_lens)) return fail(m, NVL_ERR_INVALID, "nvl_decode_sampled_lookup: history id outside the vocabulary");
    const SampledReq rq{params, history_ptrs, history_lens, uniforms};
    if (const char* why = sampled_check(rq, n_seqs, first_tokens, 1, n_steps, m->cfg.max_seq_len, (int64_t)n_steps * n_seqs))
        return fail(m, NVL_ERR_INVALID, std::string("nvl_decode_sampled_lookup: ") + why);
    SpecLoop loop(n_seqs, n_steps);       // (the host's copy of the histories is for drafting only)
    for (int i = 0; i < n_seqs; i++) loop.hist[(size_t)i].assign(history_ptrs[i], history_ptrs[i] + history_lens[i]);
    sampled_stage_histories(m, n_seqs, rq);
    while (loop.plan(k, seq_ids, [&](int i) { return cache_room(m, h_slot[(size_t)i]); })) {
        loop.draft_by_lookup(ngram);
        const int na = loop.na, S = loop.S;
        const VsBlock vs = bind_vs(m->vs_host, na);
        *vs.params = *params;
        for (int a = 0; a < na; a++) {
            const int i = loop.who[(size_t)a];
            vs.keep[a] = loop.keep[(size_t)a]; vs.hist_row[a] = i;
            for (int j = 0; j < S; j++) {       // row j is decode step done + j of the sequence; rows past the last step are never emitted
                const int t = loop.done[(size_t)i] + j;
                vs.u[a * S + j] = t < n_steps ? uniforms[(size_t)t * n_seqs + i] : 0.f;
            }
        }
        rc = verify_batch(m, "nvl_decode_sampled_lookup", na, KvRef::slab(loop.ids.data()), loop.toks.data(), loop.k_pass, 0, loop.acc.data(),
                          loop.got.data(), loop.keep.data(), VerifyKind::in_loop());
        if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }      // (the staged histories read the caller's arrays)
        loop.emit(out_tokens);
    }
    if (passes_out) *passes_out = loop.passes;
    return NVL_OK;
    NVL_CATCH(m)
}

// nvl_decode_greedy with the reference runner's sampling step instead of the argmax (tensor_model_runner.go:89-93):
// every step draws SampleWithHistory(logits, seq.TokenIDs, params) on the device and feeds the token back.
// history_ptrs[i]/history_lens[i] = Sequence.TokenIDs as the first decode step sees it (prompt + the token sampled from
// the prefill = first_tokens[i]); uniforms is [n_steps][n_seqs] (one rand.Float32() per sequence per step, in the
// order the host's serial loop would draw them).
namespace {
// `keep`: nvl_draft_sampled — every step's final distribution stays in m->draft_q and the model records what it holds
int decode_sampled_impl(nvl_model* m, const std::string& who, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                        const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                        const int32_t* history_lens, const float* uniforms, int32_t* out_tokens, bool keep) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, who + ": model not finalized");
    if (m->paged) return fail(m, NVL_ERR_STATE, who + ": not available in paged-KV mode");
    if (m->f32) return fail(m, NVL_ERR_STATE, who + ": bf16 models only");
    if (n_seqs <= 0 || n_steps <= 0 || !seq_ids || !first_tokens || !params || !history_ptrs || !history_lens || !uniforms || !out_tokens)
        return fail(m, NVL_ERR_INVALID, who + ": null/empty arguments");
    if (n_seqs > m->opts.max_seqs || n_seqs > m->opts.max_batch_tokens)
        return fail(m, NVL_ERR_INVALID, who + ": n_seqs exceeds max_seqs / max_batch_tokens");
    if (!sampling_params_ok(params)) return fail(m, NVL_ERR_INVALID, who + ": bad sampling parameters");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    const int T = m->cfg.max_seq_len;
    std::vector<int> h_slot;
    if (const int rc = plan_slab(m, Batch::uniform(who.c_str(), n_seqs, first_tokens, 1, n_steps), seq_ids, nullptr, h_slot, T)) return rc;
    const Meta hm = bind_meta(m, m->meta_host, n_seqs);
    const SampledReq rq{params, history_ptrs, history_lens, uniforms};
    if (const char* why = sampled_check(rq, n_seqs, first_tokens, 1, n_steps, T, (int64_t)n_steps * n_seqs, false)) return fail(m, NVL_ERR_INVALID, who + ": " + why);
    std::vector<int32_t> hist((size_t)n_seqs * T, 0), hlen(history_lens, history_lens + n_seqs);
    for (int i = 0; i < n_seqs; i++) std::copy(history_ptrs[i], history_ptrs[i] + hlen[(size_t)i], hist.begin() + (size_t)i * T);
    // device state of the sampler
    reserve_sample_rows(m, n_seqs);
    reserve_sample_hist(m);
    if ((int64_t)n_steps * n_seqs > m->samp_u_cap) {
        dfree(m->samp_u_steps);
        m->samp_u_cap = (int64_t)n_steps * n_seqs;
        m->samp_u_steps = dmalloc<float>(m->samp_u_cap);
    }
    NVL_HIP(hipMemcpyAsync(m->samp_hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, m->stream));
    NVL_HIP(hipMemcpyAsync(m->samp_hist_len, hlen.data(), hlen.size() * 4, hipMemcpyHostToDevice, m->stream));
    NVL_HIP(hipMemcpyAsync(m->samp_u_steps, uniforms, (size_t)n_steps * n_seqs * 4, hipMemcpyHostToDevice, m->stream));
    if (keep) {
        const int64_t need = (int64_t)n_steps * n_seqs * round_up(m->V, 4);
        if (need > m->draft_q_elems) {
            NVL_HIP(hipStreamSynchronize(m->stream));
            dfree(m->draft_q); m->draft_q = nullptr; m->draft_q_elems = 0;
            m->draft_q = dmalloc<float>(need); m->draft_q_elems = need;
        }
    }
    decode_loop(m, hm, n_seqs, n_steps, out_tokens, params, m->samp_u_steps, keep ? m->draft_q : nullptr);   // (synchronises: the host vectors stay alive)
    advance_slots(m, h_slot, [&](int) { return n_steps; });
    if (keep) {
        m->draft_n = n_seqs; m->draft_k = n_steps;
        m->draft_ids.assign(seq_ids, seq_ids + n_seqs); m->draft_tok.assign(out_tokens, out_tokens + (size_t)n_steps * n_seqs);
        m->draft_valid = true;
    }
    return NVL_OK;
    NVL_CATCH(m)
}
}  // namespace

extern "C" int nvl_decode_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                                  const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                  const int32_t* history_lens, const float* uniforms, int32_t* out_tokens) {
    return decode_sampled_impl(m, "nvl_decode_sampled", n_seqs, seq_ids, first_tokens, n_steps, params, history_ptrs, history_lens,
                               uniforms, out_tokens, false);
}

// ---- speculative decoding with a draft MODEL ----
// The draft phase: nvl_decode_sampled with n_steps = k whose per-step final distributions q_0 .. q_{k-1} stay on the device.
extern "C" int nvl_draft_sampled(nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int k,
                                 const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                 const int32_t* history_lens, const float* uniforms, int32_t* out_tokens) {
    if (!draft) return NVL_ERR_INVALID;
    if (k < 1 || k > 7) return fail(draft, NVL_ERR_INVALID, "nvl_draft_sampled: k outside 1..7");
    if (draft->n_mamba) return fail(draft, NVL_ERR_STATE, "nvl_draft_sampled: a Mamba2 state cannot be rolled back");
    return decode_sampled_impl(draft, "nvl_draft_sampled", n_seqs, seq_ids, first_tokens, k, params, history_ptrs, history_lens,
                               uniforms, out_tokens, true);
}

namespace {
// the draws of a speculative pass in the pass's uniform block: accept draw j in row j's slot, the final draw in row k's
std::vector<float> spec_merge_draws(int n_seqs, int k, const float* ua, const float* uf) {
    std::vector<float> u((size_t)n_seqs * (1 + k));
    for (int i = 0; i < n_seqs; i++) {
        for (int j = 0; j < k; j++) u[(size_t)i * (1 + k) + j] = ua[(size_t)i * k + j];
        u[(size_t)i * (1 + k) + k] = uf[i];
    }
    return u;
}
// what must hold between the two models, and between the call and the proposals the draft keeps
int spec_pair_refusals(nvl_model* t, nvl_model* d, const char* who) {
    if (!d->finalized) return fail(t, NVL_ERR_STATE, std::string(who) + ": draft model not finalized");
    if (t->device != d->device) return fail(t, NVL_ERR_INVALID, std::string(who) + ": target and draft live on different devices");
    if (t->V != d->V) return fail(t, NVL_ERR_INVALID, std::string(who) + ": target and draft differ in vocab_size");
    return NVL_OK;
}
int spec_proposals_check(nvl_model* t, nvl_model* d, const char* who, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                         int k_kept) {
    if (!d->draft_valid || !d->draft_q) return fail(t, NVL_ERR_STATE, std::string(who) + ": the draft holds no valid proposals (nvl_draft_sampled first)");
    if (d->draft_n != n_seqs || d->draft_k != k_kept) return fail(t, NVL_ERR_INVALID, std::string(who) + ": n_seqs / k are not those of the kept proposals");
    for (int i = 0; i < n_seqs; i++) {
        if (d->draft_ids[(size_t)i] != seq_ids[i]) return fail(t, NVL_ERR_INVALID, std::string(who) + ": sequence ids are not those of the kept proposals");
        for (int j = 0; j < k; j++)
            if (tokens[(size_t)i * (1 + k) + j + 1] != d->draft_tok[(size_t)j * n_seqs + i])
                return fail(t, NVL_ERR_INVALID, std::string(who) + ": a draft token is not the id the draft sampled at that step");
    }
    return NVL_OK;
}
}  // namespace

extern "C" int nvl_verify_speculative(nvl_model* target, nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* tokens,
                                      int k, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                      const int32_t* history_lens, const float* accept_uniforms, const float* final_uniforms,
                                      int32_t* n_accepted_out, int32_t* out_tokens, float* accept_prob_out) {
    if (!target || !draft || target == draft) return NVL_ERR_INVALID;
    nvl_model* m = target;
    if (!seq_ids || !tokens || !params || !history_ptrs || !history_lens || !accept_uniforms || !final_uniforms || !n_accepted_out || !out_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_verify_speculative: null arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    int rc = verify_refusals(m, "nvl_verify_speculative", n_seqs, k, 1);
    if (rc) return rc;
    if ((rc = spec_pair_refusals(m, draft, "nvl_verify_speculative"))) return rc;
    if ((rc = spec_proposals_check(m, draft, "nvl_verify_speculative", n_seqs, seq_ids, tokens, k, k))) return rc;
    const std::vector<float> u = spec_merge_draws(n_seqs, k, accept_uniforms, final_uniforms);
    const SampledReq rq{params, history_ptrs, history_lens, u.data()};
    const SpecReq spec{draft->draft_q, round_up(m->V, 4), 1, n_seqs, accept_prob_out};
    return verify_batch(m, "nvl_verify_speculative", n_seqs, KvRef::slab(seq_ids), tokens, k, 1, n_accepted_out, out_tokens, nullptr,
                        VerifyKind::speculative(rq, spec));
    NVL_CATCH(m)
}

// nvl_decode_sampled's contract from a draft model's proposals + speculative verify passes.  Per pass over the active
// sequences: the draft samples k_pass + 1 steps (the last one only to cache the row of d_k, its id is discarded: then the
// draft's cache holds every row the target may keep, and truncating it to the target's new length is all the rollback there
// is), the target verifies 1 + k_pass rows under the rejection rule, the draft is truncated.  Histories are restaged from the
// host on every pass.  A pass of one row (k_pass = 0) is a plain sampled step of the target.
extern "C" int nvl_decode_speculative(nvl_model* target, nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens,
                                      int n_steps, int k, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                                      const int32_t* history_lens, const float* uniforms, int32_t* out_tokens, int32_t* passes_out,
                                      int32_t* accepted_out) {
    if (!target || !draft || target == draft) return NVL_ERR_INVALID;
    nvl_model* m = target;
    if (!seq_ids || !first_tokens || !params || !history_ptrs || !history_lens || !uniforms || !out_tokens || n_steps <= 0)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_speculative: null/empty arguments");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    int rc = verify_refusals(m, "nvl_decode_speculative", n_seqs, k, 1);
    if (rc) return rc;
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_decode_speculative: not available in paged-KV mode");
    if ((rc = spec_pair_refusals(m, draft, "nvl_decode_speculative"))) return rc;
    if (draft->paged || draft->f32) return fail(m, NVL_ERR_STATE, "nvl_decode_speculative: the draft must be a bf16 slab model");
    if (draft->n_mamba) return fail(m, NVL_ERR_STATE, "nvl_decode_speculative: a Mamba2 draft cannot be rolled back");
    if (n_seqs > draft->opts.max_seqs || n_seqs > draft->opts.max_batch_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_decode_speculative: n_seqs exceeds the draft's max_seqs / max_batch_tokens");
    const int U = 2 * k + 1, T = std::min(m->cfg.max_seq_len, draft->cfg.max_seq_len);
    std::vector<int> dslot((size_t)n_seqs), tslot;
    if ((rc = plan_slab(m, Batch::uniform("nvl_decode_speculative", n_seqs, first_tokens, 1, n_steps), seq_ids, nullptr, tslot, T))) return rc;
    for (int i = 0; i < n_seqs; i++) {
        auto id = draft->seq_slot.find(seq_ids[i]);
        if (id == draft->seq_slot.end()) return fail(m, NVL_ERR_UNKNOWN_SEQ, "nvl_decode_speculative: sequence has no KV slot on the draft");
        dslot[(size_t)i] = id->second;
        if (m->slot_len[(size_t)tslot[(size_t)i]] != draft->slot_len[(size_t)id->second])
            return fail(m, NVL_ERR_INVALID, "nvl_decode_speculative: target and draft hold a sequence at different cached lengths");
    }
    if (!history_in_vocab(m, n_seqs, history_ptrs, history_lens)) return fail(m, NVL_ERR_INVALID, "nvl_decode_speculative: history id outside the vocabulary");
    const SampledReq rq0{params, history_ptrs, history_lens, uniforms};
    if (const char* why = sampled_check(rq0, n_seqs, first_tokens, 1, n_steps, T, (int64_t)n_steps * n_seqs * U))
        return fail(m, NVL_ERR_INVALID, std::string("nvl_decode_speculative: ") + why);
    SpecLoop loop(n_seqs, n_steps);
    for (int i = 0; i < n_seqs; i++) loop.hist[(size_t)i].assign(history_ptrs[i], history_ptrs[i] + history_lens[i]);
    if (accepted_out) for (int i = 0; i < n_seqs; i++) accepted_out[i] = 0;
    std::vector<int32_t> first, dtok, hl; std::vector<float> du, ua, uf;
    std::vector<const int32_t*> hp;
    // the draft runs k_pass + 1 steps: k_pass + 1 more positions and k_pass + 1 more history ids must fit (the history usually
    // holds one id more than the cache; both are >= 0 here: P + n_steps and history + n_steps fit, checked above)
    const auto room = [&](int i) { return T - std::max(m->slot_len[(size_t)tslot[(size_t)i]], (int)loop.hist[(size_t)i].size()) - 1; };
    while (loop.plan(k, seq_ids, room)) {
        const int na = loop.na, S = loop.S, k_pass = loop.k_pass;
        const std::vector<int>& who = loop.who;
        first.resize((size_t)na); hp.resize((size_t)na); hl.resize((size_t)na);
        dtok.assign((size_t)S * na, 0); du.assign((size_t)S * na, 0.f); ua.assign((size_t)na * std::max(k_pass, 1), 0.f); uf.resize((size_t)na);
        for (int a = 0; a < na; a++) {
            const std::vector<int32_t>& h = loop.hist[(size_t)who[(size_t)a]];
            const float* u = uniforms + ((size_t)loop.passes * n_seqs + who[(size_t)a]) * U;      // pass t's block of sequence i
            first[(size_t)a] = h.back(); hp[(size_t)a] = h.data(); hl[(size_t)a] = (int32_t)h.size();
            for (int j = 0; j < k_pass; j++) { du[(size_t)j * na + a] = u[j]; ua[(size_t)a * k_pass + j] = u[k + j]; }
            uf[(size_t)a] = u[2 * k];
        }
        // the draft phase: k_pass proposals and the cached row of the last one
        rc = decode_sampled_impl(draft, "nvl_decode_speculative (draft)", na, loop.ids.data(), first.data(), S, params, hp.data(), hl.data(),
                                 du.data(), dtok.data(), true);
        if (rc) return fail(m, rc, std::string("nvl_decode_speculative: the draft refused: ") + draft->err);      // (it changed nothing)
        // the draft's rollback, and what undoes this pass after a refusal (earlier passes stay): the draft goes where the target is
        auto draft_to_target = [&] { for (int a = 0; a < na; a++) draft->slot_len[(size_t)dslot[(size_t)who[(size_t)a]]] = m->slot_len[(size_t)tslot[(size_t)who[(size_t)a]]]; };
        for (int a = 0; a < na; a++)
            for (int j = 0; j < k_pass; j++) loop.toks[(size_t)a * S + 1 + j] = dtok[(size_t)j * na + a];
        const KvRef kv = KvRef::slab(loop.ids.data());
        if (k_pass > 0) {
            if ((rc = spec_proposals_check(m, draft, "nvl_decode_speculative", na, loop.ids.data(), loop.toks.data(), k_pass, S))) { draft_to_target(); return rc; }
            const std::vector<float> u = spec_merge_draws(na, k_pass, ua.data(), uf.data());
            const SpecReq spec{draft->draft_q, round_up(m->V, 4), 1, na, nullptr};
            rc = verify_batch(m, "nvl_decode_speculative", na, kv, loop.toks.data(), k_pass, 1, loop.acc.data(), loop.got.data(), loop.keep.data(),
                              VerifyKind::speculative({params, hp.data(), hl.data(), u.data()}, spec));
        } else
            rc = verify_batch(m, "nvl_decode_speculative", na, kv, loop.toks.data(), 0, 0, loop.acc.data(), loop.got.data(), loop.keep.data(),
                              VerifyKind::sampled({params, hp.data(), hl.data(), uf.data()}));
        draft_to_target();
        if (rc) return rc;
        loop.emit(out_tokens, accepted_out);
    }
    if (passes_out) *passes_out = loop.passes;
    return NVL_OK;
    NVL_CATCH(m)
}

// =================================================================================================
// debug / parity taps, stats
// =================================================================================================
extern "C" int nvl_set_debug(nvl_model* m, int keep_hidden) {
    if (!m) return NVL_ERR_INVALID;
    m->keep_hidden = keep_hidden == 1;      // 1: per-layer residual stream, every residual add completed in its own launch
    m->tap = keep_hidden == 2;              // 2: the same record taken beside the unmodified product path (pending adds included)
    m->stamping = keep_hidden == 4;         // 4: in-kernel time stamps of the decode kernels (nvl_get_stamps), eager launches
#ifndef NVL_STAMPS
    if (m->stamping) {      // the product library carries no stamp sites (common.h NvlStamps): the diagnostic build does
        m->stamping = false;
        return fail(m, NVL_ERR_STATE, "nvl_set_debug: mode 4 needs the diagnostic build (make -C csrc diag -> libnvllm_hip_diag.so, NVLLM_LIB)");
    }
#endif
    if (m->stamping) {
        NVL_TRY(m)
        NVL_HIP(hipSetDevice(m->device));
        if (!m->stamp_buf) m->stamp_buf = (unsigned long long*)dmalloc_bytes((int64_t)STAMP_MAX_LAUNCH * STAMP_MAX_WG * 8 * 8);
        NVL_HIP(hipStreamSynchronize(m->stream));
        NVL_HIP(hipMemset(m->stamp_buf, 0, (size_t)STAMP_MAX_LAUNCH * STAMP_MAX_WG * 8 * 8));
        m->stamp_launches = 0; m->stamp_recs.clear();
        NVL_CATCH(m)
    }
    return NVL_OK;
}
// nvl_set_debug(m, 4) ... forward passes ... nvl_get_stamps: per stamped launch {site, phase, workgroups} in `recs`
// (3 ints each) and its stamps [workgroups][8] of the 100 MHz clock back to back in `stamps`.  Returns the launch count.
extern "C" int nvl_get_stamps(nvl_model* m, int32_t* recs, int rec_cap, uint64_t* stamps, int64_t stamp_cap) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->stamp_buf) return fail(m, NVL_ERR_STATE, "nvl_get_stamps: nvl_set_debug(m, 4) first");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamSynchronize(m->stream));
    const int n = (int)m->stamp_recs.size();
    int64_t off = 0;
    for (int i = 0; i < n && i < rec_cap; i++) {
        const auto& r = m->stamp_recs[(size_t)i];
        recs[3 * i] = r.site; recs[3 * i + 1] = r.phase; recs[3 * i + 2] = r.nwg;
        if (off + (int64_t)r.nwg * 8 > stamp_cap) return fail(m, NVL_ERR_INVALID, "nvl_get_stamps: stamp buffer too small");
        NVL_HIP(hipMemcpy(stamps + off, m->stamp_buf + (size_t)i * STAMP_MAX_WG * 8, (size_t)r.nwg * 64, hipMemcpyDeviceToHost));
        off += (int64_t)r.nwg * 8;
    }
    return n;
    NVL_CATCH(m)
}
extern "C" int nvl_get_hidden(nvl_model* m, int layer, float* out, int64_t n_floats) {
    if (!m || !out) return NVL_ERR_INVALID;
    if (!m->hidden || layer < 0 || layer >= m->L) return fail(m, NVL_ERR_STATE, "nvl_get_hidden: nothing recorded");
    NVL_TRY(m)
    const int64_t per = (int64_t)m->hidden_last_M * m->H;   // [L][M][H] of the recording call
    if (n_floats > per) n_floats = per;
    NVL_HIP(hipMemcpy(out, m->hidden + (int64_t)layer * per, (size_t)n_floats * 4, hipMemcpyDeviceToHost));
    return NVL_OK;
    NVL_CATCH(m)
}

namespace {
// K and V of positions 0..T-1 of one block list, laid out as the reference does ([nKV, T, hd] fp32, kv_cache.go:5-6)
void read_kv(nvl_model* m, const int32_t* blocks, int n_blocks, int T, int layer, float* k_out, float* v_out) {
    const int hd = m->hd, BS = m->Tmax;
    const int64_t n = m->layer_stride;
    std::vector<char> kb((size_t)n * m->kv_esize), vb((size_t)n * m->kv_esize);
    auto rd = [&](const std::vector<char>& b, int64_t i) -> float {
        if (m->kv8) {                   // s * e4m3fn(code), the value the attention kernels use
            const float s = &b == &kb ? m->k_scale[layer] : m->v_scale[layer];
            return e4m3fn_value(((const uint8_t*)b.data())[i]) * s;
        }
        if (m->f32) return ((const float*)b.data())[i];
        uint32_t u = ((uint32_t)((const uint16_t*)b.data())[i]) << 16;
        float f; memcpy(&f, &u, 4); return f;
    };
    for (int bi = 0; bi < n_blocks && bi * BS < T; bi++) {
        const size_t off = ((size_t)blocks[bi] * m->slot_stride + (size_t)layer * m->layer_stride) * m->kv_esize;
        NVL_HIP(hipMemcpy(kb.data(), (char*)m->kcache + off, kb.size(), hipMemcpyDeviceToHost));
        NVL_HIP(hipMemcpy(vb.data(), (char*)m->vcache + off, vb.size(), hipMemcpyDeviceToHost));
        const int t1 = std::min(T, (bi + 1) * BS);
        for (int h = 0; h < m->nKV; h++)
            for (int t = bi * BS; t < t1; t++)
                for (int d = 0; d < hd; d++) {
                    const int r = t - bi * BS;
                    const int64_t o = ((int64_t)h * T + t) * hd + d;
                    if (k_out) k_out[o] = rd(kb, ((int64_t)h * BS + r) * hd + d);
                    if (v_out) v_out[o] = rd(vb, ((int64_t)h * BS + r) * hd + d);
                }
    }
}
}  // namespace

extern "C" int nvl_get_kv(nvl_model* m, int64_t seq_id, int layer, float* k_out, float* v_out) {
    if (!m) return NVL_ERR_INVALID;
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return fail(m, NVL_ERR_UNKNOWN_SEQ, "nvl_get_kv: unknown sequence");
    if (layer < 0 || layer >= m->L) return fail(m, NVL_ERR_INVALID, "nvl_get_kv: bad layer");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    const int32_t slot = it->second;
    const int T = m->slot_len[(size_t)slot];
    read_kv(m, &slot, 1, T, layer, k_out, v_out);
    return T;
    NVL_CATCH(m)
}

extern "C" int nvl_get_mamba_state(nvl_model* m, int64_t seq_id, int layer, float* out) {
    if (!m || !out) return NVL_ERR_INVALID;
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return fail(m, NVL_ERR_UNKNOWN_SEQ, "nvl_get_mamba_state: unknown sequence");
    if (layer < 0 || layer >= m->L || !m->layers[(size_t)layer].mamba) return fail(m, NVL_ERR_INVALID, "nvl_get_mamba_state: not a Mamba2 layer");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamSynchronize(m->stream));
    const float* src = m->ssm_state + (int64_t)it->second * m->ssm_slot_stride + (int64_t)m->layers[(size_t)layer].mamba_idx * m->ssm_layer_stride;
    NVL_HIP(hipMemcpy(out, src, (size_t)m->ssm_layer_stride * 4, hipMemcpyDeviceToHost));
    return (int)m->ssm_layer_stride;
    NVL_CATCH(m)
}

extern "C" int nvl_get_mamba_conv_state(nvl_model* m, int64_t seq_id, int layer, float* out) {
    if (!m || !out) return NVL_ERR_INVALID;
    auto it = m->seq_slot.find(seq_id);
    if (it == m->seq_slot.end()) return fail(m, NVL_ERR_UNKNOWN_SEQ, "nvl_get_mamba_conv_state: unknown sequence");
    if (layer < 0 || layer >= m->L || !m->layers[(size_t)layer].mamba) return fail(m, NVL_ERR_INVALID, "nvl_get_mamba_conv_state: not a Mamba2 layer");
    if (!m->conv_tail) return 0;       // K == 1: the window is the token itself
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamSynchronize(m->stream));
    const float* src = m->conv_tail + (int64_t)it->second * m->conv_tail_slot_stride + (int64_t)m->layers[(size_t)layer].mamba_idx * m->conv_tail_layer_stride;
    NVL_HIP(hipMemcpy(out, src, (size_t)m->conv_tail_layer_stride * 4, hipMemcpyDeviceToHost));
    return (int)m->conv_tail_layer_stride;
    NVL_CATCH(m)
}

extern "C" int nvl_get_weight(nvl_model* m, int kind, int layer, float* out, int64_t in_features, int64_t out_features) {
    if (!m || !out) return NVL_ERR_INVALID;
    DevTensor* t = tensor_slot(m, kind, layer);
    if (!t || is_1d(kind)) return fail(m, NVL_ERR_INVALID, "nvl_get_weight: not a 2-D weight kind");
    if (!t->present()) return fail(m, NVL_ERR_STATE, "nvl_get_weight: the tensor is not on the device (never uploaded, or fused away by nvl_finalize)");
    if (t->rows != out_features || t->cols != in_features) return fail(m, NVL_ERR_INVALID, "nvl_get_weight: shape mismatch");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    NVL_HIP(hipStreamSynchronize(m->stream));
    const int64_t N = t->rows, K = t->cols, n_el = t->rows_pad * K;
    if (t->qs) {     // quantized weight: W~, the values every GEMM path computes with (wq.h wf_value_at)
        std::vector<uint8_t> codes((size_t)wf_code_bytes(t->wf, n_el)), sc((size_t)wf_scale_bytes(t->wf, t->rows_pad, K));
        NVL_HIP(hipMemcpy(codes.data(), t->p, codes.size(), hipMemcpyDeviceToHost));
        NVL_HIP(hipMemcpy(sc.data(), t->qs, sc.size(), hipMemcpyDeviceToHost));
        for (int64_t n = 0; n < N; n++)
            for (int64_t k = 0; k < K; k++) out[k * N + n] = wf_value_at(t->wf, codes.data(), sc.data(), n, k, K);
        return NVL_OK;
    }
    std::vector<char> raw((size_t)n_el * m->wsize);
    NVL_HIP(hipMemcpy(raw.data(), t->p, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t n = 0; n < N; n++)
        for (int64_t k = 0; k < K; k++) {
            float v;
            if (m->f32) v = ((const float*)raw.data())[n * K + k];
            else { const uint32_t u = ((uint32_t)((const uint16_t*)raw.data())[fm_index(n, k, K)]) << 16; memcpy(&v, &u, 4); }
            out[k * N + n] = v;      // the reference's [in, out]
        }
    return NVL_OK;
    NVL_CATCH(m)
}

extern "C" int nvl_get_kv_paged(nvl_model* m, const int32_t* block_table, int n_blocks, int n_tokens, int layer,
                                float* k_out, float* v_out) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->paged) return fail(m, NVL_ERR_STATE, "nvl_get_kv_paged: the model is not in paged-KV mode");
    if (!block_table || n_blocks <= 0 || n_tokens < 0 || n_tokens > n_blocks * m->Tmax || layer < 0 || layer >= m->L)
        return fail(m, NVL_ERR_INVALID, "nvl_get_kv_paged: bad arguments");
    for (int i = 0; i < n_blocks; i++)
        if (block_table[i] < 0 || block_table[i] >= m->num_blocks) return fail(m, NVL_ERR_INVALID, "nvl_get_kv_paged: block id out of range");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    read_kv(m, block_table, n_blocks, n_tokens, layer, k_out, v_out);
    return n_tokens;
    NVL_CATCH(m)
}

extern "C" int nvl_set_profile(nvl_model* m, int on) {
    if (!m) return NVL_ERR_INVALID;
    m->profile = on != 0;
    return NVL_OK;
}
extern "C" int nvl_get_stats(nvl_model* m, nvl_stats* out) {
    if (!m || !out) return NVL_ERR_INVALID;
    *out = m->stats;
    return NVL_OK;
}
extern "C" int nvl_reset_stats(nvl_model* m) {
    if (!m) return NVL_ERR_INVALID;
    const double wb = m->stats.weight_bytes;
    m->stats = nvl_stats{};
    m->stats.weight_bytes = wb;
    for (auto& ph : m->site_stats) for (auto& st : ph) st = SiteStat{};
    return NVL_OK;
}
static const char* const k_site_names[KS_COUNT] = {
    "other", "qkv_proj", "attention", "o_proj", "ffn_up", "ffn_down", "lm_head", "norm", "moe_router", "moe_plan", "moe_up",
    "moe_down", "moe_combine", "embed", "argmax", "rope_kv", "mamba_in_proj", "mamba_conv", "mamba_scan", "mamba_gate_norm",
    "mamba_out_proj", "tp_allreduce", "logprobs", "spec_reject"};
extern "C" const char* nvl_kernel_site_name(int site) { return site >= 0 && site < KS_COUNT ? k_site_names[site] : ""; }
extern "C" int nvl_get_kernel_stats(nvl_model* m, nvl_kernel_stat* out, int cap) {
    if (!m || (cap > 0 && !out)) return NVL_ERR_INVALID;
    int n = 0;
    for (int ph = 0; ph < 2; ph++)
        for (int st = 0; st < KS_COUNT; st++) {
            const SiteStat& ss = m->site_stats[ph][st];
            if (!ss.launches) continue;
            if (n < cap) out[n] = nvl_kernel_stat{st, ph, ss.launches, ss.ms, ss.flops, ss.bytes};
            n++;
        }
    return n;
}

// =================================================================================================
// runner: ModelRunner.Run semantics (tensor_model_runner.go:55-97)
// =================================================================================================
// =================================================================================================
// on-device sampling: tensor.SampleWithHistory, sampling.go:33-102
// =================================================================================================
namespace {
// rows of device logits -> sampled ids on the host.  `err` receives the reason when the arguments are refused.
int sample_rows(hipStream_t st, SampleBufs& b, const float* logits_dev, int64_t ld, int rows, int V,
                const nvl_sampling_params* sp, const int32_t* const* hist_ptrs, const int32_t* hist_lens,
                const float* uniforms, int32_t* out_host, float* probs_host, std::string& err) {
    if (rows <= 0 || V <= 0 || !sp || !uniforms || !out_host) { err = "null/empty arguments"; return NVL_ERR_INVALID; }
    if (!(sp->repetition_penalty == sp->repetition_penalty) || !(sp->temperature == sp->temperature) || !(sp->top_p == sp->top_p)) {
        err = "NaN sampling parameter"; return NVL_ERR_INVALID;
    }
    if (sp->repetition_penalty == 0.f) { err = "repetition_penalty 0 (the reference would divide by zero)"; return NVL_ERR_INVALID; }
    std::vector<int32_t> off((size_t)rows + 1, 0), hist;
    for (int i = 0; i < rows; i++) {
        const int n = (hist_ptrs && hist_lens && hist_ptrs[i]) ? hist_lens[i] : 0;
        if (n < 0) { err = "negative history length"; return NVL_ERR_INVALID; }
        for (int j = 0; j < n; j++) {
            if (hist_ptrs[i][j] < 0) { err = "negative token id in the history (the reference would panic)"; return NVL_ERR_INVALID; }
            hist.push_back(hist_ptrs[i][j]);
        }
        off[(size_t)i + 1] = (int32_t)hist.size();
        if (!(uniforms[i] >= 0.f && uniforms[i] <= 1.f)) { err = "uniform draw outside [0, 1]"; return NVL_ERR_INVALID; }
    }
    const int64_t elems = (int64_t)rows * round_up(V, 4);
    if (elems > b.elems) {
        dfree(b.work); dfree(b.cnt);
        b.work = dmalloc<float>(elems); b.cnt = dmalloc<int32_t>(elems); b.elems = elems;
        NVL_HIP(hipMemsetAsync(b.cnt, 0, (size_t)elems * 4, st));
    }
    if ((int64_t)hist.size() > b.hist_cap) {
        dfree(b.hist); b.hist_cap = round_up((int64_t)hist.size(), 4096); b.hist = dmalloc<int32_t>(b.hist_cap);
    }
    if (rows > b.rows_cap) {
        dfree(b.off); dfree(b.out); dfree(b.u);
        b.rows_cap = (int)round_up(rows, 64);
        b.off = dmalloc<int32_t>(b.rows_cap + 1); b.out = dmalloc<int32_t>(b.rows_cap); b.u = dmalloc<float>(b.rows_cap);
    }
    if (probs_host && elems > b.probs_elems) { dfree(b.probs); b.probs = dmalloc<float>(elems); b.probs_elems = elems; }
    if (!hist.empty()) NVL_HIP(hipMemcpyAsync(b.hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, st));
    NVL_HIP(hipMemcpyAsync(b.off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    NVL_HIP(hipMemcpyAsync(b.u, uniforms, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    SampleArgs a{};
    a.logits = logits_dev; a.ld = ld; a.work = b.work; a.cnt = b.cnt; a.hist = b.hist; a.hist_off = b.off;
    a.uniforms = b.u; a.out = b.out; a.probs_out = probs_host ? b.probs : nullptr; a.ldp = V;
    a.V = V; a.top_k = sp->top_k; a.temperature = sp->temperature; a.top_p = sp->top_p; a.rep_penalty = sp->repetition_penalty;
    hipLaunchKernelGGL(sample_row_kernel<false>, dim3(rows), dim3(SAMPLE_THREADS), 0, st, a);
    NVL_HIP(hipGetLastError());
    NVL_HIP(hipMemcpyAsync(out_host, b.out, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (probs_host) NVL_HIP(hipMemcpyAsync(probs_host, b.probs, (size_t)rows * V * 4, hipMemcpyDeviceToHost, st));
    NVL_HIP(hipStreamSynchronize(st));   // (also keeps the host vectors alive until the copies are done)
    return NVL_OK;
}
}  // namespace

extern "C" int nvl_sample(nvl_model* m, int n_rows, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                          const int32_t* history_lens, const float* uniforms, int32_t* out_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_sample: model not finalized");
    if (n_rows <= 0 || n_rows > m->last_rows) return fail(m, NVL_ERR_INVALID, "nvl_sample: n_rows exceeds the logits rows of the last forward");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    std::string err;
    // (captured sampled verify passes hold the scratch addresses sample_rows is about to replace)
    if ((int64_t)n_rows * round_up(m->V, 4) > m->samp.elems || n_rows > m->samp.rows_cap) clear_graphs(m);
    const int rc = sample_rows(m->stream, m->samp, m->logits, m->Vpad, n_rows, m->V, params, history_ptrs, history_lens,
                               uniforms, out_tokens, nullptr, err);
    return rc ? fail(m, rc, "nvl_sample: " + err) : NVL_OK;
    NVL_CATCH(m)
}

// =================================================================================================
// log-probabilities on the device (logprob.h): what generic_model.go:467-470 / :595-604 logits are turned into by a
// perplexity tool or a server's `logprobs` (cmd/check-logits/main.go prints logits; nothing in the reference reduces them)
// =================================================================================================
namespace {
// rows of device logits -> per-row results on the host.  `scaling`: the LogitsScaling divisor still to apply (0 = none).
int logprob_rows(hipStream_t st, LogprobBufs& b, const float* logits_dev, int64_t ld, int rows, int V, float scaling,
                 const int32_t* targets, int top_k, float* logprob_out, int32_t* argmax_out, int32_t* topk_ids_out,
                 float* topk_lp_out, std::string& err) {
    if (rows <= 0 || V <= 0 || ld < V) { err = "bad shape"; return NVL_ERR_INVALID; }
    if (top_k < 0 || top_k > LOGPROB_MAX_K) { err = "top_k outside [0, 8]"; return NVL_ERR_INVALID; }
    if (targets)
        for (int i = 0; i < rows; i++)
            if (targets[i] < -1 || targets[i] >= V) { err = "target id outside [-1, V)"; return NVL_ERR_INVALID; }
    reserve_logprob_bufs(b, rows, rows, V);
    if (targets) NVL_HIP(hipMemcpyAsync(b.targets(), targets, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    LogprobArgs a{};
    a.x = logits_dev; a.ld = ld; a.V = V; a.scaling = scaling;
    a.top_k = (topk_ids_out || topk_lp_out) ? top_k : 0;
    a.targets = targets ? b.targets() : nullptr; a.logprob = b.logprob(); a.argmax = b.argmax();
    a.topk_ids = b.topk_ids(); a.topk_lp = b.topk_lp();
    launch_logprobs(st, a, rows, b.part);
    NVL_HIP(hipGetLastError());
    if (logprob_out) NVL_HIP(hipMemcpyAsync(logprob_out, b.logprob(), (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (argmax_out) NVL_HIP(hipMemcpyAsync(argmax_out, b.argmax(), (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    if (a.top_k > 0 && topk_ids_out) NVL_HIP(hipMemcpyAsync(topk_ids_out, b.topk_ids(), (size_t)rows * top_k * 4, hipMemcpyDeviceToHost, st));
    if (a.top_k > 0 && topk_lp_out) NVL_HIP(hipMemcpyAsync(topk_lp_out, b.topk_lp(), (size_t)rows * top_k * 4, hipMemcpyDeviceToHost, st));
    NVL_HIP(hipStreamSynchronize(st));
    return NVL_OK;
}
}  // namespace

extern "C" int nvl_logprobs(nvl_model* m, int n_rows, const int32_t* targets, int top_k, float* logprob_out,
                            int32_t* argmax_out, int32_t* topk_ids_out, float* topk_logprob_out) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_logprobs: model not finalized");
    if (n_rows <= 0 || n_rows > m->last_rows) return fail(m, NVL_ERR_INVALID, "nvl_logprobs: n_rows exceeds the logits rows of the last forward");
    NVL_TRY(m)
    NVL_HIP(hipSetDevice(m->device));
    std::string err;
    int rc;
    {   // every forward tail has applied LogitsScaling in place (enqueue_forward): scaling 0 here, never twice
        KScope ks(m, KC_OTHER, 0, KS_LOGPROBS, (double)n_rows * m->V * 4.0);
        rc = logprob_rows(m->stream, m->lpb, m->logits, m->Vpad, n_rows, m->V, 0.f, targets, top_k, logprob_out, argmax_out,
                          topk_ids_out, topk_logprob_out, err);
    }
    if (m->profile) { NVL_HIP(hipStreamSynchronize(m->stream)); drain_profile(m); }
    return rc ? fail(m, rc, "nvl_logprobs: " + err) : NVL_OK;
    NVL_CATCH(m)
}

namespace {
int runner_impl(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* const* token_ptrs,
                const int32_t* token_lens, int is_prefill, int32_t* next_tokens, float* logits_out,
                const nvl_sampling_params* sp, const float* uniforms);
}
extern "C" int nvl_runner_run(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* const* token_ptrs,
                              const int32_t* token_lens, int is_prefill, int32_t* next_tokens, float* logits_out) {
    return runner_impl(m, n_seqs, seq_ids, token_ptrs, token_lens, is_prefill, next_tokens, logits_out, nullptr, nullptr);
}
extern "C" int nvl_runner_run_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* const* token_ptrs,
                                      const int32_t* token_lens, int is_prefill, const nvl_sampling_params* params,
                                      const float* uniforms, int32_t* next_tokens) {
    if (!m) return NVL_ERR_INVALID;
    if (!params || !uniforms) return fail(m, NVL_ERR_INVALID, "nvl_runner_run_sampled: null sampling arguments");
    return runner_impl(m, n_seqs, seq_ids, token_ptrs, token_lens, is_prefill, next_tokens, nullptr, params, uniforms);
}
namespace {
// after a forward over the sequences `who` (indices into the caller's arrays; logits rows in that order): replace the
// greedy ids by SampleWithHistory(logits, seq.TokenIDs, params) (tensor_model_runner.go:93)
int runner_sample(nvl_model* m, const std::vector<int>& who, const int32_t* const* token_ptrs, const int32_t* token_lens,
                  const nvl_sampling_params* sp, const float* uniforms, int32_t* next_tokens) {
    std::vector<const int32_t*> hp(who.size()); std::vector<int32_t> hl(who.size()), out(who.size()); std::vector<float> u(who.size());
    for (size_t j = 0; j < who.size(); j++) { hp[j] = token_ptrs[who[j]]; hl[j] = token_lens[who[j]]; u[j] = uniforms[who[j]]; }
    const int rc = nvl_sample(m, (int)who.size(), sp, hp.data(), hl.data(), u.data(), out.data());
    if (rc) return rc;
    for (size_t j = 0; j < who.size(); j++) next_tokens[who[j]] = out[j];
    return NVL_OK;
}
// pins the slots of the sequences of the forward call being assembled, so that opening a slot for one of them never
// evicts another (released on scope exit, also on errors)
struct PinScope {
    nvl_model* m; std::vector<int> slots;
    explicit PinScope(nvl_model* m_) : m(m_) {}
    void pin(int64_t seq_id) {
        auto it = m->seq_slot.find(seq_id);
        if (it != m->seq_slot.end() && !m->slot_pin[(size_t)it->second]) { m->slot_pin[(size_t)it->second] = 1; slots.push_back(it->second); }
    }
    ~PinScope() { for (int s : slots) m->slot_pin[(size_t)s] = 0; }
};
int runner_impl(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* const* token_ptrs,
                const int32_t* token_lens, int is_prefill, int32_t* next_tokens, float* logits_out,
                const nvl_sampling_params* sp, const float* uniforms) {
    if (!m) return NVL_ERR_INVALID;
    if (!m->finalized) return fail(m, NVL_ERR_STATE, "nvl_runner_run: model not finalized");
    if (m->paged) return fail(m, NVL_ERR_STATE, "nvl_runner_run: the model is in paged-KV mode (use nvl_runner_run_paged)");
    if (n_seqs <= 0 || !seq_ids || !token_ptrs || !token_lens || !next_tokens)
        return fail(m, NVL_ERR_INVALID, "nvl_runner_run: null/empty arguments");
    NVL_TRY(m)      // (host containers below may throw bad_alloc: nothing may cross the C ABI)
    // Partition: sequences that can take the 1-token decode path vs sequences that must be (re)prefilled: an unknown id
    // (never seen, closed, or EVICTED since) or a cache whose length does not match is re-prefilled from the full history.
    std::vector<int> dec, pre;
    for (int i = 0; i < n_seqs; i++) {
        if (!token_ptrs[i] || token_lens[i] <= 0) return fail(m, NVL_ERR_INVALID, "nvl_runner_run: sequence without tokens");
        if (token_lens[i] > m->cfg.max_seq_len) return fail(m, NVL_ERR_POSITION, "nvl_runner_run: sequence longer than max_seq_len");
        for (int j = 0; j < i; j++) if (seq_ids[j] == seq_ids[i]) return fail(m, NVL_ERR_INVALID, "nvl_runner_run: duplicate sequence in batch");
        bool can_decode = false;
        if (!is_prefill) {
            auto it = m->seq_slot.find(seq_ids[i]);
            can_decode = it != m->seq_slot.end() && m->slot_len[(size_t)it->second] == token_lens[i] - 1;
        }
        (can_decode ? dec : pre).push_back(i);
    }
    const int V = m->V;
    // ---- decode group: one token per sequence at position len-1 (:78-80).  Runs before any slot is (re)opened below,
    // so no decodable sequence of this batch can be evicted before its step.
    for (size_t base = 0; base < dec.size(); base += (size_t)m->opts.max_seqs) {
        const size_t n = std::min(dec.size() - base, (size_t)m->opts.max_seqs);
        std::vector<int64_t> ids(n); std::vector<int32_t> toks(n), lens(n, 1), pos(n), out(n);
        for (size_t j = 0; j < n; j++) {
            const int i = dec[base + j];
            ids[j] = seq_ids[i]; toks[j] = token_ptrs[i][token_lens[i] - 1]; pos[j] = token_lens[i] - 1;
        }
        std::vector<float> lg(logits_out ? n * (size_t)V : 0);
        const int rc = nvl_forward(m, (int)n, ids.data(), toks.data(), lens.data(), pos.data(), 0,
                                   logits_out ? lg.data() : nullptr, out.data());
        if (rc) return rc;
        for (size_t j = 0; j < n; j++) {
            next_tokens[dec[base + j]] = out[j];
            if (logits_out) memcpy(logits_out + (size_t)dec[base + j] * V, &lg[j * (size_t)V], (size_t)V * 4);
        }
        if (sp) {
            const std::vector<int> who(dec.begin() + (long)base, dec.begin() + (long)(base + n));
            const int rs = runner_sample(m, who, token_ptrs, token_lens, sp, uniforms, next_tokens);
            if (rs) return rs;
        }
    }
    // ---- prefill group: discard the cache, run the whole history from position 0 (:63-66,75);
    // packed into forward calls of at most max_batch_tokens; a longer history is fed in chunks.  A sequence without a
    // slot takes a free one, or — the engine never calls ClearCache — the least-recently-forwarded slot outside the
    // call being assembled (seq_open_impl).
    auto reset_evict = [&](int64_t id) -> int {
        const int rc = seq_open_impl(m, id, true);
        if (rc) return rc;
        m->slot_len[(size_t)m->seq_slot[id]] = 0;
        return NVL_OK;
    };
    for (int i : pre) {      // this call's own sequences are the most recently used: victims come from outside the batch first
        auto it = m->seq_slot.find(seq_ids[i]);
        if (it != m->seq_slot.end()) m->slot_tick[(size_t)it->second] = ++m->tick;
    }
    size_t k = 0;
    while (k < pre.size()) {
        std::vector<int64_t> ids; std::vector<int32_t> toks, lens, pos; std::vector<int> who;
        int64_t budget = m->opts.max_batch_tokens;
        PinScope pins(m);
        while (k < pre.size() && (int)ids.size() < m->opts.max_seqs) {
            const int i = pre[k];
            if (token_lens[i] > budget) break;
            int rc = reset_evict(seq_ids[i]);
            if (rc) return rc;
            pins.pin(seq_ids[i]);
            ids.push_back(seq_ids[i]); lens.push_back(token_lens[i]); pos.push_back(0); who.push_back(i);
            toks.insert(toks.end(), token_ptrs[i], token_ptrs[i] + token_lens[i]);
            budget -= token_lens[i];
            k++;
        }
        if (ids.empty()) {   // one history longer than max_batch_tokens: chunked prefill of that sequence
            const int i = pre[k];
            int rc = reset_evict(seq_ids[i]);
            if (rc) return rc;
            int done = 0; int32_t out = 0;
            std::vector<float> lg(logits_out ? (size_t)V : 0);
            while (done < token_lens[i]) {
                const int32_t n = (int32_t)std::min<int64_t>(m->opts.max_batch_tokens, token_lens[i] - done);
                const int32_t p0 = done;
                // hybrid models: the reference prefills the history in ONE Forward, whose Mamba2 convolution window spans
                // the chunk seams (mamba2.go:183-254): chunks after the first take the previous chunk's tail (mamba.h)
                m->conv_chain = done == 0 ? 1 : 2;
                rc = nvl_forward(m, 1, &seq_ids[i], token_ptrs[i] + done, &n, &p0, 0, logits_out ? lg.data() : nullptr, &out);
                m->conv_chain = 0;
                if (rc) return rc;
                done += n;
            }
            next_tokens[i] = out;
            if (logits_out) memcpy(logits_out + (size_t)i * V, lg.data(), (size_t)V * 4);
            if (sp) {
                const int rs = runner_sample(m, std::vector<int>{i}, token_ptrs, token_lens, sp, uniforms, next_tokens);
                if (rs) return rs;
            }
            k++;
            continue;
        }
        std::vector<int32_t> out(ids.size());
        std::vector<float> lg(logits_out ? ids.size() * (size_t)V : 0);
        const int rc = nvl_forward(m, (int)ids.size(), ids.data(), toks.data(), lens.data(), pos.data(), 0,
                                   logits_out ? lg.data() : nullptr, out.data());
        if (rc) return rc;
        for (size_t j = 0; j < who.size(); j++) {
            next_tokens[who[j]] = out[j];
            if (logits_out) memcpy(logits_out + (size_t)who[j] * V, &lg[j * (size_t)V], (size_t)V * 4);
        }
        if (sp) {
            const int rs = runner_sample(m, who, token_ptrs, token_lens, sp, uniforms, next_tokens);
            if (rs) return rs;
        }
    }
    return NVL_OK;
    NVL_CATCH(m)
}
}  // namespace

#include "ops_impl.h"
#include "loader.h"
