// model.h — host-side state of one nvl_model handle (device weights in kernel layout, KV slabs,
// workspaces, the HIP stream) and the kernel launch helpers shared by nvllm.hip and ops.hip.
#pragma once
#include <condition_variable>
#include <array>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nvllm.h"
#include "attn.h"
#include "kv8.h"
#include "common.h"
#include "elem.h"
#include "sample.h"
#include "spec.h"
#include "logprob.h"
#include "gemm.h"
#include "wq.h"
#include "mamba.h"
#include "tp_p2p.h"

namespace nvl {

struct DevTensor {
    void* p = nullptr;      // canonical device copy: 2-D [rows_pad][cols] in weight dtype, 1-D fp32
    void* qs = nullptr;     // quantized weights (wf != WF_BF16): p holds the codes, qs their scales in the format's layout (wfmt.h)
    int wf = WF_BF16;       // stored format (wfmt.h WF_*; INT4: with its group size, wf_int4)
    int64_t rows = 0, cols = 0, rows_pad = 0;
    bool present() const { return p != nullptr; }
};

struct LayerW {
    DevTensor t[NVL_T_COUNT];
    // frozen by finalize()
    void* w_qkv = nullptr; int n_qkv = 0; float* b_qkv = nullptr;
    void* w1 = nullptr; int n1 = 0;      // fused rows (2F for SwiGLU, F for GELU)
    void* qs_qkv = nullptr; void* qs1 = nullptr;   // quantized weights: the scales of w_qkv / w1 (they follow the fused rows / 16-row tiles)
    void* moe_in = nullptr;              // [E][2I (interleaved in bf16 mode)][H]
    void* moe_out_cat = nullptr;         // bf16: W_down of all experts along K, [H_pad][E*I] (decode "dense-masked" form)
    // quantized experts (nvl_set_expert_dtype / nvl_set_mx_expert_dtype / nvl_set_gq_expert_dtype): moe_in holds codes in the
    // same interleaved order, qs_moe_in its scales; moe_out_q the down codes over K = E*I, [H_pad][E*I] (the layout of
    // moe_out_cat: moe_out_cat = moe_out_q when the decode form applies), qs_moe_out its scales (wq.h wf_down_scale_dims) —
    // fp8: [E][H_pad], one row per expert; MXFP4: [H_pad/16][E*I/32][16] bytes, beside the code tiles; INT4:
    // [H_pad/16][E*I/g][16] group words, beside the code tiles too
    void* qs_moe_in = nullptr;
    void* moe_out_q = nullptr; void* qs_moe_out = nullptr;
    bool mamba = false;                  // a Mamba2 block (attention tensors absent); index among the Mamba2 layers
    int mamba_idx = -1;
};

enum KClass { KC_GEMM = 0, KC_ATTN = 1, KC_OTHER = 2 };
// where in the layer a launch sits (per-kernel roofline entries of nvl_get_kernel_stats; names in nvllm.hip)
enum KSite { KS_OTHER = 0, KS_QKV, KS_ATTN, KS_OPROJ, KS_FFN_UP, KS_FFN_DOWN, KS_LM_HEAD, KS_NORM, KS_MOE_ROUTER, KS_MOE_PLAN,
             KS_MOE_UP, KS_MOE_DOWN, KS_MOE_COMBINE, KS_EMBED, KS_ARGMAX, KS_ROPE, KS_MAMBA_IN, KS_MAMBA_CONV, KS_MAMBA_SCAN,
             KS_MAMBA_GATE, KS_MAMBA_OUT, KS_ALLREDUCE, KS_LOGPROBS, KS_SPEC_REJECT, KS_COUNT };

struct ProfRec { hipEvent_t a, b; int cls; double flops; int site, phase; double bytes; };
struct SiteStat { double ms = 0, flops = 0, bytes = 0; uint64_t launches = 0; };

}  // namespace nvl

// in-process tensor-parallel group (tests on one GPU): see tp_allreduce in nvllm.hip
// device scratch of the sampler (sample.h); grows on demand
struct SampleBufs {
    float* work = nullptr; int32_t* cnt = nullptr; int64_t elems = 0;     // [rows][V] each; cnt is kept zero-filled
    int32_t* hist = nullptr; int64_t hist_cap = 0;
    int32_t* off = nullptr; int32_t* out = nullptr; float* u = nullptr; int rows_cap = 0;
    float* probs = nullptr; int64_t probs_elems = 0;
};

// device scratch of the log-probability kernels (logprob.h); grows on demand
struct LogprobBufs {
    void* part = nullptr; int64_t part_words = 0;     // pass-1 partials of one launch
    int32_t* io = nullptr; int64_t io_rows = 0;       // per row: target | logprob | argmax | top-k ids [8] | top-k logprobs [8]
    int32_t* targets() const { return io; }
    float* logprob() const { return (float*)(io + io_rows); }
    int32_t* argmax() const { return io + 2 * io_rows; }
    int32_t* topk_ids() const { return io + 3 * io_rows; }
    float* topk_lp() const { return (float*)(io + (3 + nvl::LOGPROB_MAX_K) * io_rows); }
};

struct nvl_local_group {
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, arrived = 0, refs = 0;
    bool aborted = false;        // a member failed: every waiter and every later all-reduce of the group errors out
    uint64_t gen = 0;
    float* bufs[8] = {nullptr};
    float* scratch = nullptr;
    int64_t scratch_floats = 0;
};

struct nvl_model {
    nvl_model_config cfg{};
    nvl_runtime_opts opts{};
    bool f32 = false;            // NVL_PRECISION_F32
    bool finalized = false;
    // 8-bit KV cache (kv_cache_dtype = NVL_KV_FP8_E4M3, kv8.h): e4m3fn codes, 1 byte per element; per-layer fp32 scales
    bool kv8 = false;
    int kv_esize = 2;                      // bytes per cached K/V element (wsize, or 1 in 8-bit mode)
    std::vector<float> k_scale, v_scale;   // [num_layers], default 1 (Mamba2 layers' entries unused)
    bool kv_written = false;               // a forward has been enqueued: the scales are fixed from then on
    // quantized weights: the stored format of the projections (wf), of the MoE experts (ef: WF_BF16 or wf itself, INT4 with the
    // same group size) and of the MXFP4 LM head / tied embedding (hf: WF_BF16 or WF_MXFP4 — the fp8 head follows wf itself).
    // Only the nvl_set_*_dtype entry points write them, and only as wfmt.h's wf_decide() answers: the rules of every setter are
    // there, once.  What differs by format after that is a wf_* function of wfmt.h (host facts) or wq.h (launches)
    int wf = nvl::WF_BF16, ef = nvl::WF_BF16, hf = nvl::WF_BF16;
    bool w2d_uploaded = false;             // a 2-D tensor has been uploaded: the weight dtype is fixed from then on
    bool expert_uploaded = false;          // an expert tensor has been uploaded: the expert dtype is fixed from then on
    struct QRef { int wf; const void* scales; int64_t rows_pad; };
    std::map<const void*, QRef> qmap;      // finalized quantized weights by code pointer (gemm() dispatch)
    nvl::bf16_t* wq_scratch = nullptr; int64_t wq_scratch_elems = 0;   // tile path: W~ of one projection (the largest but the LM head)
    nvl::bf16_t* eq_scratch = nullptr; int64_t eq_scratch_elems = 0;   // grouped GEMMs: W~ of one layer's experts (up, then down)
    // 8-bit activations of the tile step (nvl_set_act_dtype NVL_ACT_FP8_E4M3, a8.h): codes [a8_rows][a8_k] + scales [a8_rows]
    bool a8 = false;
    uint8_t* a8_codes = nullptr; float* a8_scale = nullptr; int64_t a8_rows = 0, a8_k = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // derived (nH, nKV, F are the LOCAL sizes of this tensor-parallel rank; *_full the model's)
    int H = 0, nH = 0, nKV = 0, hd = 0, F = 0, V = 0, Vpad = 0, L = 0, group = 1;
    int tp = 1, tp_rank = 0, nH_full = 0, nKV_full = 0, F_full = 0;
    bool tp_force = false;
    void* tp_comm = nullptr;          // ncclComm_t
    nvl_local_group* tp_local = nullptr;   // in-process emulation (tests on one GPU)
    float* tp_part = nullptr;         // [Mmax][H] fp32 partial of a row-parallel projection
    // hand-written all-reduce over peer-mapped buffers (tp_p2p.h): own comm buffer + the peers' (IPC-opened) ones
    char* p2p_buf = nullptr; size_t p2p_bytes = 0; char* p2p_peer[8] = {nullptr}; bool p2p_ready = false;
    int64_t p2p_off_in1 = 0, p2p_off_in2 = 0, p2p_off_res = 0, p2p_in1_stride = 0, p2p_in2_stride = 0, p2p_res_stride = 0;
    int n_qkv = 0, Tmax = 0;     // Tmax: tokens per KV block (slab mode: the whole slot; paged: kv_block_size)
    int paged = 0, num_blocks = 0, blocks_per_seq = 1, table_cap = 0;   // KV addressing (see kv_locate)
    float attn_scale = 0.f, resid_alpha = 1.f;
    size_t wsize = 2;            // bytes per weight/activation element

    nvl::DevTensor g[NVL_T_COUNT];       // model-level tensors
    std::vector<nvl::LayerW> layers;
    void* lm_head = nullptr;             // [Vpad][H] (aliases tok_emb when tied)
    float *rope_cos = nullptr, *rope_sin = nullptr;

    // KV slabs
    void *kcache = nullptr, *vcache = nullptr;
    int64_t slot_stride = 0, layer_stride = 0;    // elements
    std::map<int64_t, int> seq_slot;
    std::vector<int> free_slots;
    std::vector<int> slot_len;
    std::vector<uint64_t> slot_tick;   // last forward that touched the slot (LRU eviction in the runner entry points)
    std::vector<char> slot_pin;        // 1 while the slot's sequence is part of the forward call being assembled
    uint64_t tick = 0;

    // workspaces
    float* x = nullptr;          // residual stream fp32 [Mmax][H]
    void* xn = nullptr;          // normed activations (ActT)
    float* qkv = nullptr;        // fp32 [Mmax][n_qkv]
    void* q = nullptr;           // ActT [Mmax][nH*hd]
    void* attn_out = nullptr;    // ActT [Mmax][nH*hd]
    float* attn_part = nullptr;  // bf16: partial results of a decode attention whose keys are split over workgroups (attn.h AttnArgs::part)
    int32_t* attn_part_cnt = nullptr;   // ... and their arrival tickets per (sequence, kv head)
    void* hbuf = nullptr;        // ActT [Mmax][F]   (MoE: [Mmax*k][I])
    float* h2 = nullptr;         // fp32 [Mmax][2F]  (f32 mode un-fused gate|up; MoE f32 too)
    void* xn_last = nullptr;     // ActT [rows][H]
    float* logits = nullptr;     // fp32 [logit_rows][Vpad]
    int64_t logit_rows = 0;
    int32_t* argmax_dev = nullptr; float* argmax_pval = nullptr; int32_t* argmax_pidx = nullptr;
    // MoE
    float* router_logits = nullptr;   // [Mmax][128]
    int32_t* expert_ids = nullptr; float* expert_w = nullptr;
    int32_t *seg_start = nullptr, *perm_token = nullptr, *slot_of = nullptr;
    float* moe_eo = nullptr;          // [Mmax*k][H]
    float* moe_gate = nullptr;        // decode: [64][E] routing weights (0 = not routed)
    void* moe_hall = nullptr;         // decode: bf16 [64][E*I] gate-weighted SwiGLU outputs of every touched expert
    float* moe_part = nullptr;        // decode: [MOE_DOWN_SLICES][64][H] K-slice partials of the down projection
    void* moe_xg = nullptr;           // bf16: the normed rows in expert order, fragment-major [round_up(Mmax*k, 64)][H] (prefill)
    int32_t *moe_counts = nullptr, *moe_cursor = nullptr, *moe_tile_map = nullptr, *moe_n_mtiles = nullptr;
    int moe_form = 0;                 // the form the last moe() call took (NVL_MOE_FORM_*; nvl_op_moe_stages reports it)
    // decode split-K: partial slices of the last residual GEMM, consumed by the next norm launch
    float* rs_part = nullptr;    // deferred RMSNorm: [H/16][64] partial sums of x^2 (gemm.h)
    int attn_ran[3] = {0, 0, 0};      // the last attention launch: kernel form (NVL_ATTN_RAN_*), waves per workgroup, key split (nvl_op_attention_batch reports them)
    int ctx_hint = 0;    // longest context (keys) of the batch being enqueued; 0 = unknown (decode attention sizing)
    float* sk_part = nullptr; int sk_max_slices = 4; int pending_slices = 0, pending_rows = 0; float pending_alpha = 1.f; const float* pending_part = nullptr;
    int sk_rows = 64;             // rows the sk_part slices are allocated for
    int pending_from = 0;         // which residual projection left the pending slices (0 = O projection, 1 = FFN-down)
    int dense_ran[NVL_DENSE_RAN_INTS] = {0};   // what the residual projections and norms of the last layer tail ran (nvllm.h NVL_DENSE_RAN_*; resid_gemm / launch_norm write it, nvl_op_dense_stages reports it)
    int gemm_ran = 0, norm_ran = 0;   // the last bf16 projection's instance (NVL_GEMM_RAN_*, gemm()) and the last norm launch's kernel (NVL_NORM_RAN_*, launch_norm)
    int front_ran[NVL_QKV_RAN_INTS] = {0};     // what the last layer front ran (nvllm.h NVL_QKV_RAN_*; embed / qkv_front write it, nvl_op_qkv_stages reports it)
    const int32_t* pending_slot_of = nullptr; const float* pending_gate_w = nullptr;   // MoE combine folded into the next norm
    // per-call metadata (one pinned host block mirrored on the device)
    int32_t* meta_host = nullptr; int32_t* meta_dev = nullptr; int64_t meta_ints = 0;
    // Mamba2 (hybrid models): sizes, per-slot SSM state [slot][mamba layer][heads][hd][ss] fp32, workspaces
    int n_mamba = 0, mEH = 0, mConv = 0, mP = 0, m_nh = 0, m_hd = 0, m_ss = 0, m_ng = 0, m_K = 0;
    float* ssm_state = nullptr; int64_t ssm_layer_stride = 0, ssm_slot_stride = 0;
    float *mproj = nullptr, *mxbc = nullptr, *mdelta = nullptr, *my = nullptr; void* myn = nullptr;
    float* conv_tail = nullptr; int64_t conv_tail_layer_stride = 0, conv_tail_slot_stride = 0;   // chunked prefill, or every call of a carried model (mamba.h MambaArgs::chain)
    int conv_chain = 0;          // set by runner_impl around the chunks of one long history
    bool conv_carried = false;   // nvl_set_mamba_conv_state(NVL_MAMBA_CONV_CARRIED): every pass runs chain 3
    float *ssd_z = nullptr, *ssd_decay = nullptr; int64_t ssd_z_floats = 0, ssd_decay_floats = 0;   // chunk-parallel SSD scan scratch (mamba.h)
    SampleBufs samp;             // nvl_sample scratch
    LogprobBufs lpb;             // nvl_logprobs / nvl_score scratch
    int32_t* samp_hist = nullptr; int32_t* samp_hist_len = nullptr; int64_t samp_hist_cap = 0;   // nvl_decode_sampled: device-kept histories
    float* samp_u_steps = nullptr; int64_t samp_u_cap = 0;
    // nvl_draft_sampled: the final distribution of every draft step, [steps][n_seqs][round_up(V, 4)] on the
    // device, and what it holds; any later forward pass of this model invalidates it (enqueue_forward)
    float* draft_q = nullptr; int64_t draft_q_elems = 0;
    bool draft_valid = false; int draft_n = 0, draft_k = 0;
    std::vector<int64_t> draft_ids; std::vector<int32_t> draft_tok;      // sequence ids in order; sampled ids [k][n_seqs]
    float* spec_ap = nullptr;    // a speculative verify pass's {p(d), q(d)} pairs [max_seqs][7][2] (allocated on first use)
    int last_rows = 0;           // logits rows the last forward left in `logits`
    int32_t* ring = nullptr; int64_t ring_ints = 0;   // nvl_decode_greedy: [steps][seqs] tokens on the device
    int32_t* ring_pos0 = nullptr;                     // position of every sequence when the fused loop started (ring row index)
    // hipGraph replay of decode passes (one graph per launch configuration; first sight eager, second captured, then replayed)
    std::map<std::array<int, 5>, hipGraphExec_t> graphs;
    std::set<std::array<int, 5>> graph_seen;
    std::vector<hipGraphExec_t> graphs_retired;       // evicted execs, destroyed after the next stream sync (reap_graphs)
    bool graphs_ok = true;
    int32_t* am_host = nullptr;                       // pinned: argmax ids of a replayed decode pass
    int32_t* verify_dev = nullptr; int32_t* verify_host = nullptr;    // a verify pass's accept counts + ids (device, pinned)
    int32_t* vs_dev = nullptr; int32_t* vs_host = nullptr;            // a sampled verify pass's parameters, keeps, history rows, draws
    // debug
    // nvl_set_debug mode 4: in-kernel time stamps of the decode kernels (common.h nvl_stamp), one record per launch
    bool stamping = false; unsigned long long* stamp_buf = nullptr; int stamp_launches = 0;
    struct StampRec { int site, phase, nwg; };
    std::vector<StampRec> stamp_recs;
    bool tap = false;            // nvl_set_debug mode 2: record every layer's residual stream without leaving the product path
    bool keep_hidden = false; float* hidden = nullptr; int64_t hidden_tokens = 0; int hidden_last_M = 0;
    // stats
    nvl_stats stats{};
    nvl::SiteStat site_stats[2][nvl::KS_COUNT];     // [phase: 0 prefill, 1 decode][site], filled when profiling
    int site = 0, phase = 0;     // set by the forward pass just before a launch (consumed by KScope)
    double kv_tok = 0;           // cached + new keys of the batch being enqueued (attention's algorithmic KV bytes)
    double site_bytes = 0;       // algorithmic bytes of the next launch (0 = let the helper compute them)
    bool profile = false;
    std::vector<nvl::ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
