/*
 * nvllm.h — C ABI of libnvllm_hip.so: the MI355X (gfx950) forward path that
 * replaces nano-vllm-go's purego/tensor prefill + decode hot path.
 *
 * Drop-in boundary.  A Go maintainer binds these with cgo (stub in
 * INTEGRATION.md) and implements nanovllm.ModelRunner on top of them; nothing
 * else in nano-vllm-go changes.  Every entry point names the reference
 * interface it replaces (file:line under the reference repository).
 *
 *   - plain C, opaque handles, plain pointers + sizes, no C++/torch types;
 *   - every function returns 0 on success or a negative nvl_status; the text
 *     of the last failure is available from nvl_last_error();
 *   - the library never aborts where the reference panics (shape mismatch
 *     tensor.go:64-68, RoPE overflow rope.go:84-86): those are error codes;
 *   - host buffers are borrowed for the duration of the call only (cgo pointer
 *     rules); results are written into caller-provided host buffers;
 *   - a model handle owns one HIP stream and is NOT re-entrant (the reference's
 *     engine is single-goroutine: nanovllm/llm_engine.go:62-98).
 */
#ifndef NVLLM_H
#define NVLLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVL_ABI_VERSION 3      /* 2: Mamba2 / hybrid layers (config fields, tensor kinds), nvl_stats.evictions, kernel stats;
                                  3: nvl_get_weight, nvl_get_stamps, nvl_tp_p2p_rearm, debug modes 2 / 4 (additions only) */

typedef enum nvl_status {
    NVL_OK = 0,
    NVL_ERR_INVALID = -1,      /* bad argument / shape mismatch (reference: panic tensor.go:64-68) */
    NVL_ERR_POSITION = -2,     /* pos >= max_seq_len           (reference: panic rope.go:84-86)   */
    NVL_ERR_UNKNOWN_SEQ = -3,  /* decode for a sequence with no cache slot                         */
    NVL_ERR_NO_SLOT = -4,      /* all KV slots in use                                              */
    NVL_ERR_OOM = -5,          /* hipMalloc failed                                                 */
    NVL_ERR_HIP = -6,          /* any other HIP runtime error                                      */
    NVL_ERR_STATE = -7,        /* call out of order (e.g. forward before finalize)                 */
    NVL_ERR_NO_DEVICE = -8     /* no gfx950 device visible: the library has NO CPU fallback        */
} nvl_status;

/* ---- model description: flat mirror of tensor.ModelConfig (purego/tensor/config.go:58-122) ---- */
enum { NVL_ATTN_MHA = 0, NVL_ATTN_MQA = 1, NVL_ATTN_GQA = 2 };        /* config.go:18-22 */
enum { NVL_NORM_LAYER = 0, NVL_NORM_RMS = 1 };                        /* config.go:27-30 */
enum { NVL_POS_LEARNED = 0, NVL_POS_ROPE = 1, NVL_POS_NONE = 2 };     /* config.go:35-40 */
enum { NVL_ACT_GELU = 0, NVL_ACT_SWIGLU = 1 };                        /* config.go:45-48 */
enum { NVL_BLOCK_SEQUENTIAL = 0, NVL_BLOCK_PARALLEL = 1 };            /* config.go:53-56 */

typedef struct nvl_model_config {
    int32_t vocab_size, hidden, num_layers, num_heads, num_kv_heads, head_dim;
    int32_t ffn_dim, max_seq_len;
    int32_t attention_type, norm_type, position_type, activation_type, block_style;
    double  rope_base;       /* config.go:89; ignored for MQA, which hard-wires 10000 (mqa.go:35) */
    float   norm_eps;
    int32_t tied_embedding;
    int32_t use_moe, num_experts, num_experts_per_tok;
    float   embedding_multiplier, attention_multiplier, residual_multiplier, logits_scaling;
    /* Mamba2 / hybrid layers (config.go:100-115; Granite-4: attention + Mamba2 blocks): layer li is a Mamba2 block when
     * bit li of mamba_layer_mask is set (HybridLayers[li] == "mamba" / "mamba2", generic_model.go:50-53, 74-76).
     * mamba_head_dim 0 = expand * hidden / mamba_num_heads (mamba2.go:58-61).  All zero: no Mamba2 layers. */
    int32_t  mamba_expand, mamba_state_size, mamba_num_heads, mamba_head_dim, mamba_n_groups, mamba_conv_kernel;
    uint64_t mamba_layer_mask[2];
} nvl_model_config;

/* Arithmetic the device path computes in. */
enum {
    NVL_PRECISION_BF16 = 0, /* bf16 weights + bf16 GEMM/attention operands on MFMA, fp32 accumulate,
                               fp32 residual stream / norms / softmax / RoPE (the product path)   */
    NVL_PRECISION_F32  = 1  /* fp32 weights, fp32 operands everywhere (slow; the tight-tolerance
                               parity mode used by the tests)                                     */
};

typedef struct nvl_runtime_opts {
    int32_t device;            /* HIP device ordinal                                               */
    int32_t precision;         /* NVL_PRECISION_*                                                  */
    int32_t max_seqs;          /* KV slots (concurrent sequences); replaces the unbounded
                                  map[int64]*KVCache of tensor_model_runner.go:13                  */
    int32_t max_batch_tokens;  /* largest sum(seq_lens) one nvl_forward call may carry             */
    int32_t tp_rank, tp_size;  /* tensor-parallel shard of this process (1 = none); consumer of the
                                  reference's inert Config.TensorParallelSize (nanovllm/config.go:61) */
    int32_t tp_force_single;   /* 1 with tp_size = 1: diagnostics — run the tensor-parallel projection +
                                  all-reduce path on a one-rank group (needs nvl_tp_init)             */
    int32_t kv_num_blocks;     /* > 0: PAGED KV — a pool of this many blocks addressed through the host's block
                                  tables (nanovllm/block_manager.go, Sequence.BlockTable): nvl_forward_paged /
                                  nvl_runner_run_paged; the slot calls (nvl_seq_*, nvl_forward) are refused.
                                  0: one contiguous slab per sequence slot                              */
    int32_t kv_block_size;     /* tokens per block in paged mode: 0 = 256 (Sequence.BlockSize, sequence.go:51);
                                  a multiple of 64                                                     */
    int32_t kv_cache_dtype;    /* NVL_KV_*: element type of the KV cache (was `reserved`; 0 keeps today's behaviour)      */
} nvl_runtime_opts;

/* KV cache element type (nvl_runtime_opts.kv_cache_dtype).  Anything else is refused by nvl_create (NVL_ERR_INVALID). */
enum {
    NVL_KV_AUTO = 0,        /* the model's precision (bf16 / f32)                                                  */
    NVL_KV_FP8_E4M3 = 1     /* OCP e4m3fn codes (1 byte per element: twice the tokens per byte of cache) + one fp32
                               scale per layer for K and one for V.  bf16 precision only, no
                               tensor parallelism.  nvl_get_kv / nvl_get_kv_paged return s * e4m3(code).            */
};

typedef struct nvl_model nvl_model;

/* ---- tensors: the layout contract of generic_loader.go:353-604 ---- */
typedef enum nvl_tensor_kind {
    NVL_T_TOK_EMB = 0,     /* [V, H]                 TransformerModel.TokenEmbedding generic_model.go:8 */
    NVL_T_POS_EMB,         /* [max_seq, H]           PosEmbedding                    generic_model.go:9 */
    NVL_T_LM_HEAD,         /* IN_OUT: [H, V]         LMHead (omit when tied)         generic_model.go:18 */
    NVL_T_FINAL_NORM_W,    /* [H]                    LNFinal.Weight                                  */
    NVL_T_FINAL_NORM_B,    /* [H]  absent => RMSNorm LNFinal.Bias           tensor.go:197            */
    /* per layer */
    NVL_T_ATTN_NORM_W,     /* AttnLN (sequential) / InputLN (parallel)      generic_model.go:26-28   */
    NVL_T_ATTN_NORM_B,
    NVL_T_FFN_NORM_W,
    NVL_T_FFN_NORM_B,
    NVL_T_WQ,              /* IN_OUT: [H, nH*hd]     attention.go:12,200  mqa.go:14                  */
    NVL_T_WK,              /* IN_OUT: [H, nKV*hd]    attention.go:13,201                             */
    NVL_T_WV,
    NVL_T_WKV,             /* IN_OUT: [H, 2*hd]      MQA fused K|V        mqa.go:15                  */
    NVL_T_WO,              /* IN_OUT: [nH*hd, H]                                                     */
    NVL_T_BQ, NVL_T_BK, NVL_T_BV, NVL_T_BO,   /* MHA biases               attention.go:19-23       */
    NVL_T_W1,              /* IN_OUT: [H, 2F] gate|up (SwiGLU) or [H, F]   transformer.go:30        */
    NVL_T_B1,
    NVL_T_W2,              /* IN_OUT: [F, H]                                                         */
    NVL_T_B2,
    NVL_T_ROUTER,          /* IN_OUT: [H, E]                               moe.go:12                */
    NVL_T_MOE_IN,          /* [E, 2I, H] exactly as the reference keeps it (un-transposed) moe.go:176 */
    NVL_T_MOE_OUT,         /* [E, H, I]                                                              */
    /* Mamba2Layer (mamba2.go:9-27), as loadMamba2 leaves them (generic_loader.go:461-512: PyTorch layouts, NO transpose) */
    NVL_T_MAMBA_IN_PROJ,   /* OUT_IN: [EH + conv_dim + heads, H]  InProj, used as MatMul(x, Transpose(InProj)) mamba2.go:90 */
    NVL_T_MAMBA_CONV_W,    /* [conv_dim * K]  ConvWeight [conv_dim, 1, K] flattened                  */
    NVL_T_MAMBA_CONV_B,    /* [conv_dim]                                                             */
    NVL_T_MAMBA_A_LOG,     /* [heads]                                                                */
    NVL_T_MAMBA_D,         /* [heads]                                                                */
    NVL_T_MAMBA_DT_BIAS,   /* [heads]                                                                */
    NVL_T_MAMBA_NORM,      /* [EH]                                                                   */
    NVL_T_MAMBA_OUT_PROJ,  /* OUT_IN: [H, EH]  OutProj, MatMul(y, Transpose(OutProj))           mamba2.go:175 */
    NVL_T_COUNT
} nvl_tensor_kind;

enum { NVL_DTYPE_F32 = 0, NVL_DTYPE_BF16 = 1, NVL_DTYPE_F16 = 2 };    /* generic_loader.go:645-663 */
enum {
    NVL_LAYOUT_IN_OUT = 0, /* [in, out]: what the reference holds after Transpose (generic_loader.go:398-403) */
    NVL_LAYOUT_OUT_IN = 1  /* [out, in]: the checkpoint's own PyTorch layout, uploaded without the host transpose */
};

/* Per-layer K / V scales of an 8-bit cache (arrays of num_layers; default 1.0; Mamba2 layers' entries ignored).
 * NVL_ERR_STATE on a model without an 8-bit cache or after the first forward; NVL_ERR_INVALID for a non-finite or
 * non-positive scale.  nvl_load_safetensors sets them from *.self_attn.k_scale / v_scale when the checkpoint has them. */
int nvl_set_kv_scales(nvl_model* m, const float* k_scale, const float* v_scale);

/* Storage type of the projection weights.  The reference keeps every weight fp32
 * (generic_loader.go:398-403, loadTensorFromData); this is the library's own opt-in, reached only through this call. */
enum {
    NVL_W_AUTO = 0,        /* the precision's own type (bf16 / f32): today's behaviour                                     */
    NVL_W_FP8_E4M3 = 1     /* WQ/WK/WV/WKV/WO/W1/W2 and the LM head (the token embedding when tied) as OCP e4m3fn codes with
                            * one fp32 scale per output row: s = amax/448 (1 for a zero row), q = e4m3fn_rne(w / s).  Every path
                            * computes with W~ = bf16_rne(s * e4m3(q)); nvl_get_weight returns W~; nvl_stats.weight_bytes
                            * counts codes + scales.  Position embedding, router, Mamba2 projections stay bf16; MoE experts too
                            * unless nvl_set_expert_dtype(m, NVL_EXPERT_FP8_E4M3). */
};
/* After nvl_create, before the first 2-D upload (else NVL_ERR_STATE).  NVL_ERR_INVALID for an unknown value, and for
 * NVL_W_FP8_E4M3 with f32 precision or tensor parallelism.  In fp8 mode nvl_upload_tensor refuses a non-finite weight. */
int nvl_set_weight_dtype(nvl_model* m, int dtype);
/* MoE expert weights (MOE_IN / MOE_OUT) with 8-bit projection weights. */
enum {
    NVL_EXPERT_AUTO = 0,       /* the experts stay bf16 (also under NVL_W_FP8_E4M3): today's behaviour                       */
    NVL_EXPERT_FP8_E4M3 = 1    /* MOE_IN / MOE_OUT as OCP e4m3fn codes with one fp32 scale per (expert, output row), under the
                                * contract of NVL_W_FP8_E4M3: s = amax/448, q = e4m3fn_rne(w / s), W~ = bf16_rne(s * e4m3(q)) on
                                * every path; nvl_get_weight returns W~; nvl_stats.weight_bytes counts codes + scales.  Decode
                                * streams the codes; prefill dequantizes one layer's experts at a time into a scratch buffer. */
};
/* After nvl_set_weight_dtype(m, NVL_W_FP8_E4M3), before the first expert upload and nvl_finalize (else NVL_ERR_STATE).
 * NVL_ERR_INVALID for an unknown value, a model without MoE, f32 precision, or no 8-bit projection weights. */
int nvl_set_expert_dtype(nvl_model* m, int dtype);
/* Activation operand of the projections that run on the tile (prefill) GEMM path, with 8-bit weights. */
enum {
    NVL_ACT_AUTO = 0,      /* bf16 activations: the weights' own mode (W8A16 with NVL_W_FP8_E4M3): today's behaviour           */
    NVL_ACT_FP8_E4M3 = 1   /* W8A8: each tile-path launch quantizes its activation rows to OCP e4m3fn with one fp32 scale per
                            * row (s_a = amax/448, 1 for a zero row, q = e4m3fn_rne(a / s_a), NaN -> NaN) and multiplies codes
                            * x codes on the scaled FP8 MFMA: y = (acc * s_a[m]) * s_w[n], then the usual epilogue.  Decode-form
                            * launches (M <= 64, the 64-row groups, the short-prefill QKV groups) keep bf16 activations.        */
};
/* After nvl_set_weight_dtype(m, NVL_W_FP8_E4M3), before nvl_finalize (else NVL_ERR_STATE).  NVL_ERR_INVALID for an unknown
 * value and for NVL_ACT_FP8_E4M3 without 8-bit weights (so also with f32 precision or tensor parallelism). */
int nvl_set_act_dtype(nvl_model* m, int dtype);
/* Convolution window of the Mamba2 layers across calls.  The reference's Mamba2Layer.causalConv1d pads
 * EVERY Forward call with zeros and never uses its ConvCache field (mamba2.go:27,181-254,356): a decode call convolves its
 * one token with K-1 zeros, and so does the first token after every seam of a prompt fed in several calls.  That is the
 * default here too (PER_CALL), so prefill(P) + decode(t) is the reference's function of its calls, not the model's
 * function of the P + t tokens.  CARRIED makes it the latter: recommended for real hybrid checkpoints. */
enum { NVL_MAMBA_CONV_PER_CALL = 0,   /* every call zero-pads (mamba2.go:181-254): today's behaviour */
       NVL_MAMBA_CONV_CARRIED  = 1 }; /* the window reaches into the sequence's previous calls        */
/* After nvl_create, before nvl_finalize (else NVL_ERR_STATE).  NVL_ERR_INVALID for a NULL model, an unknown mode and a model
 * without Mamba2 layers.  A convolution width K of 1 is accepted and changes nothing.
 * Contract of CARRIED: for sequence i of a call, its token at absolute position p and window element q = p - back
 * (back = 0 .. K-1): q >= seq_pos[i] is this call's raw xBC row; 0 <= q < seq_pos[i] is the kept row of position q; q < 0
 * is zero.  A sequence whose call starts at position 0 never reads what its slot kept (an evicted or reset slot does not
 * leak).  After every call each of its sequences keeps the last K-1 rows of concat(old rows, or zeros at seq_pos == 0,
 * this call's raw rows): positions before 0 are zeros in the kept rows, and a call shorter than K-1 keeps the newest old
 * rows.  The rows are the fp32 in-projection output in both precisions.  This holds per sequence for any batch (ragged,
 * permuted slots, prefill rows mixed with decode rows) through nvl_forward, nvl_score, nvl_runner_run*, nvl_decode_greedy
 * and nvl_decode_sampled, graph replay included.  The SSM reset at position 0 stays; speculative calls, nvl_seq_truncate,
 * paged and tensor-parallel hybrids stay refused.  No memory is added: the rows live in the buffer the runner's chunked
 * prefill already used.  A decode pass pays no extra launch for it (nvl_set_tuning key 39). */
int nvl_set_mamba_conv_state(nvl_model* m, int mode);
/* Pre-quantized 8-bit weight, taken as it is (the dtype of nvl_load_safetensors' F8_E4M3 tensors): codes [rows][cols] OCP
 * e4m3fn in the checkpoint's [out, in] order (layout must be NVL_LAYOUT_OUT_IN), scales [rows] fp32, W~ = bf16(s * e4m3(q)).
 * Counterpart of nvl_upload_tensor (generic_loader.go:353-604) for a kind this model stores 8-bit; NVL_ERR_INVALID for any
 * other kind, a shape mismatch, a NaN code (0x7f / 0xff) or a non-finite / non-positive scale.  With NVL_EXPERT_FP8_E4M3
 * it takes MOE_IN / MOE_OUT too: rows = E * out, cols = in, scales [E * out] (expert e's rows e*out .. e*out + out - 1). */
int nvl_upload_tensor_fp8(nvl_model* m, int kind, int layer, const uint8_t* codes, const float* scales, int64_t rows,
                          int64_t cols, int layout);
/* MXFP4 storage of the projection weights: OCP e2m1 elements with one e8m0 scale per block of 32
 * consecutive input features of one output row.  The reference keeps every weight fp32 (generic_loader.go:398-403,
 * loadTensorFromData); this is the library's own opt-in, reached only through this call. */
enum {
    NVL_MX_NONE = 0,       /* no MX storage: today's behaviour                                                            */
    NVL_MX_FP4_E2M1 = 1    /* WQ/WK/WV/WKV/WO/W1/W2 as e2m1 codes.  Per 32-block: e = clamp(floor(log2(amax)) - 2, -120, 125)
                            * (0 for an all-zero block), stored as E = e + 127; q = e2m1_rne(|w| / 2^e) on {0, .5, 1, 1.5, 2, 3,
                            * 4, 6}, ties to the even mantissa bit, saturating at 6; the sign is bit 3.  Every path computes with
                            * W~ = +-grid[q] * 2^e (exact in bf16); nvl_get_weight returns W~; nvl_stats.weight_bytes counts
                            * codes + scales.  Embeddings, router and Mamba2 projections stay bf16; MoE experts too unless
                            * nvl_set_mx_expert_dtype(m, NVL_MXE_FP4_E2M1); the LM head and the tied token embedding too
                            * unless nvl_set_mx_head_dtype(m, NVL_MXH_FP4_E2M1). */
};
/* After nvl_create, before the first 2-D upload (else NVL_ERR_STATE).  NVL_ERR_INVALID for an unknown value, and for
 * NVL_MX_FP4_E2M1 with f32 precision, tensor parallelism or NVL_W_FP8_E4M3 (which in turn is refused once MX is set, and
 * with it nvl_set_act_dtype / nvl_set_expert_dtype).  In MX mode nvl_upload_tensor refuses a non-finite weight.
 * NVL_MX_NONE is refused (NVL_ERR_INVALID) while nvl_set_mx_expert_dtype holds NVL_MXE_FP4_E2M1 or nvl_set_mx_head_dtype
 * holds NVL_MXH_FP4_E2M1. */
int nvl_set_mx_weight_dtype(nvl_model* m, int dtype);
/* MoE expert weights (MOE_IN / MOE_OUT) of a model with MXFP4 projection weights. */
enum {
    NVL_MXE_NONE = 0,          /* the experts stay bf16 (also under NVL_MX_FP4_E2M1): today's behaviour                       */
    NVL_MXE_FP4_E2M1 = 1       /* MOE_IN / MOE_OUT as e2m1 codes under the contract of NVL_MX_FP4_E2M1: one e8m0 scale per 32
                                * consecutive input features of one (expert, output row), the same exponent rule, clamp, ties
                                * and saturation; W~ = +-grid[q] * 2^e on every path; nvl_get_weight returns W~;
                                * nvl_stats.weight_bytes counts codes + scales.  Decode streams the codes; prefill dequantizes
                                * one layer's experts at a time into a scratch buffer.  nvl_upload_tensor refuses a non-finite
                                * expert weight. */
};
/* After nvl_set_mx_weight_dtype(m, NVL_MX_FP4_E2M1), before the first expert upload and nvl_finalize (else NVL_ERR_STATE).
 * NVL_ERR_INVALID for a NULL model, an unknown value, a model without MoE, f32 precision, or no MXFP4 projection weights. */
int nvl_set_mx_expert_dtype(nvl_model* m, int dtype);
/* LM head and tied token embedding of a model with MXFP4 projection weights. */
enum {
    NVL_MXH_NONE = 0,          /* the LM head and the token embedding stay bf16 (also under NVL_MX_FP4_E2M1): today's behaviour */
    NVL_MXH_FP4_E2M1 = 1       /* LM_HEAD as e2m1 codes under the contract of NVL_MX_FP4_E2M1, byte for byte: one e8m0 scale per
                                * 32 consecutive input features of one output (vocabulary) row, the same exponent rule, clamp,
                                * ties and saturation; W~ = +-grid[q] * 2^e on every path.  TOK_EMB is stored the same way when
                                * tied_embedding is set (the rule of NVL_W_FP8_E4M3): the gathered embedding row is W~, exact in
                                * bf16, and the embedding multiplier and the learned position row (bf16) apply to it as always.
                                * An untied model whose LM head is absent runs the bf16 head on its bf16 embedding.  Position
                                * embedding, router and Mamba2 projections stay bf16.  nvl_get_weight returns W~ for both kinds;
                                * nvl_stats.weight_bytes counts codes + scales; nvl_upload_tensor refuses a non-finite head or
                                * embedding weight; nvl_upload_tensor_mxfp4 takes LM_HEAD, and TOK_EMB when tied (rows = vocab_size,
                                * cols = hidden). */
};
/* After nvl_set_mx_weight_dtype(m, NVL_MX_FP4_E2M1) and before the first 2-D upload (else NVL_ERR_STATE).  NVL_ERR_INVALID
 * for a NULL model, an unknown value, f32 precision, or no MXFP4 projection weights (which covers tensor parallelism and
 * NVL_W_FP8_E4M3).  While it holds NVL_MXH_FP4_E2M1, nvl_set_mx_weight_dtype(m, NVL_MX_NONE) is refused (NVL_ERR_INVALID). */
int nvl_set_mx_head_dtype(nvl_model* m, int dtype);
/* Pre-quantized MXFP4 weight, taken as it is: codes [rows][cols/2], two per byte with the even input feature in the low
 * nibble (OCP MX order), scales [rows][cols/32] e8m0 bytes, both in the checkpoint's [out, in] order (layout must be
 * NVL_LAYOUT_OUT_IN).  NVL_ERR_INVALID for a kind this model does not store as MXFP4, a shape mismatch, cols % 32 != 0,
 * and a scale byte outside [7, 252] (0xff is the e8m0 NaN).  With NVL_MXE_FP4_E2M1 it takes MOE_IN / MOE_OUT too: rows =
 * E * out, cols = in, codes [E * out][in / 2], scales [E * out][in / 32] (expert e's rows e*out .. e*out + out - 1). */
int nvl_upload_tensor_mxfp4(nvl_model* m, int kind, int layer, const uint8_t* codes, const uint8_t* scales, int64_t rows,
                            int64_t cols, int layout);
/* INT4 group-quantized storage of the projection weights: the W4A16 format of AWQ / GPTQ checkpoints.
 * The reference keeps every weight fp32 (generic_loader.go:398-403, loadTensorFromData); this is the library's own opt-in,
 * reached only through this call. */
enum {
    NVL_GQ_NONE = 0,       /* no group-quantized storage: today's behaviour                                                */
    NVL_GQ_UINT4 = 1       /* WQ/WK/WV/WKV/WO/W1/W2 as unsigned 4-bit codes with one fp16 scale s and one 4-bit zero point z per
                            * group of group_size (32, 64 or 128) consecutive input features of one output row; the input width
                            * must be a multiple of it.  Quantizer, per group, in fp32 with correctly rounded division and
                            * round-half-even: lo = min(0, min w), hi = max(0, max w), r = hi - lo; r == 0: s = 1, z = 0, q = 0;
                            * else s = fp16_rne(r / 15) (2^-24 if that rounds to 0), z = clamp(rint(-lo / s), 0, 15),
                            * q = clamp(rint(w / s) + z, 0, 15).  Every path computes with W~ = bf16_rne(fp32(s) * (q - z))
                            * (the product is exact in fp32: one rounding); nvl_get_weight returns W~.  nvl_stats.weight_bytes
                            * counts, per stored row (rows are padded to the weight row tile), in / 2 bytes of codes and
                            * 4 bytes per group: one 32-bit word {fp16 s, z}.  The LM head, both embeddings, the router and
                            * the Mamba2 projections stay bf16, as AWQ / GPTQ checkpoints keep them fp16; the MoE experts too
                            * unless nvl_set_gq_expert_dtype(m, NVL_GQE_UINT4). */
};
/* After nvl_create, before the first 2-D upload (else NVL_ERR_STATE).  NVL_ERR_INVALID for a NULL model, an unknown dtype, a
 * group_size outside {32, 64, 128}, and for NVL_GQ_UINT4 with f32 precision, tensor parallelism, NVL_W_FP8_E4M3 or
 * NVL_MX_FP4_E2M1 already set (each of those two setters in turn refuses once NVL_GQ_UINT4 is set).  In this mode
 * nvl_upload_tensor quantizes the covered kinds from F32 / BF16 / F16 in either layout (tensor.go:62-88 keeps them fp32) and
 * refuses a non-finite weight and a group with r / 15 > 65504. */
int nvl_set_gq_weight_dtype(nvl_model* m, int dtype, int group_size);
/* Pre-quantized INT4 weight, taken as it is (the loader's path for .qweight / .qzeros / .scales; generic_loader.go:398-403
 * reads fp32 only): codes [rows][cols/2], two per byte with the even input feature in the low nibble; scales
 * [rows][cols/group_size] as fp16 bit patterns; zeros [rows][cols/group_size] with values 0..15; all in [out, in] order
 * (layout must be NVL_LAYOUT_OUT_IN).  NVL_ERR_INVALID for a kind this model does not store this way, a shape mismatch,
 * cols % group_size != 0, a zero above 15, or a scale that is NaN, infinite or <= 0. */
int nvl_upload_tensor_int4(nvl_model* m, int kind, int layer, const uint8_t* codes, const uint16_t* scales, const uint8_t* zeros,
                           int64_t rows, int64_t cols, int layout);
/* MoE expert weights (MOE_IN / MOE_OUT) of a model with INT4 projection weights.  No checkpoint
 * reading comes with it: nvl_load_safetensors maps no AWQ / GPTQ MoE layout (the Granite mapping keeps its fused expert
 * tensors, which such checkpoints do not carry); the experts arrive through nvl_upload_tensor / nvl_upload_tensor_int4. */
enum {
    NVL_GQE_NONE = 0,          /* the experts stay bf16 (also under NVL_GQ_UINT4): today's behaviour                          */
    NVL_GQE_UINT4 = 1          /* MOE_IN / MOE_OUT under the contract of NVL_GQ_UINT4, byte for byte, with the model's own
                                * group size g: one {fp16 s, 4-bit z} word per g consecutive input features of one (expert,
                                * output row), the same quantizer (lo / hi include 0, r == 0 gives s = 1 and z = q = 0, the
                                * 2^-24 floor, rint, the clamps); W~ = bf16_rne(fp32(s) * (q - z)) on every path;
                                * nvl_get_weight returns W~; nvl_stats.weight_bytes counts codes + 4 bytes per group.  Decode
                                * streams the codes; prefill dequantizes one layer's experts at a time into a scratch buffer.
                                * nvl_upload_tensor quantizes the experts from F32 / BF16 / F16 and refuses a non-finite
                                * expert weight and a group with r / 15 > 65504.  nvl_upload_tensor_int4 takes MOE_IN / MOE_OUT
                                * too: rows = E * out, cols = in, codes [E * out][in / 2], scales and zeros [E * out][in / g]
                                * (expert e's rows e*out .. e*out + out - 1), under its usual validation. */
};
/* After nvl_set_gq_weight_dtype(m, NVL_GQ_UINT4, g), before the first expert upload and nvl_finalize (else NVL_ERR_STATE).
 * NVL_ERR_INVALID for a NULL model, an unknown value, a model without MoE, f32 precision, no INT4 projection weights, and
 * hidden % g != 0 or expert width % g != 0 (a group must not straddle two experts of the concatenated down matrix).  While
 * it holds NVL_GQE_UINT4, nvl_set_gq_weight_dtype refuses NVL_GQ_NONE and another group size (NVL_ERR_INVALID). */
int nvl_set_gq_expert_dtype(nvl_model* m, int dtype);

/* ---- lifecycle ---- */

/* Replaces tensor.NewTransformerModel (generic_model.go:41-61) + the runner's model ownership
 * (tensor_model_runner.go:21-33).  Fails with NVL_ERR_NO_DEVICE when no GPU is present. */
int nvl_create(const nvl_model_config* cfg, const nvl_runtime_opts* opts, nvl_model** out);

/* Replaces loadTensorFromData + the per-kind placement in loadAttention/loadFFN/loadMoE/loadNorm
 * (generic_loader.go:353-604,619-671).  `data` may be a host or a device pointer.  2-D kinds
 * take (rows, cols) in the order of `layout`; 1-D kinds rows = n, cols = 1; MoE kinds pass
 * rows = E*out, cols = in. */
int nvl_upload_tensor(nvl_model* m, int kind, int layer, const void* data, int dtype,
                      int64_t rows, int64_t cols, int layout);

/* Replaces tensor.LoadModelFromDirectory / LoadModel / LoadShardedModel (generic_loader.go:184-265, 1016-1163): `path`
 * is a .safetensors file, or a directory holding model.safetensors or model.safetensors.index.json + shards.  The
 * file is mmap'ed and every weight is handed to the device in the checkpoint's dtype (F32/F16/BF16) and [out, in]
 * layout: no fp32 host copy of the model, no host transposes.  The WeightMapping (:60-181) is chosen from the
 * checkpoint's tensor names (GPT-2 / Falcon / Llama / Granite-MoE); names are also tried with a "transformer."
 * prefix (:622-629).  Call between nvl_create and nvl_finalize. */
int nvl_load_safetensors(nvl_model* m, const char* path);
/* LoadModelConfig (generic_loader.go:808-972) over the New*Config templates (config.go:125-376): HF config.json (or
 * the reference's model_info.json) -> nvl_model_config.  Reference quirks kept: max_position_embeddings and
 * rope_scaling are not read.  Errors are reported through nvl_last_error(NULL). */
int nvl_load_config_json(const char* path, nvl_model_config* cfg);

/* Helpers for checkpoints that keep fused projections (generic_loader.go:674-765):
 * GPT-2 c_attn [H, 3H] split by columns; Falcon query_key_value given in the reference's
 * post-transpose form [H, (nH+2)*hd]; both fp32, host pointers. */
int nvl_upload_gpt2_qkv(nvl_model* m, int layer, const float* c_attn_w, const float* c_attn_b);
int nvl_upload_falcon_qkv(nvl_model* m, int layer, const float* qkv_in_out);

/* Freezes weights into the kernels' layouts, builds RoPE tables (rope.go:18-50, in fp64 on the
 * host exactly as the reference), allocates KV slots and workspaces. */
int nvl_finalize(nvl_model* m);

/* Replaces TensorModelRunner.Close (tensor_model_runner.go:114-117). */
void nvl_destroy(nvl_model* m);

/* ---- tensor parallelism (the reference's Config.TensorParallelSize is inert: nanovllm/config.go:61) ----
 * A model created with tp_size = T > 1 is rank tp_rank's shard: column-parallel Q/K/V and gate/up, row-parallel O and
 * down, one all-reduce (sum, fp32) after the O projection and one after the down projection; embeddings, norms and the
 * LM head are replicated, so every rank produces the same logits and the same greedy token.  Upload the FULL tensors:
 * each rank keeps its slice.  One process per GPU: rank 0 calls nvl_tp_get_unique_id, ships the 128 bytes to the other
 * ranks by any channel, and every rank calls nvl_tp_init (collective; RCCL over xGMI) before its first nvl_forward.
 * nvl_tp_attach_local joins the T shard models of ONE process on ONE device into an emulated group (each driven
 * from its own host thread) — used to test the sharded arithmetic where only one GPU exists. */
int nvl_tp_get_unique_id(void* id_out, int bytes);
int nvl_tp_init(nvl_model* m, const void* id, int bytes);
int nvl_tp_attach_local(nvl_model** models, int n);
/* Hand-written all-reduce over the xGMI mesh (csrc/tp_p2p.h) in place of ncclAllReduce: one-shot direct peer stores for
 * decode-sized payloads, reduce-scatter + all-gather on the mesh for prefill-sized ones, bf16 payload with fp32
 * accumulation in the bf16 mode, the residual add fused.  One process per GPU: every rank exports the IPC handle of its
 * comm buffer (64 bytes, after nvl_finalize), the host gathers the tp_size handles in rank order by whatever channel it has,
 * and every rank attaches them.  Both calls are collective in that sense.  RCCL (nvl_tp_init) stays available and is used
 * when no peer buffers are attached. */
int nvl_tp_p2p_export(nvl_model* m, void* handle_out, int bytes);                 /* bytes >= 64 */
int nvl_tp_p2p_attach(nvl_model* m, const void* handles, int bytes_per_handle);   /* tp_size handles, rank order */
/* A rank waits a bounded time for its peers inside an all-reduce (nvl_set_tuning key 29, milliseconds, default 30 000); when
 * the wait gives up the forward call fails and the group stays unusable until EVERY rank has called nvl_tp_p2p_rearm while
 * no rank is inside a forward call (collective in that sense). */
int nvl_tp_p2p_rearm(nvl_model* m);

/* ---- sequences: replace map[int64]*KVCache (tensor_model_runner.go:11-18,59-68,100-112) ---- */
int nvl_seq_open(nvl_model* m, int64_t seq_id);     /* get-or-create a KV slot                     */
int nvl_seq_reset(nvl_model* m, int64_t seq_id);    /* NewKVCache on prefill (:63-66)              */
int nvl_seq_close(nvl_model* m, int64_t seq_id);    /* ClearCache (:100-104)                       */
int nvl_seq_close_all(nvl_model* m);                /* ClearAllCaches (:107-111)                   */
int nvl_seq_len(nvl_model* m, int64_t seq_id);      /* cached tokens, or <0                        */

/* ---- the hot path ---- */
enum {
    NVL_FWD_ALL_LOGITS = 1u   /* logits for every row (what generic_model.go:467-470 computes);
                                 default is the last row of each sequence only (what every caller
                                 keeps: GetLogitsForLastToken, generic_model.go:595-604)            */
};

/* Batched replacement of TransformerModel.ForwardWithCache (generic_model.go:276-480) +
 * GetLogitsForLastToken (:595-604) + greedy argmax (cmd/ask/main.go:389-402) for n_seqs
 * independent sequences.  `tokens` is the concatenation of each sequence's NEW tokens
 * (seq_lens[i] of them, appended at position pos_offsets[i], which must equal the sequence's
 * cached length).  logits_out (optional) receives [n_seqs, V] (or [sum(seq_lens), V] with
 * NVL_FWD_ALL_LOGITS); argmax_out (optional) receives one greedy token per sequence. */
int nvl_forward(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens,
                const int32_t* seq_lens, const int32_t* pos_offsets, uint32_t flags,
                float* logits_out, int32_t* argmax_out);

/* ---- paged KV: the host's block manager owns the cache ---- */
/* One forward pass like nvl_forward, for a model created with kv_num_blocks > 0.  The KV cache of sequence i is the
 * block list block_tables[table_offsets[i] .. table_offsets[i+1]) (Sequence.BlockTable, sequence.go:23): position p
 * lives in its block p / block_size at row p % block_size.  pos_offsets[i] tokens are already cached — after a
 * prefix-cache hit that is Sequence.NumCachedTokens (block_manager.go:128-203), in decode len-1 — and only
 * seq_lens[i] new tokens are computed and written; blocks may be shared between sequences (same prefix), including
 * within one call.  The table must cover pos_offsets[i] + seq_lens[i] tokens.  The library keeps no per-sequence
 * state in this mode. */
int nvl_forward_paged(nvl_model* m, int n_seqs, const int32_t* tokens, const int32_t* seq_lens,
                      const int32_t* pos_offsets, const int32_t* block_tables, const int32_t* table_offsets,
                      uint32_t flags, float* logits_out, int32_t* argmax_out);
/* ModelRunner.Run for a block-table-aware runner: prefill computes tokens [num_cached_tokens[i], len) of each
 * sequence (all of them when num_cached_tokens is NULL; a fully cached prompt recomputes its last token), decode the
 * last token at len-1.  Greedy ids in next_tokens; sample with nvl_sample afterwards if wanted. */
int nvl_runner_run_paged(nvl_model* m, int n_seqs, const int32_t* const* token_ptrs, const int32_t* token_lens,
                         const int32_t* num_cached_tokens, const int32_t* const* block_table_ptrs,
                         const int32_t* block_table_lens, int is_prefill, int32_t* next_tokens, float* logits_out);
/* nvl_decode_greedy for a paged-KV model.  positions[i] = tokens already cached for sequence i; its block table must
 * cover positions[i] + n_steps tokens (the block manager allocates ahead).  out_tokens [n_steps][n_seqs]. */
int nvl_decode_greedy_paged(nvl_model* m, int n_seqs, const int32_t* first_tokens, const int32_t* positions, int n_steps,
                            const int32_t* block_tables, const int32_t* table_offsets, int32_t* out_tokens);
/* Debug/parity for paged mode: the K and V rows of `n_tokens` positions of one block list, as nvl_get_kv. */
int nvl_get_kv_paged(nvl_model* m, const int32_t* block_table, int n_blocks, int n_tokens, int layer, float* k_out,
                     float* v_out);

/* The greedy generation loop of cmd/ask (generateResponse, cmd/ask/main.go:315-360, without its EOS/"User" stop: the
 * caller truncates) for a batch, as ONE call: n_steps decode steps of one token per sequence starting from
 * first_tokens (the tokens sampled from the prefill), each step's device argmax fed back without a host round trip.
 * out_tokens receives [n_steps][n_seqs].  Same arithmetic, bit for bit, as n_steps calls of nvl_forward. */
int nvl_decode_greedy(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                      int32_t* out_tokens);

/* Greedy speculative decoding.  The reference generates one token per pass (cmd/ask/main.go:315-360: the
 * loop; generic_model.go:276-480: the pass); these calls run the same pass over 1 + k rows per sequence and keep the longest
 * draft prefix the model itself would have produced greedily.
 *
 * nvl_verify_greedy: tokens [n_seqs][1+k] — tokens[i][0] is sequence i's next input token (what first_tokens carries for
 * nvl_decode_greedy), tokens[i][1..k] the draft.  One pass at positions P_i .. P_i + k (P_i = the cached length); the greedy
 * id g[i][j] of every row is computed on the device, a_i = the length of the longest prefix with tokens[i][j+1] == g[i][j].
 * n_accepted_out[i] = a_i; out_tokens [n_seqs][1+k]: out_tokens[i][0..a_i] = g[i][0..a_i], the rest -1.  Afterwards the
 * cached length is P_i + a_i + 1 (rows behind it are dead and get overwritten).  Only n_seqs x (2 + k) int32 come back; the
 * n_seqs x (1+k) logits rows stay as the last forward group, in token order, for nvl_logprobs / nvl_sample.
 * In bf16 with a bf16 cache the pass runs the multi-position decode attention (nvl_set_tuning key 38); in f32 and over an
 * 8-bit cache it runs the existing kernels.  A pass of at most 64 rows whose shape was seen before is replayed as a graph.
 * k outside 1..7 or n_seqs x (1+k) > max_batch_tokens: NVL_ERR_INVALID; P_i + 1 + k > max_seq_len: NVL_ERR_POSITION; no
 * slot: NVL_ERR_UNKNOWN_SEQ; a model with Mamba2 layers (its state cannot be rolled back), a tensor-parallel model or a
 * paged model: NVL_ERR_STATE.  A refused call changes no length. */
int nvl_verify_greedy(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                      int32_t* n_accepted_out, int32_t* out_tokens);
/* nvl_verify_greedy for a paged-KV model: nvl_forward_paged's table arguments, pos_offsets[i] = P_i; the tables must cover
 * P_i + 1 + k tokens.  The library keeps no lengths in this mode: the caller advances by a_i + 1. */
int nvl_verify_greedy_paged(nvl_model* m, int n_seqs, const int32_t* tokens, int k, const int32_t* pos_offsets,
                            const int32_t* block_tables, const int32_t* table_offsets, int32_t* n_accepted_out,
                            int32_t* out_tokens);
/* Roll a slab sequence back to new_len <= its cached length (longer or negative: NVL_ERR_INVALID; a Mamba2 model or a
 * paged model: NVL_ERR_STATE). */
int nvl_seq_truncate(nvl_model* m, int64_t seq_id, int new_len);
/* Prompt-lookup drafting; pure host code, callable without a device.  For g = min(ngram, n-1) down to 1: the largest
 * s < n - g with history[s..s+g) == history[n-g..n); the draft is the tokens after that match, up to k of them, missing
 * entries repeating the last one taken.  No match at any g: every entry is history[n-1].  Returns the number of real
 * (unpadded) draft tokens, or NVL_ERR_INVALID (NULL, n < 1, k < 1). */
int nvl_lookup_draft(const int32_t* history, int n, int k, int ngram, int32_t* draft_out);
/* nvl_decode_greedy's contract (out_tokens [n_steps][n_seqs], cached length P_i + n_steps afterwards) driven by
 * nvl_lookup_draft + nvl_verify_greedy passes over the sequences that still need tokens; an overshoot of the last pass
 * is truncated.  history_ptrs[i] / history_lens[i]: the sequence's tokens as the first step sees them, ending with
 * first_tokens[i] (NULL: the history starts at first_tokens[i]).  passes_out (may be NULL): passes run, between
 * ceil(n_steps / (k+1)) and n_steps.  Slab mode only; refusals as nvl_verify_greedy; an error in a later pass leaves the
 * sequences where the passes before it put them.
 * Equivalence to nvl_decode_greedy: the ids are the same wherever the model's top-2 logit margin exceeds the precision's
 * stated logits tolerance (f32: always in practice).  1 + k rows take other projection forms than one row, so the
 * logits are not bit-identical. */
int nvl_decode_greedy_lookup(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                             int k, int ngram, const int32_t* const* history_ptrs, const int32_t* history_lens,
                             int32_t* out_tokens, int32_t* passes_out);

/* Debug/parity: copy the residual stream after layer `layer` of the LAST nvl_forward call,
 * [sum(seq_lens), H] fp32 (requires nvl_set_debug(m, 1 or 2) before the call).  Mode 1 completes every residual add in its
 * own launch (no split-K partials left to the next norm, no deferred RMSNorm, no graph replay): the layer outputs of a
 * simplified kernel sequence.  Mode 2 records the same values BESIDE the unmodified product path — kernel selection is
 * exactly what an untapped call runs; adds still pending for the next norm are included in the copy only. */
int nvl_set_debug(nvl_model* m, int keep_hidden);
int nvl_get_hidden(nvl_model* m, int layer, float* out, int64_t n_floats);
/* Measurement: nvl_set_debug(m, 4) makes the decode-sized projection and attention kernels of the following forward calls
 * (eager launches, no graph replay) record, per workgroup, the chip's 100 MHz constant clock at six points of their life —
 * entered / first loads issued / first data used / own stream done / workgroup's stream done / stores retired.
 * nvl_get_stamps returns the launches recorded so far: recs[3 i] = {site (nvl_kernel_site_name), phase, workgroups}, and the
 * stamps [workgroups][8] of the launches back to back.  scripts/decode_timeline.py prints the step's timeline from them.
 * Only in the diagnostic build of the library (make -C csrc diag -> libnvllm_hip_diag.so, -DNVL_STAMPS): the product library
 * has no stamp sites — compiled in and disabled they cost 3-7 % per decode projection — and answers mode 4 with
 * NVL_ERR_STATE.  The stamps perturb what they time (they pin the instruction schedule around them): use them to see where a
 * launch waits, and the kernel trace of the product build to decide whether a change paid. */
int nvl_get_stamps(nvl_model* m, int32_t* recs, int rec_cap, uint64_t* stamps, int64_t stamp_cap);
/* Debug/parity: copy a sequence's cache for one layer as the reference lays it out,
 * K and V each [nKV, T, hd] fp32 (kv_cache.go:5-6).  Returns T. */
int nvl_get_kv(nvl_model* m, int64_t seq_id, int layer, float* k_out, float* v_out);
/* Mamba2Layer.SSMState of a sequence's slot for a Mamba2 layer, [heads, head_dim, state] fp32 (mamba2.go:29-30; per
 * SEQUENCE here, per layer in the reference).  Returns the number of floats, or < 0. */
int nvl_get_mamba_state(nvl_model* m, int64_t seq_id, int layer, float* out);
/* The kept convolution rows of a sequence's slot for a Mamba2 layer (nvl_set_mamba_conv_state; also what the runner's chunked
 * prefill left): [K-1][conv_dim] fp32 raw xBC rows, oldest row first.  Returns the number of floats (0 when K == 1), or < 0. */
int nvl_get_mamba_conv_state(nvl_model* m, int64_t seq_id, int layer, float* out);
/* Debug/parity: read a 2-D weight back from the device as the reference holds it after loading ([in, out] fp32,
 * generic_loader.go:398-403) — whatever layout the kernels keep it in.  kind = NVL_T_*; out is [in_features][out_features].
 * Available between the upload and nvl_finalize for the projections finalize fuses (Q, K, V, KV, W1, MoE-in), at any
 * time for the others; a tensor-parallel rank returns its own slice.  Returns 0, or NVL_ERR_STATE when the tensor is gone.
 * This is how the reference's own fixture for this path (purego/tensor/falcon_split_test.go:7-158: the fused Falcon QKV
 * split) is replayed against nvl_upload_falcon_qkv itself (tests/test_loader_gpu.py). */
int nvl_get_weight(nvl_model* m, int kind, int layer, float* out, int64_t in_features, int64_t out_features);

/* ---- runner: ModelRunner.Run semantics (nanovllm/model_runner.go:9-16) ---- */
/* Replaces TensorModelRunner.Run (tensor_model_runner.go:55-97) for a scheduler batch:
 * token_ptrs[i]/token_lens[i] is Sequence.TokenIDs (full history).  is_prefill != 0 discards the
 * sequence's cache and processes the whole history from position 0 (:63-66,75); otherwise only
 * the last token at position len-1 (:78-80) — and a sequence the library holds no cache for (or
 * a stale one) is transparently re-prefilled.  Returns greedy tokens in next_tokens[n_seqs]
 * and, when logits_out != NULL, the last-row logits [n_seqs, V] for host-side sampling
 * (tensor.SampleWithHistory stays in Go: sampling.go:33-102). */
int nvl_runner_run(nvl_model* m, int n_seqs, const int64_t* seq_ids,
                   const int32_t* const* token_ptrs, const int32_t* token_lens,
                   int is_prefill, int32_t* next_tokens, float* logits_out);

/* ---- sampling on the device (tensor.SampleWithHistory, purego/tensor/sampling.go:33-102) ---- */
/* tensor.SamplingParams (sampling.go:10-15).  Reference quirks kept: temperature <= 0 or == 1 leaves the logits
 * unscaled (:71; there is no greedy branch), top_k <= 0 or >= V is "off" (:78), top_p >= 1 is "off" (:83), the
 * repetition penalty is multiplied by the token's count, the last 10 history tokens counting 3 (:46-66). */
typedef struct nvl_sampling_params {
    float   temperature;
    float   top_p;
    int32_t top_k;
    float   repetition_penalty;
} nvl_sampling_params;
/* Sample one id per logits row of the LAST nvl_forward / nvl_runner_run group (rows in that call's sequence order), on
 * the device: only ids cross PCIe.  history_ptrs[i]/history_lens[i] is the row's previousTokens (may be NULL/0);
 * uniforms[i] replaces the rand.Float32() draw of sampleMultinomial (sampling.go:205), so the Go host keeps its
 * math/rand stream: call rand.Float32() once per sequence, in order, and pass the values.  Sums run in a fixed tree
 * order instead of the reference's sequential one: the id can differ from the Go result only when r lies within
 * float rounding of a CDF step (tests/test_sampling_gpu.py states the bound). */
int nvl_sample(nvl_model* m, int n_rows, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
               const int32_t* history_lens, const float* uniforms, int32_t* out_tokens);
/* The decode loop of a sampling runner as ONE call (nvl_decode_greedy with SampleWithHistory instead of the argmax): each
 * of the n_steps steps samples one id per sequence on the device from the step's logits and the sequence's history
 * (Sequence.TokenIDs: history_ptrs/lens give it as the first step sees it, the sampled ids are appended on the device)
 * and feeds it back.  uniforms is [n_steps][n_seqs]: the rand.Float32() draws in the order the host's serial loop over
 * sequences (tensor_model_runner.go:58) would make them.  out_tokens [n_steps][n_seqs].  bf16 slab mode. */
int nvl_decode_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                       const nvl_sampling_params* params, const int32_t* const* history_ptrs, const int32_t* history_lens,
                       const float* uniforms, int32_t* out_tokens);
/* Sampled speculative decoding.  The reference runner never decodes greedily: every step ends in
 * SampleWithHistory(logits, seq.TokenIDs, defaultSampling) (tensor_model_runner.go:89-93, sampling.go:33-102), so these are
 * nvl_verify_greedy / nvl_decode_greedy_lookup under that sampler.  A prompt-lookup draft is a point mass, so exact
 * speculative sampling needs no rejection step: row j is SAMPLED from the model's own filtered distribution with that decode
 * step's draw, and the draft token is accepted iff it is the token drawn.  Given the same draws the emitted ids are the
 * ones the sequential sampler (nvl_sample step by step, nvl_decode_sampled) produces, up to what 1 + k rows per pass do to
 * the logits (nvl_decode_greedy_lookup's remark).
 *
 * nvl_verify_sampled (sampling.go:33-102 per row, tensor_model_runner.go:89-93): tokens [n_seqs][1+k] as nvl_verify_greedy.
 * history_ptrs[i] / history_lens[i] = Sequence.TokenIDs as row 0 sees it: it ends with tokens[i][0] (nvl_decode_sampled's
 * contract for first_tokens).  Row j of sequence i sees that history extended by tokens[i][1..j], read on the device from
 * the pass's own token rows; the "last 10 tokens count 3" window (sampling.go:46-66) runs over the concatenation.
 * uniforms [n_seqs][1+k]: uniforms[i][j] is the rand.Float32() draw of sequence i's decode step j counted from this pass.
 * Only the draws of rows 0..a_i are consumed; a caller who wants the Go host's math/rand stream unchanged passes the draws
 * of the rows behind the accepted prefix again, in order, as the first draws of that sequence's next pass.
 * s[i][j] = the sampled id; a_i = the longest prefix with tokens[i][j+1] == s[i][j]; n_accepted_out / out_tokens / the cached
 * length P_i + a_i + 1 / the logits rows left behind / graph replay (parameters, draws and histories are contents of device
 * buffers, never baked in) as nvl_verify_greedy.  f32 and bf16, every weight and KV mode; key 38 as there.
 * Refusals: nvl_verify_greedy's, and NVL_ERR_INVALID for a history that is missing or does not end with tokens[i][0],
 * history_lens[i] + k > max_seq_len, a negative history id, a uniform outside [0, 1], NaN parameters or
 * repetition_penalty == 0.  A refused call changes no length. */
int nvl_verify_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                       const nvl_sampling_params* params, const int32_t* const* history_ptrs, const int32_t* history_lens,
                       const float* uniforms, int32_t* n_accepted_out, int32_t* out_tokens);
/* nvl_verify_sampled (sampling.go:33-102, tensor_model_runner.go:89-93) for a paged-KV model: nvl_verify_greedy_paged's
 * table arguments.  No lengths are kept: the caller advances by a_i + 1. */
int nvl_verify_sampled_paged(nvl_model* m, int n_seqs, const int32_t* tokens, int k, const int32_t* pos_offsets,
                             const int32_t* block_tables, const int32_t* table_offsets, const nvl_sampling_params* params,
                             const int32_t* const* history_ptrs, const int32_t* history_lens, const float* uniforms,
                             int32_t* n_accepted_out, int32_t* out_tokens);
/* nvl_decode_sampled's contract (sampling.go:33-102 per step, tensor_model_runner.go:89-93; out_tokens [n_steps][n_seqs],
 * cached length P_i + n_steps afterwards) driven by nvl_lookup_draft + sampled verify passes over the sequences that still
 * need tokens, as nvl_decode_greedy_lookup drives the greedy ones (overshoot truncated, a last pass of one row).  uniforms
 * [n_steps][n_seqs]: decode step t of sequence i always uses uniforms[t][i], however the passes group the steps; draws of
 * unaccepted rows are not consumed.  The histories (required, each ending with first_tokens[i], ids inside the vocabulary:
 * drafts are taken from them) are uploaded once; the accept kernel appends what each pass emits, so a pass uploads only
 * drafts and draws.  f32 and bf16, slab mode only; refusals as nvl_verify_sampled, with history_lens[i] + n_steps >
 * max_seq_len refused too.  passes_out may be NULL. */
int nvl_decode_sampled_lookup(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int n_steps,
                              int k, int ngram, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                              const int32_t* history_lens, const float* uniforms, int32_t* out_tokens, int32_t* passes_out);
/* ---- speculative decoding with a draft MODEL ----
 * The reference draws one token per step from SampleWithHistory (sampling.go:33-102, tensor_model_runner.go:89-93).  With
 * proposals x ~ q from a second, smaller model the law of every emitted token stays the target's filtered distribution p
 * under the rejection rule: accept x with probability min(1, p(x) / q(x)), otherwise draw from norm(max(0, p - q)).  Both
 * steps run on the device over V-wide rows (csrc/spec.h): no distribution crosses PCIe.  The draws differ in meaning from the
 * sequential sampler's (an accept test is no multinomial draw), so the Go host's math/rand stream cannot be preserved here:
 * the emitted ids are a sample of the same law, not the ids rand.Float32() would have produced.
 *
 * nvl_draft_sampled: nvl_decode_sampled on the draft model with n_steps = k (1..7) - the same validation, the same ids bit
 * for bit, out_tokens [k][n_seqs], uniforms [k][n_seqs] - which also keeps every step's final distribution q_j (after
 * penalty, temperature, top-k, top-p and the renormalisation, sampling.go:33-102) on the device: k x n_seqs x
 * round_up(V, 4) floats, allocated on first use, freed by nvl_destroy.  The model records n_seqs, k, the sequence ids in
 * order and the sampled ids; any later forward-type call on it (nvl_forward*, nvl_decode_*, nvl_verify_*, nvl_score*,
 * nvl_runner_run*) invalidates them.  bf16 slab models only (nvl_decode_sampled's rule); a Mamba2 model is refused with
 * NVL_ERR_STATE (its state cannot be rolled back).  Synchronises before returning. */
int nvl_draft_sampled(nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens, int k,
                      const nvl_sampling_params* params, const int32_t* const* history_ptrs, const int32_t* history_lens,
                      const float* uniforms, int32_t* out_tokens);
/* The verify pass of that scheme (sampling.go:33-102 per row, tensor_model_runner.go:89-93).  tokens [n_seqs][1+k]:
 * tokens[i][0] the next input token, tokens[i][j+1] = d_j the id the draft sampled at step j (checked against the kept
 * proposals).  The target runs nvl_verify_sampled's pass: 1 + k rows, the sampler with the history extension, so p_j, row
 * j's final distribution, sees history ++ tokens[i][1..j]; histories as nvl_verify_sampled.  accept_uniforms [n_seqs][k],
 * final_uniforms [n_seqs], all in [0, 1].  Row j is accepted iff  accept_uniforms[i][j] * q_j(d_j) < p_j(d_j), product and
 * compare in fp32 as written (q_j(d_j) == 0 accepts iff p_j(d_j) > 0); a_i = the number of leading accepted rows.
 * a_i < k: the emitted id e is the first index whose running sum of r = max(p_a - q_a, 0) reaches final_uniforms[i] * sum(r)
 * (the sampler's multinomial scan, fallback V - 1; p_a itself should rounding leave sum(r) == 0).  a_i == k: e is that scan
 * of p_k - bit for bit what the sampler draws for row k with that uniform.  n_accepted_out [n_seqs] = a_i; out_tokens
 * [n_seqs][1+k] = d_0 .. d_{a_i - 1}, e, then -1 (nvl_verify_greedy's layout); accept_prob_out (may be NULL) [n_seqs][k][2] =
 * {p_j(d_j), q_j(d_j)} of every row, so a host can replay each decision.  Afterwards the target's cached length is
 * P_i + a_i + 1 and its n_seqs x (1+k) logits rows are the last forward group; the draft's cache is not touched (the
 * caller truncates it: nvl_seq_truncate).  f32 and bf16 targets, every weight and KV mode nvl_verify_sampled serves, key 38
 * as there; the pass is launched eagerly (no graph replay).
 * Refusals: nvl_verify_sampled's on the target; NVL_ERR_INVALID for draft == target (or a NULL model: no message is kept),
 * different devices, different vocab_size, a tokens[i][j+1] that is not the draft's id of step j, n_seqs / k / sequence
 * ids other than those of the kept proposals; NVL_ERR_STATE when the draft holds no valid proposals.  The message is kept
 * on the target.  A refused call changes no length on either model. */
int nvl_verify_speculative(nvl_model* target, nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, int k,
                           const nvl_sampling_params* params, const int32_t* const* history_ptrs, const int32_t* history_lens,
                           const float* accept_uniforms, const float* final_uniforms, int32_t* n_accepted_out,
                           int32_t* out_tokens, float* accept_prob_out);
/* nvl_decode_sampled's contract (sampling.go:33-102 per step, tensor_model_runner.go:89-93; out_tokens [n_steps][n_seqs])
 * from draft phases + speculative verify passes; both models end at the cached length P_i + n_steps and must hold every
 * sequence at the same cached length on entry (NVL_ERR_INVALID otherwise).  Pass scheduling as nvl_decode_sampled_lookup: the
 * sequences that still need tokens, k shrunk to the shortest remainder and to max_seq_len (of either model, the draft's
 * extra step and its history counted), overshoot cut,
 * a last pass of one row = a plain sampled step of the target.  uniforms [n_steps][n_seqs][2k+1]: pass t (there are at most
 * n_steps) gives sequence i its draft draws [0..k), its accept draws [k..2k) and its final draw [2k]; a pass of k' < k
 * drafts uses the first k' of each group.  Every pass the draft samples one step more than it proposes (that id is
 * discarded, its draw is 0): the step caches the row of the last proposal, so after any outcome the draft is rolled back
 * by truncation to the target's new length alone.  Histories (required, as nvl_decode_sampled_lookup) are restaged from
 * the host every pass.  passes_out and accepted_out [n_seqs] (the accepted drafts per sequence in total) may be NULL.  The
 * draft must be a bf16 slab model without Mamba2 layers (NVL_ERR_STATE); other refusals as nvl_verify_speculative.  Everything
 * that depends on the arguments is checked before the first pass; should a pass fail later (a HIP error), that pass is
 * undone on the draft (truncated to the target's length) while earlier passes stay: both models then hold the same lengths,
 * seq_len(target) - P_i ids of out_tokens' column i are valid. */
int nvl_decode_speculative(nvl_model* target, nvl_model* draft, int n_seqs, const int64_t* seq_ids, const int32_t* first_tokens,
                           int n_steps, int k, const nvl_sampling_params* params, const int32_t* const* history_ptrs,
                           const int32_t* history_lens, const float* uniforms, int32_t* out_tokens, int32_t* passes_out,
                           int32_t* accepted_out);
/* TensorModelRunner.Run including its sampling step (tensor_model_runner.go:55-97): nvl_runner_run, then
 * SampleWithHistory(lastTokenLogits, seq.TokenIDs, defaultSampling) per sequence on the device. */
int nvl_runner_run_sampled(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* const* token_ptrs,
                           const int32_t* token_lens, int is_prefill, const nvl_sampling_params* params,
                           const float* uniforms, int32_t* next_tokens);

/* ---- log-probabilities on the device (no reference counterpart: cmd/check-logits/main.go prints raw
 * logits, generic_model.go:467-470 computes every row's and :595-604 keeps the last) ----
 * Per logits row, with x' the final logits (LogitsScaling applied, generic_model.go:473-477):
 *   logprob = x'_t - logsumexp(x') for the row's target id t (t = -1: no target, +0.0f is written),
 *   argmax  = the greedy id (first strict maximum, cmd/ask/main.go:389-402; the id nvl_forward's argmax_out carries),
 *   the top_k (0..8) most probable ids and their log-probabilities, value descending then id ascending ([rows][top_k];
 *   entry 0 is the argmax; a row with fewer than top_k logits above -inf pads with id -1, -inf).
 * The sums run in fp32 in a fixed tree order (reproducible bit for bit); |logprob error| <= 1e-5 + 2^-21 max|x'| against
 * float64 on the same logits.  Any output pointer may be NULL; targets may be NULL (= all -1). */
/* The rows of the LAST forward group — exactly the rows nvl_sample sees, in that order (generic_model.go:595-604: one per
 * sequence, or every row after NVL_FWD_ALL_LOGITS, generic_model.go:467-470) — after nvl_forward (replayed decode passes
 * included), nvl_forward_paged, nvl_runner_run*, nvl_decode_*; f32 and bf16; on a tensor-parallel rank too (the logits are
 * replicated).  n_rows > the rows left, top_k outside [0, 8] or a target outside [-1, V): NVL_ERR_INVALID. */
int nvl_logprobs(nvl_model* m, int n_rows, const int32_t* targets, int top_k, float* logprob_out, int32_t* argmax_out,
                 int32_t* topk_ids_out, float* topk_logprob_out);
/* nvl_forward (generic_model.go:276-480; the same validation, KV append and Mamba2 state update, so a long document can be
 * scored over several calls and decoding can go on afterwards) returning, per NEW token row (generic_model.go:467-470: all
 * sum(seq_lens) of them), the quantities above instead of logits: targets / logprob_out / argmax_out are [sum(seq_lens)],
 * the top-k outputs [sum(seq_lens)][top_k].  Final norm + LM head + reduction run over chunks of at most R rows
 * (nvl_set_tuning key 37, default 1024): the device never holds more than R x Vpad logits, and 4 x (2 + 2 top_k) bytes per
 * row cross PCIe.  The pass takes the all-rows path (no deferred final norm, no graph replay) in every weight / KV /
 * activation mode of the model.  Afterwards no logits rows are left: nvl_sample / nvl_logprobs answer NVL_ERR_INVALID
 * until the next forward; the next token of a sequence is argmax_out of its last row.  Tensor-parallel models:
 * NVL_ERR_STATE. */
int nvl_score(nvl_model* m, int n_seqs, const int64_t* seq_ids, const int32_t* tokens, const int32_t* seq_lens,
              const int32_t* pos_offsets, const int32_t* targets, int top_k, float* logprob_out, int32_t* argmax_out,
              int32_t* topk_ids_out, float* topk_logprob_out);
/* nvl_score over block tables: nvl_forward_paged's arguments (generic_model.go:276-480 through Sequence.BlockTable,
 * sequence.go:23), then nvl_score's. */
int nvl_score_paged(nvl_model* m, int n_seqs, const int32_t* tokens, const int32_t* seq_lens, const int32_t* pos_offsets,
                    const int32_t* block_tables, const int32_t* table_offsets, const int32_t* targets, int top_k,
                    float* logprob_out, int32_t* argmax_out, int32_t* topk_ids_out, float* topk_logprob_out);

/* ---- measurement (the reference only has wall-clock prints: cmd/ask/main.go:196-198) ---- */
typedef struct nvl_stats {
    uint64_t forward_calls, prefill_tokens, decode_tokens;
    double   prefill_ms, decode_ms;       /* device time of nvl_forward calls, by phase (HIP events) */
    /* per-kernel-class device time, only when nvl_set_profile(m, 1): HIP events around each launch */
    double   gemm_ms, gemm_flops;         /* all MFMA projection GEMMs (QKV, O, FFN, LM head)         */
    uint64_t gemm_launches;
    double   attn_ms, attn_flops;
    uint64_t attn_launches;
    double   other_ms;                    /* norms, RoPE/KV write, activation, embedding, argmax      */
    uint64_t other_launches;
    double   weight_bytes;                /* bytes of weights resident on the device                  */
    uint64_t evictions;                   /* KV slots reclaimed from the least-recently-forwarded sequence by
                                             nvl_runner_run / _sampled when every slot was taken            */
    uint64_t graph_replays;               /* decode passes issued as ONE hipGraphLaunch (a pass whose launch configuration was
                                             seen before is captured once and replayed; nvl_set_tuning key 21 = 0 turns it off) */
} nvl_stats;
/* Per-launch-site view of the same events (nvl_set_profile on): one entry per (phase, site) that launched — QKV / O /
 * FFN-up / FFN-down projections, attention, LM head, norms, MoE stages ... — with its launch count, summed device time
 * and summed ALGORITHMIC work (flops, bytes: every weight byte once + operands in / results out; attention: every
 * cached key and value once), so a caller can print achieved TFLOP/s or GB/s per kernel next to the roofline. */
typedef struct nvl_kernel_stat {
    int32_t  site;        /* name: nvl_kernel_site_name(site) */
    int32_t  phase;       /* 0 = prefill passes (some sequence carried more than one token), 1 = decode passes */
    uint64_t launches;
    double   ms, flops, bytes;
} nvl_kernel_stat;
int nvl_get_kernel_stats(nvl_model* m, nvl_kernel_stat* out, int cap);   /* returns the number of entries (may exceed cap) */
const char* nvl_kernel_site_name(int site);
int nvl_set_profile(nvl_model* m, int per_kernel_events);
int nvl_get_stats(nvl_model* m, nvl_stats* out);
int nvl_reset_stats(nvl_model* m);

const char* nvl_last_error(const nvl_model* m);   /* m may be NULL: last error of nvl_create */
int nvl_abi_version(void);
int nvl_device_count(void);                        /* number of visible HIP devices, 0 if none */
int nvl_sizeof(int which);                         /* 0 nvl_model_config, 1 nvl_runtime_opts, 2 nvl_stats: lets a
                                                      binding (cgo/ctypes) verify its struct mirrors */

/* ---- op-level entry points (host fp32 in / host fp32 out; used by the parity tests) ----
 * Each runs the SAME device kernel the model path uses, on one op, in `precision`. */
/* MatMul tensor.go:62-88: c[m,n] = a[m,k] x b[k,n] (b in the reference's [in,out] layout) */
int nvl_op_matmul(int device, int precision, const float* a, const float* b, float* c,
                  int m, int k, int n);
/* LayerNorm tensor.go:193-250 (bias == NULL => RMSNorm) */
int nvl_op_layernorm(int device, const float* x, const float* w, const float* bias, float eps,
                     float* y, int rows, int hidden);
/* Softmax tensor.go:128-160 over the last dim */
int nvl_op_softmax(int device, const float* x, float* y, int rows, int cols);
/* GELU tensor.go:181-190 / SiLU mamba2.go:360-367 */
int nvl_op_gelu(int device, const float* x, float* y, int64_t n);
int nvl_op_silu(int device, const float* x, float* y, int64_t n);
/* ApplyRoPESingleTensor rope.go:153-205 on t [heads, seq, hd] in place */
int nvl_op_rope(int device, float* t, int heads, int seq, int hd, int start_pos, double base,
                int max_seq);
/* GQA/MQA/MHA core on projected heads (attention.go:354-470, mqa.go:184-243):
 * q [nH,S,hd], k/v [nKV,T,hd] (keys 0..T-1, the last S are the new tokens) -> out [nH,S,hd] */
int nvl_op_attention(int device, int precision, const float* q, const float* k, const float* v,
                     int nH, int nKV, int S, int T, int hd, float scale, float* out);
/* The multi-position decode attention of a verify pass (generic_model.go:276-480 over S = 2..8 new positions of one
 * sequence; attn.h attn_decode_mq_bf16_kernel) alone, bf16, whatever nvl_set_tuning key 38 says: nvl_op_attention's
 * argument conventions. */
int nvl_op_attention_mq(int device, const float* q, const float* k, const float* v, int nH, int nKV, int S, int T, int hd,
                        float scale, float* out);
/* Mamba2Layer.Forward between its two projections (mamba2.go:107-170; mamba.h) through the model's own dispatch: causal
 * conv + SiLU and softplus(dt), the scan (sequential, or in bf16 the chunked SSD forms that nvl_set_tuning key 30 selects),
 * gate + RMS norm.  proj [M][EH + conv_dim + nh] (EH = nh x hd, conv_dim = EH + 2 x ng x ss) holds the token rows of
 * n_seqs sequences back to back, sequence i with seq_len[i] tokens from position seq_pos[i] in state slot seq_slot[i]
 * (distinct, < n_slots).  conv_w [conv_dim][K]; conv_b, a_log, D, dt_bias, norm_w may be NULL.  state
 * [n_slots][nh][hd][ss] and tail [n_slots][K-1][conv_dim] (may be NULL) are read and written in place; chain 0 / 1 / 2 is
 * the conv tail of a chained prefill (mamba.h MambaArgs::chain), non-zero only with n_seqs == 1; chain 3 is the carried window
 * of NVL_MAMBA_CONV_CARRIED for any n_seqs (a tail is required when K > 1; with every seq_len == 1 and nvl_set_tuning key 39
 * at 1 the pass runs mamba_conv_step_kernel).  Out: xbc [M][conv_dim],
 * delta [M][nh], y [M][EH] before gating, normed [M][EH] (bf16: the rounded out_proj operand).  A geometry the kernels do
 * not cover is NVL_ERR_INVALID, before anything is launched. */
int nvl_op_mamba_mixer(int device, int precision, const float* proj, int n_seqs, const int32_t* seq_len,
                       const int32_t* seq_pos, const int32_t* seq_slot, int n_slots, int nh, int hd, int ss, int ng, int K,
                       const float* conv_w, const float* conv_b, const float* a_log, const float* D, const float* dt_bias,
                       const float* norm_w, float* state, float* tail, int chain, float* xbc, float* delta, float* y,
                       float* normed);
/* 8-bit KV cache.  The device quantizer and read path on an array: codes[i] = e4m3fn(x[i] / scale)
 * (round-to-nearest-even, saturating to +-448, NaN -> NaN code), back[i] = scale * bf16(codes[i]) in fp32. */
int nvl_op_fp8_kv_roundtrip(int device, const float* x, int64_t n, float scale, uint8_t* codes, float* back);
/* nvl_op_attention (bf16 only) over an 8-bit cache: k / v are quantized on the device with k_scale / v_scale by the
 * same quantizer, then the 8-bit attention kernels run (S == 1: decode kernel, key split at long T; else prefill). */
int nvl_op_attention_kv8(int device, const float* q, const float* k, const float* v, int nH, int nKV, int S, int T,
                         int hd, float scale, float k_scale, float v_scale, float* out);
/* The attention of one layer on a BATCH laid out as the paged front end lays it out (generic_model.go:276-480 over
 * block_manager.go's block tables), through the model's own attention dispatch: n_seqs sequences, sequence i with
 * seq_len[i] new rows (token rows back to back in sequence order) behind seq_pos[i] cached keys; row j sees keys
 * 0 .. seq_pos[i] + j.  k_pool / v_pool [n_blocks][nKV][block_size][hd] (block_size % 64 == 0) are the layer's K / V
 * blocks, block_table [n_seqs][tbl_stride] names each sequence's blocks and reaches the kernels verbatim, unused
 * entries included.  Set up as a model has it: the longest context as the decode-attention hint, the split-K scratch and
 * its zeroed tickets; the output rows and that scratch start as 0xFF bytes (NaN), so `out` is finite only if nothing
 * unwritten was read.  Every seq_len == 1 takes the decode kernels, otherwise the prefill kernels; nvl_set_tuning keys 15 /
 * 25 / 35 act as in a model.  `form`:
 *   NVL_ATTN_OP_PLAIN  q [tokens][nH][hd], K / V of the new rows already in the pools (bf16 or f32)
 *   NVL_ATTN_OP_FUSED  bf16, every seq_len == 1: q holds the fp32 QKV rows [n_seqs][(nH + 2 nKV) hd]; the decode kernel
 *                      applies RoPE (tables [max_seq][hd] for rope_base; rope_base == 0: none), patches the new key into
 *                      its tile and appends K / V to the pools, which are written back to k_pool / v_pool as fp32
 *   NVL_ATTN_OP_MQ     bf16: PLAIN with the verify pass's flag (2..8 rows per sequence run the multi-position kernel)
 *   NVL_ATTN_OP_KV8    bf16: the pools are quantized with k_scale / v_scale by the cache's own quantizer first
 * Out: out [tokens][nH][hd]; ran[3] = {NVL_ATTN_RAN_* of the kernel that ran, waves per workgroup, workgroups per
 * (sequence, kv head) of a key split}; part_cnt [32], the split's tickets after the launch (all zero again).
 * Refused before anything is launched: what the paged front end refuses — a negative position (NVL_ERR_INVALID),
 * seq_pos + seq_len > max_seq (NVL_ERR_POSITION), a table too short for seq_pos + seq_len — and ANY table entry outside
 * [0, n_blocks).  More than 128 table entries per sequence are refused by the bf16 prefill kernel's launch. */
enum { NVL_ATTN_OP_PLAIN = 0, NVL_ATTN_OP_FUSED = 1, NVL_ATTN_OP_MQ = 2, NVL_ATTN_OP_KV8 = 3 };
enum {
    NVL_ATTN_RAN_F32 = 1,             /* attn_f32_kernel */
    NVL_ATTN_RAN_PREFILL = 2,         /* attn_prefill_bf16_kernel */
    NVL_ATTN_RAN_PREFILL_KV8 = 3,     /* attn_prefill_kv8_kernel */
    NVL_ATTN_RAN_DECODE = 4,          /* attn_decode_bf16_kernel, Q / K / V prepared by earlier launches */
    NVL_ATTN_RAN_DECODE_FUSED = 5,    /* attn_decode_bf16_kernel with RoPE + append */
    NVL_ATTN_RAN_DECODE_KV8 = 6,      /* attn_decode_kv8_kernel */
    NVL_ATTN_RAN_DECODE_MQ = 7,       /* attn_decode_mq_bf16_kernel */
    NVL_ATTN_RAN_DECODE_STAMPED = 8   /* the diagnostic instantiation of the fused form (nvl_set_debug mode 4) */
};
int nvl_op_attention_batch(int device, int precision, int form, int nH, int nKV, int hd, float scale, int n_seqs,
                           const int32_t* seq_len, const int32_t* seq_pos, float* k_pool, float* v_pool, int n_blocks,
                           int block_size, const int32_t* block_table, int tbl_stride, const float* q, double rope_base,
                           int max_seq, float k_scale, float v_scale, float* out, int32_t* ran, int32_t* part_cnt);
/* The FRONT of an attention layer as a layer of the model runs it, stage by stage (generic_model.go:295-302 embedWithOffset,
 * :304-318 attention norm, the QKV projection with its bias, rope.go:153-205 on Q and K, Q into the attention operand
 * buffer, K / V into the paged cache): the forward pass's own embed() and qkv_front() on a batch laid out as the paged
 * front end lays it out (see nvl_op_attention_batch: seq_len / seq_pos / block_table [n_seqs][tbl_stride] / n_blocks /
 * block_size / max_seq mean the same), set up as nvl_create sets a paged model up (Tmax = block_size, blocks_per_seq =
 * tbl_stride, one layer).  qkv_front() takes the model's decisions — the fused-epilogue tile kernels (EPI_QKV), the
 * decode-form projection + rope_kv_kernel for up to 64 rows and for the short-prefill row groups (nvl_set_tuning key 18),
 * rope_kv8_kernel for an 8-bit cache, the fp32 kernels, and a bf16 decode step, where the projection only stores fp32 rows
 * because the attention kernel does RoPE and the append — and nvl_set_tuning keys 0 / 11 / 18 act as in a model.
 * The op runs the NON-DEFERRED operand path only: the deferred-RMSNorm operand into the QKV projection is held by
 * nvl_op_dense_stages (yn with has_next = 1), the fused decode append by nvl_op_attention_batch (NVL_ATTN_OP_FUSED).
 * In: x [tokens][hidden], the residual stream; norm_w (/ norm_b for NVL_NORM_LAYER) [hidden] — norm_w == NULL: x is the
 * normed operand already (as behind the decode seam), rounded to the operand type on upload, no norm runs; w_qkv
 * [(nH + 2 nKV) hd][hidden], b_qkv or NULL; rope_base (0: no RoPE, the tables stay NULL); k_pool / v_pool
 * [n_blocks][nKV][block_size][hd], the layer's cache before the pass (kv8: quantized with k_scale / v_scale by the cache's
 * own quantizer first; bf16 only).  The embedding stage, when tokens != NULL: tokens / tok_pos [tokens], emb [vocab][hidden],
 * pos_emb [pos_rows][hidden] or NULL, embedding_multiplier (0 = none); x is then an OUTPUT.
 * Every output and scratch buffer is 0xFF bytes (NaN) beforehand.  Out: op [tokens][hidden], the projection's operand rows as
 * fp32; qkv [tokens][n_qkv], the fp32 projection (the store forms; NaN in the epilogue form); q [round_up(tokens, 256)][nH
 * hd], the WHOLE operand buffer (rows from tokens on stay NaN); k_pool / v_pool after the pass as fp32 (kv8: scale *
 * e4m3(code), and the raw codes in k_codes / v_codes [n_blocks][nKV][block_size][hd], either may be NULL); ran
 * [NVL_QKV_RAN_INTS].  Refused before anything is launched, with NVL_ERR_INVALID / NVL_ERR_POSITION as nvl_op_attention_batch
 * refuses: a bad shape, a negative position, seq_pos + seq_len > max_seq, a table too short, ANY table entry outside
 * [0, n_blocks), a token id outside [0, vocab). */
enum { NVL_QKV_RAN_FORM = 0, NVL_QKV_RAN_GEMM = 1, NVL_QKV_RAN_NORM = 2, NVL_QKV_RAN_EMBED = 3, NVL_QKV_RAN_INTS = 4 };
enum {      /* ran[NVL_QKV_RAN_FORM] */
    NVL_QKV_FORM_F32_STORE_ROPE = 1,        /* gemm_f32_kernel + rope_kv_kernel<float> */
    NVL_QKV_FORM_DECODE_STORE_ROPE = 2,     /* decode-form projection (<= 64 rows) + rope_kv_kernel<bf16> */
    NVL_QKV_FORM_GROUPS_STORE_ROPE = 3,     /* ... over 64-row groups (short prefill) + rope_kv_kernel<bf16> */
    NVL_QKV_FORM_EPILOGUE = 4,              /* a tile kernel with the EPI_QKV epilogue */
    NVL_QKV_FORM_STORE_ROPE_KV8 = 5,        /* projection + rope_kv8_kernel */
    NVL_QKV_FORM_STORE_ONLY = 6             /* a bf16 decode step: the projection alone (the pools stay as they were) */
};
enum {      /* ran[NVL_QKV_RAN_GEMM]: the instance launch_gemm_bf16 launched (0: none of them, e.g. the fp32 kernel) */
    NVL_GEMM_RAN_NONE = 0,
    NVL_GEMM_RAN_TILE1 = 1,                 /* 128x128, two stages */
    NVL_GEMM_RAN_TILE2 = 2,                 /* 256x128, three stages */
    NVL_GEMM_RAN_TILE3 = 3,                 /* 256x256 as 2x4 waves */
    NVL_GEMM_RAN_PINGPONG = 5,              /* the ping-pong 256x256 kernel */
    NVL_GEMM_RAN_HD128_4X2 = 6,             /* EPI_QKV, head_dim 128: 256x256 as 4x2 waves */
    NVL_GEMM_RAN_HD128_PINGPONG = 7,        /* EPI_QKV, head_dim 128: the ping-pong kernel, wave tile 64x128 */
    NVL_GEMM_RAN_DECODE = 8,                /* the decode kernels, up to 64 rows */
    NVL_GEMM_RAN_GROUPS = 9                 /* the decode kernels over 64-row groups */
};
enum {      /* ran[NVL_QKV_RAN_NORM]: 0 = no norm ran, else NVL_NORM_RAN_* (NVL_NORM_RAN_WAVE: norm_kernel);
             * ran[NVL_QKV_RAN_EMBED]: 0 = no embedding stage */
    NVL_EMBED_RAN_F32 = 1, NVL_EMBED_RAN_BF16 = 2, NVL_EMBED_RAN_W8 = 3, NVL_EMBED_RAN_W4 = 4
};
typedef struct nvl_qkv_stages {
    int32_t struct_bytes;           /* sizeof(nvl_qkv_stages) */
    int32_t kv8, nH, nKV, hd, hidden;
    int32_t n_seqs, tbl_stride, n_blocks, block_size, max_seq;
    int32_t norm_type, vocab, pos_rows;
    float norm_eps, k_scale, v_scale, embedding_multiplier;
    double rope_base;
    const int32_t *seq_len, *seq_pos, *block_table, *tokens, *tok_pos;
    const float *norm_w, *norm_b, *w_qkv, *b_qkv, *emb, *pos_emb;
    float *x, *op, *qkv, *q, *k_pool, *v_pool;
    uint8_t *k_codes, *v_codes;
    int32_t* ran;
} nvl_qkv_stages;
int nvl_op_qkv_stages(int device, int precision, const nvl_qkv_stages* io);
/* 8-bit weights: tensor.MatMul (tensor.go:62-88) with b = w [K][N] quantized by the model's upload quantizer
 * (NVL_W_FP8_E4M3), c [M][N] = bf16(a) · W~ through the model's own GEMM dispatch (M selects the decode or the tile form).
 * codes_out [N][K] / scales_out [N] (either may be NULL) receive the quantized weight.  K % 64 == 0. */
int nvl_op_matmul_fp8w(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* codes_out,
                       float* scales_out);
/* MXFP4 weights (NVL_MX_FP4_E2M1): as nvl_op_matmul_fp8w — w [K][N] quantized by the upload quantizer, c = bf16(a) · W~
 * through the model's dispatch (M selects the decode kernels, the 64-row groups or dequantize + tile).  K % 64 == 0.
 * codes_out [N][K/2] and scales_out [N][K/32] (either may be NULL) return the codes in nvl_upload_tensor_mxfp4's packing. */
int nvl_op_matmul_mxfp4w(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* codes_out,
                         uint8_t* scales_out);
/* INT4 group-quantized weights (NVL_GQ_UINT4; the reference multiplies fp32 weights, tensor.go:62-88): as nvl_op_matmul_mxfp4w —
 * w [K][N] quantized by the upload quantizer with this group_size, c = bf16(a) · W~ through the model's own dispatch.
 * K % 64 == 0 and K % group_size == 0.  codes_out [N][K/2], scales_out [N][K/group_size] (fp16 bits) and zeros_out
 * [N][K/group_size] (any may be NULL) return the quantizer's result in nvl_upload_tensor_int4's packing. */
int nvl_op_matmul_int4w(int device, const float* a, const float* w, int M, int N, int K, int group_size, float* c,
                        uint8_t* codes_out, uint16_t* scales_out, uint8_t* zeros_out);
/* 8-bit weights and activations (NVL_ACT_FP8_E4M3): as nvl_op_matmul_fp8w, through the model's dispatch in W8A8 mode.  M
 * selects the decode form (bf16(a) · W~, bit-identical to nvl_op_matmul_fp8w) or the tile form, where bf16(a) is quantized
 * per row and c = (sum_k e4m3(q_a) e4m3(q_w)) * s_a[m] * s_w[n].  a_codes_out [M][K] / a_scales_out [M] (either may be NULL)
 * receive the activation quantization of the tile form (zeros and ones when the decode form ran).  K % 64 == 0. */
int nvl_op_matmul_w8a8(int device, const float* a, const float* w, int M, int N, int K, float* c, uint8_t* a_codes_out,
                       float* a_scales_out);
/* The activation quantizer of the W8A8 tile step alone: a [M][K] fp32 is rounded to bf16 and stored as the fragment-major
 * operand of a K-wide row (lda >= K, lda % 64 == 0; the columns past K hold a % 7 junk), then quantized reading K columns
 * with row-tile stride 16 * lda.  codes [M][K] / scales [M] as nvl_op_matmul_w8a8 returns them. */
int nvl_op_act_quant_fp8(int device, const float* a, int M, int K, int lda, uint8_t* codes, float* scales);
/* FeedForward.Forward transformer.go:40-96 (w1 [H,2F] gate|up or [H,F]; w2 [F,H]) */
int nvl_op_ffn(int device, int precision, const float* x, const float* w1, const float* b1,
               const float* w2, const float* b2, int rows, int hidden, int ffn, int swiglu,
               float* y);
/* MoELayer.Forward moe.go:43-128 with separate experts (:167-226) */
int nvl_op_moe(int device, int precision, const float* x, const float* router, const float* w_in,
               const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter,
               float* y);
/* MoELayer.Forward moe.go:43-128 as a layer of the MODEL runs it (bf16 only; NVL_PRECISION_F32 is NVL_ERR_INVALID), with
 * its stages: the op sets up what finalize and the workspace allocation set up (the experts' down matrices side by side
 * along K where finalize would build them, the decode scratch, no debug taps), calls the model's MoE dispatch on a zeroed
 * residual stream with multiplier 1, and completes what that leaves pending for the next norm the way debug mode 2 reads
 * it.  So rows <= 64 take the decode ("dense-masked") form wherever a model would, and nvl_set_tuning keys 31 / 22 / 8 /
 * 2 / 16 / 17 select the other forms.  Every scratch buffer the forms own is filled with 0xFF bytes (NaN as bf16 and as
 * fp32) before the call: a read of something no launch wrote shows in y.  hidden % 64 == 0, inter % 32 == 0, n_experts <=
 * 64.  (A sorted form on inter % 64 == 32 — a width nvl_create refuses — runs on experts zero-padded to inter + 32.)
 * Out: y [rows][hidden]; router_logits [rows][n_experts], the fp32 logits the routing consumed; gate [rows][n_experts],
 * the renormalised routing weight of (token, expert), 0 where the token did not pick the expert (moe.go:63-103; the
 * sorted forms' expert ids / weights scattered on the host); *form, what ran. */
enum {
    NVL_MOE_FORM_DENSE_FUSED = 1,   /* dense-masked, router + routing in one launch */
    NVL_MOE_FORM_DENSE = 2,         /* dense-masked, router GEMM then the gate-matrix launch */
    NVL_MOE_FORM_PLAN = 3,          /* sort-based: one planning launch, grouped GEMMs */
    NVL_MOE_FORM_GROUPED = 4        /* sort-based: route / histogram / scan / scatter launches, grouped GEMMs */
};
int nvl_op_moe_stages(int device, int precision, const float* x, const float* router, const float* w_in,
                      const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter,
                      float* y, float* router_logits, float* gate, int32_t* form);
/* The dense layer tail of generic_model.go:320-326,383-418 as a layer of the model runs it, stage by stage, bf16 mode only:
 * O projection, FFN norm, FFN-up, FFN-down, the norm after the layer and the projection that reads it.  The op executes the
 * model's own decisions (which projection carries the next norm — the deferred RMSNorm —, which is split over K and left
 * pending for the next norm, the parallel block's order) through the code the forward pass runs, on workspaces sized as
 * nvl_create sizes them for max_batch_tokens = rows, every scratch buffer and output 0xFF bytes (NaN) beforehand.
 * In: x [rows][hidden] the residual stream before the O projection; attn_out [rows][q_width]; wo [hidden][q_width], bo;
 * norm_w / norm_b [hidden], the FFN norm (parallel block: the block's one norm, run first); w1 [2 ffn][hidden] (SwiGLU: gate
 * rows, then up rows) or [ffn][hidden] (GELU), b1 [ffn]; w2 [hidden][ffn], b2; next_norm_w / next_norm_b, the norm after the
 * layer; wn [n_next][hidden], the projection behind it (n_next need not be a multiple of anything).  Biases may be NULL
 * (LayerNorm needs its two).  residual_multiplier 0 = 1 (as in a model config); a parallel block applies its two multipliers
 * only when both are non-zero.  max_len = 1: a decode pass.  has_next = 1: a layer follows (its attention norm, wn its
 * QKV); 0: the last layer — the final norm on last_rows [n_last_rows] (a decode pass lists every row) and wn as the LM head.
 * Out: x1 / x2 [rows][hidden], x after the O projection / after FFN-down (a pending add completed as the debug tap
 * completes it); op1 / op2, the bf16 operand rows of FFN-up / of wn as fp32 ([rows][hidden]; op2 of a last layer that did
 * not defer: [n_last_rows][hidden]); rs1 / rs2 [rows][hidden / 8], the x^2 partials beside a deferred operand, the first
 * ran[NVL_DENSE_RAN_RS1_TILES] / [..RS2_TILES] of a row valid (0 tiles: the operand is already normalised); h [rows][ffn];
 * yn [rows or n_last_rows][n_next]; x_end [rows][hidden], x after the last launch; ran [NVL_DENSE_RAN_INTS], what ran.
 * Refuses what nvl_create refuses (hidden, ffn, q_width % 64; a negative attention_multiplier) with NVL_ERR_INVALID. */
enum {      /* ran[]: per residual projection p (0 = O projection, 1 = FFN-down) four ints at 4p */
    NVL_DENSE_RAN_PRODUCER = 0,     /* 1: the launch carried the next norm (xn_raw + x^2 partials) */
    NVL_DENSE_RAN_HALF = 1,         /* 1: on 8-row half tiles (partials per 8 columns) */
    NVL_DENSE_RAN_FORM = 2,         /* NVL_RESID_FORM_* */
    NVL_DENSE_RAN_SLICES = 3,       /* K slices left pending for the next norm (0: the add happened in the launch) */
    NVL_DENSE_RAN_NORMS = 8,        /* norm launches */
    NVL_DENSE_RAN_CONSUMER = 9,     /* [9 + p]: the norm kernel that completed projection p's pending add (NVL_NORM_RAN_*, 0 = none) */
    NVL_DENSE_RAN_RS1_TILES = 12, NVL_DENSE_RAN_RS2_TILES = 13,
    NVL_DENSE_RAN_INTS = 14
};
enum {
    NVL_RESID_FORM_TILE = 0,        /* the prefill tile kernels */
    NVL_RESID_FORM_MSPLIT = 1,      /* decode kernel, one workgroup per (weight tile, 16-row activation tile), all of K */
    NVL_RESID_FORM_GROUPS = 2,      /* decode kernel over 64-row groups, one launch */
    NVL_RESID_FORM_GROUPS_SERIAL = 3,   /* ... one launch per group */
    NVL_RESID_FORM_DECODE = 4       /* decode kernel, one workgroup per weight tile (and K slice) */
};
enum { NVL_NORM_RAN_ROW = 1, NVL_NORM_RAN_ROW_IDX = 2, NVL_NORM_RAN_TILE16 = 3, NVL_NORM_RAN_WAVE = 4 /* norm_kernel: one wave per row */ };
typedef struct nvl_dense_stages {
    int32_t struct_bytes;           /* sizeof(nvl_dense_stages) */
    int32_t rows, hidden, q_width, ffn, n_next;
    int32_t norm_type, activation_type, block_style;       /* NVL_NORM_*, NVL_ACT_*, NVL_BLOCK_* */
    int32_t max_len, has_next, n_last_rows;
    float residual_multiplier, attention_multiplier, norm_eps;
    int32_t reserved;
    const float *x, *attn_out, *wo, *bo, *norm_w, *norm_b, *w1, *b1, *w2, *b2, *next_norm_w, *next_norm_b, *wn;
    const int32_t* last_rows;
    float *x1, *op1, *rs1, *h, *x2, *op2, *rs2, *yn, *x_end;
    int32_t* ran;
} nvl_dense_stages;
int nvl_op_dense_stages(int device, int precision, const nvl_dense_stages* io);
/* The same tail with the MoE block of moe.go:43-128 between the projections, decode only (rows <= 64; RMSNorm, sequential
 * block): the O projection carries the FFN norm, the router and the expert up projection read the deferred operand
 * (moe() with deferred_norm), the expert down projection leaves its K slices pending.  router [hidden][n_experts], w_in
 * [n_experts][2 inter][hidden], w_out [n_experts][hidden][inter] as nvl_op_moe_stages takes them.  Out: x1, op1, rs1 and
 * ran as nvl_op_dense_stages gives them (ran's FFN-down record holds only the slices moe() left pending); router_logits
 * and gate [rows][n_experts]; y [rows][hidden], x after the block (the pending slices added as the debug tap adds them);
 * *form, NVL_MOE_FORM_*. */
int nvl_op_dense_moe_stages(int device, int precision, const float* x, const float* attn_out, const float* wo, const float* bo,
                            const float* norm_w, const float* router, const float* w_in, const float* w_out,
                            const float* next_norm_w, int rows, int hidden, int q_width, int n_experts, int top_k, int inter,
                            float residual_multiplier, float norm_eps, float* x1, float* op1, float* rs1,
                            float* router_logits, float* gate, float* y, int32_t* form, int32_t* ran);
/* nvl_op_moe_stages / nvl_op_dense_moe_stages with the EXPERTS' storage format as a parameter (the router and the O projection
 * stay bf16).  NVL_OP_EXPERTS_BF16 is the call above, result for result.  A quantized format builds the experts the way a
 * model gets them: w_in as [n_experts * 2 inter][hidden] and w_out as [n_experts * hidden][inter] through the upload
 * quantizer of the format, then nvl_finalize's own code (the gate|up interleave of codes and scales with its pad rows, the
 * down codes and scales side by side over K = n_experts * inter, the fp8 row scales one row per expert), registered for the
 * decode dispatch as finalize registers them, the grouped forms' W~ scratch zeroed as finalize zeroes it.  group_size: INT4
 * only (32, 64 or 128, dividing hidden and inter; anything else is NVL_ERR_INVALID before a device is touched, as is
 * NVL_PRECISION_F32).
 * Two further outputs, each optional (NULL):
 *   wt_in [n_experts][2 inter][hidden], wt_out [n_experts][hidden][inter] (quantized formats only): W~ of the experts as the
 *     device holds them after finalize, read back through the dequantize kernels of the grouped forms and de-interleaved;
 *   h [rows][n_experts * inter]: the dense-masked forms' intermediate bf16(silu(g) u gate) after the up projection, copied
 *     between the two launches; NaN where no launch wrote (the columns of an expert no row picked; every column when a
 *     sorted form ran). */
enum { NVL_OP_EXPERTS_BF16 = 0, NVL_OP_EXPERTS_FP8 = 1, NVL_OP_EXPERTS_MXFP4 = 2, NVL_OP_EXPERTS_INT4 = 3 };
int nvl_op_moe_stages_q(int device, int precision, const float* x, const float* router, const float* w_in,
                        const float* w_out, int rows, int hidden, int n_experts, int top_k, int inter,
                        int expert_format, int group_size, float* y, float* router_logits, float* gate, int32_t* form,
                        float* wt_in, float* wt_out, float* h);
int nvl_op_dense_moe_stages_q(int device, int precision, const float* x, const float* attn_out, const float* wo, const float* bo,
                              const float* norm_w, const float* router, const float* w_in, const float* w_out,
                              const float* next_norm_w, int rows, int hidden, int q_width, int n_experts, int top_k, int inter,
                              float residual_multiplier, float norm_eps, int expert_format, int group_size, float* x1,
                              float* op1, float* rs1, float* router_logits, float* gate, float* y, int32_t* form, int32_t* ran,
                              float* wt_in, float* wt_out, float* h);
/* argmax cmd/ask/main.go:389-402 (first strict maximum) */
int nvl_op_argmax(int device, const float* x, int rows, int cols, int32_t* out);

/* sampling.go:33-102 on host logits [rows, V]; probs_out (optional) receives the final renormalised distribution. */
int nvl_op_sample(int device, const float* logits, int rows, int V, const nvl_sampling_params* params,
                  const int32_t* const* history_ptrs, const int32_t* history_lens, const float* uniforms,
                  int32_t* out_tokens, float* probs_out);
/* The sampler of a sampled verify pass and its accept kernel on host logits [n_seqs * (1+k)][V] (sampling.go:33-102 per
 * row with the history extension of nvl_verify_sampled; tensor_model_runner.go:89-93).  tokens / histories / uniforms as
 * nvl_verify_sampled (k may be 0); sampled_out [n_seqs * (1+k)] returns EVERY row's id (the model-level calls return the
 * accepted ones only); n_accepted_out, out_tokens and probs_out ([n_seqs * (1+k)][V], the final distributions) may be NULL. */
int nvl_op_sample_drafts(int device, const float* logits, int n_seqs, int k, int V, const nvl_sampling_params* params,
                         const int32_t* tokens, const int32_t* const* history_ptrs, const int32_t* history_lens,
                         const float* uniforms, int32_t* sampled_out, int32_t* n_accepted_out, int32_t* out_tokens,
                         float* probs_out);
/* The rejection kernel of nvl_verify_speculative (the rule stated there; sampling.go:33-102 gives p and q their meaning,
 * tensor_model_runner.go:89-93 the step it replaces) on host distributions: p [n_seqs][1+k][V], q [n_seqs][k][V], rows
 * padded to round_up(V, 4) on upload; tokens [n_seqs][1+k] (column 0 unused), k in 1..7.  accept_prob_out may be NULL. */
int nvl_op_spec_reject(int device, const float* p, const float* q, const int32_t* tokens, int n_seqs, int k, int V,
                       const float* accept_uniforms, const float* final_uniforms, int32_t* n_accepted_out,
                       int32_t* out_tokens, float* accept_prob_out);
/* The log-probability kernels (nvl_logprobs; generic_model.go:467-470 rows, cmd/check-logits/main.go's view of them) on
 * host logits [rows][ld], V valid columns (ld >= V: the pad columns travel too and are never used), divided by
 * logits_scaling first when it is not 0 (generic_model.go:473-477). */
int nvl_op_logprobs(int device, const float* logits, int rows, int V, int ld, float logits_scaling, const int32_t* targets,
                    int top_k, float* logprob_out, int32_t* argmax_out, int32_t* topk_ids_out, float* topk_logprob_out);
/* ---- tuning / measurement (no reference counterpart) ----
 * Times one projection GEMM shape (random bf16 operands resident in HBM) with HIP events on the
 * library's stream: avg_us per launch over `iters` back-to-back launches.  epi: 0 store-fp32,
 * 1 residual-add, 2 SwiGLU, 3 GELU.  force_bnt / force_ksplit override the decode kernel's
 * automatic tile choice (0 = automatic). */
int nvl_bench_gemm(int device, int M, int N, int K, int epi, int force_bnt, int force_ksplit, int iters,
                   float* avg_us);
/* Process-wide tuning override used by tests and sweeps.  key 0: prefill GEMM kernel (0 automatic,
 * 1 = 128x128 two-stage, 2 = 256x128 three-stage, 3 = 256x256 two-stage, 5 = 256x256 ping-pong).
 * key 1: K slices of the decode residual projections (0 automatic, 1 never split, 2, 4).
 * key 2: decode (M <= 64) GEMM form: 0 automatic, 1/2/4 = narrow form with that many weight tiles per workgroup,
 * 8 = wide-N form (4 weight tiles per wave).
 * key 3: deferred RMSNorm in decode (0 off, 1 on, 2 on without the activation-tile split, 3 only the O-proj -> FFN-up seam).
 * keys 4-6 (sweeps): K split of the wide form, waves per narrow-form launch, K split of the deferred-norm residual
 * projections.  key 7: decode seam kernel, 8: MoE small-batch fusion, 9: 16-row norm kernel, 10: prefill attention
 * with 128 query rows per workgroup (0 never, 1 automatic, 2 always).  keys 11-14: decode batches of 65..512 rows (key 11, default 512; 64 = off) run the
 * projections whose 128x128 tile grid has fewer than key 12 (160) workgroups as ceil(M/64) groups of 64 rows of the
 * decode GEMM form, in one launch interleaved over the weight blocks (key 13 = 1) or one launch per group (0); up to
 * key 14 rows (64) every projection does.  key 15: waves per decode-attention workgroup (0 = from context length and
 * grid size, 2, 4, 8).  key 16: prefill MoE copies the token rows into expert order before the grouped GEMM (1, default)
 * or gathers them per lane inside it (0).  key 17: prefill MoE grouped GEMMs: 0 (default) = 256-row segments on the
 * ping-pong kernel, 128 / 256 = the lock-step tile kernels with that many rows per m-tile.
 * key 19: decode-sized MoE batches run the grouped GEMMs on the four-stage 128x128 instance (1, default) or two stages (0).
 * key 18: largest prefill batch (tokens) whose QKV projection runs as decode-form groups + rope_kv_kernel instead of the
 * fused-epilogue tile kernel (default 256: +5 % at 128 tokens, +1 % at 256, -4 % at 512).
 * key 21: hipGraph replay of decode passes (1, default; 0 = every launch eager).  key 22: decode MoE as two dense-masked
 * weight-streaming projections (1, default) or sort + grouped GEMMs (0).  key 23: largest payload (rows of the residual
 * stream) the tensor-parallel P2P all-reduce sends one-shot; above it reduce-scatter + all-gather (default 64).
 * key 25: a decode attention over >= 1024 keys in a tiny batch (<= 32 (sequence, kv head) pairs: Llama B <= 4) deals its key
 * tiles over up to 8 workgroups per pair (<= 128 in all), the last of which combines the partial results (1, default; 0 = never).
 * key 26: residual projections of 65..2048 rows split K over up to 8 workgroups per 128x128 tile, the slices summed by the
 * norm that follows (1, default; 0 = the 64-row groups of the decode form / plain tiles).
 * key 24: the decode GEMM kernels do not fetch the activation rows >= M of a padded 16-row tile (1, default).
 * key 27: deferred-norm residual projections of <= 16 rows run on 8-row half tiles, twice the workgroups (1, default).
 * key 29: milliseconds a tensor-parallel rank waits for its peers inside a P2P all-reduce before the call fails (default 30000).
 * key 30: Mamba2 prefill scan: 1 (default) the chunked SSD form on MFMA, chunks of a sequence in parallel when few (sequence, head)
 * pairs; 2 the chunked form, chunk after chunk only; 0 the sequential recurrence.
 * key 31: MoE decode routing (router logits, softmax, top-k, gate matrix) as one launch (1, default; 0 = router GEMM + gate kernel).
 * key 35: non-temporal K/V loads in the decode attention: 1 (default) when one workgroup serves a kv head's group and the launch
 * fills the chip (>= 160 workgroups) or the batch is one sequence; 0 never; 2 always.
 * key 36: weight tiles per wave of the wide decode projections (FFN-up, LM head): 0 (default) 2 for 17..32 rows and N < 65536, else 4;
 * 2 / 4 forced.
 * key 33: MoE decode: the experts' down projection carries the next RMSNorm (no K slices, no norm launch before the next QKV);
 * 0 (default): measured slower (rejected list (27)).
 * key 37: rows per chunk of nvl_score's final norm + LM head + log-probability reduction (default 1024; rounded up to a
 * multiple of 16, at least 16): the logits workspace of a scoring pass is that many rows.
 * key 38: verify passes (nvl_verify_greedy*, nvl_decode_greedy_lookup, nvl_verify_sampled*, nvl_decode_sampled_lookup) in bf16 over a bf16 cache run the multi-position
 * decode attention (1, default); 0 = rope_kv + the prefill attention kernel, the route of an nvl_forward of 1 + k rows.
 * key 39: decode passes (one row per sequence) of a model set to NVL_MAMBA_CONV_CARRIED run the convolution, the shift of the
 * kept rows and softplus(dt) as one launch per Mamba2 layer (1, default); 0 = the convolution kernel plus the tail kernel.  No
 * effect in NVL_MAMBA_CONV_PER_CALL mode.
 * The settings are PROCESS-GLOBAL and unsynchronised (every model in the process sees them): set them from one thread
 * while no forward call is running.  Every call starts a new tuning epoch: captured decode graphs bake the tuning in and are re-captured.
 * Returns the previous value. */
int nvl_set_tuning(int key, int value);

#ifdef __cplusplus
}
#endif
#endif /* NVLLM_H */
