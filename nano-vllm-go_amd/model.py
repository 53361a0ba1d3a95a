"""Host-side mirror of tensor.TransformerModel (purego/tensor/generic_model.go:4-19) over the C ABI:
same method names and argument meaning as the reference (ForwardWithCache, GetLogitsForLastToken),
device-resident weights and KV slabs underneath."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _cfg_struct(cfg: dict) -> L.ModelConfigC:
    c = L.ModelConfigC()
    for k in ("vocab_size", "hidden", "num_layers", "num_heads", "num_kv_heads", "head_dim", "ffn_dim",
              "max_seq_len", "num_experts", "num_experts_per_tok"):
        setattr(c, k, int(cfg.get(k, 0)))
    c.attention_type = L.ATTN[cfg["attention_type"]]
    c.norm_type = L.NORM[cfg["norm_type"]]
    c.position_type = L.POS[cfg["position_type"]]
    c.activation_type = L.ACT[cfg["activation_type"]]
    c.block_style = L.BLOCK[cfg["block_style"]]
    c.rope_base = float(cfg.get("rope_base", 10000.0))
    c.norm_eps = float(cfg.get("norm_eps", 1e-5))
    c.tied_embedding = int(bool(cfg.get("tied_embedding", False)))
    c.use_moe = int(bool(cfg.get("use_moe", False)))
    for k in ("embedding_multiplier", "attention_multiplier", "residual_multiplier", "logits_scaling"):
        setattr(c, k, float(cfg.get(k, 0.0)))
    for k in ("mamba_expand", "mamba_state_size", "mamba_num_heads", "mamba_head_dim", "mamba_n_groups", "mamba_conv_kernel"):
        setattr(c, k, int(cfg.get(k, 0)))
    for i, t in enumerate(cfg.get("hybrid_layers") or []):          # config.go:113 HybridLayers
        if t in ("mamba", "mamba2"):
            c.mamba_layer_mask[i >> 6] |= 1 << (i & 63)
    return c


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# The weight-format keywords of HipTransformerModel, in the order they are checked: keyword, value table, the keyword that must
# be switched on with it, the keywords it cannot be combined with, setter.  The library decides every combination
# (csrc/wfmt.h wf_decide); what is checked here is what can be said before a model exists.
_DTYPE_KEYWORDS = (
    ("weight_dtype", L.WEIGHT_DTYPE, None, (), "nvl_set_weight_dtype"),
    ("act_dtype", L.ACT_DTYPE, "weight_dtype", (), "nvl_set_act_dtype"),
    ("expert_dtype", L.EXPERT_DTYPE, "weight_dtype", (), "nvl_set_expert_dtype"),
    ("mx_weight_dtype", L.MX_WEIGHT_DTYPE, None, ("weight_dtype",), "nvl_set_mx_weight_dtype"),
    ("mx_expert_dtype", L.MX_EXPERT_DTYPE, "mx_weight_dtype", (), "nvl_set_mx_expert_dtype"),
    ("mx_head_dtype", L.MX_HEAD_DTYPE, "mx_weight_dtype", (), "nvl_set_mx_head_dtype"),
    ("gq_weight_dtype", L.GQ_WEIGHT_DTYPE, None, ("weight_dtype", "mx_weight_dtype"), "nvl_set_gq_weight_dtype"),
    ("gq_expert_dtype", L.GQ_EXPERT_DTYPE, "gq_weight_dtype", (), "nvl_set_gq_expert_dtype"),
)
_ON = {kw: next(name for name, v in table.items() if v == 1) for kw, table, *_ in _DTYPE_KEYWORDS}      # e.g. "fp8_e4m3"
# the order the setters are called in: a family's projections before what needs them
_SETTER_ORDER = ("gq_weight_dtype", "gq_expert_dtype", "mx_weight_dtype", "mx_expert_dtype", "mx_head_dtype", "weight_dtype",
                 "expert_dtype", "act_dtype")


class HipTransformerModel:
    """tensor.TransformerModel on one MI355X.  `tensors` is {(slot, layer): array} in the reference's
    post-load layout (2-D weights [in, out]); arrays may be numpy fp32 or torch tensors (fp32/bf16,
    host or device) — torch device tensors are handed over by pointer with no host copy."""

    def __init__(self, cfg: dict, tensors: dict | None, *, device: int = 0, precision: str = "bf16",
                 max_seqs: int = 8, max_batch_tokens: int | None = None, tp_rank: int = 0, tp_size: int = 1,
                 tp_force_single: bool = False, kv_num_blocks: int = 0, kv_block_size: int = 0,
                 kv_cache_dtype: str = "auto", kv_scales=None, weight_dtype: str = "auto",
                 act_dtype: str = "auto", expert_dtype: str = "auto", mx_weight_dtype: str = "none",
                 mx_expert_dtype: str = "none", mx_head_dtype: str = "none", gq_weight_dtype: str = "none",
                 gq_group_size: int = 128, gq_expert_dtype: str = "none", mamba_conv_state: str = "per_call"):
        """tensors=None defers finalize(): upload() each tensor, then call finalize().
        tp_size > 1 makes this the tp_rank-th tensor-parallel shard: pass the FULL tensors, the library keeps
        its slice; join the shards with tp_init (RCCL, one process per GPU) or attach_local_group (tests).
        kv_cache_dtype="fp8_e4m3": 8-bit K/V (bf16 precision); kv_scales=(k, v), each a scalar or one value per layer
        (nvl_set_kv_scales; a checkpoint's own *.self_attn.k_scale / v_scale, read by from_pretrained, take precedence).
        weight_dtype="fp8_e4m3": 8-bit projection weights with per-row scales (nvl_set_weight_dtype; bf16 precision, no TP);
        the model computes with W~ = bf16(s * e4m3(q)), which get_weight returns.
        act_dtype="fp8_e4m3" (needs weight_dtype="fp8_e4m3"): W8A8 — the projections on the tile (prefill) GEMM path quantize
        their activation rows to e4m3 with one scale per row and multiply codes x codes (nvl_set_act_dtype).
        expert_dtype="fp8_e4m3" (needs weight_dtype="fp8_e4m3", a MoE model): the experts' weights are 8-bit too, one scale per
        (expert, output row) (nvl_set_expert_dtype); otherwise the experts stay bf16.
        mx_weight_dtype="fp4_e2m1": MXFP4 projection weights, e2m1 codes with one e8m0 scale per 32 input features
        (nvl_set_mx_weight_dtype; bf16 precision, no TP, not with weight_dtype="fp8_e4m3"); the LM head, the embeddings and
        the MoE experts stay bf16.  The model computes with W~ = grid[q] * 2^e, which get_weight returns.
        mx_expert_dtype="fp4_e2m1" (needs mx_weight_dtype="fp4_e2m1", a MoE model): the experts' weights are MXFP4 too, one
        e8m0 scale per 32 input features of an (expert, output row) (nvl_set_mx_expert_dtype).
        mx_head_dtype="fp4_e2m1" (needs mx_weight_dtype="fp4_e2m1"): the LM head, and the token embedding of a tied model, are
        MXFP4 too, one e8m0 scale per 32 input features of a vocabulary row (nvl_set_mx_head_dtype).
        gq_weight_dtype="uint4": INT4 group-quantized projection weights, the W4A16 format of AWQ / GPTQ checkpoints — unsigned
        4-bit codes with one fp16 scale and one zero point per gq_group_size (32 / 64 / 128) input features
        (nvl_set_gq_weight_dtype; bf16 precision, no TP, not with weight_dtype / mx_weight_dtype); the LM head, the embeddings
        and the MoE experts stay bf16.  The model computes with W~ = bf16(s * (q - z)), which get_weight returns.
        gq_expert_dtype="uint4" (needs gq_weight_dtype="uint4", a MoE model whose hidden and expert widths are multiples of
        gq_group_size): the experts' weights are INT4 too, one scale and zero point per gq_group_size input features of an
        (expert, output row) (nvl_set_gq_expert_dtype).
        mamba_conv_state="carried" (a hybrid model): the Mamba2 convolution window reaches into the sequence's previous
        calls, so feeding a sequence in one call or token by token gives the same logits (nvl_set_mamba_conv_state);
        "per_call" (default) zero-pads every call as the reference does (mamba2.go:181-254)."""
        self.cfg = dict(cfg)
        self.lib = L.lib()
        self.h = C.c_void_p()
        opts = L.RuntimeOptsC(device=device, precision=L.PRECISION[precision], max_seqs=max_seqs,
                              max_batch_tokens=max_batch_tokens or cfg["max_seq_len"], tp_rank=tp_rank, tp_size=tp_size)
        if tp_force_single:
            opts.tp_force_single = 1
        # kv_num_blocks > 0: paged KV — the host's block manager (nanovllm/block_manager.go) owns the cache
        opts.kv_num_blocks, opts.kv_block_size = int(kv_num_blocks), int(kv_block_size)
        self.kv_block_size = (kv_block_size or 256) if kv_num_blocks else 0
        if kv_cache_dtype not in L.KV_CACHE_DTYPE:
            raise ValueError(f"kv_cache_dtype must be one of {sorted(L.KV_CACHE_DTYPE)}")
        opts.kv_cache_dtype = L.KV_CACHE_DTYPE[kv_cache_dtype]
        self.kv_cache_dtype = kv_cache_dtype
        self._c = _cfg_struct(cfg)
        given = dict(weight_dtype=weight_dtype, act_dtype=act_dtype, expert_dtype=expert_dtype, mx_weight_dtype=mx_weight_dtype,
                     mx_expert_dtype=mx_expert_dtype, mx_head_dtype=mx_head_dtype, gq_weight_dtype=gq_weight_dtype,
                     gq_expert_dtype=gq_expert_dtype)
        for kw, table, needs, excludes, _ in _DTYPE_KEYWORDS:
            if given[kw] not in table:
                raise ValueError(f"{kw} must be one of {sorted(table)}")
            if kw == "gq_weight_dtype" and gq_group_size not in L.GQ_GROUP_SIZES:
                raise ValueError(f"gq_group_size must be one of {L.GQ_GROUP_SIZES}")
            if table[given[kw]] and needs and given[needs] != _ON[needs]:
                raise ValueError(f'{kw}="{_ON[kw]}" needs {needs}="{_ON[needs]}"')
            if table[given[kw]] and any(given[o] == _ON[o] for o in excludes):      # (checked above: a value is off or on)
                raise ValueError(f'{kw}="{_ON[kw]}" cannot be combined with ' + " or ".join(f'{o}="{_ON[o]}"' for o in excludes))
        if mamba_conv_state not in L.MAMBA_CONV_STATE:
            raise ValueError(f"mamba_conv_state must be one of {sorted(L.MAMBA_CONV_STATE)}")
        L.check(self.lib.nvl_create(C.byref(self._c), C.byref(opts), C.byref(self.h)))
        for kw, value in given.items():
            setattr(self, kw, value)
        self.gq_group_size = gq_group_size
        for kw, table, _, _, setter in sorted(_DTYPE_KEYWORDS, key=lambda row: _SETTER_ORDER.index(row[0])):
            if not table[given[kw]]:
                continue
            fn = getattr(self.lib, setter)
            rc = fn(self.h, table[given[kw]], int(gq_group_size)) if kw == "gq_weight_dtype" else fn(self.h, table[given[kw]])
            if rc < 0:
                msg = self.lib.nvl_last_error(self.h)
                self.close()
                raise L.NvlError(rc, msg.decode() if msg else "")
        self.mamba_conv_state = mamba_conv_state
        if mamba_conv_state != "per_call":
            rc = self.lib.nvl_set_mamba_conv_state(self.h, L.MAMBA_CONV_STATE[mamba_conv_state])
            if rc < 0:
                msg = self.lib.nvl_last_error(self.h)
                self.close()
                raise L.NvlError(rc, msg.decode() if msg else "")
        if kv_scales is not None:
            self.set_kv_scales(*kv_scales)
        self.V = cfg["vocab_size"]
        self.H = cfg["hidden"]
        if tensors is not None:
            for (slot, layer), arr in tensors.items():
                self.upload(slot, layer, arr)
            self.finalize()

    def set_kv_scales(self, k_scale, v_scale):
        """per-layer K / V scales of the 8-bit cache (scalars broadcast over the layers); before the first forward"""
        n = self.cfg["num_layers"]
        k = np.broadcast_to(np.asarray(k_scale, np.float32), (n,)).copy()
        v = np.broadcast_to(np.asarray(v_scale, np.float32), (n,)).copy()
        L.check(self.lib.nvl_set_kv_scales(self.h, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), self.h)

    @classmethod
    def from_pretrained(cls, path: str, **kw):
        """tensor.LoadModelFromDirectory (generic_loader.go:1016-1040) without the fp32 host model: config.json (or
        model_info.json) through nvl_load_config_json, weights through nvl_load_safetensors (mmap -> device)."""
        import os
        c = L.ModelConfigC()
        for name in ("config.json", "model_info.json"):
            cp = os.path.join(path, name)
            if os.path.exists(cp):
                L.check(L.lib().nvl_load_config_json(cp.encode(), C.byref(c)))
                break
        else:
            raise FileNotFoundError(f"no config.json / model_info.json in {path}")
        inv = {k: {v: n for n, v in tbl.items()} for k, tbl in
               (("attention_type", L.ATTN), ("norm_type", L.NORM), ("position_type", L.POS),
                ("activation_type", L.ACT), ("block_style", L.BLOCK))}
        cfg = {}
        for name, _ in L.ModelConfigC._fields_:
            v = getattr(c, name)
            if name == "mamba_layer_mask":
                if v[0] | v[1]:
                    cfg["hybrid_layers"] = ["mamba" if (v[i >> 6] >> (i & 63)) & 1 else "attention" for i in range(c.num_layers)]
                continue
            cfg[name] = inv[name][v] if name in inv else (bool(v) if name in ("tied_embedding", "use_moe") else v)
        m = cls(cfg, None, **kw)
        L.check(m.lib.nvl_load_safetensors(m.h, path.encode()), m.h)
        m.finalize()
        return m

    def finalize(self):
        L.check(self.lib.nvl_finalize(self.h), self.h)

    # -- tensor parallel group ---------------------------------------------------------------------
    @staticmethod
    def tp_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.lib().nvl_tp_get_unique_id(buf, 128))
        return buf.raw

    def tp_init(self, unique_id: bytes):
        L.check(self.lib.nvl_tp_init(self.h, C.c_char_p(unique_id), len(unique_id)), self.h)

    def tp_p2p_export(self) -> bytes:
        """IPC handle (64 bytes) of this rank's all-reduce comm buffer (nvl_tp_p2p_export); gather them in rank order."""
        buf = C.create_string_buffer(64)
        L.check(self.lib.nvl_tp_p2p_export(self.h, buf, 64), self.h)
        return buf.raw

    def tp_p2p_attach(self, handles):
        """handles: the tp_size exported handles in rank order (nvl_tp_p2p_attach): switches the all-reduce to direct peer stores."""
        blob = b"".join(handles)
        L.check(self.lib.nvl_tp_p2p_attach(self.h, C.c_char_p(blob), 64), self.h)

    def tp_p2p_rearm(self):
        """nvl_tp_p2p_rearm: after a timed-out all-reduce, on every rank, while no rank is inside a forward call."""
        L.check(self.lib.nvl_tp_p2p_rearm(self.h), self.h)

    @staticmethod
    def attach_local_group(models):
        arr = (C.c_void_p * len(models))(*[m.h.value for m in models])
        L.check(L.lib().nvl_tp_attach_local(arr, len(models)))

    # -- weights -----------------------------------------------------------------------------
    def upload(self, slot: str, layer: int, arr, layout: int | None = None):
        if layout is None:
            layout = L.LAYOUT_OUT_IN if slot in L.OUT_IN_SLOTS else L.LAYOUT_IN_OUT
        ptr, dtype, shape, keep = _as_pointer(arr)
        if slot in L.ONE_D:
            rows, cols = int(np.prod(shape)), 1
        elif slot in ("moe_in", "moe_out"):
            rows, cols = shape[0] * shape[1], shape[2]
        else:
            rows, cols = shape
        L.check(self.lib.nvl_upload_tensor(self.h, L.SLOT_ID[slot], int(layer), ptr, dtype, rows, cols, layout), self.h)
        del keep

    def upload_mxfp4(self, slot: str, layer: int, codes, scales):
        """nvl_upload_tensor_mxfp4: pre-quantized codes [out][in/2] (even k in the low nibble) and e8m0 scales [out][in/32];
        with mx_expert_dtype="fp4_e2m1" also moe_in / moe_out, as [E * out][in/2] and [E * out][in/32]; with
        mx_head_dtype="fp4_e2m1" also lm_head, and tok_emb of a tied model, as [vocab][hidden/2] and [vocab][hidden/32]"""
        codes = np.ascontiguousarray(codes, np.uint8)
        scales = np.ascontiguousarray(scales, np.uint8)
        L.check(self.lib.nvl_upload_tensor_mxfp4(self.h, L.SLOT_ID[slot], int(layer), codes.ctypes.data_as(C.c_void_p),
                                                 scales.ctypes.data_as(C.c_void_p), codes.shape[0], codes.shape[1] * 2,
                                                 L.LAYOUT_OUT_IN), self.h)

    def upload_int4(self, slot: str, layer: int, codes, scales, zeros):
        """nvl_upload_tensor_int4: pre-quantized codes [out][in/2] (even k in the low nibble), fp16 scales [out][in/g] (float16
        values or their uint16 bit patterns) and zero points [out][in/g] (0..15); with gq_expert_dtype="uint4" also moe_in /
        moe_out, as [E * out][in/2] codes and [E * out][in/g] scales and zero points"""
        codes = np.ascontiguousarray(codes, np.uint8)
        scales = np.ascontiguousarray(scales)
        scales = scales.view(np.uint16) if scales.dtype == np.float16 else np.ascontiguousarray(scales, np.uint16)
        zeros = np.ascontiguousarray(zeros, np.uint8)
        L.check(self.lib.nvl_upload_tensor_int4(self.h, L.SLOT_ID[slot], int(layer), codes.ctypes.data_as(C.c_void_p),
                                                scales.ctypes.data_as(C.c_void_p), zeros.ctypes.data_as(C.c_void_p),
                                                codes.shape[0], codes.shape[1] * 2, L.LAYOUT_OUT_IN), self.h)

    # -- sequences (replace kvCaches map[int64]*KVCache, tensor_model_runner.go:13) ----------------
    def seq_reset(self, seq_id: int):
        L.check(self.lib.nvl_seq_reset(self.h, seq_id), self.h)

    def seq_close(self, seq_id: int):
        L.check(self.lib.nvl_seq_close(self.h, seq_id), self.h)

    def seq_close_all(self):
        L.check(self.lib.nvl_seq_close_all(self.h), self.h)

    def seq_len(self, seq_id: int) -> int:
        return self.lib.nvl_seq_len(self.h, seq_id)

    # -- forward --------------------------------------------------------------------------------
    def forward_batch(self, seq_ids, token_lists, pos_offsets, *, all_logits=False, want_logits=True):
        """nvl_forward: returns (logits [rows, V] or None, argmax [n_seqs])."""
        n = len(seq_ids)
        ids = np.asarray(seq_ids, np.int64)
        lens = np.asarray([len(t) for t in token_lists], np.int32)
        toks = np.concatenate([np.asarray(t, np.int32) for t in token_lists]).astype(np.int32)
        pos = np.asarray(pos_offsets, np.int32)
        rows = int(lens.sum()) if all_logits else n
        logits = np.empty((rows, self.V), np.float32) if want_logits else None
        am = np.empty(n, np.int32)
        L.check(self.lib.nvl_forward(self.h, n, _ptr(ids), _ptr(toks), _ptr(lens), _ptr(pos),
                                     L.FWD_ALL_LOGITS if all_logits else 0, _ptr(logits), _ptr(am)), self.h)
        return logits, am

    def forward_with_cache(self, token_ids, seq_id: int, pos_offset: int, *, all_logits=True):
        """TransformerModel.ForwardWithCache (generic_model.go:276): logits [S, V] for one sequence.
        The *KVCache argument of the reference is the sequence's device slot, named by seq_id;
        pos_offset == 0 with a fresh id (or after seq_reset) is the reference's kvCache == nil."""
        if self.seq_len(seq_id) < 0:
            L.check(self.lib.nvl_seq_open(self.h, seq_id), self.h)
        logits, _ = self.forward_batch([seq_id], [list(token_ids)], [pos_offset], all_logits=all_logits)
        return logits

    @staticmethod
    def get_logits_for_last_token(logits):
        """GetLogitsForLastToken (generic_model.go:595-604)."""
        return logits[-1].copy()

    def greedy(self, prompt, max_tokens: int, seq_id: int = 0):
        """cmd/ask/main.go:287-360 generateResponse with argmax on the device (no EOS stop)."""
        self.seq_reset(seq_id)
        all_tokens = list(prompt)
        _, am = self.forward_batch([seq_id], [all_tokens], [0], want_logits=False)
        out = [int(am[0])]
        all_tokens.append(out[-1])
        for _ in range(max_tokens - 1):
            _, am = self.forward_batch([seq_id], [[all_tokens[-1]]], [len(all_tokens) - 1], want_logits=False)
            out.append(int(am[0]))
            all_tokens.append(out[-1])
        return out

    def forward_paged(self, token_lists, pos_offsets, block_tables, *, all_logits=False, want_logits=True):
        """nvl_forward_paged: new tokens of each sequence at pos_offsets, KV through the sequences' block tables
        (Sequence.BlockTable).  Returns (logits [rows, V] or None, argmax [n_seqs])."""
        n = len(token_lists)
        lens = np.asarray([len(t) for t in token_lists], np.int32)
        toks = np.concatenate([np.asarray(t, np.int32) for t in token_lists]).astype(np.int32)
        pos = np.asarray(pos_offsets, np.int32)
        tbl = np.concatenate([np.asarray(b, np.int32) for b in block_tables]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(b) for b in block_tables])]).astype(np.int32)
        rows = int(lens.sum()) if all_logits else n
        logits = np.empty((rows, self.V), np.float32) if want_logits else None
        am = np.empty(n, np.int32)
        L.check(self.lib.nvl_forward_paged(self.h, n, _ptr(toks), _ptr(lens), _ptr(pos), _ptr(tbl), _ptr(off),
                                           L.FWD_ALL_LOGITS if all_logits else 0, _ptr(logits), _ptr(am)), self.h)
        return logits, am

    def decode_greedy_paged(self, first_tokens, positions, n_steps: int, block_tables):
        """nvl_decode_greedy_paged -> [n_steps, n_seqs]; the tables must cover positions + n_steps tokens."""
        n = len(first_tokens)
        first = np.ascontiguousarray(first_tokens, dtype=np.int32)
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        tbl = np.concatenate([np.asarray(b, np.int32) for b in block_tables]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(b) for b in block_tables])]).astype(np.int32)
        out = np.empty((n_steps, n), dtype=np.int32)
        L.check(self.lib.nvl_decode_greedy_paged(self.h, n, _ptr(first), _ptr(pos), n_steps, _ptr(tbl), _ptr(off), _ptr(out)),
                self.h)
        return out

    def get_kv_paged(self, block_table, n_tokens: int, layer: int):
        tbl = np.ascontiguousarray(block_table, dtype=np.int32)
        nkv = self.cfg["num_heads"] if self.cfg["attention_type"] == "mha" else (
            1 if self.cfg["attention_type"] == "mqa" else self.cfg["num_kv_heads"])
        k = np.empty((nkv, n_tokens, self.cfg["head_dim"]), np.float32)
        v = np.empty_like(k)
        L.check(self.lib.nvl_get_kv_paged(self.h, _ptr(tbl), tbl.size, n_tokens, layer, _ptr(k), _ptr(v)), self.h)
        return k, v

    def decode_greedy(self, seq_ids, first_tokens, n_steps: int):
        """nvl_decode_greedy: n_steps greedy decode steps with the token feedback on the device -> [n_steps, n_seqs]."""
        n = len(seq_ids)
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        first = np.ascontiguousarray(first_tokens, dtype=np.int32)
        out = np.empty((n_steps, n), dtype=np.int32)
        L.check(self.lib.nvl_decode_greedy(self.h, n, _ptr(ids), _ptr(first), n_steps, _ptr(out)), self.h)
        return out

    # -- greedy speculative decoding ----------------------------------------------------------------
    def verify_greedy(self, seq_ids, token_rows, k: int):
        """nvl_verify_greedy: token_rows [n_seqs, 1+k] (row i: the next input token, then k draft tokens) -> (n_accepted
        [n_seqs], out_tokens [n_seqs, 1+k]: the greedy ids 0..a_i, the rest -1).  The cached length grows by a_i + 1; the
        n_seqs x (1+k) logits rows stay for logprobs() / sample()."""
        n = len(seq_ids)
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        toks = np.ascontiguousarray(token_rows, dtype=np.int32).reshape(n, 1 + k)
        acc = np.empty(n, np.int32)
        out = np.empty((n, 1 + k), np.int32)
        L.check(self.lib.nvl_verify_greedy(self.h, n, _ptr(ids), _ptr(toks), int(k), _ptr(acc), _ptr(out)), self.h)
        return acc, out

    def verify_greedy_paged(self, token_rows, k: int, pos_offsets, block_tables):
        """nvl_verify_greedy_paged: verify_greedy over the sequences' block tables; the caller advances by a_i + 1."""
        n = len(pos_offsets)
        toks = np.ascontiguousarray(token_rows, dtype=np.int32).reshape(n, 1 + k)
        pos = np.ascontiguousarray(pos_offsets, dtype=np.int32)
        tbl = np.concatenate([np.asarray(b, np.int32) for b in block_tables]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(b) for b in block_tables])]).astype(np.int32)
        acc = np.empty(n, np.int32)
        out = np.empty((n, 1 + k), np.int32)
        L.check(self.lib.nvl_verify_greedy_paged(self.h, n, _ptr(toks), int(k), _ptr(pos), _ptr(tbl), _ptr(off), _ptr(acc),
                                                 _ptr(out)), self.h)
        return acc, out

    def seq_truncate(self, seq_id: int, new_len: int):
        """nvl_seq_truncate: roll a slab sequence back to new_len <= its cached length."""
        L.check(self.lib.nvl_seq_truncate(self.h, seq_id, int(new_len)), self.h)

    def greedy_lookup(self, seq_ids, first_tokens, n_steps: int, k: int = 3, ngram: int = 3, histories=None):
        """nvl_decode_greedy_lookup: decode_greedy's result [n_steps, n_seqs] from prompt-lookup drafts + verify passes.
        histories[i] = the sequence's tokens so far, ending with first_tokens[i] (None: start at the first token).
        -> (out_tokens, passes)."""
        from .ops import _histories
        n = len(seq_ids)
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        first = np.ascontiguousarray(first_tokens, dtype=np.int32)
        ptrs, lens, keep = _histories(histories, n) if histories is not None else (None, None, None)
        out = np.empty((n_steps, n), dtype=np.int32)
        passes = np.zeros(1, np.int32)
        L.check(self.lib.nvl_decode_greedy_lookup(self.h, n, _ptr(ids), _ptr(first), n_steps, int(k), int(ngram), ptrs,
                                                  _ptr(lens), _ptr(out), _ptr(passes)), self.h)
        return out, int(passes[0])

    # -- sampled speculative decoding -----------------------------------------------------------------
    @staticmethod
    def _sampled_args(who, n, rows, k, histories, uniforms, u_shape):
        """token rows [n, 1+k] (or first tokens [n]), histories and draws of a sampled call; mismatches raise ValueError
        before any library call"""
        from .ops import _histories
        if not 0 <= int(k) <= 7:
            raise ValueError(f"{who}: k must be in [0, 7]")
        if n <= 0:
            raise ValueError(f"{who}: no sequences")
        toks = np.ascontiguousarray(rows, dtype=np.int32)
        if histories is None or len(histories) != n:
            raise ValueError(f"{who}: {0 if histories is None else len(histories)} histories for {n} sequences")
        if any(h is None or len(h) == 0 for h in histories):
            raise ValueError(f"{who}: every sequence needs its history (ending with its first token)")
        u = np.ascontiguousarray(uniforms, dtype=np.float32)
        want = (n, 1 + k) if u_shape is None else u_shape
        if u.size != want[0] * want[1]:
            raise ValueError(f"{who}: {u.size} uniforms, expected {want[0]} x {want[1]}")
        ptrs, lens, keep = _histories(histories, n)
        return toks, u.reshape(want), ptrs, lens, keep

    def verify_sampled(self, seq_ids, token_rows, k: int, histories, uniforms, *, temperature=1.0, top_p=1.0, top_k=0,
                       repetition_penalty=1.2):
        """nvl_verify_sampled: verify_greedy under SampleWithHistory.  histories[i] = the sequence's ids as row 0 sees them
        (ending with token_rows[i][0]); uniforms [n_seqs, 1+k], row j being the draw of the sequence's decode step j.
        -> (n_accepted [n_seqs], out_tokens [n_seqs, 1+k]: the sampled ids 0..a_i, the rest -1)."""
        n = len(seq_ids)
        toks, u, ptrs, lens, keep = self._sampled_args("verify_sampled", n, token_rows, k, histories, uniforms, None)
        if toks.size != n * (1 + k):
            raise ValueError(f"verify_sampled: {toks.size} tokens for {n} x {1 + k} rows")
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        acc = np.empty(n, np.int32)
        out = np.empty((n, 1 + k), np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_verify_sampled(self.h, n, _ptr(ids), _ptr(toks), int(k), C.byref(sp), ptrs, _ptr(lens), _ptr(u),
                                            _ptr(acc), _ptr(out)), self.h)
        return acc, out

    def verify_sampled_paged(self, token_rows, k: int, pos_offsets, block_tables, histories, uniforms, *, temperature=1.0,
                             top_p=1.0, top_k=0, repetition_penalty=1.2):
        """nvl_verify_sampled_paged: verify_sampled over the sequences' block tables; the caller advances by a_i + 1."""
        n = len(pos_offsets)
        if len(block_tables) != n:
            raise ValueError("verify_sampled_paged: pos_offsets and block_tables differ in length")
        toks, u, ptrs, lens, keep = self._sampled_args("verify_sampled_paged", n, token_rows, k, histories, uniforms, None)
        if toks.size != n * (1 + k):
            raise ValueError(f"verify_sampled_paged: {toks.size} tokens for {n} x {1 + k} rows")
        pos = np.ascontiguousarray(pos_offsets, dtype=np.int32)
        tbl = np.concatenate([np.asarray(b, np.int32) for b in block_tables]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(b) for b in block_tables])]).astype(np.int32)
        acc = np.empty(n, np.int32)
        out = np.empty((n, 1 + k), np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_verify_sampled_paged(self.h, n, _ptr(toks), int(k), _ptr(pos), _ptr(tbl), _ptr(off), C.byref(sp),
                                                  ptrs, _ptr(lens), _ptr(u), _ptr(acc), _ptr(out)), self.h)
        return acc, out

    def sampled_lookup(self, seq_ids, first_tokens, n_steps: int, histories, uniforms, k: int = 3, ngram: int = 3, *,
                       temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2):
        """nvl_decode_sampled_lookup: decode_sampled's result [n_steps, n_seqs] from prompt-lookup drafts + sampled verify
        passes; uniforms [n_steps, n_seqs], step t of sequence i always using uniforms[t][i].  -> (out_tokens, passes)."""
        n = len(seq_ids)
        if int(n_steps) <= 0:
            raise ValueError("sampled_lookup: n_steps must be positive")
        first, u, ptrs, lens, keep = self._sampled_args("sampled_lookup", n, first_tokens, k, histories, uniforms, (int(n_steps), n))
        if first.size != n:
            raise ValueError(f"sampled_lookup: {first.size} first tokens for {n} sequences")
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        out = np.empty((n_steps, n), dtype=np.int32)
        passes = np.zeros(1, np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_decode_sampled_lookup(self.h, n, _ptr(ids), _ptr(first), int(n_steps), int(k), int(ngram), C.byref(sp),
                                                   ptrs, _ptr(lens), _ptr(u), _ptr(out), _ptr(passes)), self.h)
        return out, int(passes[0])

    # -- speculative decoding with a draft model ---------------------------------------
    def draft_sampled(self, seq_ids, first_tokens, k: int, histories, uniforms, *, temperature=1.0, top_p=1.0, top_k=0,
                      repetition_penalty=1.2):
        """nvl_draft_sampled on THIS (draft) model: decode_sampled with n_steps = k -> ids [k, n_seqs]; every step's final
        distribution stays on the device for the target's verify_speculative."""
        n = len(seq_ids)
        if not 1 <= int(k) <= 7:
            raise ValueError("draft_sampled: k must be in [1, 7]")
        first, u, ptrs, lens, keep = self._sampled_args("draft_sampled", n, first_tokens, k, histories, uniforms, (int(k), n))
        if first.size != n:
            raise ValueError(f"draft_sampled: {first.size} first tokens for {n} sequences")
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        out = np.empty((int(k), n), dtype=np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_draft_sampled(self.h, n, _ptr(ids), _ptr(first), int(k), C.byref(sp), ptrs, _ptr(lens), _ptr(u),
                                           _ptr(out)), self.h)
        return out

    def verify_speculative(self, draft, seq_ids, token_rows, k: int, histories, accept_uniforms, final_uniforms, *,
                           temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2, return_probs=False):
        """nvl_verify_speculative on THIS (target) model against the proposals `draft` keeps.  token_rows [n_seqs, 1+k]: the
        next input token, then the draft's ids; accept_uniforms [n_seqs, k], final_uniforms [n_seqs].
        -> (n_accepted [n_seqs], out_tokens [n_seqs, 1+k][, accept_prob [n_seqs, k, 2] = {p_j(d_j), q_j(d_j)}])."""
        n = len(seq_ids)
        toks, ua, ptrs, lens, keep = self._sampled_args("verify_speculative", n, token_rows, k, histories, accept_uniforms, (n, int(k)))
        if toks.size != n * (1 + k):
            raise ValueError(f"verify_speculative: {toks.size} tokens for {n} x {1 + k} rows")
        uf = np.ascontiguousarray(final_uniforms, dtype=np.float32)
        if uf.size != n:
            raise ValueError(f"verify_speculative: {uf.size} final uniforms for {n} sequences")
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        acc = np.empty(n, np.int32)
        out = np.empty((n, 1 + k), np.int32)
        ap = np.empty((n, int(k), 2), np.float32) if return_probs else None
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_verify_speculative(self.h, draft.h, n, _ptr(ids), _ptr(toks), int(k), C.byref(sp), ptrs, _ptr(lens),
                                                _ptr(ua), _ptr(uf), _ptr(acc), _ptr(out), _ptr(ap)), self.h)
        return (acc, out, ap) if return_probs else (acc, out)

    def decode_speculative(self, draft, seq_ids, first_tokens, n_steps: int, histories, uniforms, k: int = 3, *,
                           temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2):
        """nvl_decode_speculative: decode_sampled's result shape [n_steps, n_seqs] from `draft`'s proposals + speculative
        verify passes on THIS (target) model; uniforms [n_steps, n_seqs, 2k+1] (per pass: k draft draws, k accept draws, the
        final draw).  -> (out_tokens, passes, accepted [n_seqs])."""
        n = len(seq_ids)
        if int(n_steps) <= 0:
            raise ValueError("decode_speculative: n_steps must be positive")
        if not 1 <= int(k) <= 7:
            raise ValueError("decode_speculative: k must be in [1, 7]")
        first, u, ptrs, lens, keep = self._sampled_args("decode_speculative", n, first_tokens, k, histories, uniforms,
                                                        (int(n_steps) * n, 2 * int(k) + 1))
        if first.size != n:
            raise ValueError(f"decode_speculative: {first.size} first tokens for {n} sequences")
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        out = np.empty((n_steps, n), dtype=np.int32)
        passes = np.zeros(1, np.int32)
        accepted = np.zeros(n, np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_decode_speculative(self.h, draft.h, n, _ptr(ids), _ptr(first), int(n_steps), int(k), C.byref(sp), ptrs,
                                                _ptr(lens), _ptr(u), _ptr(out), _ptr(passes), _ptr(accepted)), self.h)
        return out, int(passes[0]), accepted

    def greedy_fused(self, prompt, max_tokens: int, seq_id: int = 0):
        """greedy() with the whole decode loop in one nvl_decode_greedy call."""
        self.seq_reset(seq_id)
        _, am = self.forward_batch([seq_id], [list(prompt)], [0], want_logits=False)
        out = [int(am[0])]
        if max_tokens > 1:
            out += [int(t) for t in self.decode_greedy([seq_id], [out[0]], max_tokens - 1)[:, 0]]
        return out

    def decode_sampled(self, seq_ids, first_tokens, n_steps: int, histories, uniforms, *, temperature=1.0, top_p=1.0,
                       top_k=0, repetition_penalty=1.2):
        """nvl_decode_sampled: n_steps sampled decode steps on the device -> [n_steps, n_seqs].  histories[i] = the
        sequence's token ids so far (ending with first_tokens[i]); uniforms [n_steps, n_seqs]."""
        from .ops import _histories
        n = len(seq_ids)
        ids = np.ascontiguousarray(seq_ids, dtype=np.int64)
        first = np.ascontiguousarray(first_tokens, dtype=np.int32)
        ptrs, lens, keep = _histories(histories, n)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(n_steps, n)
        out = np.empty((n_steps, n), dtype=np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_decode_sampled(self.h, n, _ptr(ids), _ptr(first), n_steps, C.byref(sp), ptrs, _ptr(lens), _ptr(u),
                                            _ptr(out)), self.h)
        return out

    def sample(self, histories, uniforms, *, temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.2):
        """nvl_sample: tensor.SampleWithHistory on the logits rows the last forward left on the device."""
        from .ops import _histories
        n = len(uniforms)
        ptrs, lens, keep = _histories(histories, n)
        u = np.ascontiguousarray(uniforms, dtype=np.float32)
        out = np.empty(n, np.int32)
        sp = L.sampling_params(temperature, top_p, top_k, repetition_penalty)
        L.check(self.lib.nvl_sample(self.h, n, C.byref(sp), ptrs, _ptr(lens), _ptr(u), _ptr(out)), self.h)
        return out

    # -- log-probabilities (logprob.h) ------------------------------------------------------------------
    def _score_args(self, token_lists, targets, top_k):
        """-> (lens, tokens, targets, output arrays) of a scoring call; the default targets are each list's next token,
        -1 for its last row.  Length mismatches raise ValueError before any library call."""
        lens = np.asarray([len(t) for t in token_lists], np.int32)
        if len(token_lists) == 0 or (lens <= 0).any():
            raise ValueError("score: every sequence needs at least one token")
        if targets is None:
            targets = [list(t[1:]) + [-1] for t in token_lists]
        if len(targets) != len(token_lists):
            raise ValueError(f"score: {len(targets)} target lists for {len(token_lists)} sequences")
        for i, (t, g) in enumerate(zip(token_lists, targets)):
            if len(g) != len(t):
                raise ValueError(f"score: sequence {i} has {len(t)} tokens but {len(g)} targets")
        if not 0 <= int(top_k) <= 8:
            raise ValueError("score: top_k must be in [0, 8]")
        toks = np.concatenate([np.asarray(t, np.int32) for t in token_lists]).astype(np.int32)
        tg = np.concatenate([np.asarray(g, np.int32) for g in targets]).astype(np.int32)
        rows = int(lens.sum())
        out = (np.empty(rows, np.float32), np.empty(rows, np.int32),
               np.empty((rows, top_k), np.int32) if top_k else None, np.empty((rows, top_k), np.float32) if top_k else None)
        return lens, toks, tg, out

    @staticmethod
    def _per_seq(lens, out):
        cuts = np.cumsum(lens)[:-1]
        return tuple(None if a is None else np.split(a, cuts) for a in out)

    def score(self, seq_ids, token_lists, pos_offsets, targets=None, top_k=0):
        """nvl_score: nvl_forward (KV append included) returning per new token row the log-probability of its target (default:
        the next token of its list; -1 = none -> 0.0), the greedy id and the top_k ids / log-probabilities instead of logits.
        -> (logprobs, argmax, topk_ids, topk_logprobs): per-sequence lists of arrays [len] / [len, top_k] (None when top_k == 0)."""
        if not (len(seq_ids) == len(token_lists) == len(pos_offsets)):
            raise ValueError("score: seq_ids, token_lists and pos_offsets differ in length")
        lens, toks, tg, out = self._score_args(token_lists, targets, top_k)
        ids = np.asarray(seq_ids, np.int64)
        pos = np.asarray(pos_offsets, np.int32)
        L.check(self.lib.nvl_score(self.h, len(lens), _ptr(ids), _ptr(toks), _ptr(lens), _ptr(pos), _ptr(tg), int(top_k),
                                   _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])), self.h)
        return self._per_seq(lens, out)

    def score_paged(self, token_lists, pos_offsets, block_tables, targets=None, top_k=0):
        """nvl_score_paged: score() over the sequences' block tables (forward_paged's arguments)."""
        if not (len(token_lists) == len(pos_offsets) == len(block_tables)):
            raise ValueError("score_paged: token_lists, pos_offsets and block_tables differ in length")
        lens, toks, tg, out = self._score_args(token_lists, targets, top_k)
        pos = np.asarray(pos_offsets, np.int32)
        tbl = np.concatenate([np.asarray(b, np.int32) for b in block_tables]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(b) for b in block_tables])]).astype(np.int32)
        L.check(self.lib.nvl_score_paged(self.h, len(lens), _ptr(toks), _ptr(lens), _ptr(pos), _ptr(tbl), _ptr(off), _ptr(tg),
                                         int(top_k), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])), self.h)
        return self._per_seq(lens, out)

    def logprobs(self, targets, top_k=0):
        """nvl_logprobs on the logits rows the last forward left on the device (the rows sample() sees), one target per
        row (-1 = none).  -> (logprobs [n], argmax [n], topk_ids [n, top_k] or None, topk_logprobs or None)."""
        tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        n = tg.size
        if not 0 <= int(top_k) <= 8:
            raise ValueError("logprobs: top_k must be in [0, 8]")
        lp, am = np.empty(n, np.float32), np.empty(n, np.int32)
        ti = np.empty((n, top_k), np.int32) if top_k else None
        tl = np.empty((n, top_k), np.float32) if top_k else None
        L.check(self.lib.nvl_logprobs(self.h, n, _ptr(tg), int(top_k), _ptr(lp), _ptr(am), _ptr(ti), _ptr(tl)), self.h)
        return lp, am, ti, tl

    # -- debug / parity taps ------------------------------------------------------------------------
    def set_debug(self, keep_hidden: bool):
        L.check(self.lib.nvl_set_debug(self.h, int(keep_hidden)), self.h)

    def get_hidden(self, n_tokens: int):
        out = np.empty((self.cfg["num_layers"], n_tokens, self.H), np.float32)
        for li in range(self.cfg["num_layers"]):
            L.check(self.lib.nvl_get_hidden(self.h, li, _ptr(out[li]), n_tokens * self.H), self.h)
        return out

    def get_mamba_state(self, seq_id: int, layer: int):
        """Mamba2Layer.SSMState of the sequence for a Mamba2 layer, [heads, head_dim, state]."""
        c = self.cfg
        hd = c.get("mamba_head_dim") or c["mamba_expand"] * c["hidden"] // c["mamba_num_heads"]
        out = np.empty((c["mamba_num_heads"], hd, c["mamba_state_size"]), np.float32)
        L.check(self.lib.nvl_get_mamba_state(self.h, seq_id, layer, _ptr(out)), self.h)
        return out

    def get_mamba_conv_state(self, seq_id: int, layer: int):
        """The raw xBC rows of the sequence's last K-1 positions kept for a Mamba2 layer, [K-1, conv_dim], oldest first."""
        c = self.cfg
        conv_dim = c["mamba_expand"] * c["hidden"] + 2 * c["mamba_n_groups"] * c["mamba_state_size"]
        out = np.empty((c["mamba_conv_kernel"] - 1, conv_dim), np.float32)
        L.check(self.lib.nvl_get_mamba_conv_state(self.h, seq_id, layer, _ptr(out)), self.h)
        return out

    def get_kv(self, seq_id: int, layer: int):
        T = self.seq_len(seq_id)
        at = self.cfg["attention_type"]
        nkv = self.cfg["num_heads"] if at == "mha" else (1 if at == "mqa" else self.cfg["num_kv_heads"])
        k = np.empty((nkv, T, self.cfg["head_dim"]), np.float32)
        v = np.empty_like(k)
        L.check(self.lib.nvl_get_kv(self.h, seq_id, layer, _ptr(k), _ptr(v)), self.h)
        return k, v

    # -- measurement -------------------------------------------------------------------------------
    def set_profile(self, on: bool):
        L.check(self.lib.nvl_set_profile(self.h, int(on)), self.h)

    def stats(self) -> dict:
        s = L.StatsC()
        L.check(self.lib.nvl_get_stats(self.h, C.byref(s)), self.h)
        return {k: getattr(s, k) for k, _ in L.StatsC._fields_}

    def kernel_stats(self) -> list:
        """nvl_get_kernel_stats: [{site, phase ('prefill'|'decode'), launches, ms, flops, bytes}, ...]."""
        n = self.lib.nvl_get_kernel_stats(self.h, None, 0)
        arr = (L.KernelStatC * max(n, 1))()
        n = min(n, self.lib.nvl_get_kernel_stats(self.h, arr, n))
        return [dict(site=self.lib.nvl_kernel_site_name(arr[i].site).decode(), phase=("prefill", "decode")[arr[i].phase],
                     launches=int(arr[i].launches), ms=arr[i].ms, flops=arr[i].flops, bytes=arr[i].bytes) for i in range(n)]

    def reset_stats(self):
        L.check(self.lib.nvl_reset_stats(self.h), self.h)

    def close(self):
        if self.h:
            self.lib.nvl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            import sys
            if sys.is_finalizing():      # interpreter shutdown: the HIP runtime may already be gone (a leaked handle must
                return                   # not turn into nvl_destroy -> hipFree after teardown); the OS reclaims the memory
            self.close()
        except Exception:
            pass


def _as_pointer(arr):
    """(pointer, nvl dtype, shape, keepalive) for numpy arrays or torch tensors."""
    if isinstance(arr, np.ndarray):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        return a.ctypes.data_as(C.c_void_p), L.DTYPE_F32, a.shape, a
    import torch  # plumbing only: device memory handed over by pointer
    t = arr.contiguous()
    if t.dtype == torch.float32:
        dt = L.DTYPE_F32
    elif t.dtype == torch.bfloat16:
        dt = L.DTYPE_BF16
    elif t.dtype == torch.float16:
        dt = L.DTYPE_F16
    else:
        raise TypeError(t.dtype)
    if t.is_cuda:
        torch.cuda.synchronize(t.device)
    return C.c_void_p(t.data_ptr()), dt, tuple(t.shape), t
