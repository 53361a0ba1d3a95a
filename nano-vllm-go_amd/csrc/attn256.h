// attn256.h — causal attention at head_dim 256 (Gemma 2 / 3, Qwen3-Next): bf16 prefill and decode kernels over the bf16 KV
// cache, the slab and paged layouts of attn.h ([nKV][Tmax][hd] per block, 64 | Tmax, the block table of AttnArgs).
//
// attn.h instantiated at HD = 256 does not exist: its prefill ring would be 192 KB of LDS, its decode ladder 256 KB at eight
// waves, and a wave of either kernel holds O^T (64 registers per 16-row sub-tile), the Q fragments (32) and a 64-key tile's
// K / V fragments (128 + 128) — with two waves per SIMD (256 registers each) that does not fit.  The split of the work here:
//   * every workgroup is FOUR waves at most, one per SIMD, so a wave owns a SIMD's whole register file: 512 registers, the
//     MFMA accumulators (O^T, the scores) in the AGPR half.  No scratch.
//   * prefill: 4 waves x 2 sub-tiles = 128 query rows per workgroup; 64-key K / V tiles by LDS-DMA through a TWO-slot ring
//     (2 x [K image | V image] = 2 x 64 KB, + 512 bytes of block table = 131 584 bytes), one tile ahead of the compute, one barrier per tile.
//   * decode: 2 or 4 waves take the 64-key tiles round-robin; each has a private 32-KB V image (64 / 128 KB per workgroup)
//     and prefetches its next tile's K behind the scores and its next tile's V behind the image fill.
// The contracts are attn.h's: scores and running max / sum in fp32; P rounded to bf16 for P.V; prefill sums the ROUNDED P
// (ones . P^T on the MFMA pipe) and rounds the output once; decode sums the unrounded P.  The tile arithmetic
// (attn_prefill_tile, attn_decode_softmax, attn_pv_tile), the combine and the key-split protocol (attn_decode_finish,
// attn_decode_merge, attn_part_floats) are attn.h's own code instantiated at 256: they take the image offsets as arguments.
#pragma once
#include "attn.h"

namespace nvl {

// ------------------------------------------------------------------------------------------
// LDS image of one 64-key tile at HD 256: rows of 512 bytes = 32 16-byte chunks = two passes over the 64 banks.  Chunk c of
// row r sits at chunk position
//     r * 32 + (c ^ x(r)),      x(r) = (r & 7) << 1 | (r >> 3) & 1        (4 bits: the 256-byte half of the row stays)
// i.e. the 32-byte segment index is XOR-ed with r & 7 (as at HD 128) and the 16-byte half inside the segment with bit 3 of r.
// Bank position of a chunk = its position mod 16.
//   K fragment reads (ds_read_b128; a 16-lane group reads rows fq = 0..15 (+ 16 t) at one chunk c): positions mod 16 are
//     (c & 15) ^ x(r), and x is a bijection of r & 15 onto 0..15: sixteen distinct 16-byte bank groups = all 64 banks once.
//     (The HD-128 pattern r & 7 alone would put rows r and r + 8 on the same banks here: the row is two bank passes long, so
//     the chunk's own bit 4 no longer separates anything.)  Any 8 consecutive lanes differ in r & 7: distinct segments.
//   V transposed reads (ds_read_b64_tr_b16; a half wave reads rows 8h .. 8h + 7 at one 32-byte segment, four lanes x 8 bytes
//     per row): bit 3 of r is constant over them, r & 7 takes all eight values: eight distinct segments = all 64 banks once.
//     Odd-half rows find the segment's two chunks swapped; every lane addresses its own 8 bytes, so the read does not care.
//   Writes: LDS-DMA pieces are 1 KiB contiguous; the decode kernel's ds_write_b128 of a row's chunks 0..15 / 16..31 by a
//     16-lane group is a permutation of sixteen chunk positions.
// x(r) depends on r & 15 only: the + 16 / + 32 row offsets of the tile pieces are compile-time byte offsets.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int kv256_x(int row) { return ((row & 7) << 1) | ((row >> 3) & 1); }
__device__ __forceinline__ int kv256_img_chunk(int row, int c) { return row * 32 + (c ^ kv256_x(row)); }
// fragment read offsets of lane (fq, fg), bytes inside an image: the roles of attn_k_off / attn_v_off
__device__ __forceinline__ int attn256_k_off(int fq, int fg, int ks) { return 16 * kv256_img_chunk(fq, ks * 4 + fg); }
__device__ __forceinline__ int attn256_v_off(int fq, int fg, int d) {
    const int q4 = fq >> 2, p4 = fq & 3;
    return 16 * kv256_img_chunk(4 * fg + q4, 2 * d + (p4 >> 1)) + 8 * (p4 & 1);
}

constexpr int A256_HD = 256, A256_TILE_BYTES = 64 * A256_HD * 2;      // one K or V image: 32 KB
constexpr int PF256_WAVES = 4, PF256_QROWS = PF256_WAVES * PF_TQ * 16, PF256_NBUF = 2;
constexpr int attn256_prefill_lds_bytes() { return PF256_NBUF * 2 * A256_TILE_BYTES + 128 * 4; }      // ring + block table
constexpr int attn256_decode_lds_bytes(int nw) { return nw * A256_TILE_BYTES; }
// floats of one key-split partial record (attn_part_floats<HD>) for the head size of a model: the hosts' allocations
inline int attn_part_floats_rt(int hd) { return hd == 64 ? attn_part_floats<64>() : hd == 128 ? attn_part_floats<128>() : attn_part_floats<256>(); }

// ------------------------------------------------------------------------------------------
// Prefill.  grid (kv head, sequence, 128-row query tile), query tiles longest first as in attn.h; 256 threads.  Query rows are
// (position, head-in-group), position-major; wave w owns rows 32 w .. 32 w + 31 of the tile as two 16-row sub-tiles.
// Ring: tile kt sits in slot kt & 1.  Per tile:
//     s_waitcnt vmcnt(0) (my 16 pieces of tile kt landed: nothing else is in flight)  |  barrier  |
//     issue tile kt + 1 into the other slot (every wave has passed the barrier behind its last read of it)  |  compute kt
// so one whole tile (64 KB) is in flight under each tile's 64 MFMAs per wave.  Wave w moves pieces 16 w .. 16 w + 15 of the
// tile's [32 K pieces | 32 V pieces] list: waves 0, 1 the K image, waves 2, 3 the V image.  A piece is two image rows; the
// permutation goes into the SOURCE address (lane l of a piece lands at byte 16 l of it).
// Inside the loop the only vector-memory operations are the LDS-DMA pieces (block ids come from LDS: attn.h).
// ------------------------------------------------------------------------------------------
template <bool WINDOW, bool SOFTCAP = false>
__global__ __launch_bounds__(PF256_WAVES * 64, 1) void attn256_prefill_kernel(AttnArgs p) {
    constexpr int HD = A256_HD, KS = HD / 32, DT = HD / 16, CPR = HD / 8, TQ = PF_TQ, QROWS = PF256_QROWS;
    constexpr int TILE_BYTES = A256_TILE_BYTES, PW = 2 * (TILE_BYTES / 1024) / PF256_WAVES;      // 16 pieces per wave and tile
    // 2 x [K image | V image], then this sequence's block table (<= 128 blocks: host-checked).  No static LDS: the ring starts
    // at LDS address 0, so every LDS-DMA destination M0 carries stays below 128 KB.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* sblk = (int32_t*)(smem + PF256_NBUF * 2 * TILE_BYTES);

    const int seq = blockIdx.y, kvh = blockIdx.x, qt = gridDim.z - 1 - blockIdx.z;
    const int R = p.seq_len[seq] * p.group;    // query rows of this (seq, kv head)
    if (qt * QROWS >= R) return;
    const int tok0 = p.seq_tok_start[seq], pos0 = p.seq_pos[seq];
    const int32_t* tbl = p.blk_table + (int64_t)seq * p.tbl_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fq = lane & 15, fg = lane >> 4;
    if (tid < p.tbl_stride && tid < 128) sblk[tid] = tbl[tid];

    // this lane's query row of sub-tile qi; rows past R are clamped to the tile's first row (valid) and never stored
    const int w_row0 = qt * QROWS + wave * (TQ * 16);
    bf16x8 qf[TQ][KS];
    int qpos[TQ];
#pragma unroll
    for (int qi = 0; qi < TQ; qi++) {
        const int r = w_row0 + qi * 16 + fq, row = r < R ? r : qt * QROWS;
        const int si = row / p.group, hd_ = kvh * p.group + (row - si * p.group);
        qpos[qi] = pos0 + si;
        const bf16_t* qp = (const bf16_t*)p.q + (int64_t)(tok0 + si) * p.q_stride + hd_ * HD;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) qf[qi][ks] = *(const bf16x8*)(qp + ks * 32 + fg * 8);
    }
    // the Q fragments are complete before the first DMA is issued: no register is pending on a vector load in the loop
#pragma unroll
    for (int qi = 0; qi < TQ; qi++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) asm volatile("" : "+v"(qf[qi][ks]));
    __syncthreads();                      // sblk is visible

    // key tiles of the workgroup and of this wave (attn_prefill_setup at 128 rows)
    const int last_row = min(qt * QROWS + QROWS - 1, R - 1), w_last = min(w_row0 + TQ * 16 - 1, R - 1);
    const int n_kt = (pos0 + last_row / p.group) / 64 + 1;
    const int wave_n_kt = w_row0 < R ? (pos0 + w_last / p.group) / 64 + 1 : 0;
    const int wave_first_limit = pos0 + w_row0 / p.group;
    AttnPrefillWindow win{};
    if constexpr (WINDOW) {
        const int w_first = min(w_row0, R - 1);
        win = AttnPrefillWindow{p.window - 1, attn_window_kt_lo(pos0 + qt * QROWS / p.group, p.window),
                                attn_window_kt_lo(pos0 + w_first / p.group, p.window), pos0 + w_last / p.group - p.window + 1};
    }
    const int kt_lo = WINDOW ? win.kt_lo : 0;            // (< n_kt: the tile of the first row's lowest key)

    int src_off[PW];                 // byte offset of this lane's 16 bytes inside the (K or V) tile, per piece
#pragma unroll
    for (int i = 0; i < PW; i++) {
        const int jj = (wave * PW + i) % (TILE_BYTES / 1024);
        const int row = 2 * jj + (lane >> 5), c = (lane & 31) ^ kv256_x(row);
        src_off[i] = (row * HD + c * 8) * 2;
    }
    const uint32_t smem_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)smem;
    const void* my_cache = wave * PW >= TILE_BYTES / 1024 ? p.vcache : p.kcache;      // (wave-uniform)
    auto issue = [&](int kt, int buf) {
        const int bi = kv_block_index(p, kt * 64), krow0 = kt * 64 - bi * p.Tmax;      // (64 | Tmax: no straddling)
        const int blk = __builtin_amdgcn_readfirstlane(sblk[bi]);
        const bf16_t* base = (const bf16_t*)my_cache + (int64_t)blk * p.slot_stride + ((int64_t)kvh * p.Tmax + krow0) * HD;
        const uint32_t dst = smem_lds + buf * (2 * TILE_BYTES) + wave * (PW * 1024);   // (K pieces first, then V pieces)
#pragma unroll
        for (int i = 0; i < PW; i++) lds_dma16(base, (uint32_t)src_off[i], dst + i * 1024);
    };

    int k_off[KS], v_off[DT];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) k_off[ks] = attn256_k_off(fq, fg, ks);
#pragma unroll
    for (int d = 0; d < DT; d++) v_off[d] = attn256_v_off(fq, fg, d);
    f32x4 o[TQ][DT] = {};
    f32x4 lacc[TQ] = {};
    float m_run[TQ] = {-INFINITY, -INFINITY};
    const float sl2 = p.scale * 1.4426950408889634f;     // exp2 domain
    const float cap_a = SOFTCAP ? attn_cap_a(p) : 0.f, cap_c2 = SOFTCAP ? attn_cap_c2(p) : 0.f;

    issue(kt_lo, 0);
    int buf = 0;
    for (int kt = kt_lo; kt < n_kt; kt++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < n_kt) issue(kt + 1, buf ^ 1);
        const char* kimg = smem + buf * (2 * TILE_BYTES);
        const char* vimg = kimg + TILE_BYTES;
        buf ^= 1;
        if (kt >= wave_n_kt) continue;                   // (wave-uniform) every row of this wave is masked out here
        if (WINDOW && kt < win.wave_kt_lo) continue;     // (wave-uniform) ... or the tile lies below all of their windows
        attn_prefill_tile<HD, WINDOW, SOFTCAP>(fg, qpos, kt, wave_first_limit, sl2, kimg, vimg, k_off, v_off, qf, o, lacc, m_run, win, cap_a, cap_c2);
    }
#pragma unroll
    for (int qi = 0; qi < TQ; qi++) {
        const int row = w_row0 + qi * 16 + fq;
        if (row >= R) continue;
        const int si = row / p.group, hd_ = kvh * p.group + (row - si * p.group);
        const float inv = 1.0f / lacc[qi][0];
#pragma unroll
        for (int d = 0; d < DT; d++)    // O[q][d = 16d + 4fg + r], written in the next GEMM's operand layout
            act_store4<bf16_t>((bf16_t*)p.out, tok0 + si, hd_ * HD + d * 16 + fg * 4, p.out_stride, o[qi][d] * inv);
    }
}

// ------------------------------------------------------------------------------------------
// Decode: one new row per sequence, Q pre-rotated and K / V already appended (rope_kv_kernel / qk_norm_rope_kv_kernel: not
// fused).  grid (kv head x 16-head query tile, sequence, key split); NW = 2 or 4 waves.  The tiles kt_lo + vw, + nvw, .. of the
// NW x gridDim.z virtual waves as in attn_decode_bf16_kernel; per tile and wave
//     S^T = K . Q^T   K fragments straight HBM -> VGPR (32 x 16 bytes per lane), 32 MFMAs
//     V               32 loads of one contiguous KiB (two rows) each -> the wave's LDS image -> transposed reads, 32 MFMAs
// Software pipeline over the wave's own tiles, with no register beyond one tile's fragments: the NEXT tile's K loads leave
// once the scores have consumed the K registers (they fly under the softmax, the image fill and P.V), the next tile's V loads
// once the image holds the V registers (they fly under P.V and the next scores).  Vector loads return in order, so the
// compiler's counted waits are exact: the scores wait for K with the 32 V loads behind them still in flight.
// The leading arguments repeat AttnArgs fields for the kernarg preload (attn.h).
// ------------------------------------------------------------------------------------------
// SOFTCAP: attn_score2 per 16-key sub-tile, where its f32x4 leaves the MFMA (this kernel sits at 492 of 512 registers).
template <int NW, bool WINDOW, bool SOFTCAP = false>
__global__ __launch_bounds__(NW * 64, 1) void attn256_decode_kernel(const int32_t* __restrict__ a_seq_pos, const int32_t* __restrict__ a_blk_table,
                                                                    int a_tbl_stride, int a_bs_shift, int a_Tmax, int a_group, AttnArgs p) {
    static_assert(NW == 2 || NW == 4, "a wave per SIMD at most: 512 registers each, 32 KB of LDS each");
    constexpr int HD = A256_HD, KS = HD / 32, DT = HD / 16, NVL = 32, TILE_BYTES = A256_TILE_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [NW] wave-private V images (later: the partial O^T)
    __shared__ float red_m[NW][16];
    __shared__ float red_l[NW][16];
    NvlStampsT<false> stamps(nullptr, 0);
    const int QT = (a_group + 15) >> 4;
    const int seq = blockIdx.y, kvh = blockIdx.x / QT, qt = blockIdx.x - kvh * QT;
    const int32_t* tbl = a_blk_table + (int64_t)seq * a_tbl_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = seq, pos0 = a_seq_pos[seq];              // (decode launches carry one token per sequence, in sequence order)
    const int fq = lane & 15, fg = lane >> 4;                // MFMA role: query head qt*16 + fq of the group, k group fg
    const int dch = lane & 31, ksub = lane >> 5;             // row role: 16-byte chunk dch of key row 2 i + ksub
    const bool row_ok = qt * 16 + fq < a_group;
    const int head = kvh * a_group + (row_ok ? qt * 16 + fq : 0);
    char* vimg = smem + wave * TILE_BYTES;
    const int n_kt = pos0 / 64 + 1;
    const int kt_lo = WINDOW ? attn_window_kt_lo(pos0, p.window) : 0, wm1 = WINDOW ? p.window - 1 : 0;
    const int vw = kt_lo + blockIdx.z * NW + wave, nvw = NW * gridDim.z;
    const float sl2 = p.scale * 1.4426950408889634f;
    const float cap_a = SOFTCAP ? attn_cap_a(p) : 0.f, cap_c2 = SOFTCAP ? attn_cap_c2(p) : 0.f;

    bf16x8 qf[KS];
    {
        const bf16_t* qp = (const bf16_t*)p.q + (int64_t)tok * p.q_stride + head * HD;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) qf[ks] = *(const bf16x8*)(qp + ks * 32 + fg * 8);
    }
    f32x4 o[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;     // exp2 domain
    int v_off[DT];
#pragma unroll
    for (int d = 0; d < DT; d++) v_off[d] = attn256_v_off(fq, fg, d);
    // where this lane's V chunk of load i goes: row 2 i + ksub, chunk dch; x(row) repeats every 8 loads
    int w_off[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w_off[i] = 16 * kv256_img_chunk(2 * i + ksub, dch);

    bf16x8 kf[4][KS];
    bf16x8 vch[NVL];
    auto tile_base = [&](int kt) {
        const int bi = a_bs_shift >= 0 ? (kt * 64) >> a_bs_shift : (kt * 64) / a_Tmax, krow0 = kt * 64 - bi * a_Tmax;
        return (int64_t)tbl[bi] * p.slot_stride + ((int64_t)kvh * a_Tmax + krow0) * HD;      // (bi < tbl_stride: kt < n_kt)
    };
    auto run = [&](auto nt_tag) __attribute__((always_inline)) {
        constexpr bool NT = decltype(nt_tag)::value;         // non-temporal K/V loads (AttnArgs::kv_nt: attn.h)
        auto load_k = [&](int kt) __attribute__((always_inline)) {
            const bf16_t* kbase = (const bf16_t*)p.kcache + tile_base(kt);
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int ks = 0; ks < KS; ks++) {
                    const bf16x8* src = (const bf16x8*)(kbase + (int64_t)(t * 16 + fq) * HD + ks * 32 + fg * 8);
                    if constexpr (NT) kf[t][ks] = __builtin_nontemporal_load(src); else kf[t][ks] = *src;
                }
        };
        auto load_v = [&](int kt) __attribute__((always_inline)) {
            const bf16_t* vbase = (const bf16_t*)p.vcache + tile_base(kt);
#pragma unroll
            for (int i = 0; i < NVL; i++) {                                                                 // 1 KiB, contiguous
                const bf16x8* src = (const bf16x8*)(vbase + (int64_t)lane * 8 + i * 512);
                if constexpr (NT) vch[i] = __builtin_nontemporal_load(src); else vch[i] = *src;
            }
        };
        if (vw < n_kt) { load_k(vw); load_v(vw); }
        for (int kt = vw; kt < n_kt; kt += nvw) {
            const bool more = kt + nvw < n_kt;               // (wave-uniform)
            f32x4 s[1][4];
            float tmax = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[ks], acc, 0, 0, 0);
                const int lim = pos0 - kt * 64 - fg * 4;      // last visible key, relative to this lane's first
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = attn_score2<SOFTCAP>(acc[r], sl2, cap_a, cap_c2);
                    v = (WINDOW ? attn_in_window(t * 16 + r, lim - wm1, wm1) : (t * 16 + r <= lim)) ? v : -INFINITY;
                    acc[r] = v;
                    tmax = fmaxf(tmax, v);
                }
                s[0][t] = acc;
            }
            if (more) load_k(kt + nvw);
            attn_decode_softmax<HD, 1>(s, tmax, m_run, l_run, o);      // (every tile dealt holds a visible key: finite maximum)
            // a wave's LDS accesses execute in order: the fill may overwrite the image the last tile's reads came from
#pragma unroll
            for (int i = 0; i < NVL; i++) *(bf16x8*)(vimg + w_off[i & 7] + (i >> 3) * (16 * 32 * 16)) = vch[i];
            if (more) load_v(kt + nvw);
            attn_pv_tile<HD, 1, false>(vimg, v_off, &s[0], &o, nullptr);
        }
    };
    if (p.kv_nt) run(std::true_type{}); else run(std::false_type{});
    attn_decode_finish<HD, NW>(p, smem, vimg, red_m, red_l, o, m_run, l_run, seq, tok, head, row_ok, wave, lane, fq, fg, 1.0f, stamps);
}

}  // namespace nvl
