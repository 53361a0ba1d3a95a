// loader.h — safetensors -> device, without the reference's fp32 host expansion and host transposes
// (SURVEY §8 f-2).  Host-only C++; included at the end of nvllm.hip.
//
// Replaces tensor.LoadModelFromDirectory / LoadModel / LoadShardedModel (purego/tensor/generic_loader.go:184-265,
// 1016-1163) and LoadModelConfig (:808-972).  The checkpoint is mmap'ed; every 2-D weight goes to nvl_upload_tensor
// in the checkpoint's own dtype (F32 / F16 / BF16, :645-663) and PyTorch [out, in] layout — the dtype conversion,
// the [in, out] view the reference builds with Transpose (:398-403, :533-552) and the tiling into the kernels'
// operand layout all happen on the device.  Only the fused projections go through a host fp32 copy (GPT-2 c_attn,
// Falcon query_key_value: split rules of :674-748), because their split is defined on the fp32 [in, out] matrix.
// Differences from the reference, on purpose: sharded checkpoints may hold MoE layers (the reference's shard path has
// none, :1270-1273); a tensor is looked up under its name and under "transformer." + name in every file (:622-629).
#pragma once
#include "int4_unpack.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace nvl_loader {

// ---------------------------------------------------------------------------------------------
// JSON (just what config.json / safetensors headers need)
// ---------------------------------------------------------------------------------------------
struct JVal {
    enum Kind { NUL, BOOL, NUM, STR, ARR, OBJ } kind = NUL;
    bool b = false;
    double num = 0;
    std::string str;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const std::string& k) const {
        if (kind != OBJ) return nullptr;
        for (auto& kv : obj) if (kv.first == k) return &kv.second;
        return nullptr;
    }
};

struct JParser {
    const char* p; const char* end;
    int depth = 0;                         // nesting is capped: a hostile header must not recurse the stack away
    static constexpr int MAX_DEPTH = 64;
    JParser(const char* s, size_t n) : p(s), end(s + n) {}
    [[noreturn]] void bad(const char* what) { throw std::runtime_error(std::string("json: ") + what); }
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
    JVal parse() { ws(); JVal v = value(); ws(); return v; }
    struct Depth { int& d; explicit Depth(int& d_) : d(d_) { ++d; } ~Depth() { --d; } };
    JVal value() {
        if (p >= end) bad("unexpected end");
        Depth guard(depth);
        if (depth > MAX_DEPTH) bad("nesting deeper than 64 levels");
        JVal v;
        switch (*p) {
            case '{': {
                v.kind = JVal::OBJ; p++; ws();
                if (p < end && *p == '}') { p++; return v; }
                for (;;) {
                    ws();
                    if (p >= end || *p != '"') bad("expected a key");
                    std::string k = string();
                    ws();
                    if (p >= end || *p != ':') bad("expected ':'");
                    p++; ws();
                    v.obj.emplace_back(std::move(k), value());
                    ws();
                    if (p < end && *p == ',') { p++; continue; }
                    if (p < end && *p == '}') { p++; return v; }
                    bad("expected ',' or '}'");
                }
            }
            case '[': {
                v.kind = JVal::ARR; p++; ws();
                if (p < end && *p == ']') { p++; return v; }
                for (;;) {
                    ws();
                    v.arr.push_back(value());
                    ws();
                    if (p < end && *p == ',') { p++; continue; }
                    if (p < end && *p == ']') { p++; return v; }
                    bad("expected ',' or ']'");
                }
            }
            case '"': v.kind = JVal::STR; v.str = string(); return v;
            case 't': lit("true"); v.kind = JVal::BOOL; v.b = true; return v;
            case 'f': lit("false"); v.kind = JVal::BOOL; v.b = false; return v;
            case 'n': lit("null"); return v;
            default: {
                char* e = nullptr;
                v.num = std::strtod(p, &e);          // (headers are NUL-terminated copies: strtod cannot run off the end)
                if (e == p) bad("unexpected character");
                v.kind = JVal::NUM; p = e; return v;
            }
        }
    }
    void lit(const char* s) { const size_t n = strlen(s); if ((size_t)(end - p) < n || strncmp(p, s, n) != 0) bad("bad literal"); p += n; }
    std::string string() {
        std::string out; p++;
        while (p < end && *p != '"') {
            if (*p == '\\') {
                if (++p >= end) bad("bad escape");
                switch (*p) {
                    case 'n': out += '\n'; break; case 't': out += '\t'; break; case 'r': out += '\r'; break;
                    case 'b': out += '\b'; break; case 'f': out += '\f'; break;
                    case 'u': {     // keep BMP code points as UTF-8; names in checkpoints are ASCII anyway
                        if (end - p < 5) bad("bad \\u escape");
                        const unsigned cp = (unsigned)std::strtoul(std::string(p + 1, 4).c_str(), nullptr, 16);
                        if (cp < 0x80) out += (char)cp;
                        else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 63)); }
                        else { out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 63)); out += (char)(0x80 | (cp & 63)); }
                        p += 4; break;
                    }
                    default: out += *p;
                }
                p++;
            } else out += *p++;
        }
        if (p >= end) bad("unterminated string");
        p++;
        return out;
    }
};

inline std::string read_text(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::string s; char buf[1 << 16]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}
inline bool exists(const std::string& path, bool* is_dir = nullptr) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return false;
    if (is_dir) *is_dir = S_ISDIR(st.st_mode);
    return true;
}

// ---------------------------------------------------------------------------------------------
// safetensors: 8-byte LE header length, JSON header {name: {dtype, shape, data_offsets}}, raw little-endian data
// (generic_loader.go:184-199, loader.go:13-17)
// ---------------------------------------------------------------------------------------------
constexpr int ST_F8_E4M3 = 100;     // loader-only dtype tag of an F8_E4M3 tensor (never passed to nvl_upload_tensor)
constexpr int ST_I32 = 101;         // ... of an I32 tensor: the packed .qweight / .qzeros / .g_idx of AWQ / GPTQ checkpoints
// scale: an F8_E4M3 "<name>.weight"'s "<name>.weight_scale" (linked after every file is read), or NULL
struct StTensor { const uint8_t* data = nullptr; int dtype = 0; std::vector<int64_t> shape; size_t bytes = 0; int64_t numel = 1;
                  const StTensor* scale = nullptr; };

struct StFile {
    int fd = -1; void* map = MAP_FAILED; size_t size = 0;
    ~StFile() { if (map != MAP_FAILED) munmap(map, size); if (fd >= 0) close(fd); }
};

struct StSet {
    std::vector<std::unique_ptr<StFile>> files;
    std::map<std::string, StTensor> tensors;

    void add_file(const std::string& path) {
        std::unique_ptr<StFile> f(new StFile);
        f->fd = open(path.c_str(), O_RDONLY);
        if (f->fd < 0) throw std::runtime_error("cannot open " + path);
        struct stat st; fstat(f->fd, &st); f->size = (size_t)st.st_size;
        if (f->size < 8) throw std::runtime_error(path + ": not a safetensors file");
        f->map = mmap(nullptr, f->size, PROT_READ, MAP_PRIVATE, f->fd, 0);
        if (f->map == MAP_FAILED) throw std::runtime_error("mmap failed for " + path);
        const uint8_t* base = (const uint8_t*)f->map;
        uint64_t hlen = 0; memcpy(&hlen, base, 8);
        if (hlen > f->size - 8) throw std::runtime_error(path + ": header length exceeds the file");
        const std::string header((const char*)base + 8, (size_t)hlen);
        const JVal root = JParser(header.c_str(), header.size()).parse();
        if (root.kind != JVal::OBJ) throw std::runtime_error(path + ": header is not a JSON object");
        const uint8_t* data = base + 8 + hlen;
        const size_t data_len = f->size - 8 - (size_t)hlen;
        for (auto& kv : root.obj) {
            if (kv.first == "__metadata__") continue;
            const JVal *dt = kv.second.get("dtype"), *sh = kv.second.get("shape"), *off = kv.second.get("data_offsets");
            if (!dt || !sh || !off || off->arr.size() != 2) throw std::runtime_error(path + ": malformed entry " + kv.first);
            StTensor t;
            if (dt->str == "F32") t.dtype = NVL_DTYPE_F32; else if (dt->str == "BF16") t.dtype = NVL_DTYPE_BF16;
            else if (dt->str == "F16") t.dtype = NVL_DTYPE_F16; else if (dt->str == "F8_E4M3") t.dtype = ST_F8_E4M3;
            else if (dt->str == "I32") t.dtype = ST_I32;
            else t.dtype = -1;      // refused only if the model needs it (:660-662)
            for (auto& d : sh->arr) {      // dimensions: non-negative integers whose product stays far inside int64
                if (d.kind != JVal::NUM || !(d.num >= 0) || d.num > 4.0e12 || d.num != (double)(int64_t)d.num)
                    throw std::runtime_error(path + ": bad dimension in the shape of " + kv.first);
                const int64_t dim = (int64_t)d.num;
                if (dim != 0 && t.numel > ((int64_t)1 << 46) / dim)
                    throw std::runtime_error(path + ": shape of " + kv.first + " overflows");
                t.shape.push_back(dim); t.numel *= dim;
            }
            if (off->arr[0].kind != JVal::NUM || off->arr[1].kind != JVal::NUM || !(off->arr[0].num >= 0) || !(off->arr[1].num >= 0) ||
                off->arr[0].num > 9.0e15 || off->arr[1].num > 9.0e15)
                throw std::runtime_error(path + ": bad data_offsets of " + kv.first);
            const size_t b = (size_t)off->arr[0].num, e = (size_t)off->arr[1].num;
            if (e < b || e > data_len) throw std::runtime_error(path + ": data_offsets of " + kv.first + " outside the file");
            t.data = data + b; t.bytes = e - b;
            if (t.dtype >= 0 && t.bytes != (size_t)t.numel * (t.dtype == NVL_DTYPE_F32 || t.dtype == ST_I32 ? 4 : t.dtype == ST_F8_E4M3 ? 1 : 2))
                throw std::runtime_error(path + ": byte size of " + kv.first + " does not match its shape");
            tensors[kv.first] = std::move(t);
        }
        files.push_back(std::move(f));
    }
    // a file, or a directory with model.safetensors or model.safetensors.index.json + shards (:1016-1040, :1042-1075)
    void open_path(const std::string& path) {
        bool dir = false;
        if (!exists(path, &dir)) throw std::runtime_error("no such file or directory: " + path);
        if (!dir) { add_file(path); return; }
        const std::string idx = path + "/model.safetensors.index.json";
        if (exists(idx)) {
            const std::string txt = read_text(idx);
            const JVal root = JParser(txt.c_str(), txt.size()).parse();
            const JVal* wm = root.get("weight_map");
            if (!wm || wm->kind != JVal::OBJ) throw std::runtime_error(idx + ": no weight_map");
            std::vector<std::string> shards;
            for (auto& kv : wm->obj) {
                const std::string& sn = kv.second.str;      // a shard is a plain file name inside the model directory
                if (kv.second.kind != JVal::STR || sn.empty() || sn.find('/') != std::string::npos || sn.find('\\') != std::string::npos ||
                    sn == "." || sn.find("..") != std::string::npos)
                    throw std::runtime_error(idx + ": weight_map names a shard outside the model directory: '" + sn + "'");
                if (std::find(shards.begin(), shards.end(), sn) == shards.end()) shards.push_back(sn);
            }
            for (auto& s : shards) add_file(path + "/" + s);
            return;
        }
        add_file(path + "/model.safetensors");
    }
    // FP8 checkpoints (compressed-tensors naming): "<name>.weight" F8_E4M3 + "<name>.weight_scale"; "input_scale" is ignored
    // (activations stay bf16).  Run once after every file is added.
    void link_scales() {
        for (auto& kv : tensors) {
            if (kv.second.dtype != ST_F8_E4M3) continue;
            const std::string& n = kv.first;
            if (n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0) {
                auto it = tensors.find(n + "_scale");
                if (it != tensors.end()) kv.second.scale = &it->second;
            }
        }
    }
    const StTensor* find(const std::string& name) const {           // :619-632
        auto it = tensors.find(name);
        if (it == tensors.end()) it = tensors.find("transformer." + name);
        return it == tensors.end() ? nullptr : &it->second;
    }
    const StTensor& need(const std::string& name) const {
        const StTensor* t = find(name);
        if (!t) throw std::runtime_error("required tensor '" + name + "' not found (also tried: transformer." + name + ")");
        if (t->dtype < 0) throw std::runtime_error("unsupported dtype for tensor '" + name + "'");
        return *t;
    }
};

inline float f32_of(const StTensor& t, int64_t i);
// the per-row scales of an F8_E4M3 [N, K] weight: weight_scale F32 / BF16 of shape [N], [N, 1] or a scalar (broadcast);
// anything else (block-wise [N/b, K/b], per-input-channel, ...) is refused
inline std::vector<float> f8_row_scales(const StTensor& t, const std::string& what) {
    if (t.shape.size() != 2) throw std::runtime_error("F8_E4M3 tensor " + what + ": a 2-D weight was expected");
    if (!t.scale) throw std::runtime_error("F8_E4M3 tensor " + what + " has no weight_scale");
    const StTensor& s = *t.scale;
    if (s.dtype != NVL_DTYPE_F32 && s.dtype != NVL_DTYPE_BF16) throw std::runtime_error(what + "_scale: F32 or BF16 expected");
    const int64_t N = t.shape[0];
    const bool scalar = s.numel == 1 && s.shape.size() <= 2;
    const bool per_row = (s.shape.size() == 1 && s.shape[0] == N) || (s.shape.size() == 2 && s.shape[0] == N && s.shape[1] == 1);
    if (!scalar && !per_row)
        throw std::runtime_error(what + "_scale: only per-output-channel ([N] or [N,1]) or scalar scales are supported (block-wise scales are not)");
    std::vector<float> v((size_t)N);
    for (int64_t r = 0; r < N; r++) {
        v[(size_t)r] = f32_of(s, scalar ? 0 : r);
        if (!(v[(size_t)r] > 0.f) || !std::isfinite(v[(size_t)r])) throw std::runtime_error(what + "_scale: scales must be finite and positive");
    }
    return v;
}
// the per-(expert, output row) scales of an F8_E4M3 MoE expert weight [E, out, in]: weight_scale F32 / BF16 of shape
// [E, out] or [E, out, 1], per expert ([E] or [E, 1, 1], broadcast over the rows) or a scalar; block-wise scales are refused
inline std::vector<float> f8_expert_scales(const StTensor& t, const std::string& what) {
    if (t.shape.size() != 3) throw std::runtime_error("F8_E4M3 tensor " + what + ": a 3-D [E, out, in] expert weight was expected");
    if (!t.scale) throw std::runtime_error("F8_E4M3 tensor " + what + " has no weight_scale");
    const StTensor& s = *t.scale;
    if (s.dtype != NVL_DTYPE_F32 && s.dtype != NVL_DTYPE_BF16) throw std::runtime_error(what + "_scale: F32 or BF16 expected");
    const int64_t E = t.shape[0], N = t.shape[1];
    const auto& d = s.shape;
    const bool scalar = s.numel == 1 && d.size() <= 3;
    const bool per_row = (d.size() == 2 && d[0] == E && d[1] == N) || (d.size() == 3 && d[0] == E && d[1] == N && d[2] == 1);
    const bool per_expert = (d.size() == 1 && d[0] == E) || (d.size() == 3 && d[0] == E && d[1] == 1 && d[2] == 1);
    if (!scalar && !per_row && !per_expert)
        throw std::runtime_error(what + "_scale: only per-(expert, output channel) ([E,out] or [E,out,1]), per-expert ([E] or [E,1,1]) "
                                 "or scalar scales are supported (block-wise scales are not)");
    std::vector<float> v((size_t)(E * N));
    for (int64_t r = 0; r < E * N; r++) {
        v[(size_t)r] = f32_of(s, scalar ? 0 : (per_row ? r : r / N));
        if (!(v[(size_t)r] > 0.f) || !std::isfinite(v[(size_t)r])) throw std::runtime_error(what + "_scale: scales must be finite and positive");
    }
    return v;
}
inline float f32_of(const StTensor& t, int64_t i) {                  // :769-805
    if (t.dtype == ST_F8_E4M3) {         // W~ = bf16(s * e4m3(code)): what an 8-bit-weight model computes with
        const int64_t K = t.shape.size() == 2 ? t.shape[1] : 1;
        const float s = t.scale ? f32_of(*t.scale, t.scale->numel == 1 ? 0 : i / K) : 1.0f;
        if ((t.data[i] & 0x7F) == 0x7F) throw std::runtime_error("F8_E4M3 tensor holds a NaN code");
        return nvl::w8_value(t.data[i], s);
    }
    if (t.dtype == NVL_DTYPE_F32) { float f; memcpy(&f, t.data + i * 4, 4); return f; }
    uint16_t h; memcpy(&h, t.data + i * 2, 2);
    uint32_t u;
    if (t.dtype == NVL_DTYPE_BF16) u = (uint32_t)h << 16;
    else {
        const uint32_t s = (h >> 15) & 1u, e = (h >> 10) & 31u, m = h & 1023u;
        if (e == 0) {
            if (m == 0) u = s << 31;
            else { int k = 0; uint32_t mm = m; while (!(mm & 1024u)) { mm <<= 1; k++; } u = (s << 31) | ((uint32_t)(113 - k) << 23) | ((mm & 1023u) << 13); }
        } else if (e == 31) u = (s << 31) | 0x7F800000u | (m << 13);
        else u = (s << 31) | ((e + 112u) << 23) | (m << 13);
    }
    float f; memcpy(&f, &u, 4); return f;
}

}  // namespace nvl_loader

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
namespace {
using nvl_loader::StSet; using nvl_loader::StTensor; using nvl_loader::JVal;

// an F8_E4M3 weight [N, K] with its row scales: as it is into a kind the model stores 8-bit (checkpoint order [out, in]),
// else W~ = bf16(s * e4m3(q)) through nvl_upload_tensor (exact in bf16)
void up2d_f8(nvl_model* m, int kind, int layer, const uint8_t* codes, const std::vector<float>& sc, int64_t N, int64_t K, int layout) {
    for (int64_t i = 0; i < N * K; i++)
        if ((codes[i] & 0x7F) == 0x7F) throw std::runtime_error("loader: F8_E4M3 weight holds a NaN code");
    int rc;
    if (q_kind(m, kind) == WF_FP8 && (layout == NVL_LAYOUT_OUT_IN || kind == NVL_T_TOK_EMB)) {
        rc = nvl_upload_tensor_fp8(m, kind, layer, codes, sc.data(), N, K, NVL_LAYOUT_OUT_IN);
    } else {
        std::vector<float> w((size_t)(N * K));
        for (int64_t r = 0; r < N; r++)
            for (int64_t k = 0; k < K; k++) w[(size_t)(r * K + k)] = nvl::w8_value(codes[r * K + k], sc[(size_t)r]);
        rc = nvl_upload_tensor(m, kind, layer, w.data(), NVL_DTYPE_F32, N, K, layout);
    }
    if (rc) throw std::runtime_error(std::string("loader: ") + nvl_last_error(m));
}
void up2d(nvl_model* m, int kind, int layer, const StTensor& t, int layout) {
    if (t.shape.size() != 2) throw std::runtime_error("loader: a 2-D tensor was expected");
    if (t.dtype == nvl_loader::ST_F8_E4M3) {
        if (layout != NVL_LAYOUT_OUT_IN && kind != NVL_T_TOK_EMB)
            throw std::runtime_error("loader: F8_E4M3 weights are supported in the [out, in] layout only");
        up2d_f8(m, kind, layer, t.data, nvl_loader::f8_row_scales(t, "weight"), t.shape[0], t.shape[1], layout);
        return;
    }
    const int rc = nvl_upload_tensor(m, kind, layer, t.data, t.dtype, t.shape[0], t.shape[1], layout);
    if (rc) throw std::runtime_error(std::string("loader: ") + nvl_last_error(m));
}
// INT4 group-quantized checkpoints (AWQ / GPTQ, int4_unpack.h): "<base>.qweight" + ".qzeros" + ".scales" (I32 / I32 / F16,
// GPTQ also ".g_idx") where a covered projection's "<base>.weight" would be.  true: unpacked into `out` (rows appended: the
// Q|K|V-free pairs gate | up are concatenated by calling it twice); false: the checkpoint has no such tensor.
bool gq_unpack(nvl_model* m, const StSet& st, const std::string& base, nvl_int4::Canon* out) {
    const StTensor* qw = st.find(base + ".qweight");
    if (!qw) return false;
    if (nvl::wf_base(m->wf) != nvl::WF_INT4)
        throw std::runtime_error("loader: " + base + " is INT4 group-quantized (.qweight); call nvl_set_gq_weight_dtype with the checkpoint's group_size first");
    const StTensor *qz = st.find(base + ".qzeros"), *sc = st.find(base + ".scales"), *gi = st.find(base + ".g_idx");
    if (!qz || !sc) throw std::runtime_error("loader: " + base + ".qweight without .qzeros / .scales");
    if (qw->dtype != nvl_loader::ST_I32 || qz->dtype != nvl_loader::ST_I32 || sc->dtype != NVL_DTYPE_F16)
        throw std::runtime_error("loader: " + base + ": qweight / qzeros / scales must be I32 / I32 / F16");
    int layout = 0, g = 0;
    int64_t K = 0, N = 0;
    std::string e = nvl_int4::detect(qw->shape, qz->shape, sc->shape, &layout, &K, &N, &g);
    if (!e.empty()) throw std::runtime_error("loader: " + base + ": " + e);
    if (g != nvl::wf_group(m->wf))
        throw std::runtime_error("loader: " + base + ": group size " + std::to_string(g) + " differs from the model's " + std::to_string(nvl::wf_group(m->wf)));
    if (gi && (gi->dtype != nvl_loader::ST_I32 || gi->numel != K)) throw std::runtime_error("loader: " + base + ".g_idx must be I32 [K]");
    nvl_int4::Canon c;
    if (layout == nvl_int4::LAYOUT_AWQ) e = nvl_int4::unpack_awq((const int32_t*)qw->data, (const int32_t*)qz->data, (const uint16_t*)sc->data, K, N, g, &c);
    else e = nvl_int4::unpack_gptq((const int32_t*)qw->data, (const int32_t*)qz->data, (const uint16_t*)sc->data, gi ? (const int32_t*)gi->data : nullptr, K, N, g, &c);
    if (!e.empty()) throw std::runtime_error("loader: " + base + ": " + e);
    if (out->N && out->K != c.K) throw std::runtime_error("loader: " + base + ": input width differs from its pair's");
    out->K = c.K; out->g = c.g; out->N += c.N;
    out->codes.insert(out->codes.end(), c.codes.begin(), c.codes.end());
    out->scales.insert(out->scales.end(), c.scales.begin(), c.scales.end());
    out->zeros.insert(out->zeros.end(), c.zeros.begin(), c.zeros.end());
    return true;
}
void gq_upload(nvl_model* m, int kind, int layer, const nvl_int4::Canon& c) {
    if (nvl_upload_tensor_int4(m, kind, layer, c.codes.data(), c.scales.data(), c.zeros.data(), c.N, c.K, NVL_LAYOUT_OUT_IN))
        throw std::runtime_error(std::string("loader: ") + nvl_last_error(m));
}
// a projection "<base>.weight" [out, in], or its INT4 group-quantized form
void up2d_proj(nvl_model* m, int kind, int layer, const StSet& st, const std::string& base) {
    nvl_int4::Canon c;
    if (gq_unpack(m, st, base, &c)) gq_upload(m, kind, layer, c);
    else up2d(m, kind, layer, st.need(base + ".weight"), NVL_LAYOUT_OUT_IN);
}
void up1d(nvl_model* m, int kind, int layer, const StTensor& t) {
    if (t.dtype == nvl_loader::ST_F8_E4M3) throw std::runtime_error("loader: an F8_E4M3 1-D tensor is not supported");
    const int rc = nvl_upload_tensor(m, kind, layer, t.data, t.dtype, t.numel, 1, NVL_LAYOUT_IN_OUT);
    if (rc) throw std::runtime_error(std::string("loader: ") + nvl_last_error(m));
}
// loadNorm (:595-604): weight required, bias (".weight" -> ".bias") optional
void load_norm(nvl_model* m, const StSet& st, const std::string& key, int kind_w, int kind_b, int layer) {
    up1d(m, kind_w, layer, st.need(key));
    std::string bk = key;
    const size_t p = bk.find(".weight");
    if (p != std::string::npos) bk.replace(p, 7, ".bias");
    if (const StTensor* b = st.find(bk)) if (b->dtype >= 0) up1d(m, kind_b, layer, *b);
}
std::vector<float> to_f32(const StTensor& t) {
    std::vector<float> v((size_t)t.numel);
    for (int64_t i = 0; i < t.numel; i++) v[(size_t)i] = nvl_loader::f32_of(t, i);
    return v;
}
}  // namespace

// FP8-KV checkpoints: the per-layer scalar *.self_attn.k_scale / v_scale, taken when the model has an 8-bit cache
inline void load_kv_scales(nvl_model* m, const StSet& st, const std::string& p, int l) {
    if (!m->kv8) return;
    const StTensor* k = st.find(p + ".self_attn.k_scale");
    const StTensor* v = st.find(p + ".self_attn.v_scale");
    for (const StTensor* t : {k, v})
        if (t && (t->dtype < 0 || t->numel != 1)) throw std::runtime_error(p + ": k_scale / v_scale must be scalars");
    const float ks = k ? f32_of(*k, 0) : m->k_scale[(size_t)l], vs = v ? f32_of(*v, 0) : m->v_scale[(size_t)l];
    if (!(ks > 0.f) || !(vs > 0.f) || !std::isfinite(ks) || !std::isfinite(vs))
        throw std::runtime_error(p + ": k_scale / v_scale must be finite and positive");
    m->k_scale[(size_t)l] = ks; m->v_scale[(size_t)l] = vs;
}

extern "C" int nvl_load_safetensors(nvl_model* m, const char* path) {
    if (!m || !path) return NVL_ERR_INVALID;
    if (m->finalized) return fail(m, NVL_ERR_STATE, "nvl_load_safetensors: model already finalized");
    NVL_TRY(m)
    StSet st;
    st.open_path(path);
    st.link_scales();
    const nvl_model_config& c = m->cfg;
    // which WeightMapping (:60-181) — told from the checkpoint's own names
    const bool gpt2 = st.find("wte.weight") != nullptr;
    const bool falcon = st.find("transformer.word_embeddings.weight") != nullptr || st.find("word_embeddings.weight") != nullptr;
    const bool llama = st.find("model.embed_tokens.weight") != nullptr;       // Llama and Granite-MoE share the naming
    if (gpt2 + falcon + llama != 1) throw std::runtime_error("nvl_load_safetensors: cannot tell the architecture from the tensor names");
    const int OI = NVL_LAYOUT_OUT_IN, IO = NVL_LAYOUT_IN_OUT;

    if (gpt2) {                                                                // GetGPT2Mapping (:60-78): weights already [in, out]
        up2d(m, NVL_T_TOK_EMB, 0, st.need("wte.weight"), IO);
        if (const StTensor* pe = st.find("wpe.weight")) up2d(m, NVL_T_POS_EMB, 0, *pe, IO);
        for (int l = 0; l < c.num_layers; l++) {
            const std::string p = "h." + std::to_string(l);
            if (st.need(p + ".attn.c_attn.weight").dtype == nvl_loader::ST_F8_E4M3)
                throw std::runtime_error("loader: F8_E4M3 weights are supported in the [out, in] layout only");
            const std::vector<float> w = to_f32(st.need(p + ".attn.c_attn.weight"));     // splitGPT2QKV (:674-702)
            std::vector<float> b;
            if (const StTensor* bt = st.find(p + ".attn.c_attn.bias")) b = to_f32(*bt);
            if (nvl_upload_gpt2_qkv(m, l, w.data(), b.empty() ? nullptr : b.data())) throw std::runtime_error(nvl_last_error(m));
            up2d(m, NVL_T_WO, l, st.need(p + ".attn.c_proj.weight"), IO);
            if (const StTensor* bo = st.find(p + ".attn.c_proj.bias")) up1d(m, NVL_T_BO, l, *bo);
            up2d(m, NVL_T_W1, l, st.need(p + ".mlp.c_fc.weight"), IO);
            up2d(m, NVL_T_W2, l, st.need(p + ".mlp.c_proj.weight"), IO);
            // (the FFN biases are looked up as "...c_fc.weight.bias" by the reference and never found: :559-560 — not loaded)
            load_norm(m, st, p + ".ln_1.weight", NVL_T_ATTN_NORM_W, NVL_T_ATTN_NORM_B, l);
            load_norm(m, st, p + ".ln_2.weight", NVL_T_FFN_NORM_W, NVL_T_FFN_NORM_B, l);
        }
        load_norm(m, st, "ln_f.weight", NVL_T_FINAL_NORM_W, NVL_T_FINAL_NORM_B, 0);
    } else if (falcon) {                                                       // GetFalconMapping (:81-98): PyTorch [out, in]
        up2d(m, NVL_T_TOK_EMB, 0, st.need("transformer.word_embeddings.weight"), IO);
        for (int l = 0; l < c.num_layers; l++) {
            const std::string p = "transformer.h." + std::to_string(l);
            const StTensor& qkv = st.need(p + ".self_attention.query_key_value.weight");   // [(nH+2)*hd, H]
            if (qkv.shape.size() != 2) throw std::runtime_error("query_key_value: 2-D expected");
            const int64_t R = qkv.shape[0], K = qkv.shape[1];
            std::vector<float> t((size_t)(R * K));                             // Transpose BEFORE splitting (:366-369)
            for (int64_t r = 0; r < R; r++)
                for (int64_t k = 0; k < K; k++) t[(size_t)(k * R + r)] = nvl_loader::f32_of(qkv, r * K + k);
            if (nvl_upload_falcon_qkv(m, l, t.data())) throw std::runtime_error(nvl_last_error(m));
            up2d(m, NVL_T_WO, l, st.need(p + ".self_attention.dense.weight"), OI);
            up2d(m, NVL_T_W1, l, st.need(p + ".mlp.dense_h_to_4h.weight"), OI);
            up2d(m, NVL_T_W2, l, st.need(p + ".mlp.dense_4h_to_h.weight"), OI);
            load_norm(m, st, p + ".input_layernorm.weight", NVL_T_ATTN_NORM_W, NVL_T_ATTN_NORM_B, l);   // parallel block: InputLN
        }
        load_norm(m, st, "transformer.ln_f.weight", NVL_T_FINAL_NORM_W, NVL_T_FINAL_NORM_B, 0);
        if (!c.tied_embedding) if (const StTensor* lm = st.find("lm_head.weight")) up2d(m, NVL_T_LM_HEAD, 0, *lm, OI);
    } else {                                                                   // GetLlamaMapping / GetGraniteMoEMapping (:101-141)
        up2d(m, NVL_T_TOK_EMB, 0, st.need("model.embed_tokens.weight"), IO);
        for (int l = 0; l < c.num_layers; l++) {
            const std::string p = "model.layers." + std::to_string(l);
            const bool is_mamba = l < 128 && ((c.mamba_layer_mask[l >> 6] >> (l & 63)) & 1);
            const bool hybrid = (c.mamba_layer_mask[0] | c.mamba_layer_mask[1]) != 0;
            if (hybrid) {
                // GetGraniteMapping (:145-181) + loadMamba2 (:461-512): Mamba2 tensors keep the checkpoint's layouts; every block
                // of the hybrid has the shared MLP (shared_mlp.input_linear = gate | up already fused, output_linear)
                if (is_mamba) {
                    up2d(m, NVL_T_MAMBA_IN_PROJ, l, st.need(p + ".mamba.in_proj.weight"), OI);
                    up2d(m, NVL_T_MAMBA_OUT_PROJ, l, st.need(p + ".mamba.out_proj.weight"), OI);
                    up1d(m, NVL_T_MAMBA_CONV_W, l, st.need(p + ".mamba.conv1d.weight"));          // [conv_dim, 1, K]
                    if (const StTensor* t = st.find(p + ".mamba.conv1d.bias")) up1d(m, NVL_T_MAMBA_CONV_B, l, *t);
                    up1d(m, NVL_T_MAMBA_A_LOG, l, st.need(p + ".mamba.A_log"));
                    up1d(m, NVL_T_MAMBA_D, l, st.need(p + ".mamba.D"));
                    up1d(m, NVL_T_MAMBA_DT_BIAS, l, st.need(p + ".mamba.dt_bias"));
                    up1d(m, NVL_T_MAMBA_NORM, l, st.need(p + ".mamba.norm.weight"));
                } else {
                    up2d(m, NVL_T_WQ, l, st.need(p + ".self_attn.q_proj.weight"), OI);
                    up2d(m, NVL_T_WK, l, st.need(p + ".self_attn.k_proj.weight"), OI);
                    up2d(m, NVL_T_WV, l, st.need(p + ".self_attn.v_proj.weight"), OI);
                    up2d(m, NVL_T_WO, l, st.need(p + ".self_attn.o_proj.weight"), OI);
                    load_kv_scales(m, st, p, l);
                }
                up2d(m, NVL_T_W1, l, st.need(p + ".shared_mlp.input_linear.weight"), OI);
                up2d(m, NVL_T_W2, l, st.need(p + ".shared_mlp.output_linear.weight"), OI);
                load_norm(m, st, p + ".input_layernorm.weight", NVL_T_ATTN_NORM_W, NVL_T_ATTN_NORM_B, l);
                load_norm(m, st, p + ".post_attention_layernorm.weight", NVL_T_FFN_NORM_W, NVL_T_FFN_NORM_B, l);
                continue;
            }
            up2d_proj(m, NVL_T_WQ, l, st, p + ".self_attn.q_proj");        // (or the projection's .qweight / .qzeros / .scales)
            up2d_proj(m, NVL_T_WK, l, st, p + ".self_attn.k_proj");
            up2d_proj(m, NVL_T_WV, l, st, p + ".self_attn.v_proj");
            up2d_proj(m, NVL_T_WO, l, st, p + ".self_attn.o_proj");
            load_kv_scales(m, st, p, l);
            if (c.use_moe) {                                                   // loadMoE (:566-592)
                up2d(m, NVL_T_ROUTER, l, st.need(p + ".block_sparse_moe.router.layer.weight"), OI);   // [E, H]: "always transpose"
                for (int which = 0; which < 2; which++) {
                    const std::string name = p + (which ? ".block_sparse_moe.output_linear.weight" : ".block_sparse_moe.input_linear.weight");
                    const StTensor& e = st.need(name);
                    if (e.shape.size() != 3) throw std::runtime_error("expert weights: 3-D [E, out, in] expected");
                    if (e.dtype == nvl_loader::ST_F8_E4M3) {     // codes as they are into 8-bit experts, else W~ (up2d_f8)
                        up2d_f8(m, which ? NVL_T_MOE_OUT : NVL_T_MOE_IN, l, e.data, nvl_loader::f8_expert_scales(e, name),
                                e.shape[0] * e.shape[1], e.shape[2], OI);
                        continue;
                    }
                    const int rc = nvl_upload_tensor(m, which ? NVL_T_MOE_OUT : NVL_T_MOE_IN, l, e.data, e.dtype,
                                                     e.shape[0] * e.shape[1], e.shape[2], IO);
                    if (rc) throw std::runtime_error(nvl_last_error(m));
                }
            } else if (st.find(p + ".mlp.gate_proj.qweight")) {                 // INT4 pair: gate rows, then up rows (groups lie along k)
                nvl_int4::Canon w1;
                if (!gq_unpack(m, st, p + ".mlp.gate_proj", &w1) || !gq_unpack(m, st, p + ".mlp.up_proj", &w1))
                    throw std::runtime_error("loader: " + p + ".mlp: gate_proj / up_proj must both be INT4 group-quantized");
                gq_upload(m, NVL_T_W1, l, w1);
                up2d_proj(m, NVL_T_W2, l, st, p + ".mlp.down_proj");
            } else {                                                           // loadFFN (:513-563): gate | up -> W1
                const StTensor& g = st.need(p + ".mlp.gate_proj.weight");
                const StTensor* u = st.find(p + ".mlp.up_proj.weight");
                if (u && g.dtype == nvl_loader::ST_F8_E4M3) {                 // 8-bit pair: codes and row scales side by side
                    if (u->dtype != g.dtype || u->shape != g.shape || g.shape.size() != 2) throw std::runtime_error("gate_proj / up_proj mismatch");
                    std::vector<uint8_t> cat(g.bytes + u->bytes);
                    memcpy(cat.data(), g.data, g.bytes);
                    memcpy(cat.data() + g.bytes, u->data, u->bytes);
                    std::vector<float> sc = nvl_loader::f8_row_scales(g, p + ".mlp.gate_proj.weight");
                    const std::vector<float> su = nvl_loader::f8_row_scales(*u, p + ".mlp.up_proj.weight");
                    sc.insert(sc.end(), su.begin(), su.end());
                    up2d_f8(m, NVL_T_W1, l, cat.data(), sc, 2 * g.shape[0], g.shape[1], OI);
                } else if (u) {
                    if (u->dtype != g.dtype || u->shape != g.shape || g.shape.size() != 2) throw std::runtime_error("gate_proj / up_proj mismatch");
                    std::vector<uint8_t> cat(g.bytes + u->bytes);              // [2F, H] in the checkpoint's dtype == ([H, F] | [H, F])^T
                    memcpy(cat.data(), g.data, g.bytes);
                    memcpy(cat.data() + g.bytes, u->data, u->bytes);
                    const int rc = nvl_upload_tensor(m, NVL_T_W1, l, cat.data(), g.dtype, 2 * g.shape[0], g.shape[1], OI);
                    if (rc) throw std::runtime_error(nvl_last_error(m));
                } else {
                    up2d(m, NVL_T_W1, l, g, OI);                               // a checkpoint with the pair already fused
                }
                up2d(m, NVL_T_W2, l, st.need(p + ".mlp.down_proj.weight"), OI);
            }
            load_norm(m, st, p + ".input_layernorm.weight", NVL_T_ATTN_NORM_W, NVL_T_ATTN_NORM_B, l);
            load_norm(m, st, p + ".post_attention_layernorm.weight", NVL_T_FFN_NORM_W, NVL_T_FFN_NORM_B, l);
        }
        load_norm(m, st, "model.norm.weight", NVL_T_FINAL_NORM_W, NVL_T_FINAL_NORM_B, 0);
        // LM head (:245-258): own matrix unless tied; a missing one falls back to the transposed embedding
        if (!c.tied_embedding) if (const StTensor* lm = st.find("lm_head.weight")) up2d(m, NVL_T_LM_HEAD, 0, *lm, OI);
    }
    NVL_HIP(hipStreamSynchronize(m->stream));   // the mmaps go away when `st` does
    return NVL_OK;
    NVL_CATCH(m)
}

// LoadModelConfig (generic_loader.go:808-972) on top of the New*Config templates (config.go:125-376)
extern "C" int nvl_load_config_json(const char* path, nvl_model_config* out) {
    if (!path || !out) return NVL_ERR_INVALID;
    try {
        const std::string txt = nvl_loader::read_text(path);
        const JVal raw = nvl_loader::JParser(txt.c_str(), txt.size()).parse();
        if (raw.kind != JVal::OBJ) throw std::runtime_error("config is not a JSON object");
        auto str = [&](const char* k) { const JVal* v = raw.get(k); return v && v->kind == JVal::STR ? v->str : std::string(); };
        auto num = [&](const char* k, double& dst) { const JVal* v = raw.get(k); if (v && v->kind == JVal::NUM) { dst = v->num; return true; } return false; };
        nvl_model_config c;
        memset(&c, 0, sizeof c);
        // ---- templates (config.go:125-376); `architecture` first, then model_type (:822-836, :975-1007), default GPT-2
        std::string arch = str("architecture");
        const std::string mt = str("model_type");
        if (arch != "gpt2" && arch != "falcon" && arch != "llama") {
            if (mt == "gpt2") arch = "gpt2";
            else if (mt == "falcon" || mt == "RefinedWeb" || mt == "RefinedWebModel") arch = "falcon";
            else if (mt == "llama" || mt == "LlamaForCausalLM") arch = "llama";
            else if (mt == "granitemoe") arch = "granitemoe";
            else if (mt == "granitemoehybrid") arch = "granitehybrid";
            else arch = "gpt2";
        }
        c.rope_base = 10000.0; c.norm_eps = 1e-5f;
        if (arch == "gpt2") {            // NewGPT2Config (config.go:125-148)
            c.vocab_size = 50257; c.hidden = 768; c.num_layers = 12; c.num_heads = 12; c.num_kv_heads = 12; c.head_dim = 64; c.ffn_dim = 3072;
            c.max_seq_len = 1024; c.attention_type = NVL_ATTN_MHA; c.norm_type = NVL_NORM_LAYER; c.position_type = NVL_POS_LEARNED;
            c.activation_type = NVL_ACT_GELU; c.block_style = NVL_BLOCK_SEQUENTIAL; c.tied_embedding = 1;
        } else if (arch == "falcon") {   // NewFalconConfig("7b") (config.go:151-194)
            c.vocab_size = 65024; c.hidden = 4544; c.num_layers = 32; c.num_heads = 71; c.num_kv_heads = 1; c.head_dim = 64; c.ffn_dim = 18176;
            c.max_seq_len = 2048; c.attention_type = NVL_ATTN_MQA; c.norm_type = NVL_NORM_LAYER; c.position_type = NVL_POS_ROPE;
            c.activation_type = NVL_ACT_GELU; c.block_style = NVL_BLOCK_PARALLEL; c.tied_embedding = 0;
        } else if (arch == "llama") {    // NewLlamaConfig("7b") (config.go:197-242)
            c.vocab_size = 32000; c.hidden = 4096; c.num_layers = 32; c.num_heads = 32; c.num_kv_heads = 8; c.head_dim = 128; c.ffn_dim = 11008;
            c.max_seq_len = 4096; c.attention_type = NVL_ATTN_GQA; c.norm_type = NVL_NORM_RMS; c.position_type = NVL_POS_ROPE;
            c.activation_type = NVL_ACT_SWIGLU; c.block_style = NVL_BLOCK_SEQUENTIAL; c.tied_embedding = 0; c.norm_eps = 1e-6f;
        } else if (arch == "granitehybrid") {   // NewGraniteConfig (config.go:241-330): "350m" when hidden_size <= 800, else "1b" (:993-1001)
            double hs = 768;
            num("hidden_size", hs);
            const bool small = hs <= 800;
            c.vocab_size = 49152; c.hidden = small ? 768 : 1536; c.num_layers = small ? 32 : 40; c.num_heads = 12; c.num_kv_heads = 4;
            c.head_dim = small ? 64 : 128; c.ffn_dim = small ? 2048 : 4096; c.max_seq_len = small ? 32768 : 128000;
            c.attention_type = NVL_ATTN_GQA; c.norm_type = NVL_NORM_RMS; c.position_type = NVL_POS_NONE; c.activation_type = NVL_ACT_SWIGLU;
            c.block_style = NVL_BLOCK_SEQUENTIAL; c.tied_embedding = 1; c.norm_eps = 1e-5f;
            c.mamba_expand = 2; c.mamba_state_size = 128; c.mamba_conv_kernel = 4; c.mamba_num_heads = 48; c.mamba_head_dim = small ? 32 : 0;
            c.mamba_n_groups = small ? 1 : 8;
            const int nl = c.num_layers;
            for (int i = 0; i < nl; i++) c.mamba_layer_mask[i >> 6] |= 1ull << (i & 63);
            if (small) for (int a : {10, 13, 17, 27}) c.mamba_layer_mask[0] &= ~(1ull << a);      // template pattern, layer_types overrides
        } else {                         // NewGraniteMoEConfig("350m") (config.go:333-376); use_moe comes from num_local_experts
            c.vocab_size = 49155; c.hidden = 1024; c.num_layers = 24; c.num_heads = 16; c.num_kv_heads = 8; c.head_dim = 64; c.ffn_dim = 512;
            c.max_seq_len = 4096; c.attention_type = NVL_ATTN_GQA; c.norm_type = NVL_NORM_RMS; c.position_type = NVL_POS_ROPE;
            c.activation_type = NVL_ACT_SWIGLU; c.block_style = NVL_BLOCK_SEQUENTIAL; c.tied_embedding = 1; c.norm_eps = 1e-6f;
            c.use_moe = 0; c.num_experts = 32; c.num_experts_per_tok = 8;
        }
        // ---- overrides, in the reference's order (:838-968)
        double v;
        if (num("vocab_size", v)) c.vocab_size = (int)v;
        if (num("n_embd", v)) c.hidden = (int)v;
        if (num("hidden_size", v)) c.hidden = (int)v;
        if (num("n_layer", v)) c.num_layers = (int)v;
        if (num("num_hidden_layers", v)) c.num_layers = (int)v;
        if (num("num_layers", v)) c.num_layers = (int)v;
        if (num("n_head", v)) c.num_heads = (int)v;
        if (num("num_attention_heads", v)) c.num_heads = (int)v;
        if (num("num_heads", v)) c.num_heads = (int)v;
        if (num("num_key_value_heads", v)) c.num_kv_heads = (int)v;
        if (num("num_kv_heads", v)) c.num_kv_heads = (int)v;
        if (const JVal* mq = raw.get("multi_query")) if (mq->kind == JVal::BOOL && mq->b) c.num_kv_heads = 1;
        if (num("head_dim", v)) c.head_dim = (int)v;
        if (c.head_dim == 0 && c.hidden > 0 && c.num_heads > 0) c.head_dim = c.hidden / c.num_heads;   // (:884-886)
        if (num("rope_theta", v)) c.rope_base = v;
        if (num("rms_norm_eps", v)) c.norm_eps = (float)v;
        if (num("layer_norm_epsilon", v)) c.norm_eps = (float)v;
        if (num("n_inner", v)) c.ffn_dim = (int)v;
        if (num("intermediate_size", v)) c.ffn_dim = (int)v;
        if (c.ffn_dim == 0 && c.hidden > 0) c.ffn_dim = 4 * c.hidden;
        if (const JVal* t = raw.get("tie_word_embeddings")) if (t->kind == JVal::BOOL) c.tied_embedding = t->b ? 1 : 0;
        if (num("embedding_multiplier", v)) c.embedding_multiplier = (float)v;
        if (num("attention_multiplier", v)) c.attention_multiplier = (float)v;
        if (num("residual_multiplier", v)) c.residual_multiplier = (float)v;
        if (num("logits_scaling", v)) c.logits_scaling = (float)v;
        // Granite hybrid fields (:917-946)
        if (const JVal* lt = raw.get("layer_types")) if (lt->kind == JVal::ARR) {
            c.mamba_layer_mask[0] = c.mamba_layer_mask[1] = 0;
            for (size_t i = 0; i < lt->arr.size() && i < 128; i++)
                if (lt->arr[i].kind == JVal::STR && (lt->arr[i].str == "mamba" || lt->arr[i].str == "mamba2"))
                    c.mamba_layer_mask[i >> 6] |= 1ull << (i & 63);
        }
        if (num("mamba_expand", v)) c.mamba_expand = (int)v;
        if (num("mamba_d_state", v)) c.mamba_state_size = (int)v;
        if (num("mamba_n_heads", v)) c.mamba_num_heads = (int)v;
        if (num("mamba_d_head", v)) c.mamba_head_dim = (int)v;
        if (num("mamba_n_groups", v)) c.mamba_n_groups = (int)v;
        if (num("mamba_d_conv", v)) c.mamba_conv_kernel = (int)v;
        // (the reference sets UseMoE for ANY num_local_experts, 0 included; a hybrid checkpoint says 0 and its blocks
        // run the dense shared MLP: 0 experts is treated as "no MoE" here)
        if (num("num_local_experts", v)) { c.num_experts = (int)v; c.use_moe = v > 0 ? 1 : 0; }
        if (num("num_experts_per_tok", v)) c.num_experts_per_tok = (int)v;
        *out = c;
        return NVL_OK;
    } catch (const std::exception& e) {
        g_create_err = std::string("nvl_load_config_json: ") + e.what();
        return NVL_ERR_INVALID;
    }
}
