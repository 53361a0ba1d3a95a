"""INT4 group-quantized projection weights (AWQ / GPTQ W4A16), the parts that need no GPU: the ABI additions
and their Python mirrors, the option's ValueErrors, the register budgets of the INT4-weight decode kernels (hipcc
cross-compiles them here), and the checkpoint unpackers of csrc/int4_unpack.h in a stand-alone driver under the sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
HEADER = os.path.join(ROOT, "include", "nvllm.h")
NEW = ("nvl_set_gq_weight_dtype", "nvl_upload_tensor_int4", "nvl_op_matmul_int4w")
AWQ_ORDER = [0, 2, 4, 6, 1, 3, 5, 7]


def test_abi_additions(pkg):
    L = pkg._lib
    assert all(n in pkg.declared_symbols() for n in NEW)
    assert all(hasattr(L.lib(), n) for n in NEW)
    assert L.lib().nvl_abi_version() == 3


def test_python_mirrors_match_the_header(pkg):
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(NVL_GQ_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert enum == {"NVL_GQ_NONE": 0, "NVL_GQ_UINT4": 1}
    assert pkg._lib.GQ_WEIGHT_DTYPE == {"none": enum["NVL_GQ_NONE"], "uint4": enum["NVL_GQ_UINT4"]}
    assert len(pkg._lib.lib().nvl_set_gq_weight_dtype.argtypes) == 3
    assert len(pkg._lib.lib().nvl_upload_tensor_int4.argtypes) == 9
    assert len(pkg._lib.lib().nvl_op_matmul_int4w.argtypes) == 11
    assert re.search(r"int nvl_set_gq_weight_dtype\(nvl_model\* m, int dtype, int group_size\);", text)
    assert re.search(r"int nvl_upload_tensor_int4\(nvl_model\* m, int kind, int layer, const uint8_t\* codes, const uint16_t\* scales,"
                     r"\s+const uint8_t\* zeros,\s+int64_t rows, int64_t cols, int layout\);", text)
    assert re.search(r"int nvl_op_matmul_int4w\(int device, const float\* a, const float\* w, int M, int N, int K, int group_size,"
                     r"\s+float\* c,\s+uint8_t\* codes_out, uint16_t\* scales_out, uint8_t\* zeros_out\);", text)


def test_the_pinned_enums_and_mirrors_are_unchanged(pkg):
    text = open(HEADER).read()
    find = lambda prefix: dict((k, int(v)) for k, v in re.findall(r"\b(" + prefix + r"[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert find("NVL_W_") == {"NVL_W_AUTO": 0, "NVL_W_FP8_E4M3": 1}
    assert find("NVL_MX_") == {"NVL_MX_NONE": 0, "NVL_MX_FP4_E2M1": 1}
    assert find("NVL_MXE_") == {"NVL_MXE_NONE": 0, "NVL_MXE_FP4_E2M1": 1}
    assert find("NVL_MXH_") == {"NVL_MXH_NONE": 0, "NVL_MXH_FP4_E2M1": 1}
    assert find("NVL_EXPERT_") == {"NVL_EXPERT_AUTO": 0, "NVL_EXPERT_FP8_E4M3": 1}
    assert pkg._lib.WEIGHT_DTYPE == {"auto": 0, "fp8_e4m3": 1}
    assert pkg._lib.MX_WEIGHT_DTYPE == {"none": 0, "fp4_e2m1": 1}
    assert len(pkg._lib.SLOTS) == 33
    assert [pkg._lib.lib().nvl_sizeof(i) for i in range(4)] == [144, 40, 128, 16]


def test_null_model_is_refused(pkg):
    L = pkg._lib.lib()
    assert L.nvl_set_gq_weight_dtype(None, 1, 128) == -1
    assert L.nvl_upload_tensor_int4(None, 0, 0, None, None, None, 1, 128, 1) == -1
    assert L.nvl_set_weight_dtype(None, 7) == -1


def test_option_value_errors(pkg):
    """raised before the library is asked for a device"""
    cfg = pkg.synth.tiny_config("llama")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_weight_dtype="int4")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_weight_dtype="uint4", gq_group_size=48)
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_weight_dtype="uint4", weight_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        pkg.HipTransformerModel(cfg, None, gq_weight_dtype="uint4", mx_weight_dtype="fp4_e2m1")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_int4_decode_kernels_build_for_gfx950(tmp_path):
    """the INT4-weight decode kernels (narrow and wide, MT 1 / 2 / 4, the 64-row groups, HALF, every epilogue) cross-compile
    and are held to the MXFP4 forms' budgets (<= 12 spilled registers, <= 512 VGPRs)"""
    s = tmp_path / "nvllm.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=6",
                           "-Wno-unused-function", "-Wno-unused-variable", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "nano-vllm-go_amd", "csrc", "nvllm.hip"), "-o", str(s)],
                          stderr=subprocess.DEVNULL, timeout=900)
    meta = s.read_text()
    kern = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name: *(\S+)", blk).group(1)
        kern[name] = (int(re.search(r"\.vgpr_count: *(\d+)", blk).group(1)),
                      int(re.search(r"\.vgpr_spill_count: *(\d+)", blk).group(1)))
    gq = {k: v for k, v in kern.items() if "gemm_skinny_int4w_kernel" in k or "gemm_skinny_wide_int4w_kernel" in k}
    mx = [k for k in kern if "gemm_skinny_mxfp4w_kernel" in k or "gemm_skinny_wide_mxfp4w_kernel" in k]
    for mt in (1, 2, 4):
        assert [k for k in gq if re.search(r"gemm_skinny_int4w_kernelILi%dE" % mt, k)], mt
        assert [k for k in gq if re.search(r"gemm_skinny_wide_int4w_kernelILi%dE" % mt, k)], mt
    # every form the MXFP4 base set has: the same template arguments under the other kernel name, but for U (the third: the
    # k-steps per register set, which the INT4 64-row-group kernels halve to stay inside the register budget)
    strip = lambda k, a, b: re.sub(r"(kernelILi\d+ELi\d+E)Li\d+E", r"\1", re.sub(r"^_ZN3nvl\d+", "", k).replace(a, b).rsplit("EEvNS_8GemmArgs", 1)[0])
    have = {strip(k, "int4w", "Xw") for k in gq}
    missing = [k for k in mx if strip(k, "mxfp4w", "Xw") not in have]
    assert not missing, missing
    assert [k for k in gq if re.search(r"gemm_skinny_int4w_kernelILi4E\w+Lb1ELb0EEE", k)]       # PASSES (64-row groups)
    assert [k for k in gq if re.search(r"gemm_skinny_int4w_kernelILi1E\w+Lb0ELb1EEE", k)]       # HALF
    bad = {k: v for k, v in gq.items() if v[1] > 12 or v[0] > 512}
    assert not bad, bad
    assert "w4g_quant_rows_kernel" in meta and "w4g_place_kernel" in meta and "w4g_dequant_kernel" in meta


# ---- the checkpoint unpackers, stand-alone under the sanitizers ----
def pack_awq(q, z, s):
    """q [N][K] codes, z [N][K/g], s [N][K/g] float16 -> (qweight I32 [K, N/8], qzeros I32 [K/g, N/8], scales F16 [K/g, N])"""
    def pack_cols(m):                                       # m [rows][N] -> [rows][N/8], nibble i = column 8j + AWQ_ORDER[i]
        rows, n = m.shape
        out = np.zeros((rows, n // 8), np.uint32)
        for i, o in enumerate(AWQ_ORDER):
            out |= m[:, o::8].astype(np.uint32) << np.uint32(4 * i)
        return out
    return pack_cols(q.T), pack_cols(z.T), np.ascontiguousarray(s.T)


def pack_gptq(q, z, s):
    """-> (qweight I32 [K/8, N], qzeros I32 [K/g, N/8] holding z - 1, scales F16 [K/g, N])"""
    n, k = q.shape
    qw = np.zeros((k // 8, n), np.uint32)
    for i in range(8):
        qw |= q.T[i::8, :].astype(np.uint32) << np.uint32(4 * i)
    zt = (z.T.astype(np.int64) - 1)
    assert (zt >= 0).all()
    qz = np.zeros((zt.shape[0], n // 8), np.uint32)
    for i in range(8):
        qz |= zt[:, i::8].astype(np.uint32) << np.uint32(4 * i)
    return qw, qz, np.ascontiguousarray(s.T)


def case_text(layout, qw, qz, sc, g_idx=None):
    parts = [str(layout), *map(str, qw.shape), *map(str, qz.shape), *map(str, sc.shape), str(0 if g_idx is None else len(g_idx))]
    parts += [" ".join(map(str, qw.ravel().tolist())), " ".join(map(str, qz.ravel().tolist())),
              " ".join(map(str, sc.view(np.uint16).ravel().tolist()))]
    if g_idx is not None:
        parts.append(" ".join(map(str, np.asarray(g_idx).tolist())))
    return "\n".join(parts)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("int4_unpack") / "int4_unpack_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "int4_unpack_driver.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        r = subprocess.run([str(exe)], input="\n".join(cases) + "\n0\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def random_canon(rng, n, k, g, zmin=0):
    q = rng.integers(0, 16, (n, k)).astype(np.uint8)
    z = rng.integers(zmin, 16, (n, k // g)).astype(np.uint8)
    s = rng.uniform(1e-3, 0.1, (n, k // g)).astype(np.float16)
    return q, z, s


@pytest.mark.parametrize("g", [32, 64, 128])
def test_unpackers_return_the_canonical_arrays(driver, g):
    rng = np.random.default_rng(g)
    n, k = 24, 2 * g
    cases, want = [], []
    for layout in (1, 2):
        q, z, s = random_canon(rng, n, k, g, zmin=1 if layout == 2 else 0)
        qw, qz, sc = (pack_awq if layout == 1 else pack_gptq)(q, z, s)
        cases.append(case_text(layout, qw, qz, sc, None if layout == 1 else np.arange(k) // g))
        want.append((layout, q, z, s))
    out = driver(cases)
    assert len(out) == 8
    for i, (layout, q, z, s) in enumerate(want):
        assert out[4 * i] == f"OK {layout} {k} {n} {g}"
        codes = np.array(out[4 * i + 1].split(), np.int64)
        assert np.array_equal(codes, (q[:, 0::2] | (q[:, 1::2] << 4)).ravel())
        assert np.array_equal(np.array(out[4 * i + 2].split(), np.int64), s.view(np.uint16).ravel())
        assert np.array_equal(np.array(out[4 * i + 3].split(), np.int64), z.ravel())


def test_unpackers_refuse(driver):
    rng = np.random.default_rng(5)
    n, k, g = 16, 128, 64
    q, z, s = random_canon(rng, n, k, g, zmin=1)
    qw, qz, sc = pack_gptq(q, z, s)
    zero15 = qz.copy()
    zero15[1, 0] |= np.uint32(15 << 8)                      # a stored zero of 15: z = 16
    act = np.arange(k) // g
    act[[3, 70]] = act[[70, 3]]                             # act-order: g_idx is not k / g
    aw, az, asc = pack_awq(q, z, s)
    out = driver([case_text(2, qw, zero15, sc), case_text(2, qw, qz, sc, act),
                  case_text(2, qw, qz[:, :1], sc),          # qzeros not [K/g, N/8]: not 4-bit
                  case_text(1, aw[:96], az, asc),           # K / groups = 48: no supported group size
                  case_text(2, qw, qz, sc)])
    assert out[0].startswith("REFUSED") and "zero point of 15" in out[0]
    assert out[1].startswith("REFUSED") and "act-order" in out[1]
    assert out[2].startswith("REFUSED") and "4-bit" in out[2]
    assert out[3].startswith("REFUSED") and "group size" in out[3]
    assert out[4] == f"OK 2 {k} {n} {g}"
