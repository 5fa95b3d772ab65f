"""CV_16BF (bfloat16) hand-off tensors without a GPU: the type encoding, validation, refusals, the host rounding helper the GPU
tests compare against, the kernel names, and the v_cvt_pk_bf16_f32 conversion in the built K1 kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rne_bf16(f):
    """fp32 -> bf16 bits, round to nearest even, overflow to +-inf; NaNs stay NaNs (quiet, sign kept)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(f, np.float32))
    return np.where(nan, ((u >> 16).astype(np.uint16) | 0x0040), r).astype(np.uint16)


def widen_bf16(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def special_values():
    """Every class the conversion distinguishes: ties (even and odd), the overflow boundary, fp32 subnormals, values that round
    into bf16 subnormals, +-0, +-inf, NaN."""
    allb = widen_bf16(np.arange(65536, dtype=np.uint16))
    s = np.unique(allb[np.isfinite(allb)])
    mid = ((s[:-1].astype(np.float64) + s[1:].astype(np.float64)) / 2).astype(np.float32)  # ties: exact in fp32
    big = np.float32(3.3895314e38)  # the largest bf16
    extra = np.array([big, np.nextafter(big, np.float32(np.inf)), 3.39e38, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, 0.0, -0.0,
                      1e-45, -1e-45, 1.1754942e-38, 1.1754944e-38, 5e-39, -5e-39, 9.1835e-41, 1e-40, np.nan], np.float32)
    return np.concatenate([s, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), extra]).astype(np.float32)


def _same_bits(a, b):
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    nan_a = ((a & 0x7F80) == 0x7F80) & ((a & 0x7F) != 0)
    nan_b = ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a], b[~nan_b]))


def test_type_encoding():
    assert capi.DEPTH_16BF == 0x1007 and cvgs.CV_16BF == capi.DEPTH_16BF
    for cn in (1, 2, 3, 4):
        t = getattr(cvgs, "CV_16BFC%d" % cn)
        assert t == cvgs.make_type(capi.DEPTH_16F, cn) | 0x1000
        assert capi.type_depth(t) == capi.DEPTH_16F and capi.type_cn(t) == cn and capi.type_is_bf16(t)
        assert cvgs.elem_size(t) == 2 * cn
        assert not capi.type_is_bf16(cvgs.make_type(capi.DEPTH_16F, cn))
    hdr = open(os.path.join(ROOT, "include", "cvgs_hip.h")).read()
    assert "#define CVGS_TYPE_FLAG_BF16 0x1000" in hdr and "CVGS_TYPE_IS_BF16" in hdr
    # convertTo spells the bf16 cast (aux) and computes (alpha, beta) in fp32
    ops = cvgs.convertTo(cvgs.CV_8UC3, cvgs.CV_16BFC3, 1.0 / 255.0, 0.5).ops
    assert ops[0][:2] == (capi.OP_CAST, capi.DEPTH_32F) and ops[-1][:2] == (capi.OP_CAST, capi.DEPTH_16BF)


def test_rne_helper_matches_torch():
    torch = pytest.importorskip("torch")
    vals = special_values()
    rng = np.random.default_rng(H.SEED)
    pats = rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for v in (vals, pats):
        want = torch.from_numpy(v.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert _same_bits(rne_bf16(v), want)
    # every bf16 widens exactly and rounds back to itself
    b = np.arange(65536, dtype=np.uint16)
    assert _same_bits(rne_bf16(widen_bf16(b)), b)


def _chain(read_kind, out_type, ops, src_type=cvgs.CV_8UC3):
    """A lowered chain over fake device pointers (validation never dereferences them)."""
    cn = capi.type_cn(out_type)
    if read_kind == "pixel":
        rd = cvgs.ReadIOp(capi.READ_PIXEL, src_type, [cvgs.GpuMat(20, 30, src_type, 1 << 24, 4096)], 1)
    elif read_kind == "resize":
        rd = cvgs.resize(src_type, cvgs.INTER_LINEAR, [cvgs.GpuMat(20, 30, src_type, 1 << 24, 4096)] * 2, (16, 8), 2)
    elif read_kind == "nv12":
        rd = cvgs.read_nv12([cvgs.GpuMat(20, 30, cvgs.CV_8UC1, 1 << 24, 64)] * 2, (16, 8), capi.YUV_FULL, capi.BT601, False)
    else:
        rd = cvgs.warp(cvgs.WARP_AFFINE, src_type, [cvgs.GpuMat(20, 30, src_type, 1 << 24, 4096)] * 2, [[[1, 0, 0], [0, 1, 0]]] * 2, (16, 8))
    w, h = (30, 20) if read_kind == "pixel" else (16, 8)
    n = 1 if read_kind == "pixel" else 2
    out = cvgs.GpuMat(n, cn * w * h, cvgs.make_type(capi.DEPTH_16F, 1) | (out_type & 0x1000), 1 << 28, cn * w * h * 2)
    return cvgs.lower([rd] + ops + [cvgs.split(out_type, out, (w, h))])


def _validate(lowered):
    lib = capi.load_library()
    rc = lib.cvgs_validate(C.byref(lowered.desc))
    return rc, lib.cvgs_last_error().decode() if rc else ""


@pytest.mark.parametrize("kind", ["pixel", "resize", "nv12", "warp"])
def test_validate_accepts_bf16_chains(kind):
    f, b = cvgs.CV_32FC3, cvgs.CV_16BFC3
    first = [cvgs.convertTo(cvgs.CV_8UC3, f)] if kind == "pixel" else []
    ops = first + [cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.convertTo(f, b)]
    assert _validate(_chain(kind, b, ops)) == (0, "")
    # CAST_TRUNC to bf16, integer sources straight to bf16, and a bf16 source read per pixel / through the resize / through a warp
    assert _validate(_chain("pixel", b, [cvgs.cast(cvgs.CV_8UC3, b)]))[0] == 0
    assert _validate(_chain("pixel", b, [cvgs.convertTo(cvgs.CV_8UC3, b, 1.0 / 255.0)]))[0] == 0
    src_ops = [cvgs.convertTo(b, f)] if kind == "pixel" else []
    if kind != "nv12":
        assert _validate(_chain(kind, f, src_ops, src_type=b))[0] == 0


def test_validate_refuses_arithmetic_and_gray_on_bf16():
    b, f = cvgs.CV_16BFC3, cvgs.CV_32FC3
    for op in (cvgs.multiply(b, [2.0] * 3), cvgs.add(b, [1.0] * 3), cvgs.subtract(b, [1.0] * 3), cvgs.divide(b, [2.0] * 3)):
        rc, msg = _validate(_chain("pixel", b, [op], src_type=b))
        assert rc == capi.ERR_UNSUPPORTED and "bf16" in msg, msg
    gray = cvgs.PointwiseIOp(b, cvgs.CV_16BFC1, [(capi.OP_GRAY, 0 | (1 << 2) | (2 << 4), None)])
    rc, msg = _validate(_chain("pixel", cvgs.CV_16BFC1, [gray], src_type=b))
    assert rc == capi.ERR_UNSUPPORTED and "bf16" in msg, msg
    # a write type that says fp16 where the chain produced bf16 (and the other way round) is refused
    rc, _ = _validate(_chain("pixel", cvgs.CV_16FC3, [cvgs.convertTo(cvgs.CV_8UC3, f), cvgs.PointwiseIOp(f, cvgs.CV_16FC3, [(capi.OP_CAST, capi.DEPTH_16BF, None)])]))
    assert rc == capi.ERR_INVALID
    # the flag means nothing beside another depth: a CAST to "32F | flag" stays a bad destination depth
    rc, msg = _validate(_chain("pixel", f, [cvgs.PointwiseIOp(cvgs.CV_8UC3, f, [(capi.OP_CAST, capi.DEPTH_32F | 0x1000, None)])]))
    assert rc == capi.ERR_INVALID and "CAST" in msg


def test_kernel_name_bf16_twin():
    """The K1 headline chain with a bf16 tensor names the fp16 kernel's bf16 twin (a dry run: no GPU needed)."""
    f = cvgs.CV_32FC3
    names = []
    for h in (cvgs.CV_16FC3, cvgs.CV_16BFC3):
        ops = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
               cvgs.convertTo(f, h)]
        names.append(_name(h, ops))
    assert names[0] == "k1_u8c3_swap_mul_sub_div_f16" and names[1] == "k1_u8c3_swap_mul_sub_div_bf16", names


def _name(h, ops):
    cn = capi.type_cn(h)
    rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [cvgs.GpuMat(200, 300, cvgs.CV_8UC3, 1 << 24, 4096)] * 4, (64, 128), 4)
    out = cvgs.GpuMat(4, cn * 64 * 128, cvgs.make_type(capi.DEPTH_16F, 1) | (h & 0x1000), 1 << 28, cn * 64 * 128 * 2)
    return cvgs.kernel_name(rd, *ops, cvgs.split(h, out, (64, 128)))


def _device_isa(so):
    """The gfx950 disassembly of every code object in a HIP shared library (its .hip_fatbin section holds one offload bundle per
    translation unit)."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fatbin")
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fb, so, os.path.join(d, "copy.so")], check=True)
        data = open(fb, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [i for i in range(0, len(data), 8) if data.startswith(magic, i)]
        isa = []
        for k, a in enumerate(starts):
            part, co = os.path.join(d, "b%d" % k), os.path.join(d, "b%d.co" % k)
            open(part, "wb").write(data[a:starts[k + 1] if k + 1 < len(starts) else len(data)])
            subprocess.run(["/opt/rocm/llvm/bin/clang-offload-bundler", "--type=o", "--input=" + part, "--output=" + co, "--unbundle",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
            isa.append(subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout)
        return "\n".join(isa)


def test_k1_bf16_kernel_uses_packed_conversion():
    """The bf16 K1 tick kernel (the headline program, device tables) converts with v_cvt_pk_bf16_f32: no software rounding sequence."""
    so = os.path.join(ROOT, "cvgpuspeedup_amd", "lib", "libcvgs_hip.so")
    assert os.path.exists(so), "libcvgs_hip.so not built: run build() first"
    isa = _device_isa(so)
    funcs = {}
    name = None
    for line in isa.splitlines():
        if line.endswith(">:") and "<" in line:
            name = line[line.index("<") + 1:-2]
            funcs[name] = []
        elif name:
            funcs[name].append(line)
    # k1_resize_split<3 channels, 0 (segments: the cvgs_execute_many tick with device tables), rows per wave, program, SRC_U8, __bf16 (DF16b), ...>
    tick = [n for n in funcs if "k1_resize_split" in n and "ILi3ELi0E" in n and "DF16b" in n]
    assert tick, "no bf16 K1 tick kernel in the library"
    for n in tick:
        body = "\n".join(funcs[n])
        assert "v_cvt_pk_bf16_f32" in body, n
    # and the fp16 twins stay fp16
    f16 = [n for n in funcs if "k1_resize_split" in n and "ILi3ELi0E" in n and "DF16_" in n]
    assert len(tick) == len(f16) >= 4, (len(tick), len(f16))
    assert f16 and all("v_cvt_pk_bf16_f32" not in "\n".join(funcs[n]) for n in f16)
