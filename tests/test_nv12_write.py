"""CVGS_WRITE_NV12 on the CPU: the contract's literals against their float64 derivation, the fp32 restatement (tests/nv12_write_model.py) against
the float64 model, identity transcoding through the oracle's NV12 read, validation and refusals with their messages, the dry-run kernel
names, the unchanged descriptor sizes and the C++ facade's spellings.  The stored bytes are the GPU suite's (tests/test_zz_gpu_nv12_write.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import nv12_write_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cvgpuspeedup_amd", "include")
LIBDIR = os.path.join(ROOT, "cvgpuspeedup_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = os.path.join(ROOT, "cvgpuspeedup_amd", "csrc", "k_nv12_write.hip")
HEADER = os.path.join(ROOT, "include", "cvgs_hip.h")
NAMES = {M.BT601: "CVGS_BT601", M.BT709: "CVGS_BT709", M.BT2020: "CVGS_BT2020"}


# ---- the literals -----------------------------------------------------------------------------------------------------------------------------
def test_every_literal_lies_within_5e_7_of_its_float64_derivation():
    for prim in (M.BT601, M.BT709, M.BT2020):
        for lit, exact in zip(M.LITERALS[prim], M.derived(prim)):
            assert abs(lit - exact) <= 5e-7, (prim, lit, exact)
            assert abs(float(np.float32(lit)) - exact) <= 5e-7
    assert abs(M.SY - 219.0 / 255.0) <= 5e-7 and abs(M.SC - 224.0 / 255.0) <= 5e-7


def test_the_kernels_and_the_header_hold_the_models_literals():
    src = open(KERNELS).read()
    blocks = re.findall(r"primaries == (CVGS_BT\d+)\) \{([^}]*)\}|else \{ (k\.kr[^}]*)\}", src)
    got = {}
    for name, body, last in blocks:
        vals = [float(v) for v in re.findall(r"= ([0-9.]+)f;", body or last)]
        got[name or "CVGS_BT2020"] = tuple(vals)
    for prim, name in NAMES.items():
        assert got[name] == M.LITERALS[prim], (name, got.get(name))
    assert "kNv12wSy = %sf, kNv12wSc = %sf" % (M.SY, M.SC) in src
    head = open(HEADER).read()
    for prim in NAMES:
        kr, kg, kb, cu, cv = M.LITERALS[prim]
        assert "cu %.6f cv %.6f" % (cu, cv) in head and "%s, %s, %s" % (kr, kg, kb) in head
    assert "sy %.6f  sc %.6f" % (M.SY, M.SC) in head and "CVGS_WRITE_NV12 = 6" in head


# ---- the restatement against the float64 model -------------------------------------------------------------------------------------------------
def test_fp32_restatement_against_the_float64_model():
    """Seeded random float R, G, B in [0, 255], 128 x 128: bytes that differ differ by one code, and at most 0.1 % of them differ."""
    rgb = (np.random.RandomState(5).rand(128, 128, 3) * 255.0).astype(np.float32)
    for rng, prim in M.PAIRS:
        for layout in (M.NV12, M.NV21):
            a, b = M.write_f32(rgb, rng, prim, layout), M.write_f64(rgb, rng, prim, layout)
            d = np.concatenate([np.abs(a[i].astype(np.int32) - b[i].astype(np.int32)).ravel() for i in (0, 1)])
            share = float((d != 0).mean())
            print("range %d primaries %d layout %d: largest difference %d, share of differing bytes %.5f %%" % (rng, prim, layout, d.max(), 100 * share))
            assert d.max() <= 1 and share <= 0.001, (rng, prim, layout, d.max(), share)


def test_the_layout_only_swaps_the_chroma_bytes_and_grey_is_centred():
    rgb = (np.random.RandomState(6).rand(8, 16, 3) * 255.0).astype(np.float32)
    l0, c0 = M.write_f32(rgb, M.LIMITED, M.BT601, M.NV12)
    l1, c1 = M.write_f32(rgb, M.LIMITED, M.BT601, M.NV21)
    assert (l0 == l1).all() and (c0[:, 0::2] == c1[:, 1::2]).all() and (c0[:, 1::2] == c1[:, 0::2]).all()
    grey = np.full((4, 4, 3), 255.0, np.float32)
    for rng, prim in M.PAIRS:
        l, c = M.write_f32(grey, rng, prim)
        assert (l == (235 if rng == M.LIMITED else 255)).all() and (c == 128).all()
    l, c = M.write_f32(np.array([[[np.nan, 1e9, -1e9]] * 2] * 2, np.float32), M.FULL, M.BT709)
    assert (l == 0).all()  # NaN -> 0


# ---- identity transcoding ------------------------------------------------------------------------------------------------------------------------
def oracle_rgb(oracle, surface, w, h, rng, prim, layout=capi.YUV_NV12):
    """The float R, G, B picture the oracle's full-resolution NV12 read makes of a surface [3h/2, w]."""
    mat = cvgs.GpuMat(h, w, cvgs.CV_8UC1, surface.ctypes.data, surface.strides[0], owner=surface)
    ref = np.zeros((1, h * w * 3), np.float32)
    oracle.execute(cvgs.lower([cvgs.read_nv12(mat, None, rng, prim, alpha=False, layout=layout),
                               cvgs.write(cvgs.CV_32FC3, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (w, h))]))
    return ref.reshape(h, w, 3)


@pytest.mark.parametrize("rng,prim", M.PAIRS)
def test_identity_transcoding_returns_the_surface_byte_for_byte(oracle, rng, prim):
    """read_nv12 at full resolution (the oracle's), written back with the same range and primaries: the source surface, every code 0..255
    in luma and chroma."""
    w, h = 64, 32
    s = M.random_surface(w, h, 11)
    assert len(np.unique(s[:h])) == 256 and len(np.unique(s[h:])) == 256
    for layout in (M.NV12, M.NV21):
        luma, chroma = M.write_f32(oracle_rgb(oracle, s, w, h, rng, prim, layout), rng, prim, layout)
        assert (luma == s[:h]).all() and (chroma == s[h:]).all(), (rng, prim, layout)


# ---- validation and refusals -------------------------------------------------------------------------------------------------------------------
def _surface(w=16, h=8, step=None):
    step = step or w
    buf = np.zeros((h * 3 // 2, step), np.uint8)
    return cvgs.GpuMat(h, w, cvgs.CV_8UC1, buf.ctypes.data, step, owner=buf)


def _source(w=16, h=8, cv_type=None):
    cv_type = cvgs.CV_8UC3 if cv_type is None else cv_type
    a = np.zeros((h, w * cvgs.elem_size(cv_type)), np.uint8)
    return cvgs.GpuMat(h, w, cv_type, a.ctypes.data, a.strides[0], owner=a)


def _chain(read=None, mid=(), out=None, **kw):
    read = read or cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [_source()], (16, 8))
    return cvgs.lower([read] + list(mid) + [out or cvgs.write_nv12(_surface(), **kw)])


def _status(lib, low):
    rc = lib.cvgs_validate(C.byref(low.desc))
    return rc, lib.cvgs_last_error().decode()


def test_a_valid_chain_validates_and_the_python_builder_checks_its_arguments(lib):
    assert capi.WRITE_NV12 == 6
    low = _chain(color_range=capi.YUV_LIMITED, primaries=capi.BT2020, layout=capi.YUV_NV21)
    assert low.desc.write.kind == 6 and low.desc.write.yuv_params == (1 | (2 << 4) | (1 << 8)) and low.desc.write.dst_type == cvgs.CV_32FC3
    assert _status(lib, low)[0] == capi.OK
    with pytest.raises(ValueError):
        cvgs.write_nv12(_surface(15, 8, 16))
    with pytest.raises(ValueError):
        cvgs.write_nv12(_surface(16, 6).roi(0, 0, 16, 5))
    with pytest.raises(ValueError):
        cvgs.write_nv12(_surface(), layout=capi.YUV_I420)
    with pytest.raises(ValueError):
        cvgs.write_nv12(_source())


def test_malformed_descriptors_are_invalid_each_with_its_message(lib):
    def bad(low, msg, code=capi.ERR_INVALID):
        rc, err = _status(lib, low)
        assert rc == code and msg in err, (rc, err)

    # the value: CV_32FC3 only
    # (the Python builder checks the type chain itself: the stage is added to the descriptor by hand)
    low = _chain()
    low.desc.ops[0].opcode, low.desc.ops[0].aux, low.desc.n_ops = capi.OP_CAST, capi.DEPTH_8U, 1
    low.desc.write.dst_type = cvgs.CV_8UC3
    bad(low, "CV_32FC3")
    low = _chain()
    low.desc.ops[0].opcode, low.desc.ops[0].aux, low.desc.n_ops = capi.OP_ADD_ALPHA, 0 | (1 << 2) | (2 << 4), 1
    low.desc.write.dst_type = cvgs.CV_32FC4
    bad(low, "CV_32FC3")
    low = _chain()
    low.desc.write.dst_type = cvgs.CV_8UC3
    bad(low, "write type does not match")
    # the colour parameters
    for params in (2, 3 << 4, 2 << 8, 7 << 8, 1 << 12, -1):
        low = _chain()
        low.desc.write.yuv_params = params
        bad(low, "yuv_params" if params in (2, 3 << 4, 1 << 12, -1) else "CVGS_YUV_NV12 or CVGS_YUV_NV21")
    # the target
    low = _chain()
    low.desc.write.planes2d = None
    bad(low, "planes2d is null")
    for field, value, msg in (("width", 14, "wrong size"), ("height", 6, "wrong size"), ("step", 15, "wrong size"), ("data", None, "missing"),
                              ("uv_offset", -2, "uv_offset")):
        low = _chain()
        arr = (capi.Image2D * 1).from_address(low.desc.write.planes2d)
        setattr(arr[0], field, value)
        bad(low, msg)
    # odd sizes, as the NV12 read says
    odd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [_source()], (15, 8))
    low = cvgs.lower([odd, cvgs.write_nv12(_surface(16, 8))])
    arr = (capi.Image2D * 1).from_address(low.desc.write.planes2d)
    arr[0].width = 15
    bad(low, "even dimensions")
    # the range of write kinds ends behind this one
    low = _chain()
    low.desc.write.kind = 7
    bad(low, "bad write kind")


def test_every_other_write_kind_goes_on_ignoring_the_field(lib):
    out = np.zeros((1, 3 * 16 * 8), np.float32)
    low = cvgs.lower([cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [_source()], (16, 8)), cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), (16, 8))])
    name = C.create_string_buffer(128)
    assert lib.cvgs_kernel_name(C.byref(low.desc), name, 128) == 0
    low.desc.write.yuv_params = 0x7fffffff
    other = C.create_string_buffer(128)
    assert lib.cvgs_validate(C.byref(low.desc)) == 0 and lib.cvgs_kernel_name(C.byref(low.desc), other, 128) == 0 and other.value == name.value


def test_what_has_no_kernel_is_refused_as_unsupported_with_its_reason(lib):
    def refused(low, msg):
        rc, err = _status(lib, low)
        assert rc == capi.ERR_UNSUPPORTED and msg in err, (rc, err)
        assert lib.cvgs_execute(C.byref(low.desc), None) == capi.ERR_UNSUPPORTED  # refused before anything is enqueued

    f3, d3 = cvgs.CV_32FC3, cvgs.make_type(capi.DEPTH_64F, 3)
    refused(_chain(mid=[cvgs.convertTo(f3, d3), cvgs.convertTo(d3, f3)]), "CV_64F")
    refused(_chain(read=cvgs.resize(cvgs.make_type(capi.DEPTH_64F, 3), cvgs.INTER_LINEAR, [_source(cv_type=cvgs.make_type(capi.DEPTH_64F, 3))], (16, 8))), "CV_64F")
    refused(_chain(out=cvgs.write_nv12(_surface()).mirrored_to([4096])), "mirrors")
    refused(_chain(read=cvgs.warp(cvgs.WARP_AFFINE, cvgs.CV_8UC3, [_source()], [[[1, 0, 0], [0, 1, 0]]], (16, 8))), "warp reads")
    refused(_chain(read=cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [_source()], (16, 8))), "INTER_AREA")


def test_the_queue_and_the_circular_tensor_refuse_the_kind_before_they_look_at_a_handle(lib):
    low = _chain()
    ptrs = cvgs.Queue.chain_pointers([low, low])
    t = C.c_uint64()
    calls = (lambda: lib.cvgs_queue_submit(None, C.byref(low.desc), C.byref(t)),
             lambda: lib.cvgs_queue_submit_many(None, ptrs, 2, C.byref(t)),
             lambda: lib.cvgs_queue_submit_on(None, C.byref(low.desc), None, 0, C.byref(t)),
             lambda: lib.cvgs_queue_submit_many_on(None, ptrs, 2, None, 0, C.byref(t)))
    for call in calls:
        assert call() == capi.ERR_UNSUPPORTED
        assert "queue: NV12 / NV21 surface writes (CVGS_WRITE_NV12) are served by cvgs_execute / cvgs_execute_many only" in lib.cvgs_last_error().decode()
    assert lib.cvgs_circular_update(None, C.byref(low.desc), None) == capi.ERR_UNSUPPORTED
    assert "CircularTensor::update: NV12 / NV21 surface writes" in lib.cvgs_last_error().decode()


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------------------
def test_dry_run_kernel_names(lib):
    surf = np.zeros((96, 96), np.uint8)
    src = cvgs.GpuMat(64, 96, cvgs.CV_8UC1, surf.ctypes.data, 96, owner=surf)
    out = cvgs.write_nv12(_surface(34, 14, 58), capi.YUV_LIMITED, capi.BT709)
    for layout in (capi.YUV_NV12, capi.YUV_NV21):
        rd = cvgs.read_nv12(src, (34, 14), capi.YUV_LIMITED, capi.BT601, alpha=False, layout=layout)
        assert cvgs.kernel_name(rd, out) == "nv12w_nv12_resize"
        assert cvgs.kernel_name(rd, out, flags=capi.CHAIN_FORCE_GENERIC) == "nv12w_interp"
    f3 = cvgs.CV_32FC3
    # a program, an alpha channel, another layout, another read: the interpreted kernel
    rd = cvgs.read_nv12(src, (34, 14), alpha=False)
    assert cvgs.kernel_name(rd, cvgs.multiply(f3, [0.5] * 3), out) == "nv12w_interp"
    rd4 = cvgs.read_nv12(src, (34, 14), alpha=True)
    assert cvgs.kernel_name(rd4, cvgs.cvtColor(cvgs.COLOR_RGBA2RGB, cvgs.CV_32FC4, f3), out) == "nv12w_interp"
    planar = np.zeros((96, 96), np.uint8)
    i420 = cvgs.GpuMat(64, 96, cvgs.CV_8UC1, planar.ctypes.data, 96, owner=planar)
    assert cvgs.kernel_name(cvgs.read_nv12(i420, (34, 14), alpha=False, layout=capi.YUV_I420), out) == "nv12w_interp"
    assert cvgs.kernel_name(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [_source()], (34, 14)), out) == "nv12w_interp"
    same = cvgs.write_nv12(_surface(96, 64))
    assert cvgs.kernel_name(cvgs.read_nv12(src, None, alpha=False), same) == "nv12w_interp"
    px = cvgs.ReadIOp(capi.READ_PIXEL, cvgs.CV_8UC3, [_source(96, 64)], 1)
    assert cvgs.kernel_name(px, cvgs.convertTo(cvgs.CV_8UC3, f3), same) == "nv12w_interp"


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_descriptors_keep_their_size_and_the_field_its_place(lib):
    assert lib.cvgs_abi_version() == 6
    assert C.sizeof(capi.WriteDesc) == 56 and capi.WriteDesc.yuv_params.offset == 52 and capi.WriteDesc.yuv_params.size == 4
    assert C.sizeof(capi.ChainDesc) == 848 and C.sizeof(capi.ReadDesc) == 104
    low = _chain()
    assert low.desc.struct_size == 848 and _status(lib, low)[0] == capi.OK  # the library checks struct_size against ITS sizeof
    low.desc.struct_size = 852
    assert _status(lib, low)[0] == capi.ERR_INVALID


# ---- the C++ facade -----------------------------------------------------------------------------------------------------------------------------
LOWERING = r"""
#include <cvGPUSpeedup.h>
#include <cstddef>
#include <cstdio>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, cvgs_last_error()); return 1; } } while (0)
static_assert(sizeof(cvgs_chain_desc) == 848 && sizeof(cvgs_write_desc) == 56 && offsetof(cvgs_write_desc, yuv_params) == 52, "ABI 6 keeps its layout");
static_assert(CVGS_WRITE_NV12 == 6 && CVGS_WRITE_YUV_PARAMS(CVGS_YUV_LIMITED, CVGS_BT2020, CVGS_YUV_NV21) == 0x121, "the kind and its parameter word");
int main() {
    static unsigned char in[96 * 96], out[4][21 * 34];
    cv::cuda::GpuMat src(96, 96, CV_8UC1, in, 96), dst(21, 34, CV_8UC1, out[0], 34);
    const cv::Size d(34, 14);
    char name[64];
    fk::ChainBuilder a, b, c;
    fk::lowerChain(a, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12, fk::Limited, fk::bt601>(src), d), cvGS::writeNV12<fk::Limited, fk::bt709>(dst));
    CHECK(a.d.write.kind == CVGS_WRITE_NV12 && a.d.write.dst_type == CV_32FC3 && a.d.write.yuv_params == CVGS_WRITE_YUV_PARAMS(1, 1, 0) && a.d.n_ops == 0);
    CHECK(a.d.write.planes2d[0].height == 14 && a.d.write.planes2d[0].width == 34 && a.d.write.planes2d[0].uv_offset == 0);
    CHECK(cvgs_validate(&a.d) == CVGS_OK);
    CHECK(cvgs_kernel_name(&a.d, name, sizeof(name)) == CVGS_OK && std::string(name) == "nv12w_nv12_resize");
    // a BGR chain reorders in front of the write; NV21; the default parameters are full range, BT.709
    fk::lowerChain(b, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<cv::COLOR_YUV2BGR_NV12>(src), d), cvGS::cvtColor<cv::COLOR_BGR2RGB, CV_32FC3>(), cvGS::writeNV21(dst));
    CHECK(b.d.write.yuv_params == CVGS_WRITE_YUV_PARAMS(0, 1, 1) && cvgs_validate(&b.d) == CVGS_OK);
    CHECK(cvgs_kernel_name(&b.d, name, sizeof(name)) == CVGS_OK && std::string(name) == "nv12w_interp");
    // a batch of crops of a packed frame, one surface each
    static unsigned char frame[61 * 97 * 3];
    cv::cuda::GpuMat f(61, 97, CV_8UC3, frame, 97 * 3);
    std::array<cv::cuda::GpuMat, 4> crops, outs;
    for (int i = 0; i < 4; ++i) { crops[i] = f(cv::Rect(i, i, 40 + i, 30)); outs[i] = cv::cuda::GpuMat(21, 34, CV_8UC1, out[i], 34); }
    fk::lowerChain(c, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 4>(crops, d, 4), cvGS::cvtColor<cv::COLOR_BGR2RGB, CV_32FC3>(), cvGS::writeNV12<fk::Full, fk::bt601>(outs));
    CHECK(c.d.read.batch == 4 && c.d.write.planes == 4 && c.d.write.planes2d[3].data == out[3] && cvgs_validate(&c.d) == CVGS_OK);
    std::printf("ok\n");
    return 0;
}
"""


def test_facade_spellings_lower_to_write_kind_6(tmp_path):
    src = tmp_path / "nv12_write_lowering.cpp"
    src.write_text(LOWERING)
    exe = tmp_path / "nv12_write_lowering"
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-command-line-argument", "-Wno-unused-variable", "-I" + INC,
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src), "-o", str(exe), "-L" + LIBDIR, "-lcvgs_hip", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_facade_refuses_any_other_value_type_at_compile_time(tmp_path):
    head = ('#include <cvGPUSpeedup.h>\nint main() { cv::cuda::GpuMat m, s; std::array<cv::cuda::GpuMat, 2> crops; fk::ChainBuilder b; %s return 0; }\n')
    bad = {
        "u8c3": "fk::lowerChain(b, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 2>(crops, cv::Size(8, 8), 2), cvGS::convertTo<CV_32FC3, CV_8UC3>(), cvGS::writeNV12(s));",
        "rgba": "fk::lowerChain(b, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGBA_NV12>(m), cv::Size(8, 8)), cvGS::writeNV21(s));",
    }
    good = "fk::lowerChain(b, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 2>(crops, cv::Size(8, 8), 2), cvGS::writeNV12(s));"
    for name, body in list(bad.items()) + [("float3", good)]:
        src = tmp_path / (name + ".cpp")
        src.write_text(head % body)
        r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I" + INC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src)],
                           capture_output=True, text=True)
        if name == "float3":
            assert r.returncode == 0, r.stderr[-2000:]
            continue
        assert r.returncode != 0, "%s compiled but must not" % name
        assert ("static assertion failed" in r.stderr or "static_assert" in r.stderr) and "take a float3 value (CV_32FC3" in r.stderr, r.stderr[-800:]
