"""INTER_AREA (CVGS_READ_RESIZE_AREA) without a GPU: the builders and what validates, the plane table and its hull, the properties of the
arithmetic contract on the numpy restatement (tests/area_model.py), the restatement against the float64 model, and the C++ facade's spelling.

fp32 restatement against the float64 model over the GPU test's case list (every source type x both targets x every crop, plus the
96 -> 1 column case): the largest deviation, relative to the largest source magnitude of the case, was 1.85e-06 (16SC4, the 90 x 6 crop
into 33 x 7: its y axis does not shrink, so it takes the bilinear taps, whose position s = ty * fy is rounded to fp32 -- half an ulp of a
position near 5 is 2.4e-07 -- and moves weight between two rows that differ by up to twice the largest magnitude; the shrinking cases
stay below 3e-07);
test_fp32_restatement_against_the_float64_model holds it under 4 x that value.  The margin is for other seeds' weights, not for kernel
error: the kernels are held to the restatement bit for bit (tests/test_gpu_area.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cvgpuspeedup_amd", "include")
LIBDIR = os.path.join(ROOT, "cvgpuspeedup_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"
RECORDED_F32_VS_F64 = 1.85e-06
F32 = np.float32


def _frame(depth=capi.DEPTH_8U, cn=3):
    host = M.make_source(depth, cn)
    return host, cvgs.GpuMat.from_array(host, cvgs.make_type(depth, cn))


def _k1_like(rd, cn, out, dsize, extra=False, half=None):
    f = cvgs.make_type(capi.DEPTH_32F, cn)
    ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f), cvgs.multiply(f, [0.3] * cn),
           cvgs.subtract(f, [40.0] * cn), cvgs.divide(f, [57.0] * cn)]
    if extra:
        ops.append(cvgs.add(f, [1.0] * cn))
    t = f
    if half is not None:
        t = cvgs.make_type(capi.DEPTH_16F, cn) | (capi.TYPE_FLAG_BF16 if half == "bf16" else 0)
        ops.append(cvgs.convertTo(f, t))
    return ops + [cvgs.split(t, out, dsize)]


def _out(batch, cn, dsize, scalar=None):
    scalar = cvgs.CV_32FC1 if scalar is None else scalar
    a = np.zeros((batch, cn * dsize[0] * dsize[1]), np.float32)
    return cvgs.GpuMat(batch, cn * dsize[0] * dsize[1], scalar, a.ctypes.data, a.strides[0], owner=a)


# ---- builders and validation ---------------------------------------------------------------------------------------------------------------
def test_resize_inter_area_lowers_to_kind_6_and_validates(lib):
    assert cvgs.INTER_AREA == 3 and capi.READ_RESIZE_AREA == 6 and cvgs.INTER_AREA in cvgs.SUPPORTED_INTERPOLATIONS
    assert lib.cvgs_abi_version() == 6
    host, g = _frame()
    crops = [g.roi(*c) for c in M.CROPS[:5]]
    batched = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, crops, (16, 8), 4, [1.0, 2.0, 3.0])
    single = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, g, (16, 8))
    for rd, batch in ((batched, 5), (single, 1)):
        assert rd.kind == capi.READ_RESIZE_AREA and rd.out_type() == cvgs.CV_32FC3
        low = cvgs.lower([rd, cvgs.split(cvgs.CV_32FC3, _out(batch, 3, (16, 8)), (16, 8))])
        assert low.desc.read.kind == 6 and low.desc.read.batch == batch
        assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    # the bilinear spelling is what it was
    assert cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, crops, (16, 8)).kind == capi.READ_RESIZE_LINEAR
    with pytest.raises(ValueError):
        cvgs.resize(cvgs.CV_8UC3, 0, crops, (16, 8))  # INTER_NEAREST
    with pytest.raises(ValueError):
        cvgs.resize(cvgs.CV_8UC3, 2, crops, (16, 8))  # INTER_CUBIC


def test_resize_boxes_takes_an_interpolation(lib):
    host, g = _frame()
    assert cvgs.resize_boxes(g, 4096, 4, (16, 8)).kind == capi.READ_RESIZE_LINEAR
    rd = cvgs.resize_boxes(g, 4096, 4, (16, 8), interp=cvgs.INTER_AREA)
    assert rd.kind == capi.READ_RESIZE_AREA and rd.table_hull == (host.ctypes.data, host.ctypes.data + host.nbytes)
    low = cvgs.lower(_k1_like(rd, 3, _out(4, 3, (16, 8)), (16, 8)))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    assert cvgs.kernel_name(*_k1_like(rd, 3, _out(4, 3, (16, 8)), (16, 8))) == "area_u8c3_swap_mul_sub_div"
    with pytest.raises(ValueError):
        cvgs.resize_boxes(g, 4096, 4, (16, 8), interp=0)
    with pytest.raises(ValueError):
        cvgs.resize_boxes(g, 4096, 4, (16, 8), yuv=(capi.YUV_FULL, capi.BT709, 0), interp=cvgs.INTER_AREA)


def test_a_dry_run_never_names_a_bilinear_kernel(lib):
    dsize = (16, 8)
    for depth, cn, want in ((capi.DEPTH_8U, 3, "area_u8c3_swap_mul_sub_div"), (capi.DEPTH_8U, 4, "area_u8c4_swap_mul_sub_div")):
        host, g = _frame(depth, cn)
        for n in (1, 14, 70, 300):  # inline, inline, staged table, beyond K1's large argument block
            crops = [g.roi(*M.CROPS[i % len(M.CROPS)]) for i in range(n)]
            rd = cvgs.resize(cvgs.make_type(depth, cn), cvgs.INTER_AREA, crops, dsize)
            assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize)) == want
            assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize), flags=capi.CHAIN_FORCE_GENERIC) == "area_interp"
            assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize), flags=capi.CHAIN_NO_THREAD_FUSION) == want
        rd = cvgs.resize(cvgs.make_type(depth, cn), cvgs.INTER_AREA, [g.roi(*c) for c in M.CROPS], dsize)
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(14, cn, dsize), dsize, extra=True)) == "area_u8c%d_interp" % cn
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(14, cn, dsize), dsize, extra=True), flags=capi.CHAIN_FORCE_GENERIC) == "area_interp"
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(14, cn, dsize, cvgs.CV_16FC1), dsize, half="f16")) == want + "_f16"
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(14, cn, dsize, cvgs.CV_16BFC1), dsize, half="bf16")) == want + "_bf16"
        # packed pixels, other depths: the interpreted kernel
        f = cvgs.make_type(capi.DEPTH_32F, cn)
        assert cvgs.kernel_name(rd, cvgs.write(f, _out(14, cn, dsize), dsize)) == "area_interp"
    for depth, cn in ((capi.DEPTH_8U, 1), (capi.DEPTH_16U, 3), (capi.DEPTH_16S, 4), (capi.DEPTH_32F, 1)):
        host, g = _frame(depth, cn)
        rd = cvgs.resize(cvgs.make_type(depth, cn), cvgs.INTER_AREA, [g.roi(*c) for c in M.CROPS], dsize)
        f = cvgs.make_type(capi.DEPTH_32F, cn)
        assert cvgs.kernel_name(rd, cvgs.write(f, _out(14, cn, dsize), dsize)) == "area_interp"


def test_what_has_no_area_kernel_is_refused_with_its_reason(lib):
    dsize = (16, 8)
    # CV_64F sources and CV_64F values
    src64 = np.zeros((M.SRC_H, M.SRC_W, 3), np.float64)
    g64 = cvgs.GpuMat.from_array(src64, cvgs.CV_64FC3)
    low = cvgs.lower([cvgs.resize(cvgs.CV_64FC3, cvgs.INTER_AREA, [g64], dsize), cvgs.split(cvgs.CV_32FC3, _out(1, 3, dsize), dsize)])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"CV_64F" in lib.cvgs_last_error() and b"INTER_AREA" in lib.cvgs_last_error()
    host, g = _frame()
    rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [g.roi(*c) for c in M.CROPS[:3]], dsize)
    out64 = np.zeros((3, 3 * 16 * 8), np.float64)
    low = cvgs.lower([rd, cvgs.convertTo(cvgs.CV_32FC3, cvgs.CV_64FC3),
                      cvgs.split(cvgs.CV_64FC3, cvgs.GpuMat(3, 3 * 16 * 8, cvgs.CV_64FC1, out64.ctypes.data, out64.strides[0], owner=out64), dsize)])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"CV_64F" in lib.cvgs_last_error()
    # mirrors
    ops = _k1_like(rd, 3, _out(3, 3, dsize), dsize)
    ops[-1].mirrored_to([4096])
    low = cvgs.lower(ops)
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"mirrors on INTER_AREA" in lib.cvgs_last_error()
    # the descriptor queue and the CircularTensor: refused for what the chain is, before the handle is looked at
    low = cvgs.lower(_k1_like(rd, 3, _out(3, 3, dsize), dsize))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK
    ticket = C.c_uint64()
    ptrs = (C.POINTER(capi.ChainDesc) * 1)(C.pointer(low.desc))
    for rc in (lib.cvgs_queue_submit(None, C.byref(low.desc), C.byref(ticket)), lib.cvgs_queue_submit_on(None, C.byref(low.desc), None, 0, C.byref(ticket)),
               lib.cvgs_queue_submit_many(None, ptrs, 1, C.byref(ticket)), lib.cvgs_queue_submit_many_on(None, ptrs, 1, None, 0, C.byref(ticket))):
        assert rc == capi.ERR_UNSUPPORTED and b"queue" in lib.cvgs_last_error() and b"INTER_AREA" in lib.cvgs_last_error()
    one = cvgs.lower(_k1_like(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, g, dsize), 3, _out(1, 3, dsize), dsize))
    assert lib.cvgs_circular_update(None, C.byref(one.desc), None) == capi.ERR_UNSUPPORTED
    assert b"CircularTensor" in lib.cvgs_last_error() and b"INTER_AREA" in lib.cvgs_last_error()
    # the box builder writes ONE layout, under the bilinear kind's name
    d = cvgs.box_table_desc(g, 4096, 8192, 4, dsize, kind=capi.READ_RESIZE_AREA)
    arr = (capi.BoxTableDesc * 1)(d)
    assert lib.cvgs_plane_tables_from_boxes(arr, 1, None) == capi.ERR_UNSUPPORTED and b"CVGS_READ_RESIZE_LINEAR" in lib.cvgs_last_error()
    # a read kind beyond the new one is still malformed
    low.desc.read.kind = 7
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID


# ---- tables --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", [cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])
def test_the_plane_table_is_the_bilinear_chains_table(lib, ar):
    host, g = _frame()
    crops = [g.roi(*c) for c in M.CROPS]
    for dsize in M.TARGETS + (M.NARROW_TARGET,):
        a = cvgs.build_plane_table(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, crops, dsize, None, None, ar))
        b = cvgs.build_plane_table(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, crops, dsize, None, None, ar))
        assert len(a) == 48 * len(crops) == lib.cvgs_plane_table_bytes(len(crops)) and a == b


def test_the_hull_is_the_whole_view_of_every_plane(lib):
    frame = np.zeros((480, 640, 3), np.uint8)
    g = cvgs.GpuMat.from_array(frame, cvgs.CV_8UC3)
    crops = [(10, 20, 100, 50), (300, 400, 64, 80), (5, 470, 30, 10)]
    rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [g.roi(*c) for c in crops], (16, 8))
    lo, hi = cvgs.table_hull(rd)
    base, step = frame.ctypes.data, 640 * 3
    assert lo == base + 20 * step + 10 * 3                  # first byte of the top row of the top-most crop
    assert hi == base + 479 * step + (300 + 64) * 3         # one past the last byte of the bottom row: row 479 ends crops 1 and 2, crop 1 further right
    one = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [g.roi(*crops[2])], (16, 8))
    assert cvgs.table_hull(one) == (base + 470 * step + 5 * 3, base + 479 * step + 35 * 3)


# ---- properties of the contract, on the restatement --------------------------------------------------------------------------------------------
def _plane(host, crop, dsize, cn=3, depth=capi.DEPTH_8U, model=M.area_plane_f32):
    g = cvgs.GpuMat.from_array(host, cvgs.make_type(depth, cn))
    P = M.plane_params(cvgs.resize(cvgs.make_type(depth, cn), cvgs.INTER_AREA, [g.roi(*crop)], dsize))[0]
    x, y, w, h = crop
    return model(host[y:y + h, x:x + w], P, dsize[0], dsize[1], [0.0] * 4), P


def test_a_2x_shrink_is_the_exact_block_mean(lib):
    for depth, cn in ((capi.DEPTH_8U, 3), (capi.DEPTH_16U, 3), (capi.DEPTH_16S, 4)):
        host = M.make_source(depth, cn)
        for crop, dsize in (((8, 4, 32, 16), (16, 8)), ((9, 1, 66, 14), (33, 7))):
            got, P = _plane(host, crop, dsize, cn, depth)
            assert P["fx"] == 2.0 and P["fy"] == 2.0
            x, y, w, h = crop
            blocks = host[y:y + h, x:x + w].astype(np.int64).reshape(dsize[1], 2, dsize[0], 2, cn).sum(axis=(1, 3))
            want = (blocks.astype(np.float64) / 4.0).astype(F32)  # exact: sums below 2^24, a quarter is a power of two
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_an_identity_view_reproduces_its_source(lib):
    for depth, cn in ((capi.DEPTH_8U, 3), (capi.DEPTH_16S, 4), (capi.DEPTH_32F, 1)):
        host = M.make_source(depth, cn)
        for crop, dsize in (((10, 10, 16, 8), (16, 8)), ((20, 30, 33, 7), (33, 7))):
            got, P = _plane(host, crop, dsize, cn, depth)
            x, y, w, h = crop
            assert np.array_equal(got.view(np.uint32), host[y:y + h, x:x + w].astype(F32).view(np.uint32))


def test_shrinking_weights_are_positive_and_sum_to_the_footprint(lib):
    """Every live weight > 0 and |W - (b - a)| <= 4 * 2^-24 * f, for every source extent 2 .. 97 into every target extent that shrinks it."""
    checked = 0
    for n in range(2, 98):
        for n_out in (1, 2, 3, 7, 8, 16, 33, 40):
            f = F32(np.float64(n) / np.float64(n_out))
            if not f > 1.0:
                continue
            idx, wt, live, W = M.axis_taps_f32(n_out, f, n)
            t = np.arange(n_out)
            a = t.astype(F32) * f
            b = np.minimum((t + 1).astype(F32) * f, F32(n))
            assert (b > a).all()
            assert (wt[live] > 0).all(), (n, n_out)
            assert (idx[live] >= 0).all() and (idx[live] < n).all()
            assert (np.abs(W.astype(np.float64) - (b.astype(np.float64) - a.astype(np.float64))) <= 4 * 2.0 ** -24 * float(f)).all(), (n, n_out)
            checked += 1
    assert checked > 300


def test_fp32_restatement_against_the_float64_model(lib):
    worst = 0.0
    for name, (depth, cn) in {"8UC1": (capi.DEPTH_8U, 1), "8UC3": (capi.DEPTH_8U, 3), "8UC4": (capi.DEPTH_8U, 4), "16UC3": (capi.DEPTH_16U, 3),
                              "16SC4": (capi.DEPTH_16S, 4), "32FC1": (capi.DEPTH_32F, 1)}.items():
        host = M.make_source(depth, cn)
        top = float(np.abs(host.astype(np.float64)).max())
        cases = [(c, d) for d in M.TARGETS for c in M.CROPS] + [((0, 0, 96, 61), M.NARROW_TARGET)]
        for crop, dsize in cases:
            a, _ = _plane(host, crop, dsize, cn, depth)
            b, _ = _plane(host, crop, dsize, cn, depth, M.area_plane_f64)
            dev = float(np.abs(a.astype(np.float64) - b).max()) / top
            worst = max(worst, dev)
            assert dev <= 4 * RECORDED_F32_VS_F64, (name, crop, dsize, dev)
    print("largest fp32 / float64 deviation relative to the largest source magnitude: %.3g" % worst)
    assert worst <= 4 * RECORDED_F32_VS_F64


# ---- the C++ facade ------------------------------------------------------------------------------------------------------------------------
LOWERING = r"""
#include <cvGPUSpeedup.h>
#include <cstdio>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, cvgs_last_error()); return 1; } } while (0)
static_assert(cvGS::isSupportedInterpolation<cv::INTER_AREA> && cvGS::isSupportedInterpolation<cv::INTER_LINEAR>, "both are served");
static_assert(!cvGS::isSupportedInterpolation<cv::INTER_CUBIC> && !cvGS::isSupportedInterpolation<cv::INTER_NEAREST>, "and nothing else");
static_assert((int)fk::INTER_AREA == (int)cv::INTER_AREA && (int)cv::INTER_AREA == 3, "INTER_AREA = 3");
int main() {
    constexpr int N = 5;
    static unsigned char frame[61 * 97 * 3];
    static float out[N * 16 * 8 * 3];
    cv::cuda::GpuMat f(61, 97, CV_8UC3, frame, 97 * 3), o(N, 16 * 8 * 3, CV_32FC1, out, 16 * 8 * 3 * 4), o1(1, 16 * 8 * 3, CV_32FC1, out, 16 * 8 * 3 * 4);
    std::array<cv::cuda::GpuMat, N> crops;
    for (int i = 0; i < N; ++i) crops[i] = f(cv::Rect(i, i, 40 + i, 30));
    const cv::Size d(16, 8);
    fk::ChainBuilder a, l, s, t;
    fk::lowerChain(a, cvGS::resize<CV_8UC3, cv::INTER_AREA, N, cvGS::PRESERVE_AR>(crops, d, 4, cv::Scalar(1, 2, 3)), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
                   cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)), cvGS::subtract<CV_32FC3>(cv::Scalar(1, 4, 6)), cvGS::divide<CV_32FC3>(cv::Scalar(57, 58, 59)),
                   cvGS::split<CV_32FC3>(o, d));
    fk::lowerChain(l, cvGS::resize<CV_8UC3, cv::INTER_LINEAR, N, cvGS::PRESERVE_AR>(crops, d, 4, cv::Scalar(1, 2, 3)), cvGS::split<CV_32FC3>(o, d));
    CHECK(a.d.read.kind == CVGS_READ_RESIZE_AREA && a.d.read.kind == 6 && a.d.read.batch == N && a.d.read.used_planes == 4);
    CHECK(a.d.read.aspect_ratio == CVGS_PRESERVE_AR && a.d.read.background[1] == 2.f && a.d.read.dst_width == 16 && a.d.read.dst_height == 8);
    CHECK(l.d.read.kind == CVGS_READ_RESIZE_LINEAR);
    CHECK(cvgs_validate(&a.d) == CVGS_OK);
    char name[64];
    CHECK(cvgs_kernel_name(&a.d, name, sizeof(name)) == CVGS_OK && std::string(name) == "area_u8c3_swap_mul_sub_div");
    // the single-image overload, and the resize still waiting for its source
    fk::lowerChain(s, cvGS::resize<CV_8UC3, cv::INTER_AREA>(f, d, 0., 0.), cvGS::split<CV_32FC3>(o1, d));
    CHECK(s.d.read.kind == CVGS_READ_RESIZE_AREA && s.d.read.batch == 1 && cvgs_validate(&s.d) == CVGS_OK);
    const auto rd = fk::Read<fk::PerThreadRead<fk::_2D, uchar3>>{cvGS::gpuMat2RawPtr2D<uchar3>(f)};
    fk::lowerChain(t, rd.then(cvGS::resize<cv::INTER_AREA>(d)), cvGS::split<CV_32FC3>(o1, d));
    CHECK(t.d.read.kind == CVGS_READ_RESIZE_AREA && cvgs_validate(&t.d) == CVGS_OK);
    std::printf("ok\n");
    return 0;
}
"""


def test_facade_spellings_lower_to_kind_6(tmp_path):
    src = tmp_path / "area_lowering.cpp"
    src.write_text(LOWERING)
    exe = tmp_path / "area_lowering"
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-command-line-argument", "-Wno-unused-variable", "-I" + INC,
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src), "-o", str(exe), "-L" + LIBDIR, "-lcvgs_hip", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_facade_refuses_cubic_and_area_over_nv12_at_compile_time(tmp_path):
    bad = {
        "cubic": ("auto x = cvGS::resize<CV_8UC3, cv::INTER_CUBIC, 2>(crops, cv::Size(8, 8), 2); (void)x;", "not supported yet"),
        "nv12_area": ("auto x = cvGS::resize<cv::INTER_AREA>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12>(m), cv::Size(8, 8)); (void)x;", "no area variant"),
        "nv12_area_ar": ("auto x = cvGS::resize<cv::INTER_AREA, cvGS::PRESERVE_AR>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12>(m), cv::Size(8, 8)); (void)x;",
                         "no area variant"),
    }
    good = "auto x = cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12>(m), cv::Size(8, 8)); (void)x;"
    for name, (body, msg) in list(bad.items()) + [("nv12_linear", (good, None))]:
        src = tmp_path / (name + ".cpp")
        src.write_text('#include <cvGPUSpeedup.h>\nint main() { cv::cuda::GpuMat m; std::array<cv::cuda::GpuMat, 2> crops; %s return 0; }\n' % body)
        r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I" + INC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src)],
                           capture_output=True, text=True)
        if msg is None:
            assert r.returncode == 0, r.stderr[-2000:]
            continue
        assert r.returncode != 0, "%s compiled but must not" % name
        assert ("static assertion failed" in r.stderr or "static_assert" in r.stderr) and msg in r.stderr, r.stderr[-800:]
