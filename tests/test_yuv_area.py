"""INTER_AREA of 4:2:0 decoder surfaces (CVGS_READ_NV12_RESIZE_AREA) without a GPU: what validates and what is refused, the plane table and
its hull, the chroma axis, the exact properties of the arithmetic contract on the numpy restatement (tests/yuv_area_model.py), the
restatement against the independent float64 model, and the C++ facade's spelling.

fp32 restatement against the float64 model over the GPU test's case list (NV12 / NV21 / P010 x every crop x both targets, plus the whole
surface into 1 x 8): the largest deviation, relative to the top code of the layout (255 or 1023), was 2.00e-06 (P010, the 90 x 6 crop
into 33 x 7: its y axis does not shrink, so it takes the bilinear taps, whose position s = ty * fy is rounded to fp32 and moves weight
between two rows -- the case that is largest for the pixel AREA kind too, 1.85e-06 there; NV21 1.86e-06 and NV12 1.63e-06 on the same crop,
every case whose axes both shrink stays below 1.3e-06).  test_fp32_restatement_against_the_float64_model prints it and holds it under 4 x
that value, the margin of tests/test_area.py.  It has two sources the pixel AREA kind does not have: the engine's colour coefficients are 6-decimal fp32 literals
where the model derives them in float64 (half a unit of the sixth decimal on a chroma excursion of up to 128 codes), and the three
products and sums of the conversion are rounded once each.  The margin is for other seeds, not for kernel error: the kernels are held to
the restatement bit for bit (tests/test_gpu_yuv_area.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from oracle import oracle_binding
from tests import area_model as A
from tests import yuv_area_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cvgpuspeedup_amd", "include")
LIBDIR = os.path.join(ROOT, "cvgpuspeedup_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"
RECORDED_F32_VS_F64 = 2.00e-06
F32 = np.float32
YUV = {"NV12": (capi.YUV_FULL, capi.BT709, 0), "NV21": (capi.YUV_LIMITED, capi.BT601, 0), "P010": (capi.YUV_LIMITED, capi.BT2020, 0)}


def _surface(name):
    layout = M.LAYOUTS[name]
    s = M.make_surface(layout)
    return s, M.luma_mat(s, layout), layout


def _read(mat, crops, dsize, layout, yuv=(capi.YUV_FULL, capi.BT709, 0), interp=cvgs.INTER_AREA, ar=cvgs.IGNORE_AR, bg=None, used=None):
    rd = cvgs.read_nv12([mat.nv12_area_roi(*c) for c in crops], dsize, yuv[0], yuv[1], bool(yuv[2]), layout, interp=interp)
    rd.ar = ar
    if bg is not None:
        rd.background = [float(v) for v in bg]
    if used is not None:
        rd.used_planes = used
    return rd


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


def _plane(surface, mat, layout, crop, dsize, yuv, model=M.yuv_area_plane_f32):
    P = A.plane_params(_read(mat, [crop], dsize, layout, yuv))[0]
    return model(surface, layout, crop, P, dsize[0], dsize[1], [0.0] * 4, yuv), P


# ---- the C-ABI: what validates, what is refused ---------------------------------------------------------------------------------------------
def test_kind_8_validates_and_its_neighbours_do_not(lib):
    assert capi.READ_NV12_RESIZE_AREA == 8 and lib.cvgs_abi_version() == 6
    for name in M.LAYOUTS:
        s, mat, layout = _surface(name)
        for alpha in (0, 1):
            rd = _read(mat, M.CROPS[:5], (16, 8), layout, (capi.YUV_LIMITED, capi.BT601, alpha))
            cn = 4 if alpha else 3
            assert rd.kind == 8 and rd.out_type() == cvgs.make_type(capi.DEPTH_32F, cn)
            low = cvgs.lower(_k1_like(rd, cn, _out(5, cn, (16, 8)), (16, 8)))
            assert low.desc.read.kind == 8 and low.desc.read.yuv_layout == layout
            assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    for kind in (7, 9):
        low.desc.read.kind = kind
        assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID
    # the bilinear spelling is what it was, and still wants even views
    s, mat, layout = _surface("NV12")
    assert cvgs.read_nv12(mat, (16, 8)).kind == capi.READ_NV12_RESIZE_LINEAR and cvgs.read_nv12(mat).kind == capi.READ_NV12
    odd = _read(mat, [(12, 14, 39, 19)], (16, 8), layout, interp=cvgs.INTER_LINEAR)
    low = cvgs.lower([odd, cvgs.split(cvgs.CV_32FC3, _out(1, 3, (16, 8)), (16, 8))])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID and b"even" in lib.cvgs_last_error()
    with pytest.raises(ValueError):
        cvgs.read_nv12(mat, (16, 8), interp=0)  # INTER_NEAREST
    with pytest.raises(ValueError):
        cvgs.read_nv12(mat, None, interp=cvgs.INTER_AREA)  # no target: nothing to resize


def test_kernel_names(lib):
    dsize = (16, 8)
    s, mat, layout = _surface("NV12")
    for alpha, cn in ((0, 3), (1, 4)):
        want = "yuv_area_c%d_swap_mul_sub_div" % cn
        for n in (1, 14, 70):  # inline, inline, staged table
            rd = _read(mat, [M.CROPS[i % len(M.CROPS)] for i in range(n)], dsize, layout, (capi.YUV_FULL, capi.BT709, alpha))
            assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize)) == want
            assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize), flags=capi.CHAIN_FORCE_GENERIC) == "yuv_area_interp"
        rd = _read(mat, M.CROPS, dsize, capi.YUV_NV21, (capi.YUV_FULL, capi.BT709, alpha))
        n = len(M.CROPS)
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize), dsize, extra=True)) == "yuv_area_c%d_interp" % cn
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize, cvgs.CV_16FC1), dsize, half="f16")) == want + "_f16"
        assert cvgs.kernel_name(*_k1_like(rd, cn, _out(n, cn, dsize, cvgs.CV_16BFC1), dsize, half="bf16")) == want + "_bf16"
        f = cvgs.make_type(capi.DEPTH_32F, cn)
        assert cvgs.kernel_name(rd, cvgs.multiply(f, [0.3] * cn), cvgs.subtract(f, [1.0] * cn), cvgs.divide(f, [3.0] * cn),
                                cvgs.split(f, _out(n, cn, dsize), dsize)) == "yuv_area_c%d_mul_sub_div" % cn
        assert cvgs.kernel_name(rd, cvgs.write(f, _out(n, cn, dsize), dsize)) == "yuv_area_interp"  # packed pixels
    s, mat, layout = _surface("P010")  # 16-bit samples: the interpreted kernel
    rd = _read(mat, M.CROPS, dsize, layout)
    assert cvgs.kernel_name(*_k1_like(rd, 3, _out(len(M.CROPS), 3, dsize), dsize)) == "yuv_area_interp"


def test_what_has_no_kernel_is_refused_with_its_reason(lib):
    dsize = (16, 8)
    s, mat, layout = _surface("NV12")
    crops = M.CROPS[:3]
    # the layouts this kind does not serve, each by its name
    for name, lay, typ in (("I420", capi.YUV_I420, None), ("YV12", capi.YUV_YV12, None), ("YUYV", capi.YUV_YUYV, cvgs.make_type(capi.DEPTH_8U, 2)),
                           ("UYVY", capi.YUV_UYVY, cvgs.make_type(capi.DEPTH_8U, 2)), ("I444", capi.YUV_I444, None)):
        rd = _read(mat, crops, dsize, layout)
        rd.yuv_layout = lay
        if typ is not None:
            rd.src_type = typ
            for m in rd.mats:
                m.cv_type = typ
        low = cvgs.lower([rd, cvgs.split(cvgs.CV_32FC3, _out(3, 3, dsize), dsize)])
        assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED, name
        assert name.encode() in lib.cvgs_last_error() and b"INTER_AREA" in lib.cvgs_last_error()
    # CV_64F values
    rd = _read(mat, crops, dsize, layout)
    out64 = np.zeros((3, 3 * 16 * 8), np.float64)
    low = cvgs.lower([rd, cvgs.convertTo(cvgs.CV_32FC3, cvgs.CV_64FC3),
                      cvgs.split(cvgs.CV_64FC3, cvgs.GpuMat(3, 3 * 16 * 8, cvgs.CV_64FC1, out64.ctypes.data, out64.strides[0], owner=out64), dsize)])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED
    assert b"CV_64F" in lib.cvgs_last_error() and b"decoder surfaces" in lib.cvgs_last_error()
    # mirrors
    ops = _k1_like(rd, 3, _out(3, 3, dsize), dsize)
    ops[-1].mirrored_to([4096])
    low = cvgs.lower(ops)
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"mirrors on INTER_AREA reads of decoder surfaces" in lib.cvgs_last_error()
    # an NV12 surface write behind it
    surf = np.zeros((8 * 3 // 2, 16), np.uint8)
    target = cvgs.GpuMat(8, 16, cvgs.CV_8UC1, surf.ctypes.data, 16, owner=surf)
    low = cvgs.lower([_read(mat, crops[:1], dsize, layout), cvgs.write_nv12([target])])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED
    assert b"NV12 surface writes behind INTER_AREA reads of decoder surfaces" in lib.cvgs_last_error()
    # the descriptor queue and the CircularTensor: refused for what the chain is, before the handle is looked at
    low = cvgs.lower(_k1_like(rd, 3, _out(3, 3, dsize), dsize))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK
    ticket = C.c_uint64()
    ptrs = (C.POINTER(capi.ChainDesc) * 1)(C.pointer(low.desc))
    for rc in (lib.cvgs_queue_submit(None, C.byref(low.desc), C.byref(ticket)), lib.cvgs_queue_submit_on(None, C.byref(low.desc), None, 0, C.byref(ticket)),
               lib.cvgs_queue_submit_many(None, ptrs, 1, C.byref(ticket)), lib.cvgs_queue_submit_many_on(None, ptrs, 1, None, 0, C.byref(ticket))):
        assert rc == capi.ERR_UNSUPPORTED and b"queue" in lib.cvgs_last_error() and b"CVGS_READ_NV12_RESIZE_AREA" in lib.cvgs_last_error()
    one = cvgs.lower(_k1_like(_read(mat, crops[:1], dsize, layout), 3, _out(1, 3, dsize), dsize))
    assert lib.cvgs_circular_update(None, C.byref(one.desc), None) == capi.ERR_UNSUPPORTED
    assert b"CircularTensor" in lib.cvgs_last_error() and b"CVGS_READ_NV12_RESIZE_AREA" in lib.cvgs_last_error()
    # the box builder writes ONE layout, under the bilinear kind's name
    d = cvgs.box_table_desc(mat, 4096, 8192, 4, dsize, kind=capi.READ_NV12_RESIZE_AREA)
    arr = (capi.BoxTableDesc * 1)(d)
    assert lib.cvgs_plane_tables_from_boxes(arr, 1, None) == capi.ERR_UNSUPPORTED and b"CVGS_READ_NV12_RESIZE_LINEAR" in lib.cvgs_last_error()
    # a device table of a P010 chain: host descriptors only, as for the bilinear kind
    s10, mat10, lay10 = _surface("P010")
    rd10 = _read(mat10, crops, dsize, lay10)
    rd10.table = 4096
    low = cvgs.lower([rd10, cvgs.split(cvgs.CV_32FC3, _out(3, 3, dsize), dsize)])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"device plane tables" in lib.cvgs_last_error()


def test_resize_boxes_lowers_to_kind_8_over_the_bilinear_kinds_table(lib):
    s, mat, layout = _surface("NV12")
    yuv = (capi.YUV_FULL, capi.BT709, 0)
    assert cvgs.resize_boxes(mat, 4096, 4, (16, 8), yuv=yuv).kind == capi.READ_NV12_RESIZE_LINEAR
    rd = cvgs.resize_boxes(mat, 4096, 4, (16, 8), yuv=yuv, layout=capi.YUV_NV21, interp=cvgs.INTER_AREA)
    assert rd.kind == capi.READ_NV12_RESIZE_AREA and rd.yuv_layout == capi.YUV_NV21
    assert rd.table_hull == (s.ctypes.data, s.ctypes.data + s.nbytes)  # the whole surface, chroma plane included
    low = cvgs.lower(_k1_like(rd, 3, _out(4, 3, (16, 8)), (16, 8)))
    assert low.desc.read.flags & capi.READ_FLAG_TABLE_ON_DEVICE and low.desc.read.table_src_hi - low.desc.read.table_src_lo == s.nbytes
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    assert cvgs.kernel_name(*_k1_like(rd, 3, _out(4, 3, (16, 8)), (16, 8))) == "yuv_area_c3_swap_mul_sub_div"
    with pytest.raises(ValueError):
        cvgs.resize_boxes(mat, 4096, 4, (16, 8), yuv=yuv, layout=capi.YUV_I420, interp=cvgs.INTER_AREA)


# ---- tables --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", [cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])
def test_the_plane_table_is_the_bilinear_nv12_chains_table(lib, ar):
    for name in M.LAYOUTS:
        s, mat, layout = _surface(name)
        for dsize in M.TARGETS + (M.NARROW_TARGET,):
            a = cvgs.build_plane_table(_read(mat, M.EVEN_CROPS, dsize, layout, ar=ar))
            b = cvgs.build_plane_table(_read(mat, M.EVEN_CROPS, dsize, layout, interp=cvgs.INTER_LINEAR, ar=ar))
            assert len(a) == 48 * len(M.EVEN_CROPS) == lib.cvgs_plane_table_bytes(len(M.EVEN_CROPS)) and a == b


def test_the_hull_is_every_luma_byte_and_every_chroma_byte_under_it(lib):
    W, H = 640, 480
    surf = np.zeros((H * 3 // 2, W), np.uint8)
    mat = cvgs.GpuMat(H, W, cvgs.CV_8UC1, surf.ctypes.data, W, owner=surf)
    base = surf.ctypes.data

    def hull(*crops):
        return cvgs.table_hull(_read(mat, crops, (16, 8), capi.YUV_NV12))

    # one even crop: first luma byte .. one past the last chroma pair of its last chroma row
    assert hull((10, 20, 100, 50)) == (base + 20 * W + 10, base + (H + 10 + 24) * W + 10 + 100)
    # an odd crop: ceil(h / 2) chroma rows of 2 * ceil(w / 2) samples -- the pair of the last column is read whole
    assert hull((10, 20, 99, 49)) == (base + 20 * W + 10, base + (H + 10 + 24) * W + 10 + 100)
    assert hull((10, 20, 99, 47)) == (base + 20 * W + 10, base + (H + 10 + 23) * W + 10 + 100)
    # several: the lowest luma byte, the highest chroma byte (rows 470 .. 479 -> chroma rows 235 .. 239)
    assert hull((10, 20, 100, 50), (300, 400, 64, 80), (4, 470, 31, 10)) == (base + 20 * W + 10, base + (H + 239) * W + 300 + 64)
    # P010: the same in 2-byte samples
    surf10 = np.zeros((H * 3 // 2, W), np.uint16)
    mat10 = cvgs.GpuMat(H, W, cvgs.CV_16UC1, surf10.ctypes.data, 2 * W, owner=surf10)
    lo, hi = cvgs.table_hull(_read(mat10, [(10, 20, 99, 49)], (16, 8), capi.YUV_P010))
    assert (lo, hi) == (surf10.ctypes.data + 20 * 2 * W + 20, surf10.ctypes.data + (H + 10 + 24) * 2 * W + 20 + 200)


# ---- the chroma axis -------------------------------------------------------------------------------------------------------------------------
def test_chroma_weights_are_positive_in_range_and_sum_to_the_footprint():
    """Every live weight > 0, every index in [0, nc), and |Wc - (bc - ac)| <= 4 * 2^-24 * f / 2 (the luma test's bound on the halved
    footprint), for every even and odd extent 1 .. 97 into every target extent; non-shrinking axes keep the luma pair's weights."""
    shrinking = other = 0
    for n in range(1, 98):
        nc = (n + 1) >> 1
        for n_out in (1, 2, 3, 7, 8, 16, 33, 40):
            f = F32(np.float64(n) / np.float64(n_out))
            idx, wt, live, W = M.chroma_axis_taps_f32(n_out, f, n)
            assert (idx[live] >= 0).all() and (idx[live] < nc).all(), (n, n_out)
            if not f > 1.0:
                li, lw, _, _ = A.axis_taps_f32(n_out, f, n)
                assert np.array_equal(idx, li >> 1) and np.array_equal(wt, lw) and (W == 1.0).all() and idx.shape[1] == 2
                other += 1
                continue
            t = np.arange(n_out)
            ac = (t.astype(F32) * f) * F32(0.5)
            bc = np.minimum((t + 1).astype(F32) * f, F32(n)) * F32(0.5)
            assert (bc > ac).all()
            assert (wt[live] > 0).all(), (n, n_out)
            assert (np.abs(W.astype(np.float64) - (bc.astype(np.float64) - ac.astype(np.float64))) <= 4 * 2.0 ** -24 * float(f) / 2).all(), (n, n_out)
            shrinking += 1
    assert shrinking > 300 and other > 100


# ---- exact properties of the contract, on the restatement ----------------------------------------------------------------------------------
def test_a_constant_surface_gives_the_conversion_of_the_constant(lib):
    for name, (yv, uv, vv) in (("NV12", (81, 90, 240)), ("NV21", (145, 54, 34)), ("P010", (700, 300, 820))):
        layout = M.LAYOUTS[name]
        s = M.make_surface(layout)
        ten = layout == capi.YUV_P010
        sh = 6 if ten else 0
        s[:M.SRC_H] = yv << sh
        s[M.SRC_H:, 0::2] = (vv if name == "NV21" else uv) << sh
        s[M.SRC_H:, 1::2] = (uv if name == "NV21" else vv) << sh
        mat = M.luma_mat(s, layout)
        for alpha in (0, 1):
            yuv = (YUV[name][0], YUV[name][1], alpha)
            want = M.convert_f32(F32(yv), F32(uv), F32(vv), yuv[0], yuv[1], ten, alpha)
            for crop, dsize in (((8, 4, 32, 16), (16, 8)), ((10, 2, 66, 14), (33, 7)), ((2, 2, 64, 32), (16, 8)), ((0, 0, 4, 32), (1, 8))):  # 2x, 2x, 4x, 4x
                got, P = _plane(s, mat, layout, crop, dsize, yuv)
                assert P["fx"] in (2.0, 4.0) and P["fy"] in (2.0, 4.0)
                assert np.array_equal(got.view(np.uint32), np.broadcast_to(want, got.shape).view(np.uint32)), (name, crop)


def test_a_2x_shrink_converts_the_block_means(lib):
    for name in M.LAYOUTS:
        s, mat, layout = _surface(name)
        for crop, dsize in (((8, 4, 32, 16), (16, 8)), ((10, 2, 66, 14), (33, 7))):
            got, P = _plane(s, mat, layout, crop, dsize, YUV[name])
            assert P["fx"] == 2.0 and P["fy"] == 2.0
            luma, pairs = M.view_codes(s, layout, crop)
            ym = (luma[..., 0].astype(np.float64).reshape(dsize[1], 2, dsize[0], 2).sum(axis=(1, 3)) / 4.0).astype(F32)  # exact: a quarter of a small integer
            want = M.convert_f32(ym, pairs[..., 0], pairs[..., 1], YUV[name][0], YUV[name][1], layout == capi.YUV_P010, 0)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, crop)


def test_an_identity_view_reproduces_the_pointwise_nv12_read(lib, oracle):
    for name in M.LAYOUTS:
        s, mat, layout = _surface(name)
        for alpha in (0, 1):
            yuv = (YUV[name][0], YUV[name][1], alpha)
            cn = 4 if alpha else 3
            for crop in ((10, 10, 16, 8), (20, 30, 34, 6)):
                dsize = (crop[2], crop[3])
                got, P = _plane(s, mat, layout, crop, dsize, yuv)
                assert P["fx"] == 1.0 and P["fy"] == 1.0
                ref = np.zeros((dsize[1], dsize[0], cn), np.float32)
                t = cvgs.make_type(capi.DEPTH_32F, cn)
                rd = cvgs.read_nv12(mat.nv12_roi(*crop), None, yuv[0], yuv[1], bool(alpha), layout)
                oracle_binding.execute(cvgs.lower([rd, cvgs.write(t, cvgs.GpuMat.from_array(ref, t))]))
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, crop, alpha)


def test_nv21_is_nv12_with_the_chroma_bytes_swapped(lib):
    s = M.make_surface(capi.YUV_NV12)
    swapped = s.copy()
    swapped[M.SRC_H:, 0::2], swapped[M.SRC_H:, 1::2] = s[M.SRC_H:, 1::2], s[M.SRC_H:, 0::2]
    yuv = (capi.YUV_LIMITED, capi.BT709, 1)
    for dsize in M.TARGETS:
        for crop in M.CROPS:
            a, _ = _plane(s, M.luma_mat(s, capi.YUV_NV12), capi.YUV_NV12, crop, dsize, yuv)
            b, _ = _plane(swapped, M.luma_mat(swapped, capi.YUV_NV21), capi.YUV_NV21, crop, dsize, yuv)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (crop, dsize)


def test_fp32_restatement_against_the_float64_model(lib):
    worst, where = 0.0, None
    for name in M.LAYOUTS:
        s, mat, layout = _surface(name)
        top = 1023.0 if layout == capi.YUV_P010 else 255.0
        cases = [(c, d) for d in M.TARGETS for c in M.CROPS] + [((0, 0, 98, 62), M.NARROW_TARGET)]
        for crop, dsize in cases:
            a, _ = _plane(s, mat, layout, crop, dsize, YUV[name])
            b, _ = _plane(s, mat, layout, crop, dsize, YUV[name], M.yuv_area_plane_f64)
            dev = float(np.abs(a.astype(np.float64) - b).max()) / top
            if dev > worst:
                worst, where = dev, (name, crop, dsize)
            assert dev <= 4 * RECORDED_F32_VS_F64, (name, crop, dsize, dev)
    print("largest fp32 / float64 deviation relative to the top code: %.3g at %s" % (worst, where))
    assert worst <= 4 * RECORDED_F32_VS_F64


# ---- the C++ facade ------------------------------------------------------------------------------------------------------------------------
LOWERING = r"""
#include <cvGPUSpeedup.h>
#include <cstdio>
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, cvgs_last_error()); return 1; } } while (0)
int main() {
    static unsigned char surf[93 * 98];
    static unsigned short surf10[93 * 98];
    static float out[4 * 16 * 8 * 4];
    cv::cuda::GpuMat nv12(93, 98, CV_8UC1, surf, 98), p010(93, 98, CV_16UC1, surf10, 98 * 2);
    cv::cuda::GpuMat o1(1, 16 * 8 * 3, CV_32FC1, out, 16 * 8 * 3 * 4), o4(4, 16 * 8 * 3, CV_32FC1, out, 16 * 8 * 3 * 4), oa(1, 16 * 8 * 4, CV_32FC1, out, 16 * 8 * 4 * 4);
    const cv::Size d(16, 8);
    char name[64];
    // the whole surface, BGR: the swap is the chain's first stage
    fk::ChainBuilder a, l, b, c, p, v;
    fk::lowerChain(a, cvGS::resizeArea(cvGS::cvtColorNV12<cv::COLOR_YUV2BGR_NV12>(nv12), d), cvGS::multiply<CV_32FC3>(cv::Scalar(0.3, 0.3, 0.3)),
                   cvGS::subtract<CV_32FC3>(cv::Scalar(1, 4, 6)), cvGS::divide<CV_32FC3>(cv::Scalar(57, 58, 59)), cvGS::split<CV_32FC3>(o1, d));
    fk::lowerChain(l, cvGS::resize<cv::INTER_LINEAR>(cvGS::cvtColorNV12<cv::COLOR_YUV2BGR_NV12>(nv12), d), cvGS::split<CV_32FC3>(o1, d));
    CHECK(a.d.read.kind == CVGS_READ_NV12_RESIZE_AREA && a.d.read.kind == 8 && a.d.read.batch == 1 && a.d.read.yuv_layout == CVGS_YUV_NV12);
    CHECK(a.d.read.dst_width == 16 && a.d.read.dst_height == 8 && a.d.read.aspect_ratio == CVGS_IGNORE_AR && a.d.read.yuv_alpha == 0);
    CHECK(l.d.read.kind == CVGS_READ_NV12_RESIZE_LINEAR);
    CHECK(cvgs_validate(&a.d) == CVGS_OK);
    CHECK(cvgs_kernel_name(&a.d, name, sizeof(name)) == CVGS_OK && std::string(name) == "yuv_area_c3_swap_mul_sub_div");
    // letterboxed, with a background (given in the IOp's channel order, entering before the swap)
    fk::lowerChain(b, cvGS::resizeArea<cvGS::PRESERVE_AR>(cvGS::cvtColorNV12<cv::COLOR_YUV2BGR_NV12>(nv12), d, cv::Scalar(1, 2, 3)), cvGS::split<CV_32FC3>(o1, d));
    CHECK(b.d.read.kind == CVGS_READ_NV12_RESIZE_AREA && b.d.read.aspect_ratio == CVGS_PRESERVE_AR);
    CHECK(b.d.read.background[0] == 3.f && b.d.read.background[1] == 2.f && b.d.read.background[2] == 1.f && cvgs_validate(&b.d) == CVGS_OK);
    // crops of the surface as a batch, RGBA
    const std::array<cv::Rect, 4> crops = {cv::Rect(0, 0, 98, 62), cv::Rect(8, 4, 32, 16), cv::Rect(10, 12, 38, 18), cv::Rect(56, 38, 42, 24)};
    fk::lowerChain(c, cvGS::resizeArea(cvGS::cvtColorNV12<cv::COLOR_YUV2RGBA_NV12, fk::Limited, fk::bt601>(nv12, crops), d), cvGS::write<CV_32FC4>(oa, d));
    CHECK(c.d.read.kind == CVGS_READ_NV12_RESIZE_AREA && c.d.read.batch == 4 && c.d.read.used_planes == 4 && c.d.read.yuv_alpha == 1);
    CHECK(c.d.read.yuv_range == CVGS_YUV_LIMITED && c.d.read.yuv_primaries == CVGS_BT601);
    // the P010 and the NV21 spellings of the IOp
    fk::lowerChain(p, cvGS::resizeArea(cvGS::cvtColorP010<cv::COLOR_YUV2RGB_NV12>(p010), d), cvGS::split<CV_32FC3>(o1, d));
    CHECK(p.d.read.kind == CVGS_READ_NV12_RESIZE_AREA && p.d.read.yuv_layout == CVGS_YUV_P010 && p.d.read.src_type == CV_16UC1 && cvgs_validate(&p.d) == CVGS_OK);
    CHECK(cvgs_kernel_name(&p.d, name, sizeof(name)) == CVGS_OK && std::string(name) == "yuv_area_interp");
    fk::RawPtr<fk::_2D, uchar> luma;
    luma.data = surf;
    luma.dims = {98u, 62u, 98u};
    const fk::YuvRead<fk::NV21, fk::Full, fk::bt709, false, float3> nv21{luma};
    fk::lowerChain(v, cvGS::resizeArea<cvGS::PRESERVE_AR_LEFT>(nv21, d), cvGS::split<CV_32FC3>(o1, d));
    CHECK(v.d.read.kind == CVGS_READ_NV12_RESIZE_AREA && v.d.read.yuv_layout == CVGS_YUV_NV21 && v.d.read.aspect_ratio == CVGS_PRESERVE_AR_LEFT && cvgs_validate(&v.d) == CVGS_OK);
    std::printf("ok\n");
    return 0;
}
"""


def test_facade_spellings_lower_to_kind_8(tmp_path):
    src = tmp_path / "yuv_area_lowering.cpp"
    src.write_text(LOWERING)
    exe = tmp_path / "yuv_area_lowering"
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-command-line-argument", "-Wno-unused-variable", "-I" + INC,
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src), "-o", str(exe), "-L" + LIBDIR, "-lcvgs_hip", "-L/opt/rocm/lib",
                        "-lamdhip64", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_facade_refuses_the_layouts_the_kind_does_not_serve_and_points_to_resize_area(tmp_path):
    bad = {
        "yuy2": ("auto x = cvGS::resizeArea(cvGS::cvtColorYUY2<cv::COLOR_YUV2RGB_YUY2>(m), cv::Size(8, 8)); (void)x;", "NV12, NV21 and P010"),
        "nv12_inter_area": ("auto x = cvGS::resize<cv::INTER_AREA>(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12>(m), cv::Size(8, 8)); (void)x;", "resizeArea"),
    }
    good = "auto x = cvGS::resizeArea(cvGS::cvtColorNV12<cv::COLOR_YUV2RGB_NV12>(m), cv::Size(8, 8)); (void)x;"
    for name, (body, msg) in list(bad.items()) + [("nv12_area", (good, None))]:
        src = tmp_path / (name + ".cpp")
        src.write_text('#include <cvGPUSpeedup.h>\nint main() { cv::cuda::GpuMat m; %s return 0; }\n' % body)
        r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I" + INC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src)],
                           capture_output=True, text=True)
        if msg is None:
            assert r.returncode == 0, r.stderr[-2000:]
            continue
        assert r.returncode != 0, "%s compiled but must not" % name
        assert ("static assertion failed" in r.stderr or "static_assert" in r.stderr) and msg in r.stderr, r.stderr[-800:]
