"""Packed 4:2:2 surfaces (CVGS_YUV_YUYV / CVGS_YUV_UYVY) on the NV12 read kinds -- the part that needs no GPU: the yardstick of the GPU
tests (the composed oracle value of tests/yuv422_cases.py, pinned here on NV12 surfaces where the oracle answers directly), what
cvgs_validate accepts and refuses, and the byte range a plane reads (cvgs_plane_table_hull)."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import yuv422_cases as Y

F3, F4 = cvgs.CV_32FC3, cvgs.CV_32FC4


def _programs(f, cn):
    norm = [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.subtract(f, [0.485, 0.456, 0.406, 0.5][:cn]), cvgs.divide(f, [0.229, 0.224, 0.225, 0.25][:cn])]
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA
    return {"none": [], "bgr_norm": [cvgs.cvtColor(swap, f)] + norm, "plain": [cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn])]}


@pytest.mark.parametrize("dst", [None, (50, 30), (200, 150), (7, 3)])
@pytest.mark.parametrize("prog", ["none", "bgr_norm", "plain"])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("range_,prim", [(capi.YUV_FULL, capi.BT709), (capi.YUV_LIMITED, capi.BT601), (capi.YUV_LIMITED, capi.BT2020)])
def test_composed_value_equals_the_oracles_direct_nv12_chain(oracle, dst, prog, alpha, range_, prim):
    """The method itself: for an NV12 surface (chroma of pixel (x, y) = U[y >> 1][x >> 1]) the composed value -- per-pixel read of the
    samples into an fp32 image, then the chain on that image -- equals the oracle's direct NV12 chain bit for bit."""
    w, h = 96, 64
    cn = 4 if alpha else 3
    f = F4 if alpha else F3
    surf = H.random_u8((h * 3 // 2, w), 4220)
    y, u, v = surf[:h], surf[h:, 0::2], surf[h:, 1::2]
    e = Y.read_stage_value(oracle, y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0), range_, prim, alpha)
    luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, surf.ctypes.data, surf.strides[0], owner=surf)
    crops = [(0, 0, w, h), (4, 2, 30, 20), (90, 60, 6, 4)] if dst is not None else [(0, 0, w, h)]
    shp = (len(crops), cn * dst[0] * dst[1]) if dst is not None else (h, w, cn)
    direct, comp = np.zeros(shp, np.float32), np.zeros(shp, np.float32)

    def chain(out):
        wr = cvgs.write(f, cvgs.GpuMat.from_array(out, f)) if dst is None else cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), dst)
        mats = [luma.nv12_roi(*c) for c in crops] if dst is not None else luma
        return [cvgs.read_nv12(mats, dst, range_, prim, alpha)] + _programs(f, cn)[prog] + [wr]

    oracle.execute(cvgs.lower(chain(direct)))
    ops = chain(comp)
    views = lambda m: (e, (m.data - surf.ctypes.data) % surf.strides[0], (m.data - surf.ctypes.data) // surf.strides[0])
    oracle.execute(cvgs.lower(Y.composed_ops(ops, views)))
    assert direct.any()
    H.assert_bit_exact(comp, direct, "composed vs direct NV12 chain")


def test_layout_constants():
    assert (capi.YUV_YUYV, capi.YUV_UYVY) == (Y.YUYV, Y.UYVY) == (5, 6)


def _chain(mat, layout, dst=None, out=None):
    f = F3
    if dst is None:
        out = np.zeros((mat.rows, mat.cols, 3), np.float32) if out is None else out
        wr = cvgs.write(f, cvgs.GpuMat.from_array(out, f))
    else:
        out = np.zeros((1, 3 * dst[0] * dst[1]), np.float32) if out is None else out
        wr = cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), dst)
    return cvgs.lower([cvgs.read_yuv422(mat, dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout), wr])


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("dst", [None, (20, 10)])
def test_validate_accepts_and_refuses(lib, layout, dst):
    surf = Y.random_surface(32, 16, 1, layout)
    m = Y.wrap_array(surf)
    ok = lambda ch: lib.cvgs_validate(C.byref(ch.desc))
    assert ok(_chain(m, layout, dst)) == capi.OK
    # crops: a plain view at an even x, any y, odd widths and heights
    for crop in [(2, 3, 5, 7), (30, 15, 1, 1), (0, 1, 3, 2), (4, 0, 28, 16)]:
        assert ok(_chain(m.yuv422_roi(*crop), layout, dst)) == capi.OK, crop
    with pytest.raises(ValueError):
        m.yuv422_roi(3, 0, 4, 4)
    ch = _chain(m, layout, dst)
    ch.desc.read.src_type = cvgs.CV_8UC1
    assert ok(ch) == capi.ERR_INVALID
    ch = _chain(m, layout, dst)
    ch.desc.read.yuv_layout = 7
    assert ok(ch) == capi.ERR_INVALID
    # one plane: no uv_offset; rows of 4-byte pixel pairs: data and step multiples of 4
    for field, value in [("uv_offset", 64), ("step", 66), ("data", surf.ctypes.data + 2)]:
        bad = cvgs.GpuMat(8, 8, Y.CV_8UC2, m.data, m.step, owner=surf)
        setattr(bad, field, value)
        assert ok(_chain(bad, layout, dst)) == capi.ERR_INVALID, field
    # a step that does not hold the whole last pair of an odd-width view
    narrow = cvgs.GpuMat(4, 3, Y.CV_8UC2, m.data, 4, owner=surf)
    assert ok(_chain(narrow, layout, dst)) == capi.ERR_INVALID


@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_device_tables_are_refused(lib, layout):
    surf = Y.random_surface(32, 16, 2, layout)
    ch = _chain(Y.wrap_array(surf), layout, (20, 10))
    ch.desc.read.flags |= capi.READ_FLAG_TABLE_ON_DEVICE
    assert lib.cvgs_validate(C.byref(ch.desc)) == capi.ERR_UNSUPPORTED


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("crop", [(2, 3, 5, 7), (30, 15, 1, 1), (0, 0, 32, 16), (6, 2, 4, 1)])
def test_hull_of_a_view_ends_with_its_last_whole_pair(lib, layout, crop):
    surf = Y.random_surface(32, 16, 3, layout)
    x, y, w, h = crop
    view = Y.wrap_array(surf).yuv422_roi(x, y, w, h)
    ch = _chain(view, layout, (20, 10))
    lo, hi = C.c_void_p(), C.c_void_p()
    assert lib.cvgs_plane_table_hull(C.byref(ch.desc.read), C.byref(lo), C.byref(hi)) == capi.OK
    assert lo.value == view.data
    assert hi.value == view.data + (h - 1) * view.step + 4 * ((w + 1) // 2)
    assert hi.value <= surf.ctypes.data + surf.nbytes


@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_kernel_names(lib, layout):
    """The resize read takes the packed 4:2:2 kernel family, the per-pixel read its pointwise source kind (no GPU needed: a dry run)."""
    surf = Y.random_surface(64, 32, 4, layout)
    m = Y.wrap_array(surf)
    f = F3
    out = np.zeros((1, 3 * 20 * 10), np.float32)
    ops = [cvgs.read_yuv422(m, (20, 10), capi.YUV_LIMITED, capi.BT709, False, layout=layout), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
           cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225]),
           cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), (20, 10))]
    assert cvgs.kernel_name(*ops) == "k_yuv422_resize_swap_mul_sub_div"
    img = np.zeros((32, 64, 3), np.float32)
    ops = [cvgs.read_yuv422(m, None, capi.YUV_LIMITED, capi.BT709, False, layout=layout), cvgs.multiply(f, [0.5] * 3), cvgs.write(f, cvgs.GpuMat.from_array(img, f))]
    assert cvgs.kernel_name(*ops) == "pointwise4_yuv422"


def test_the_cpp_facade_program_compiles():
    """cvGS::cvtColorYUY2 / cvtColorUYVY (tests/cpp/test_yuv422.cpp; run on the GPU by tests/test_gpu_yuv422.py)."""
    import os
    import subprocess
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-C", cpp, "bin/test_yuv422"], check=True, stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(cpp, "bin", "test_yuv422"))
