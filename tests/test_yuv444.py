"""Planar 4:4:4 surfaces (CVGS_YUV_I444) on the NV12 read kinds -- the part that needs no GPU: the yardstick of the GPU tests (the
composed oracle value of tests/yuv444_cases.py, pinned where the oracle answers directly and held to the float64 model of
tests/f64_model.py), what cvgs_validate accepts and refuses, the byte range a plane reads (cvgs_plane_table_hull) and the
independence logic of cvgs_execute_many, which run on the host."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as M
from tests import helpers as H
from tests import yuv444_cases as Y

F3, F4 = cvgs.CV_32FC3, cvgs.CV_32FC4
CONVERSIONS = [(capi.YUV_FULL, capi.BT709), (capi.YUV_LIMITED, capi.BT601), (capi.YUV_LIMITED, capi.BT2020)]


def _programs(f, cn):
    norm = [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.subtract(f, [0.485, 0.456, 0.406, 0.5][:cn]), cvgs.divide(f, [0.229, 0.224, 0.225, 0.25][:cn])]
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA
    return {"none": [], "bgr_norm": [cvgs.cvtColor(swap, f)] + norm, "plain": [cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn])]}


@pytest.fixture(scope="module")
def nv12_picture():
    """An NV12 surface of 96 x 64 and the same picture as 4:4:4 planes (chroma constant in 2 x 2 blocks)."""
    w, h = 96, 64
    surf = H.random_u8((h * 3 // 2, w), 4440)
    y, u, v = surf[:h], surf[h:, 0::2], surf[h:, 1::2]
    rep = lambda c: np.ascontiguousarray(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1))
    return surf, (np.ascontiguousarray(y), rep(u), rep(v))


@pytest.mark.parametrize("dst", [None, (50, 30), (200, 150), (7, 3)])
@pytest.mark.parametrize("prog", ["none", "bgr_norm", "plain"])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("range_,prim", CONVERSIONS)
def test_composed_value_equals_the_oracles_direct_nv12_chain(oracle, nv12_picture, dst, prog, alpha, range_, prim):
    """The method itself: a 4:4:4 picture whose chroma is constant in 2 x 2 blocks IS the NV12 picture of even size, so the composed
    value -- per-pixel read of the samples into an fp32 image, then the chain on that image -- equals the oracle's direct NV12 chain
    bit for bit, for the per-pixel read and for the resize."""
    surf, (y, u, v) = nv12_picture
    h, w = y.shape
    cn = 4 if alpha else 3
    f = F4 if alpha else F3
    e = Y.read_stage_value(oracle, y, u, v, range_, prim, alpha)
    luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, surf.ctypes.data, surf.strides[0], owner=surf)
    crops = [(0, 0, w, h), (4, 2, 30, 20), (90, 60, 6, 4)] if dst is not None else [(0, 0, w, h)]
    shp = (len(crops), cn * dst[0] * dst[1]) if dst is not None else (h, w, cn)
    direct, comp = np.zeros(shp, np.float32), np.zeros(shp, np.float32)

    def chain(out):
        wr = cvgs.write(f, cvgs.GpuMat.from_array(out, f)) if dst is None else cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), dst)
        mats = [luma.nv12_roi(*c) for c in crops] if dst is not None else luma
        return [cvgs.read_nv12(mats, dst, range_, prim, alpha)] + _programs(f, cn)[prog] + [wr]

    oracle.execute(cvgs.lower(chain(direct)))
    views = lambda m: (e, (m.data - surf.ctypes.data) % surf.strides[0], (m.data - surf.ctypes.data) // surf.strides[0])
    oracle.execute(cvgs.lower(Y.composed_ops(chain(comp), views)))
    assert direct.any()
    H.assert_bit_exact(comp, direct, "composed vs direct NV12 chain")


# ---- the composed value against the float64 model: a three-plane tap built from the model's public pieces ------------------------------
def _model_tap(s, x, y, range_, prim, alpha):
    """tap(ty, tx) -> Val of the view at (x, y) of surface s: the three planes' samples at one position, converted."""
    py, pu, pv = (p.astype(np.float64) for p in s.planes)

    def tap(ty, tx):
        yuv = np.stack(np.broadcast_arrays(py[y + ty, x + tx], pu[y + ty, x + tx], pv[y + ty, x + tx]), -1)
        return M.convert_yuv(yuv, 0.0, range_, prim, False, alpha)
    return tap


def _within(got, val, what):
    err = np.abs(got.astype(np.float64) - val.v)
    bad = err > val.b
    assert not bad.any(), "%s: %d elements outside the model's bound, worst ratio %.3f" % (what, int(bad.sum()), float((err / np.maximum(val.b, 1e-300)).max()))
    return float((err / np.maximum(val.b, 1e-300)).max())


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("range_,prim", CONVERSIONS + [(capi.YUV_FULL, capi.BT601), (capi.YUV_FULL, capi.BT2020), (capi.YUV_LIMITED, capi.BT709)])
def test_read_stage_value_is_within_the_float64_models_bound(oracle, range_, prim, alpha):
    s = Y.Surf(37, 23, 4450)
    e = Y.read_stage_value(oracle, *s.planes, range_, prim, alpha)
    yy, xx = np.mgrid[0:s.h, 0:s.w]
    _within(e, _model_tap(s, 0, 0, range_, prim, alpha)(yy, xx), "per-pixel read")


@pytest.mark.parametrize("view,dst", [((0, 0, 37, 23), (20, 11)), ((0, 0, 37, 23), (90, 50)), ((5, 3, 9, 7), (64, 33)), ((36, 22, 1, 1), (5, 4)),
                                      ((1, 1, 2, 1), (7, 3)), ((3, 0, 1, 5), (4, 9))])
@pytest.mark.parametrize("range_,prim,alpha", [(capi.YUV_FULL, capi.BT709, False), (capi.YUV_LIMITED, capi.BT601, True), (capi.YUV_LIMITED, capi.BT2020, False)])
def test_composed_resize_is_within_the_float64_models_bound(oracle, view, dst, range_, prim, alpha):
    """Convert each tap, then blend: the composed resize against bilinear() over the three-plane tap; the tolerance is the bound the
    model derives per element."""
    s = Y.Surf(37, 23, 4460)
    x, y, w, h = view
    cn = 4 if alpha else 3
    f = F4 if alpha else F3
    m = Y.wrap_array(s).yuv444_roi(x, y, w, h)
    out = np.zeros((1, cn * dst[0] * dst[1]), np.float32)
    Y.Expect(oracle, [s]).run([cvgs.read_yuv444(m, dst, range_, prim, alpha), cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), dst)])
    sx, sy = M.resize_coords(dst[0], w)[None, :], M.resize_coords(dst[1], h)[:, None]
    val = M.bilinear(_model_tap(s, x, y, range_, prim, alpha), sx, sy, w, h)
    got = out.reshape(cn, dst[1], dst[0]).transpose(1, 2, 0)
    _within(got, val, "resize %s -> %s" % (view, dst))


# ---- the contract: cvgs_validate, the hull, the independence check ------------------------------------------------------------------------
def test_layout_constant():
    assert capi.YUV_I444 == Y.I444 == 7


def _chain(mat, dst=None, out=None):
    f = F3
    if dst is None:
        out = np.zeros((mat.rows, mat.cols, 3), np.float32) if out is None else out
        wr = cvgs.write(f, cvgs.GpuMat.from_array(out, f))
    else:
        out = np.zeros((1, 3 * dst[0] * dst[1]), np.float32) if out is None else out
        wr = cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), dst)
    return cvgs.lower([cvgs.read_yuv444(mat, dst, capi.YUV_LIMITED, capi.BT709, False), wr])


def _mat(s, rows, cols, data, step, uv):
    m = cvgs.GpuMat(rows, cols, cvgs.CV_8UC1, data, step, owner=s.buf)
    m.uv_offset = uv
    return m


@pytest.mark.parametrize("dst", [None, (20, 10)])
def test_validate_accepts(lib, dst):
    ok = lambda ch: lib.cvgs_validate(C.byref(ch.desc))
    # even and odd sizes, a padded step, planes that are not adjacent; data, step and uv_offset with no alignment at all
    for w, h, step, uv, lead in [(32, 16, None, None, 0), (33, 17, None, None, 0), (1, 1, None, None, 0), (31, 9, 37, 9 * 37 + 5, 1), (7, 3, 11, 2 * 11 + 7, 3),
                                 (2, 5, 3, 4 * 3 + 2, 2)]:
        s = Y.Surf(w, h, 1, step=step, uv=uv, lead=lead)
        m = Y.wrap_array(s)
        assert ok(_chain(m, dst)) == capi.OK, (w, h, step, uv, lead, lib.cvgs_last_error())
    # crops: plain views at any origin, odd x and y included, of any size
    s = Y.Surf(32, 16, 2, step=35, uv=16 * 35 + 3, lead=1)
    m = Y.wrap_array(s)
    for crop in [(1, 1, 5, 7), (31, 15, 1, 1), (3, 0, 3, 2), (0, 5, 32, 11), (7, 3, 24, 13)]:
        v = m.yuv444_roi(*crop)
        assert v.uv_offset == m.uv_offset and v.data == m.data + crop[1] * m.step + crop[0]
        assert ok(_chain(v, dst)) == capi.OK, crop
    with pytest.raises(ValueError):
        m.yuv444_roi(30, 0, 4, 4)
    with pytest.raises(ValueError):
        cvgs.GpuMat(16, 32, cvgs.CV_8UC1, m.data, 35, owner=s.buf).yuv444_roi(0, 0, 4, 4)  # no uv_offset: not a 4:4:4 surface


@pytest.mark.parametrize("dst", [None, (20, 10)])
def test_validate_refuses(lib, dst):
    ok = lambda ch: lib.cvgs_validate(C.byref(ch.desc))
    s = Y.Surf(32, 16, 3, step=40)
    m = Y.wrap_array(s)
    assert ok(_chain(m, dst)) == capi.OK
    ch = _chain(m, dst)
    ch.desc.read.src_type = cvgs.make_type(cvgs.DEPTH_8U, 2)
    assert ok(ch) == capi.ERR_INVALID
    ch = _chain(m, dst)
    ch.desc.read.src_type = cvgs.make_type(cvgs.DEPTH_16U, 1)
    assert ok(ch) == capi.ERR_INVALID
    # uv_offset is always stated: 0 has no default meaning
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, 0), dst)) == capi.ERR_INVALID
    assert "uv_offset" in lib.cvgs_last_error().decode()
    # the planes of a view must not overlap: uv_offset >= (height - 1) * step + width, and exactly that is accepted
    least = 15 * 40 + 32
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, least - 1), dst)) == capi.ERR_INVALID
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, least), dst)) == capi.OK
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, -640), dst)) == capi.ERR_INVALID
    # step >= width
    assert ok(_chain(_mat(s, 16, 32, m.data, 31, 16 * 40), dst)) == capi.ERR_INVALID
    # planes more than 2^30 bytes apart (validation reads nothing)
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, 1 << 30), dst)) == capi.OK
    assert ok(_chain(_mat(s, 16, 32, m.data, 40, (1 << 30) + 1), dst)) == capi.ERR_UNSUPPORTED


def test_device_tables_are_refused(lib):
    s = Y.Surf(32, 16, 4)
    ch = _chain(Y.wrap_array(s), (20, 10))
    ch.desc.read.flags |= capi.READ_FLAG_TABLE_ON_DEVICE
    assert lib.cvgs_validate(C.byref(ch.desc)) == capi.ERR_UNSUPPORTED
    assert "device plane tables serve the NV12 / NV21 layouts only" in lib.cvgs_last_error().decode()


@pytest.mark.parametrize("crop", [(1, 3, 5, 7), (31, 15, 1, 1), (0, 0, 32, 16), (7, 2, 4, 1)])
def test_hull_of_a_view_spans_its_three_planes(lib, crop):
    s = Y.Surf(32, 16, 5, step=37, uv=16 * 37 + 11, guard=64, lead=3)
    x, y, w, h = crop
    view = Y.wrap_array(s).yuv444_roi(x, y, w, h)
    ch = _chain(view, (20, 10))
    lo, hi = C.c_void_p(), C.c_void_p()
    assert lib.cvgs_plane_table_hull(C.byref(ch.desc.read), C.byref(lo), C.byref(hi)) == capi.OK
    assert lo.value == view.data
    assert hi.value == view.data + 2 * s.uv + (h - 1) * s.step + w
    assert hi.value <= s.buf.ctypes.data + s.buf.nbytes - 64


def test_a_target_inside_the_v_plane_is_inside_the_source_range(lib):
    """The range the independence check of cvgs_execute_many compares with the other chains' targets (source_range, the function
    behind cvgs_plane_table_hull) must reach over the U and V planes: a target that lies inside chain A's V plane but behind its Y rows
    is inside that range.  (That such a tick then runs as sequential launches is asserted on the GPU: tests/test_gpu_yuv444.py.)"""
    s = Y.Surf(32, 16, 7, step=37, uv=16 * 37 + 11)
    view = Y.wrap_array(s).yuv444_roi(3, 2, 20, 9)
    ch = _chain(view, (20, 10))
    lo, hi = C.c_void_p(), C.c_void_p()
    assert lib.cvgs_plane_table_hull(C.byref(ch.desc.read), C.byref(lo), C.byref(hi)) == capi.OK
    target = view.data + 2 * s.uv + 4 * s.step  # row 4 of the view's V plane
    y_end = view.data + 8 * s.step + 20
    assert y_end <= target and lo.value <= target < hi.value


def test_kernel_names(lib):
    """The resize read takes the planar 4:4:4 kernel family, the per-pixel read its pointwise source kind (no GPU needed: a dry run)."""
    s = Y.Surf(64, 32, 6)
    m = Y.wrap_array(s)
    f = F3
    out = np.zeros((1, 3 * 20 * 10), np.float32)
    ops = [cvgs.read_yuv444(m, (20, 10), capi.YUV_LIMITED, capi.BT709, False), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
           cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225]),
           cvgs.split(f, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), (20, 10))]
    assert cvgs.kernel_name(*ops) == "k_yuv444_resize_swap_mul_sub_div"
    img = np.zeros((32, 64, 3), np.float32)
    ops = [cvgs.read_yuv444(m, None, capi.YUV_LIMITED, capi.BT709, False), cvgs.multiply(f, [0.5] * 3), cvgs.write(f, cvgs.GpuMat.from_array(img, f))]
    assert cvgs.kernel_name(*ops) == "pointwise4_yuv444"


def test_from_yuv444_tensor():
    import torch
    t = torch.zeros((3, 10, 24), dtype=torch.uint8)[:, 1:8, 3:20]
    m = cvgs.GpuMat.from_yuv444_tensor(t)
    assert (m.rows, m.cols, m.step, m.uv_offset, m.data) == (7, 17, 24, 240, t.data_ptr())
    with pytest.raises(ValueError):
        cvgs.GpuMat.from_yuv444_tensor(torch.zeros((3, 4, 4), dtype=torch.float32))
    with pytest.raises(ValueError):
        cvgs.GpuMat.from_yuv444_tensor(torch.zeros((3, 4, 8), dtype=torch.uint8)[:, :, ::2])


def test_the_cpp_facade_program_compiles():
    """cvGS::cvtColorYUV444 (tests/cpp/test_yuv444.cpp; run on the GPU by tests/test_gpu_yuv444.py)."""
    import os
    import subprocess
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.run(["make", "-C", cpp, "bin/test_yuv444"], check=True, stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(cpp, "bin", "test_yuv444"))
