"""cvgs_plane_tables_from_boxes without a GPU: the independent model of the box rule (tests/box_cases.py) against hand-pinned cases, and
every validation error of the entry point with its message -- all of it is decided on the host before the first HIP call."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import box_cases as B


@pytest.mark.parametrize("fmt,cases,W,H,yuv", [
    (B.XYXY_F32, B.PINNED_XYXY, B.W0, B.H0, False), (B.XYWH_I32, B.PINNED_XYWH, B.W0, B.H0, False),
    (B.XYXY_F32, B.PINNED_420_XYXY, B.WY, B.HY, True), (B.XYWH_I32, B.PINNED_420_XYWH, B.WY, B.HY, True)])
def test_model_matches_the_pinned_cases(fmt, cases, W, H, yuv):
    arr = B.boxes_array([b for b, _ in cases], fmt)  # through the format's own dtype, as the device sees them
    for row, (box, want) in zip(arr, cases):
        assert B.rect(row, fmt, W, H, yuv) == want, (box, want)


def test_model_count_and_coverage():
    boxes = B.boxes_array([(0, 0, 5, 5), (1, 1, 5, 5), (2, 2, 5, 5)], B.XYWH_I32)
    full = [(0, 0, 5, 5), (1, 1, 5, 5), (2, 2, 5, 5)]
    for count, live in ((None, 3), (0, 0), (1, 1), (2, 2), (3, 3), (8, 3), (-3, 0)):
        assert B.rects(boxes, B.XYWH_I32, 50, 50, count) == full[:live] + [None] * (3 - live)
    for fmt in (B.XYXY_F32, B.XYWH_I32):
        arr = B.covering_boxes(fmt, B.W0, B.H0)
        assert 1900 <= len(arr) <= 2100
        rs = [r for r in B.rects(arr, fmt, B.W0, B.H0) if r]
        assert {r[2] for r in rs} == set(range(1, B.W0 + 1)) and {r[3] for r in rs} == set(range(1, B.H0 + 1))
        assert len(rs) < len(arr) * 0.95  # invalid boxes are part of the set
        for l, t, w, h in rs:
            assert 0 <= l and 0 <= t and w >= 1 and h >= 1 and l + w <= B.W0 and t + h <= B.H0


def _desc(**kw):
    frame = kw.pop("frame", None) or cvgs.GpuMat(131, 257, cvgs.CV_8UC3, 4096, 800)
    d = cvgs.box_table_desc(frame, kw.pop("boxes", 1 << 20), kw.pop("table", 2 << 20), kw.pop("max_boxes", 24), kw.pop("dsize", (64, 128)),
                            count=kw.pop("count", None), rects=kw.pop("rects", None), **kw)
    return d


def _nv12(cols=130, rows=66, step=132, uv=0, cv_type=None):
    m = cvgs.GpuMat(rows, cols, cvgs.CV_8UC1 if cv_type is None else cv_type, 4096, step)
    m.uv_offset = uv
    return m


def _call(lib, d, n=1):
    arr = (capi.BoxTableDesc * max(n, 1))(*([d] * max(n, 1)))
    return lib.cvgs_plane_tables_from_boxes(arr, n, None), lib.cvgs_last_error()


NV = dict(kind=capi.READ_NV12_RESIZE_LINEAR)
BAD = [  # (what, descriptor mutation, status, message fragment)
    ("struct_size", lambda d: setattr(d, "struct_size", 88), capi.ERR_INVALID, b"size mismatch"),
    ("flags", lambda d: setattr(d, "flags", 1), capi.ERR_INVALID, b"flags must be 0"),
    ("read kind out of range", lambda d: setattr(d, "read_kind", 9), capi.ERR_INVALID, b"bad read kind"),
    ("pixel reads", lambda d: setattr(d, "read_kind", capi.READ_PIXEL), capi.ERR_UNSUPPORTED, b"READ_PIXEL / READ_NV12"),
    ("NV12 pixel reads", lambda d: setattr(d, "read_kind", capi.READ_NV12), capi.ERR_UNSUPPORTED, b"READ_PIXEL / READ_NV12"),
    ("affine warps", lambda d: setattr(d, "read_kind", capi.READ_WARP_AFFINE), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("perspective warps", lambda d: setattr(d, "read_kind", capi.READ_WARP_PERSPECTIVE), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("max_boxes 0", lambda d: setattr(d, "max_boxes", 0), capi.ERR_INVALID, b"max_boxes must be in [1, 65535]"),
    ("max_boxes 65536", lambda d: setattr(d, "max_boxes", 65536), capi.ERR_INVALID, b"max_boxes must be in [1, 65535]"),
    ("box format", lambda d: setattr(d, "box_format", 2), capi.ERR_INVALID, b"bad box format"),
    ("null boxes", lambda d: setattr(d, "boxes", None), capi.ERR_INVALID, b"boxes is null"),
    ("null table", lambda d: setattr(d, "table_out", None), capi.ERR_INVALID, b"table_out is null"),
    ("table alignment", lambda d: setattr(d, "table_out", (2 << 20) + 4), capi.ERR_INVALID, b"alignment"),
    ("boxes alignment", lambda d: setattr(d, "boxes", (1 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("count alignment", lambda d: setattr(d, "count", (3 << 20) + 1), capi.ERR_INVALID, b"alignment"),
    ("rects alignment", lambda d: setattr(d, "rects_out", (3 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("target 0", lambda d: setattr(d, "dst_width", 0), capi.ERR_INVALID, b"resize target must be positive"),
    ("target too large", lambda d: setattr(d, "dst_height", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24"),
    ("target x frame beyond 2^30", lambda d: setattr(d, "dst_height", 1 << 23), capi.ERR_UNSUPPORTED, b"beyond 2^30"),
    ("aspect ratio", lambda d: setattr(d, "aspect_ratio", 4), capi.ERR_INVALID, b"bad aspect ratio mode"),
    ("source type", lambda d: setattr(d, "src_type", capi.make_type(capi.DEPTH_8U, 5)), capi.ERR_INVALID, b"bad source type"),
    ("null frame", lambda d: setattr(d.frame, "data", None), capi.ERR_INVALID, b"empty source plane"),
    ("empty frame", lambda d: setattr(d.frame, "height", 0), capi.ERR_INVALID, b"empty source plane"),
    ("frame too wide", lambda d: (setattr(d.frame, "width", (1 << 24) + 1), setattr(d.frame, "step", 1 << 30)), capi.ERR_UNSUPPORTED, b"2^24 pixels"),
    ("step", lambda d: setattr(d.frame, "step", 257 * 3 - 1), capi.ERR_INVALID, b"step smaller than a row"),
    ("uv_offset on pixels", lambda d: setattr(d.frame, "uv_offset", 64), capi.ERR_INVALID, b"uv_offset belongs to the NV12 kinds"),
]
BAD_NV12 = [
    ("layout out of range", lambda d: setattr(d, "yuv_layout", 8), capi.ERR_INVALID, b"bad yuv_layout"),
    ("odd width", lambda d: setattr(d.frame, "width", 129), capi.ERR_INVALID, b"even dimensions"),
    ("odd height", lambda d: setattr(d.frame, "height", 65), capi.ERR_INVALID, b"even dimensions"),
    ("odd uv_offset", lambda d: setattr(d.frame, "uv_offset", 66 * 132 + 1), capi.ERR_INVALID, b"uv_offset must be even"),
    ("negative uv_offset", lambda d: setattr(d.frame, "uv_offset", -2), capi.ERR_INVALID, b"uv_offset must be even"),
    ("uv_offset inside the luma", lambda d: setattr(d.frame, "uv_offset", 132), capi.ERR_INVALID, b"inside the luma rows"),
    ("odd step", lambda d: setattr(d.frame, "step", 133), capi.ERR_INVALID, b"even step"),
    ("source type", lambda d: setattr(d, "src_type", cvgs.CV_8UC3), capi.ERR_INVALID, b"CV_8UC1"),
    ("luma beyond 2 GiB", lambda d: (setattr(d.frame, "height", 1 << 22), setattr(d.frame, "step", 1 << 10), setattr(d, "dst_width", 1)), capi.ERR_UNSUPPORTED, b"2 GiB"),
]


@pytest.mark.parametrize("what,mut,code,msg", BAD, ids=[b[0] for b in BAD])
def test_validation_errors(lib, what, mut, code, msg):
    d = _desc()
    mut(d)
    rc, err = _call(lib, d)
    assert rc == code and msg in err, (what, rc, err)
    with pytest.raises(capi.CvgsError):
        cvgs.plane_tables_from_boxes(None, [d])


@pytest.mark.parametrize("what,mut,code,msg", BAD_NV12, ids=[b[0] for b in BAD_NV12])
def test_validation_errors_nv12(lib, what, mut, code, msg):
    d = _desc(frame=_nv12(), **NV)
    mut(d)
    rc, err = _call(lib, d)
    assert rc == code and msg in err, (what, rc, err)


@pytest.mark.parametrize("layout,name", [(capi.YUV_I420, b"I420"), (capi.YUV_YV12, b"YV12"), (capi.YUV_P010, b"P010"), (capi.YUV_YUYV, b"YUYV"),
                                         (capi.YUV_UYVY, b"UYVY"), (capi.YUV_I444, b"I444")])
def test_other_yuv_layouts_are_unsupported_by_name(lib, layout, name):
    d = _desc(frame=_nv12(), layout=layout, **NV)
    rc, err = _call(lib, d)
    assert rc == capi.ERR_UNSUPPORTED and name in err and b"NV12 / NV21" in err, (rc, err)


def test_null_descs_and_n_out_of_range(lib):
    assert lib.cvgs_plane_tables_from_boxes(None, 1, None) == capi.ERR_INVALID and b"null descriptors" in lib.cvgs_last_error()
    d = _desc()
    for n in (0, -1, capi.MAX_CHAINS + 1):
        arr = (capi.BoxTableDesc * (capi.MAX_CHAINS + 1))(*([d] * (capi.MAX_CHAINS + 1)))
        assert lib.cvgs_plane_tables_from_boxes(arr, n, None) == capi.ERR_INVALID
        assert b"[1, CVGS_MAX_CHAINS]" in lib.cvgs_last_error()
    # the SECOND descriptor of a call is validated like the first
    arr = (capi.BoxTableDesc * 2)(d, _desc(max_boxes=0))
    assert lib.cvgs_plane_tables_from_boxes(arr, 2, None) == capi.ERR_INVALID and b"max_boxes" in lib.cvgs_last_error()


def test_binding_struct_matches_the_header():
    assert C.sizeof(capi.BoxTableDesc) == 96
    assert capi.BoxTableDesc.frame.offset == 8 and capi.BoxTableDesc.read_kind.offset == 32 and capi.BoxTableDesc.boxes.offset == 64
    assert capi.BoxTableDesc.rects_out.offset == 88


def test_read_constructor_states_the_whole_frame(lib):
    """cvgs.resize_boxes: a device-table read with batch = used_planes = max_boxes whose stated source range is the whole frame's."""
    frame = np.zeros((131, 800), np.uint8)
    g = cvgs.GpuMat(131, 257, cvgs.CV_8UC3, frame.ctypes.data, 800, owner=frame)
    out = np.zeros((24, 3 * 128 * 64), np.float32)
    rd = cvgs.resize_boxes(g, 4096, 24, (64, 128), background=[1, 2, 3], ar=cvgs.PRESERVE_AR)
    low = cvgs.lower([rd, cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), (64, 128))])
    r = low.desc.read
    assert (r.batch, r.used_planes, r.src, r.flags) == (24, 24, 4096, capi.READ_FLAG_TABLE_ON_DEVICE)
    assert (r.table_src_lo, r.table_src_hi) == (frame.ctypes.data, frame.ctypes.data + 130 * 800 + 257 * 3)
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    surf = np.zeros((99, 132), np.uint8)
    rd = cvgs.resize_boxes(cvgs.GpuMat(66, 130, cvgs.CV_8UC1, surf.ctypes.data, 132, owner=surf), 4096, 8, (32, 32), yuv=(capi.YUV_FULL, capi.BT709, 0),
                           layout=capi.YUV_NV21)
    out = np.zeros((8, 3 * 32 * 32), np.float32)
    low = cvgs.lower([rd, cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_array(out, cvgs.CV_32FC1), (32, 32))])
    assert (low.desc.read.table_src_lo, low.desc.read.table_src_hi) == (surf.ctypes.data, surf.ctypes.data + 98 * 132 + 130)
    assert low.desc.read.yuv_layout == capi.YUV_NV21 and lib.cvgs_validate(C.byref(low.desc)) == capi.OK
