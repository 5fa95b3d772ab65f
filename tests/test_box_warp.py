"""cvgs_warp_tables_from_boxes without a GPU: cvgs_warp_table_from_boxes_host (the bytes the kernel must write) against the independent
numpy model of tests/box_warp_model.py byte for byte, exact pixels of an integer box through the CPU oracle, the model's sensitivity to the
three mistakes the contract rules out, every refusal of both entry points (decided on the host before the first HIP call), and boxes_out
as the boxes of the crop builder's box rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import box_cases as B
from tests import box_warp_cases as K
from tests import box_warp_model as M
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")])
FRAME = (K.FRAME_DATA, K.W, K.H, K.STEP)


def _frame(cv_type=cvgs.CV_8UC3, rows=K.H, cols=K.W, step=K.STEP, data=K.FRAME_DATA):
    return cvgs.GpuMat(rows, cols, cv_type, data, step)


def _desc(**kw):
    return cvgs.box_warp_desc(kw.pop("frame", None) or _frame(), kw.pop("boxes", 1 << 20), kw.pop("table", 2 << 20), kw.pop("max_items", 24),
                              kw.pop("dsize", (192, 256)), kw.pop("shape", cvgs.BOX_SHAPE_EXPAND), kw.pop("scale", (1.25, 1.25)), kw.pop("pad", (0.0, 0.0)),
                              kw.pop("warp_type", cvgs.WARP_AFFINE), kw.pop("count", None), kw.pop("boxes_out", None), kw.pop("valid", None))


def _host(boxes, count, dsize, shape, scale, pad, warp_type=cvgs.WARP_AFFINE):
    """(table bytes, boxes_out bytes, valid_out bytes) from cvgs_warp_table_from_boxes_host."""
    d = _desc(max_items=len(boxes), dsize=dsize, shape=shape, scale=scale, pad=pad, warp_type=warp_type)
    raw, bo, vo = cvgs.warp_table_from_boxes_host(d, boxes, count)
    return raw, bo.astype("<f4").tobytes(), vo.astype("<i4").tobytes()


def _first_difference(got, want, width):
    g, w = np.frombuffer(got, np.uint8).reshape(-1, width), np.frombuffer(want, np.uint8).reshape(-1, width)
    bad = np.flatnonzero((g != w).any(axis=1))
    return None if bad.size == 0 else (int(bad.size), int(bad[0]), g[bad[0]].tobytes().hex(), w[bad[0]].tobytes().hex())


# ---- the host entry against the independent model, byte for byte ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dsize,scale,pad", K.configs(), ids=["%s-%dx%d-s%g,%g-p%g,%g" % (("stretch", "expand")[c[0]], c[1][0], c[1][1], *c[2], *c[3]) for c in K.configs()])
def test_host_entry_equals_the_model_byte_for_byte(lib, shape, dsize, scale, pad):
    boxes = K.all_boxes()
    got = _host(boxes, None, dsize, shape, scale, pad)
    want = M.model_bytes(FRAME, boxes, None, dsize, shape, scale, pad)
    for name, g, w, width in (("table", got[0], want[0], 64), ("boxes_out", got[1], want[1], 16), ("valid_out", got[2], want[2], 4)):
        d = _first_difference(g, w, width)
        assert d is None, "%s: %d items differ, first %d (box %s):\n got  %s\n want %s" % (name, d[0], d[1], boxes[d[1]].tolist(), d[2], d[3])


def test_the_case_set_holds_what_it_claims():
    """Valid and invalid items of every family, real ties, an overflowing narrowing, and a valid item whose boxes_out overflows."""
    boxes = K.all_boxes()
    assert 440 <= len(boxes) <= 480
    _, rect, valid = M.shape_boxes(boxes, None, (192, 256), M.EXPAND, (1.0, 1.0), (0.0, 0.0))
    at = 0
    for fam, want in ((K.integer_boxes(), "all"), (K.half_pixel_boxes(), "all"), (K.random_boxes(), "all"), (K.outside_boxes(), "all"), (K.tie_boxes(), "all"),
                      (K.degenerate_boxes(), "none"), (K.nonfinite_boxes(), "none"), (K.huge_boxes(), "some")):
        v = valid[at:at + len(fam)]
        assert {"all": v.all(), "none": not v.any(), "some": v.any() and not v.all()}[want], (at, v.tolist())
        at += len(fam)
    assert at == len(boxes)
    # (1e38, 0, 3.4e38, 10) stretched to 1 x 1 at scale 1.25: m0 = 3e38 and m2 = 2.2e38 fit, the right edge 2.2e38 + 1.5e38 does not
    _, rect, valid = M.shape_boxes(boxes, None, (1, 1), M.STRETCH, (1.25, 1.25), (0.0, 0.0))
    assert np.isinf(rect[valid.astype(bool)]).any(), "a valid item whose boxes_out overflows"
    ties = 0
    for shape, dsize, scale, pad in K.configs():
        b = K.tie_boxes().astype(np.float64)
        w1 = (b[:, 2] - b[:, 0]) * np.float64(np.float32(scale[0])) + np.float64(np.float32(pad[0]))
        h1 = (b[:, 3] - b[:, 1]) * np.float64(np.float32(scale[1])) + np.float64(np.float32(pad[1]))
        ties += int((w1 * dsize[1] == h1 * dsize[0]).sum()) if shape == M.EXPAND else 0
    assert ties >= 8, ties


@pytest.mark.parametrize("warp_type", [cvgs.WARP_AFFINE, cvgs.WARP_PERSPECTIVE], ids=["affine", "perspective"])
def test_entry_layout_and_both_read_kinds(lib, warp_type):
    """Every entry carries the frame and the target; the entry is the same for both read kinds; row 2 is 0 0 1; m1 = m3 = 0."""
    boxes = K.all_boxes()
    raw, _, vo = _host(boxes, None, (8, 6), M.EXPAND, (1.25, 1.25), (0.0, 0.0), warp_type)
    assert raw == _host(boxes, None, (8, 6), M.EXPAND, (1.25, 1.25), (0.0, 0.0))[0]
    tab = np.frombuffer(raw, ENTRY)
    assert (tab["data"] == K.FRAME_DATA).all() and (tab["w"] == K.W).all() and (tab["h"] == K.H).all() and (tab["step"] == K.STEP).all()
    assert (tab["dw"] == 8).all() and (tab["dh"] == 6).all()
    assert (tab["m"][:, [1, 3, 6, 7]] == 0).all() and (tab["m"][:, 8] == 1).all()
    valid = np.frombuffer(vo, "<i4").astype(bool)
    assert (tab["m"][~valid] == M.INVALID_M).all() and np.isfinite(tab["m"][valid]).all()


@pytest.mark.parametrize("label,count", K.counts(len(K.all_boxes())), ids=[c[0] for c in K.counts(0)])
def test_count_rule(lib, label, count):
    boxes = K.all_boxes()
    cfg = (M.EXPAND, (192, 256), (1.25, 1.25), (3.5, 3.5))
    got = _host(boxes, count, cfg[1], cfg[0], cfg[2], cfg[3])
    assert got == M.model_bytes(FRAME, boxes, count, cfg[1], cfg[0], cfg[2], cfg[3])
    live = M.live_items(count, len(boxes))
    full = _host(boxes, None, cfg[1], cfg[0], cfg[2], cfg[3])
    inv = M.table_bytes(*FRAME, M.INVALID_M[None], cfg[1])
    assert got[0] == full[0][:64 * live] + inv * (len(boxes) - live)
    assert got[1] == full[1][:16 * live] + bytes(16 * (len(boxes) - live)) and got[2] == full[2][:4 * live] + bytes(4 * (len(boxes) - live))


def test_optional_outputs_of_the_host_entry(lib):
    boxes = K.integer_boxes()
    d = _desc(max_items=len(boxes), dsize=(8, 6))
    bx = np.ascontiguousarray(boxes)
    d.boxes = bx.ctypes.data
    out = (C.c_uint8 * (64 * len(boxes)))()
    capi.check(lib.cvgs_warp_table_from_boxes_host(C.byref(d), out, None, None))
    assert bytes(out) == _host(boxes, None, (8, 6), M.EXPAND, (1.25, 1.25), (0.0, 0.0))[0]


# ---- hand-pinned arithmetic ---------------------------------------------------------------------------------------------------------------
def test_pinned_by_hand():
    """A 30 x 45 box at (10, 5), scale 1.25, target 192 x 256: 37.5 x 56.25; 37.5 * 256 = 9600 < 56.25 * 192 = 10800, so the WIDTH grows to
    10800 / 256 = 42.1875; centre (25, 27.5).  m0 = 42.1875 / 192, m4 = 56.25 / 256, m2 = 25 - 21.09375 + (m0 / 2 - 0.5)."""
    m, rect, valid = M.shape_boxes(np.array([[10, 5, 40, 50]], np.float32), None, (192, 256), M.EXPAND, (1.25, 1.25), (0, 0))
    assert valid[0] == 1
    assert rect[0].tolist() == [25 - 21.09375, 27.5 - 28.125, 25 + 21.09375, 27.5 + 28.125]
    m0, m4 = 42.1875 / 192, 56.25 / 256
    assert m[0].tolist() == [np.float32(m0), 0, np.float32(3.90625 + (m0 * 0.5 - 0.5)), 0, np.float32(m4), np.float32(-0.625 + (m4 * 0.5 - 0.5)), 0, 0, 1]
    # destination centre u samples the source centre (x0 + (u + 0.5) * m0) - 0.5: the first and last columns sit half a step inside the rectangle
    first, last = m[0][2] + 0.5, m[0][0] * 191 + m[0][2] + 0.5
    assert abs(first - (rect[0][0] + m0 / 2)) < 1e-5 and abs(last - (rect[0][2] - m0 / 2)) < 1e-4
    # STRETCH leaves the rectangle of step 3
    _, rect, _ = M.shape_boxes(np.array([[10, 5, 40, 50]], np.float32), None, (192, 256), M.STRETCH, (1.25, 1.25), (0, 0))
    assert rect[0].tolist() == [25 - 18.75, 27.5 - 28.125, 25 + 18.75, 27.5 + 28.125]


# ---- exact pixels through the CPU oracle --------------------------------------------------------------------------------------------------
def _crop_with_zero_border(frame, xa, ya, w, h):
    out = np.zeros((h, w, frame.shape[2]), np.float32)
    for v in range(h):
        for u in range(w):
            if 0 <= ya + v < frame.shape[0] and 0 <= xa + u < frame.shape[1]:
                out[v, u] = frame[ya + v, xa + u]
    return out


@pytest.mark.parametrize("box", [(2, 1, 10, 7), (-3, -2, 5, 4), (8, 4, 16, 12), (-2, -2, 15, 11), (13, 2, 20, 6), (4, 9, 9, 14), (5, 3, 6, 4)],
                         ids=["inside", "top-left", "bottom-right", "larger", "outside-right", "outside-below", "one-pixel"])
def test_integer_box_is_the_pixel_crop_with_a_zero_border(lib, oracle, box):
    """Integer edges, scale 1, pad 0, STRETCH, target = the box's size: m0 = m4 = 1, m2 = xa, m5 = ya exactly, so the warp chain's output is
    frame[ya + v, xa + u] inside the frame and 0 outside.  The chain runs on the CPU oracle over the host entry's matrix."""
    fw, fh = 13, 9
    host = H.random_u8((fh, fw * 3 + 5), seed=3)
    frame = host[:, :fw * 3].reshape(fh, fw, 3)
    mat = cvgs.GpuMat(fh, fw, cvgs.CV_8UC3, host.ctypes.data, host.strides[0], owner=host)
    xa, ya, xb, yb = box
    w, h = xb - xa, yb - ya
    d = cvgs.box_warp_desc(mat, 1 << 20, 2 << 20, 1, (w, h), cvgs.BOX_SHAPE_STRETCH, (1.0, 1.0), (0.0, 0.0))
    raw, bo, vo = cvgs.warp_table_from_boxes_host(d, np.array([box], np.float32))
    m = np.frombuffer(raw, ENTRY)["m"][0]
    assert vo[0] == 1 and m.tolist() == [1, 0, xa, 0, 1, ya, 0, 0, 1] and bo[0].tolist() == list(box)
    rd = cvgs.ReadIOp(capi.READ_WARP_AFFINE, cvgs.CV_8UC3, [mat], None, (w, h), cvgs.IGNORE_AR, None)
    rd.warp, rd.warp_sizes = [float(v) for v in m], None
    out = np.full((3, h, w), -7.0, np.float32)
    oracle.execute(cvgs.lower([rd, cvgs.split_tensor(cvgs.CV_32FC3, out.ctypes.data, w, h, 1)]))
    want = _crop_with_zero_border(frame, xa, ya, w, h).transpose(2, 0, 1)
    assert (out == want).all(), (out, want)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["shrink", "no_centre_term", "clamp_out"])
def test_the_model_is_sensitive_to_each_ruled_out_mistake(lib, variant):
    """Each wrong model differs from the right one -- and so from the host entry -- on at least one case."""
    boxes = K.all_boxes()
    differing = 0
    for shape, dsize, scale, pad in K.configs():
        right = M.model_bytes(FRAME, boxes, None, dsize, shape, scale, pad)
        wrong = M.model_bytes(FRAME, boxes, None, dsize, shape, scale, pad, variant)
        assert _host(boxes, None, dsize, shape, scale, pad) == right
        differing += int(wrong != right)
    assert differing >= 4, (variant, differing)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _set2(d, name, x, y):
    getattr(d, name)[0], getattr(d, name)[1] = x, y


NAN, INF = float("nan"), float("inf")
BAD = [  # (what, descriptor mutation, status, message fragment)
    ("struct_size", lambda d: setattr(d, "struct_size", 104), capi.ERR_INVALID, b"size mismatch"),
    ("flags", lambda d: setattr(d, "flags", 1), capi.ERR_INVALID, b"flags must be 0"),
    ("read kind out of range", lambda d: setattr(d, "read_kind", 9), capi.ERR_INVALID, b"bad read kind"),
    ("pixel reads", lambda d: setattr(d, "read_kind", capi.READ_PIXEL), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("resize reads", lambda d: setattr(d, "read_kind", capi.READ_RESIZE_LINEAR), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("NV12 reads", lambda d: setattr(d, "read_kind", capi.READ_NV12_RESIZE_LINEAR), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("max_items 0", lambda d: setattr(d, "max_items", 0), capi.ERR_INVALID, b"max_items must be in [1, 65535]"),
    ("max_items 65536", lambda d: setattr(d, "max_items", 65536), capi.ERR_INVALID, b"max_items must be in [1, 65535]"),
    ("shape 2", lambda d: setattr(d, "shape", 2), capi.ERR_INVALID, b"bad box shape"),
    ("shape -1", lambda d: setattr(d, "shape", -1), capi.ERR_INVALID, b"bad box shape"),
    ("scale 0", lambda d: _set2(d, "scale", 0.0, 1.0), capi.ERR_INVALID, b"scale (x, y) must be finite and positive"),
    ("scale negative", lambda d: _set2(d, "scale", 1.0, -1.25), capi.ERR_INVALID, b"scale (x, y) must be finite and positive"),
    ("scale NaN", lambda d: _set2(d, "scale", NAN, 1.0), capi.ERR_INVALID, b"scale (x, y) must be finite and positive"),
    ("scale inf", lambda d: _set2(d, "scale", 1.0, INF), capi.ERR_INVALID, b"scale (x, y) must be finite and positive"),
    ("pad negative", lambda d: _set2(d, "pad", -0.5, 0.0), capi.ERR_INVALID, b"pad (x, y) must be finite and not negative"),
    ("pad NaN", lambda d: _set2(d, "pad", 0.0, NAN), capi.ERR_INVALID, b"pad (x, y) must be finite and not negative"),
    ("pad inf", lambda d: _set2(d, "pad", INF, 0.0), capi.ERR_INVALID, b"pad (x, y) must be finite and not negative"),
    ("null boxes", lambda d: setattr(d, "boxes", None), capi.ERR_INVALID, b"boxes is null"),
    ("boxes alignment", lambda d: setattr(d, "boxes", (1 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("count alignment", lambda d: setattr(d, "count", (3 << 20) + 1), capi.ERR_INVALID, b"alignment"),
    ("target 0", lambda d: setattr(d, "dst_width", 0), capi.ERR_INVALID, b"warp target must be positive"),
    ("target negative", lambda d: setattr(d, "dst_height", -4), capi.ERR_INVALID, b"warp target must be positive"),
    ("target too wide", lambda d: setattr(d, "dst_width", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24"),
    ("target too tall", lambda d: setattr(d, "dst_height", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24"),
    ("source type", lambda d: setattr(d, "src_type", capi.make_type(capi.DEPTH_8U, 5)), capi.ERR_INVALID, b"bad source type"),
    ("CV_64F source", lambda d: (setattr(d, "src_type", cvgs.CV_64FC1), setattr(d.frame, "step", 1024)), capi.ERR_UNSUPPORTED, b"CV_64F"),
    ("null frame", lambda d: setattr(d.frame, "data", None), capi.ERR_INVALID, b"empty source plane"),
    ("empty frame", lambda d: setattr(d.frame, "height", 0), capi.ERR_INVALID, b"empty source plane"),
    ("frame too wide", lambda d: (setattr(d.frame, "width", (1 << 24) + 1), setattr(d.frame, "step", 1 << 30)), capi.ERR_UNSUPPORTED, b"2^24 pixels"),
    ("frame too tall", lambda d: setattr(d.frame, "height", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24 pixels"),
    ("step", lambda d: setattr(d.frame, "step", K.W * 3 - 1), capi.ERR_INVALID, b"step smaller than a row"),
    ("uv_offset", lambda d: setattr(d.frame, "uv_offset", 64), capi.ERR_INVALID, b"uv_offset belongs to the NV12 kinds"),
]
BAD_DEVICE_ONLY = [  # cvgs_warp_table_from_boxes_host writes to its own arguments and ignores the descriptor's output pointers
    ("null table", lambda d: setattr(d, "table_out", None), capi.ERR_INVALID, b"table_out is null"),
    ("table alignment", lambda d: setattr(d, "table_out", (2 << 20) + 4), capi.ERR_INVALID, b"alignment"),
    ("boxes_out alignment", lambda d: setattr(d, "boxes_out", (5 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("valid alignment", lambda d: setattr(d, "valid_out", (6 << 20) + 1), capi.ERR_INVALID, b"alignment"),
]


@pytest.mark.parametrize("what,mut,code,msg", BAD + BAD_DEVICE_ONLY, ids=[b[0] for b in BAD + BAD_DEVICE_ONLY])
def test_refusals_device_entry_point(lib, what, mut, code, msg):
    """The pointers are pretend device addresses and the stream is null: a call that got as far as a launch or a dereference would not
    return these codes."""
    d = _desc()
    mut(d)
    arr = (capi.BoxWarpDesc * 1)(d)
    rc = lib.cvgs_warp_tables_from_boxes(arr, 1, None)
    assert rc == code and msg in lib.cvgs_last_error(), (what, rc, lib.cvgs_last_error())
    with pytest.raises(capi.CvgsError):
        cvgs.warp_tables_from_boxes(None, [d])


@pytest.mark.parametrize("what,mut,code,msg", BAD, ids=[b[0] for b in BAD])
def test_refusals_host_entry_point(lib, what, mut, code, msg):
    boxes = np.zeros((24, 4), np.float32)
    cnt = C.c_int32(24)
    out = (C.c_uint8 * (64 * 24))()
    bo = np.full((24, 4), 7.0, np.float32)
    vo = np.full((24,), 7, np.int32)
    d = _desc(boxes=boxes.ctypes.data, count=C.addressof(cnt))
    mut(d)
    rc = lib.cvgs_warp_table_from_boxes_host(C.byref(d), out, bo.ctypes.data, vo.ctypes.data)
    assert rc == code and msg in lib.cvgs_last_error(), (what, rc, lib.cvgs_last_error())
    assert bytes(out) == bytes(64 * 24) and (bo == 7.0).all() and (vo == 7).all()  # nothing was written


def test_null_arguments_n_out_of_range_and_overlap(lib):
    assert lib.cvgs_warp_tables_from_boxes(None, 1, None) == capi.ERR_INVALID and b"null descriptors" in lib.cvgs_last_error()
    assert lib.cvgs_warp_table_from_boxes_host(None, None, None, None) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()
    d = _desc()
    assert lib.cvgs_warp_table_from_boxes_host(C.byref(d), None, None, None) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()
    for n in (0, -1, 17):
        arr = (capi.BoxWarpDesc * 17)(*([_desc(table=(2 << 20) + 4096 * k) for k in range(17)]))
        assert lib.cvgs_warp_tables_from_boxes(arr, n, None) == capi.ERR_INVALID and b"[1, 16]" in lib.cvgs_last_error()
    # the SECOND descriptor of a call is validated like the first
    arr = (capi.BoxWarpDesc * 2)(d, _desc(max_items=0, table=4 << 20))
    assert lib.cvgs_warp_tables_from_boxes(arr, 2, None) == capi.ERR_INVALID and b"max_items" in lib.cvgs_last_error()
    # output buffers of one call that overlap: two tables; a table and another frame's boxes_out; a table and its own valid_out;
    # boxes_out and valid_out of one frame; the last byte of one buffer and the first of the next
    T = 2 << 20
    pairs = [(_desc(), _desc(table=T + 64 * 23)), (_desc(), _desc(table=4 << 20, boxes_out=T + 64)), (_desc(valid=T + 1000), _desc(table=4 << 20)),
             (_desc(boxes_out=6 << 20, valid=(6 << 20) + 16 * 24 - 4), _desc(table=4 << 20)), (_desc(), _desc(table=T + 64 * 24 - 8))]
    for a, b in pairs:
        arr = (capi.BoxWarpDesc * 2)(a, b)
        assert lib.cvgs_warp_tables_from_boxes(arr, 2, None) == capi.ERR_INVALID and b"overlap" in lib.cvgs_last_error(), lib.cvgs_last_error()


def test_layout(lib, tmp_path):
    """A C99 -pedantic -Werror compile of the extension header pins sizeof(cvgs_box_warp_desc); the binding mirrors it."""
    D = capi.BoxWarpDesc
    assert C.sizeof(D) == 112
    assert (D.frame.offset, D.src_type.offset, D.shape.offset, D.scale.offset, D.pad.offset, D.boxes.offset, D.table_out.offset, D.valid_out.offset) == (8, 32, 48, 56, 64, 72, 88, 104)
    src = tmp_path / "ext.c"
    src.write_text('#include <stddef.h>\n#include "include/cvgs_hip_ext.h"\n'
                   'int main(void) { cvgs_box_warp_desc d; d.struct_size = (uint32_t)sizeof d;\n'
                   '  return d.struct_size == 112 && offsetof(cvgs_box_warp_desc, scale) == 56 && offsetof(cvgs_box_warp_desc, boxes) == 72\n'
                   '         && offsetof(cvgs_box_warp_desc, valid_out) == 104 && CVGS_BOX_SHAPE_EXPAND == 1 ? 0 : 1; }\n')
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + ROOT, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_program_compiles():
    """tests/cpp/test_box_warps.cpp (cvGS::DeviceWarps::updateFromBoxes + ChainBatch + recorded ticks) compiles against the facade without a
    GPU; tests/test_zzzzzzzzzzz_gpu_box_warp.py runs it."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", cpp, "bin/test_box_warps"], check=True, stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(cpp, "bin", "test_box_warps"))


# ---- boxes_out as the boxes of the crop builder --------------------------------------------------------------------------------------------
def test_boxes_out_chains_into_the_crop_builders_box_rule(lib):
    """boxes_out is a legal XYXY_F32 box list: under the crop builder's box rule (tests/box_cases.py: floor / ceil after the clamp) a valid
    item whose shaped rectangle meets the frame gives a view inside the frame that holds the clamped source box -- the crop gained the
    margin --, an invalid item's (0, 0, 0, 0) gives the invalid view, and inf from an overflowing narrowing is clamped like any value."""
    boxes = K.all_boxes()
    met = 0
    for shape, dsize, scale, pad in (c for c in K.configs() if c[2][0] >= 1.0):
        d = _desc(max_items=len(boxes), dsize=dsize, shape=shape, scale=scale, pad=pad)
        _, bo, vo = cvgs.warp_table_from_boxes_host(d, boxes)
        assert not np.isnan(bo).any()
        for i, (src, out, ok) in enumerate(zip(boxes, bo, vo)):
            r = B.rect(out, B.XYXY_F32, K.W, K.H)
            if not ok:
                assert out.tolist() == [0, 0, 0, 0] and r is None
                continue
            meets = out[2] > 0 and out[0] < K.W and out[3] > 0 and out[1] < K.H
            assert (r is not None) == bool(meets), (i, out.tolist(), r)
            if r is None:
                continue
            l, t, w, h = r
            assert 0 <= l and 0 <= t and w >= 1 and h >= 1 and l + w <= K.W and t + h <= K.H
            inner = B.rect(src, B.XYXY_F32, K.W, K.H)
            if inner is not None and np.abs(src).max() < 1e6:  # (beyond that the float32 rectangle's own rounding exceeds a pixel)
                assert l <= inner[0] and t <= inner[1] and l + w >= inner[0] + inner[2] and t + h >= inner[1] + inner[3], (i, src.tolist(), r, inner)
                met += 1
    assert met > 3000  # (the containment was checked, not skipped)
