"""cvgs_boxes_select without a GPU (include/cvgs_hip_ext.h: THE CONTRACT): the validation table, cvgs_boxes_select_host against an
independent fp32 restatement byte for byte and against an exact float64 model, the properties of a greedy NMS, ties, the edge cases,
letterbox_xform against the plane table, the C++ facade's descriptor bytes, and the shared selection text in a stand-alone program under
AddressSanitizer + UBSan.  The kernels are held to the host entry in tests/test_zzzzz_gpu_box_select.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import select_cases as SC
from tests import select_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


# ---- validation ------------------------------------------------------------------------------------------------------------------------
def _good_desc():
    """A descriptor that passes with pretend device addresses (validation dereferences nothing); the buffers do not overlap."""
    return cvgs.box_select_desc((1920, 1080), 0x10000, 0x40000, 8400, 0x100000, 0x200000, 0x210000, 0.25, 0.5, 1024, 50, classes=0x60000, count=0x80000,
                                scores_out=0x220000, index_out=0x230000)


def _refused(lib, descs, n=None, code=capi.ERR_INVALID, msg=b""):
    arr = (capi.BoxSelectDesc * len(descs))(*descs)
    rc = lib.cvgs_boxes_select(arr, len(descs) if n is None else n, None)
    assert rc == code, (rc, lib.cvgs_last_error())
    assert msg in lib.cvgs_last_error(), lib.cvgs_last_error()


NAN, INF = float("nan"), float("inf")
REFUSALS = [  # (field, value, message)
    ("struct_size", 8, b"size mismatch"),
    ("flags", 1, b"flags must be 0"),
    ("frame_width", 0, b"frame_width / frame_height must be positive"),
    ("frame_height", -3, b"frame_width / frame_height must be positive"),
    ("box_format", 2, b"bad box format"),
    ("max_candidates", 0, b"max_candidates must be in [1, 65535]"),
    ("max_candidates", 65536, b"max_candidates must be in [1, 65535]"),
    ("boxes", None, b"boxes is null"),
    ("scores", None, b"scores is null"),
    ("box_stride", 3, b"box_stride must be at least 4"),
    ("score_stride", 0, b"score_stride must be at least 1"),
    ("class_stride", 0, b"class_stride must be at least 1"),
    ("pre_nms_k", 0, b"pre_nms_k must be in [1, 1024]"),
    ("pre_nms_k", 1025, b"pre_nms_k must be in [1, 1024]"),
    ("max_out", 0, b"max_out must be in [1, pre_nms_k]"),
    ("max_out", 1025, b"max_out must be in [1, pre_nms_k]"),
    ("reserved", 1, b"reserved must be 0"),
    ("score_threshold", NAN, b"score_threshold is NaN"),
    ("iou_threshold", NAN, b"iou_threshold must be in [0, 1]"),
    ("iou_threshold", -0.01, b"iou_threshold must be in [0, 1]"),
    ("iou_threshold", 1.01, b"iou_threshold must be in [0, 1]"),
    ("scratch", None, b"scratch is null"),
    ("boxes_out", None, b"boxes_out is null"),
    ("count_out", None, b"count_out is null"),
    ("boxes", 0x10002, b"4-byte alignment"),
    ("scores", 0x40001, b"4-byte alignment"),
    ("classes", 0x60002, b"4-byte alignment"),
    ("count", 0x80003, b"4-byte alignment"),
    ("scratch", 0x100004, b"scratch needs 8-byte"),
    ("boxes_out", 0x200002, b"scratch needs 8-byte"),
    ("count_out", 0x210001, b"scratch needs 8-byte"),
    ("scores_out", 0x220002, b"scratch needs 8-byte"),
    ("index_out", 0x230002, b"scratch needs 8-byte"),
    # overlaps inside one descriptor: scratch is 8 + 7 * 4 * 1024 bytes, boxes_out 800, scores_out / index_out 200
    ("boxes_out", 0x100000 + 28000, b"overlap"),
    ("count_out", 0x200000 + 796, b"overlap"),
    ("scores_out", 0x200000 + 400, b"overlap"),
    ("index_out", 0x220000 + 196, b"overlap"),
]


def test_struct_scratch_size_and_the_host_entrys_checks(lib):
    """The layout the binding mirrors, the scratch size, and the host entry running the same checks.  (The table below changes ONE field
    of _good_desc() at a time; the unchanged descriptor is never passed to cvgs_boxes_select: its addresses are pretend ones.)"""
    d = _good_desc()
    assert C.sizeof(capi.BoxSelectDesc) == 144
    assert lib.cvgs_boxes_select_scratch_bytes(8400, 1024) == 8 + 28 * 1024
    assert lib.cvgs_boxes_select_scratch_bytes(8400, 1) == 8 + 32  # rounded up to 8
    for bad in ((0, 10), (65536, 10), (10, 0), (10, 1025)):
        assert lib.cvgs_boxes_select_scratch_bytes(*bad) == 0
    # the host entry takes the same descriptor and runs the same checks (input pointers are the only ones it uses)
    c = SC.make(1, 50)
    assert c.host()[1] >= 1
    d.struct_size = 8
    assert lib.cvgs_boxes_select_host(C.byref(d), 1, 1, None, None) == capi.ERR_INVALID and b"size mismatch" in lib.cvgs_last_error()


@pytest.mark.parametrize("field,value,msg", REFUSALS, ids=["%s=%s" % (f, v) for f, v, _ in REFUSALS])
def test_refusals(lib, field, value, msg):
    d = _good_desc()
    setattr(d, field, value)
    _refused(lib, [d], msg=msg)


@pytest.mark.parametrize("slot,value", [(0, 0.0), (0, -1.0), (0, INF), (0, NAN), (1, 0.0), (1, INF), (1, NAN), (2, INF), (2, NAN), (3, -INF), (3, NAN)])
def test_refusals_of_the_transform(lib, slot, value):
    d = _good_desc()
    d.xform[slot] = value
    _refused(lib, [d], msg=b"xform scales (sx, sy) must be finite and positive" if slot < 2 else b"xform offsets (ox, oy) must be finite")


def test_refusals_of_the_call(lib):
    d = _good_desc()
    assert lib.cvgs_boxes_select(None, 1, None) == capi.ERR_INVALID and b"null descriptors" in lib.cvgs_last_error()
    _refused(lib, [d], n=0, msg=b"n must be in [1, 16]")
    many = []
    for k in range(17):
        e = _good_desc()
        for f in ("scratch", "boxes_out", "count_out", "scores_out", "index_out"):
            setattr(e, f, getattr(e, f) + k * 0x1000000)
        many.append(e)
    _refused(lib, many, msg=b"n must be in [1, 16]")
    _refused(lib, [d, _good_desc()], msg=b"overlap")  # two frames of one call share their buffers
    e = _good_desc()
    e.frame_width = (1 << 24) + 1
    _refused(lib, [e], code=capi.ERR_UNSUPPORTED, msg=b"wider or taller than 2^24")
    e = _good_desc()
    e.frame_height = (1 << 24) + 1
    _refused(lib, [e], code=capi.ERR_UNSUPPORTED, msg=b"wider or taller than 2^24")
    assert lib.cvgs_boxes_select_host(None, 1, 1, None, None) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()
    assert lib.cvgs_boxes_select_host(C.byref(d), None, 1, None, None) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()


# ---- the host entry against the two models ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    return SC.seeded_cases()


def test_host_entry_equals_the_restatement_byte_for_byte(lib, seeded):
    """24 seeded cases: both formats, dense and interleaved [n, 6] heads read in place, classes on and off, three transforms, three counts."""
    assert len(seeded) == 24
    total_kept = dropped = 0
    for k, c in enumerate(seeded):
        got, want = c.host(), c.model()
        assert SC.same(got, want), "case %d: kept %d / %d\n%s\n%s" % (k, got[1], want[1], got[3], want[3])
        total_kept += got[1]
        dropped += int((np.asarray(c.scores[:M.live_count(c.count, c.n)]) >= c.p.score_thr).sum()) - got[1]
    assert total_kept > 24 * 8 and dropped > 24 * 20  # suppression and the threshold both had work to do


@pytest.mark.parametrize("iou_thr", [0.25, 0.5, 0.75])
def test_host_entry_equals_the_exact_model_on_integer_boxes(lib, iou_thr):
    """Integer coordinates in a 4096 x 4096 frame, identity transform, thresholds k / 4: every operation of step 7 is exact in fp32 --
    iw, ih <= 2^12 and inter, area, uni <= 2^25 are integers, fp32 holds integers up to 2^24 exactly and those beyond are reached here only
    as sums / products whose value is a multiple of a power of two it can hold (checked below: every inter, uni and thr * uni of every pair
    round-trips through float32) -- so inter > thr * uni decides what inter / uni > thr decides and no case needs excluding."""
    kept = 0
    for seed in range(6):
        c = SC.make(700 + seed, 220, W=4096, H=4096, iou_thr=iou_thr, integer=True, dirty=False, with_classes=seed % 2 == 1, pre_k=256, max_out=256)
        b = np.clip(np.asarray(c.boxes, np.float64), 0, 4096)
        assert (b == np.round(b)).all()
        iw = np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])
        ih = np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        uni = area[:, None] + area[None, :] - inter
        for v in (inter, area, area[:, None] + area[None, :], uni, iou_thr * uni):
            assert (v.astype(np.float32).astype(np.float64) == v).all()
        got, want = c.host(), c.model(f64=True)
        assert SC.same(got, want), (seed, got[1], want[1])
        assert SC.same(got, c.model())
        kept += got[1]
    assert kept > 6 * 10


def _check_properties(c, res):
    """Kept boxes do not suppress each other; every dropped member is beyond pre_k, beyond max_out, or suppressed by an earlier kept one."""
    p = c.p
    bo, kept, so, io = res
    members = [(i, M.prepare32(p, c.boxes[i], c.scores[i])) for i in range(M.live_count(c.count, c.n))]
    members = [(i, b) for i, b in members if b is not None]
    members.sort(key=lambda m: -float(c.scores[m[0]]))
    order = {i: r for r, (i, _) in enumerate(members)}
    box = dict(members)
    kept_idx = [int(v) for v in io[:kept]]
    assert all(v == -1 for v in io[kept:]) and not bo[kept:].any() and not so[kept:].view(np.uint32).any()
    assert [order[i] for i in kept_idx] == sorted(order[i] for i in kept_idx)  # kept in the order of step 6
    same_class = lambda i, j: c.classes is None or c.classes[i] == c.classes[j]
    for a in range(kept):
        assert tuple(bo[a]) == box[kept_idx[a]] and so[a] == c.scores[kept_idx[a]]
        for b in range(a):
            assert not (same_class(kept_idx[a], kept_idx[b]) and M.suppresses32(box[kept_idx[b]], box[kept_idx[a]], p.iou_thr))
    last = order[kept_idx[-1]] if kept else -1
    for i, b in members:
        if i in kept_idx or order[i] >= p.pre_k:
            continue
        by = [j for j in kept_idx if order[j] < order[i] and same_class(i, j) and M.suppresses32(box[j], b, p.iou_thr)]
        assert by or (kept == p.max_out and order[i] > last), "member %d was dropped without a reason" % i


def test_properties_of_the_selection(lib, seeded):
    for c in seeded[::3]:
        _check_properties(c, c.host())
    c = SC.make(31, 400, pre_k=40, max_out=8, score_thr=0.1)  # both limits bind
    res = c.host()
    assert res[1] == 8
    _check_properties(c, res)


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def _simple(boxes, scores, classes=None, count=None, **kw):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32)
    classes = None if classes is None else np.asarray(classes, np.int32)
    kw = dict(dict(W=100, H=100, score_thr=0.5, iou_thr=0.5, pre_k=16, max_out=4), **kw)
    return SC.Case(M.params(**kw), boxes, scores, classes, count)


def test_ties_resolve_by_index(lib):
    far = [[10 * k, 0, 10 * k + 5, 5] for k in range(8)]  # disjoint boxes: nothing is suppressed
    c = _simple(far, [0.75] * 8, max_out=8)
    assert c.host()[3].tolist() == list(range(8))
    c = _simple(far, [0.75, 0.875, 0.75, 0.875, -0.0, 0.0, 0.75, 0.875], score_thr=-1.0, max_out=8)
    assert c.host()[3].tolist() == [1, 3, 7, 0, 2, 6, 4, 5]  # -0.0 == 0.0: by index
    # overlapping equal boxes with equal scores: the lowest index survives
    c = _simple([[0, 0, 10, 10]] * 5, [0.75] * 5)
    bo, kept, so, io = c.host()
    assert kept == 1 and io.tolist() == [0, -1, -1, -1]
    # the pre_nms_k cut falls inside a tie: the lower indices make the working list
    c = _simple(far, [0.75] * 8, pre_k=3, max_out=3)
    assert c.host()[3].tolist() == [0, 1, 2]


def test_nan_and_infinite_candidates(lib):
    nan, inf = np.nan, np.inf
    boxes = [[0, 0, 10, 10], [nan, 0, 10, 10], [20, 20, 30, nan], [40, 40, 50, 50], [-inf, -inf, inf, inf], [60, 60, inf, 70]]
    c = _simple(boxes, [0.9, 0.95, 0.96, nan, 0.6, inf], iou_thr=0.9, max_out=6)
    bo, kept, so, io = c.host()
    assert io.tolist() == [5, 0, 4, -1, -1, -1] and kept == 3
    assert bo[0].tolist() == [60, 60, 100, 70] and bo[2].tolist() == [0, 0, 100, 100] and so[0] == inf
    assert SC.same((bo, kept, so, io), c.model())
    # CXCYWH: an infinite size gives inf - inf = NaN in step 3, which the clamp pins to +0
    c = _simple([[50, 50, inf, 20], [inf, 50, inf, 20]], [0.9, 0.8], fmt=M.CXCYWH)
    bo, kept, so, io = c.host()
    assert kept == 1 and bo[0].tolist() == [0, 40, 100, 60]      # box 0: (-inf, inf) clamped
    assert SC.same((bo, kept, so, io), c.model())                # box 1: xa = NaN -> 0, xb = inf -> 100, suppressed by box 0


@pytest.mark.parametrize("count,kept", [(0, 0), (-7, 0), (1, 1), (3, 3), (4, 4), (99, 4), (None, 4)])
def test_count_is_clamped(lib, count, kept):
    far = [[10 * k, 0, 10 * k + 5, 5] for k in range(4)]
    c = _simple(far, [0.9, 0.8, 0.7, 0.6], count=count)
    res = c.host()
    assert res[1] == kept and res[3].tolist() == list(range(kept)) + [-1] * (4 - kept)
    assert SC.same(res, c.model())


def test_all_suppressed_nothing_passes_max_out_one_and_the_early_stop(lib):
    big = [[0, 0, 100, 100]] + [[k, k, 99, 99] for k in range(1, 9)]
    c = _simple(big, [0.99] + [0.9] * 8, iou_thr=0.5)
    assert c.host()[1] == 1 and c.host()[3].tolist() == [0, -1, -1, -1]  # all suppressed by the first
    c = _simple(big, [0.4] * 9)
    bo, kept, so, io = c.host()
    assert kept == 0 and not bo.any() and not so.any() and (io == -1).all()  # nothing passes the threshold
    far = [[10 * k, 0, 10 * k + 5, 5] for k in range(8)]
    c = _simple(far, [0.6, 0.7, 0.8, 0.9, 0.95, 0.65, 0.75, 0.85], max_out=1, pre_k=1)
    assert c.host()[1] == 1 and c.host()[3].tolist() == [4]
    c = _simple(far, [0.6, 0.7, 0.8, 0.9, 0.95, 0.65, 0.75, 0.85], max_out=3)  # the walk stops at three of eight
    assert c.host()[3].tolist() == [4, 3, 7]
    # classes: equal boxes of different classes do not suppress each other
    c = _simple([[0, 0, 10, 10]] * 4, [0.9, 0.8, 0.7, 0.6], classes=[1, 2, 1, 3])
    assert c.host()[3].tolist() == [0, 1, 3, -1]


def test_tails_are_rewritten_over_a_poisoned_buffer(lib):
    c = _simple([[0, 0, 10, 10], [50, 50, 60, 60]], [0.9, 0.8], max_out=8, pre_k=8)
    d = capi.BoxSelectDesc.from_buffer_copy(c.desc())
    d.boxes, d.scores = c.boxes.ctypes.data, c.scores.ctypes.data
    bo = np.full((10, 4), np.float32(-77.0))
    so = np.full((10,), np.float32(-77.0))
    io = np.full((10,), 12345, np.int32)
    co = C.c_int32(999)
    capi.check(lib.cvgs_boxes_select_host(C.byref(d), bo[1:].ctypes.data, C.addressof(co), so[1:].ctypes.data, io[1:].ctypes.data))
    assert co.value == 2 and io[1:9].tolist() == [0, 1] + [-1] * 6 and not bo[3:9].any() and not so[3:9].any()
    assert (bo[0] == -77).all() and (bo[9] == -77).all() and so[0] == so[9] == -77 and io[0] == io[9] == 12345  # nothing beyond max_out
    capi.check(lib.cvgs_boxes_select_host(C.byref(d), bo[1:].ctypes.data, C.addressof(co), None, None))     # the optional outputs


# ---- letterbox_xform ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", [cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])
def test_letterbox_xform_is_the_plane_tables_geometry(lib, ar):
    """sx, sy ARE the fx, fy cvgs.build_plane_table writes for the whole-frame chain, and the offsets send the window's first pixel
    (x1, y1) to source 0: the kernels read destination pixel x at (x - x1) * fx."""
    for frame, det in (((1920, 1080), (640, 640)), ((1080, 1920), (640, 640)), ((1279, 721), (416, 320)), ((640, 640), (640, 640))):
        dummy = np.zeros(16, np.uint8)
        whole = cvgs.GpuMat(frame[1], frame[0], cvgs.CV_8UC3, dummy.ctypes.data, frame[0] * 3, owner=dummy)
        raw = np.frombuffer(cvgs.build_plane_table(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [whole], det, 1, None, ar)), np.uint8)
        fx, fy = raw[20:28].view(np.float32)
        x1, y1, x2, y2 = raw[28:44].view(np.int32)
        sx, sy, ox, oy = (np.float32(v) for v in cvgs.letterbox_xform(frame, det, ar))
        assert (sx, sy) == (fx, fy)
        assert ox == -(np.float32(x1) * fx) and oy == -(np.float32(y1) * fy)
        if ar == cvgs.IGNORE_AR:
            assert (x1, y1, x2, y2) == (0, 0, det[0] - 1, det[1] - 1) and ox == 0 and oy == 0
        elif frame != det:
            assert (x1 > 0 or y1 > 0) == (ar != cvgs.PRESERVE_AR_LEFT or y1 > 0)
        # the window maps onto the frame: its left edge to 0, its right edge (x2 + 1) to the frame's width within a pixel of rounding
        assert np.float32(x1) * sx + ox == 0 and abs(float(np.float32(x2 + 1) * sx + ox) - frame[0]) <= max(float(sx), 1.0)
        assert np.float32(y1) * sy + oy == 0 and abs(float(np.float32(y2 + 1) * sy + oy) - frame[1]) <= max(float(sy), 1.0)
        # and the descriptor takes it
        d = _good_desc()
        for k, v in enumerate((sx, sy, ox, oy)):
            d.xform[k] = v
        assert bytes(d)[88:104] == np.array([sx, sy, ox, oy], np.float32).tobytes()


# ---- the C++ facade and the shared text -----------------------------------------------------------------------------------------------------
def test_facade_lowers_to_the_same_descriptor_bytes():
    """cvGS::DeviceBoxSelect (tests/cpp/boxselect_desc.cpp) compiles against the facade without a GPU and describes a call with the bytes
    the Python binding writes for the same arguments."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CPP, "bin/boxselect_desc"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CPP, "bin", "boxselect_desc")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines())
    d = cvgs.box_select_desc((1920, 1080), 0x10000, 0x10010, 8400, 0x20000, 0x30000, 0x30400, 0.25, 0.5, 1024, 50, cvgs.CAND_CXCYWH_F32, 6, 6, 0x10014, 6,
                             0x40000, (3.0, 3.0, 0.0, -420.0), 0x30800, 0x30c00)
    assert got["desc"] == bytes(d).hex()
    p = cvgs.box_select_desc((640, 480), 0x10000, 0x18000, 1000, 0x20000, 0x30000, 0x30400, 0.5, 0.45, 300, 300)
    assert got["plain"] == bytes(p).hex()


def test_extension_header_with_the_selection_struct_is_plain_c99(tmp_path):
    src = tmp_path / "ext.c"
    src.write_text('#include "include/cvgs_hip_ext.h"\n'
                   'int main(void) { cvgs_box_select_desc d; d.struct_size = (uint32_t)sizeof d; return d.struct_size == 144 ? 0 : 1; }\n')
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + ROOT, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_shared_selection_text_under_sanitizers(lib, seeded, tmp_path):
    """tests/cpp/select_text_asan.cpp: the text the kernels and the host entry share (csrc/cvgs_geometry.h), compiled into a stand-alone
    program with -fsanitize=address,undefined and the engine's -ffp-contract=off, driven the way the kernels drive it (ranks by counting,
    working list of exactly pre_k slots, kept list of exactly max_out slots) over the seeded cases: equal to the host entry, no report."""
    exe = tmp_path / "select_text_asan"
    cxx = next(shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c))
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
             "-Werror"]
    if "clang" not in os.path.basename(cxx):  # gcc: the sanitizers' runtimes inside the program, as clang links them (nothing to load first)
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + [os.path.join(CPP, "select_text_asan.cpp"), "-o", str(exe)], check=True)
    cases = seeded + [SC.make(55, 700, pre_k=1024, max_out=1024, score_thr=0.0, iou_thr=0.9), SC.make(56, 64, pre_k=1, max_out=1)]
    path = tmp_path / "cases.txt"
    SC.text_file(cases, str(path))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
