"""cvgs_head_decode without a GPU (include/cvgs_hip_ext.h: THE CONTRACT): cvgs_head_decode_host against an independent numpy model byte
for byte, written-out edge cases with their expected values, degenerate member counts and tails, composition with
cvgs_boxes_select_host, the validation table, the C++ facade's descriptor bytes, and the shared text in a stand-alone program under
AddressSanitizer + UBSan.  The kernels are held to the host entry in tests/test_zzzzzz_gpu_head_decode.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import head_cases as HC
from tests import head_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def seeded():
    return HC.seeded_cases()


# ---- the host entry against the model -----------------------------------------------------------------------------------------------------
def test_host_entry_equals_the_model_byte_for_byte(lib, seeded):
    """30 seeded cases: three element types x five layouts ([N, A], [A, N], padded rows, padded channels, every second element) x
    objectness on and off, C in {1, 2, 80}, four thresholds (-inf among them)."""
    assert hasattr(lib, "cvgs_head_decode_host")
    assert len(seeded) == 30
    assert {c.num_classes for c in seeded} == {1, 2, 80} and {c.elem for c in seeded} == {M.F32, M.F16, M.BF16}
    assert {(c.layout, c.obj_attr >= 0) for c in seeded} == {(l, o) for l in HC.LAYOUTS for o in (False, True)}
    members = 0
    for k, c in enumerate(seeded):
        got, want = c.host(), c.model()
        assert HC.same(got, want), "case %d (%s, elem %d, C %d): count %d / %d" % (k, c.layout, c.elem, c.num_classes, got[4], want[4])
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()  # no NaN is ever stored
        members += got[4]
    assert 30 * 4 < members < sum(c.n for c in seeded)


def test_every_fp16_and_bf16_pattern_widens_as_the_model_says(lib):
    """All 65536 bit patterns of both 16-bit types through the host entry (one class, threshold -inf, so every candidate is a member and
    every non-NaN score is stored as read): fp16 subnormals, both zeros and both infinities included."""
    bits = np.arange(65536, dtype=np.uint16)
    for elem in (M.F16, M.BF16):
        raw = np.zeros((65535, 5), np.uint16)  # [N, 4 + 1]: box 0, one class score
        for chunk in (bits[:65535], bits[1:]):
            raw[:, 4] = chunk
            d = cvgs.head_desc(None, elem, 65535, 5, 1, 1, -INF, None, None, None, None, None)
            bo, so, ko, io, k = cvgs.head_decode_host(d, raw)
            w = M.widen(chunk, elem)
            want = np.where(np.isnan(w), np.float32(-INF), w)  # (a NaN never wins: the score stays -inf, which passes the threshold -inf)
            assert k == 65535 and (so.view(np.uint32) == want.view(np.uint32)).all() and (io == np.arange(65535)).all() and not ko.any()


# ---- written-out cases --------------------------------------------------------------------------------------------------------------------
def _rows(rows, num_classes, thr, obj=False, elem=M.F32, layout="NA"):
    """Candidates written out as [x, y, w, h, (obj,) class scores...]."""
    return HC.Case(np.asarray(rows, np.float32), elem, layout, num_classes, thr, obj)


BOX = [10, 20, 30, 40]


@pytest.mark.parametrize("layout", ["NA", "AN"])
def test_ties_zeros_and_nan_class_scores(lib, layout):
    c = _rows([BOX + [0.5, 0.75, 0.75, 0.25],     # a tie across classes: the lower index
               BOX + [0.75, 0.5, 0.75, 0.75],     # ... also when the tie includes the first class
               BOX + [-0.0, 0.0, -1.0, -2.0],     # -0.0 equals +0.0: class 0, and the score keeps the winner's sign bit
               BOX + [0.0, -0.0, -1.0, -2.0],
               BOX + [NAN, 0.5, 0.25, NAN],       # a NaN never wins
               BOX + [0.25, NAN, 0.875, 0.5],     # ... beside a larger finite score
               BOX + [-INF, -INF, -INF, -INF],    # -inf never beats the starting value: class 0
               BOX + [NAN, -INF, NAN, -INF]], 4, -INF, layout=layout)
    bo, so, ko, io, k = c.host()
    assert k == 8 and io.tolist() == list(range(8))
    assert ko.tolist() == [1, 0, 0, 0, 1, 2, 0, 0]
    assert so.view(np.uint32).tolist() == np.array([0.75, 0.75, -0.0, 0.0, 0.5, 0.875, -INF, -INF], np.float32).view(np.uint32).tolist()
    assert (bo == np.array(BOX, np.float32)).all()
    assert HC.same((bo, so, ko, io, k), c.model())


def test_all_class_scores_nan(lib):
    rows = [BOX + [NAN, NAN, NAN], BOX + [0.5, 0.25, 0.125]]
    bo, so, ko, io, k = _rows(rows, 3, -INF).host()          # threshold -inf: member, score -inf, class 0
    assert k == 2 and so[0] == -INF and ko[0] == 0 and io.tolist() == [0, 1]
    bo, so, ko, io, k = _rows(rows, 3, -1e30).host()         # a finite threshold: not a member
    assert k == 1 and io.tolist() == [1, -1] and so.tolist() == [0.5, 0.0] and ko.tolist() == [0, 0] and not bo[1].any()


def test_objectness(lib):
    c = _rows([BOX + [0.5, 0.25, 0.75],           # 0.5 * 0.75
               BOX + [NAN, 0.25, 0.75],           # NaN objectness: not a member, even at threshold -inf
               BOX + [0.0, INF, 0.5],             # inf * 0 = NaN: not a member
               BOX + [INF, 0.25, 0.5],            # inf * 0.5 = inf
               BOX + [-1.0, NAN, NAN],            # -1 * -inf = +inf
               BOX + [0.1, 0.3, 0.7]], 2, -INF, obj=True)  # one multiplication, rounded once
    bo, so, ko, io, k = c.host()
    assert k == 4 and io.tolist() == [0, 3, 4, 5, -1, -1] and ko.tolist() == [1, 1, 0, 1, 0, 0]
    assert so[:4].view(np.uint32).tolist() == np.array([0.375, INF, INF, np.float32(0.1) * np.float32(0.7)], np.float32).view(np.uint32).tolist()
    assert HC.same((bo, so, ko, io, k), c.model())


def test_nan_coordinates_and_infinite_ones(lib):
    rows = [[NAN, 20, 30, 40, 0.9], [10, NAN, 30, 40, 0.9], [10, 20, NAN, 40, 0.9], [10, 20, 30, NAN, 0.9], [-INF, 20, INF, 40, 0.9], BOX + [0.9]]
    bo, so, ko, io, k = _rows(rows, 1, -INF).host()
    assert k == 2 and io.tolist() == [4, 5, -1, -1, -1, -1] and bo[0].tolist() == [-INF, 20, INF, 40] and not np.isnan(bo).any()


def test_fp16_subnormals_and_bf16_truncation(lib):
    sub = np.array([0x0001, 0x03ff, 0x8001, 0x0400], np.uint16).view(np.float16)  # 2^-24, the largest subnormal, -2^-24, the smallest normal
    raw = np.zeros((4, 5), np.float16)
    raw[:, :4] = BOX
    raw[:, 4] = sub
    d = cvgs.head_desc(None, M.F16, 4, 5, 1, 1, 0.0, None, None, None, None, None)
    bo, so, ko, io, k = cvgs.head_decode_host(d, raw)
    assert k == 3 and io.tolist() == [0, 1, 3, -1]
    assert so[:3].tolist() == [2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14] and (bo[:3] == np.array(BOX, np.float32)).all()
    braw = np.zeros((2, 5), np.uint16)
    braw[:, 4] = [0x3f40, 0x3e80]  # 0.75, 0.25
    braw[:, :4] = 0x4120           # 10.0
    d = cvgs.head_desc(None, M.BF16, 2, 5, 1, 1, 0.5, None, None, None, None, None)
    bo, so, ko, io, k = cvgs.head_decode_host(d, braw)
    assert k == 1 and so.tolist() == [0.75, 0.0] and bo[0].tolist() == [10.0] * 4


# ---- degenerate member counts and the tails ------------------------------------------------------------------------------------------------
def test_no_members_all_members_and_the_tails(lib):
    c = HC.make(7, 300, 3, thr=2.0, dirty=False)
    bo, so, ko, io, k = c.host()
    assert k == 0 and not bo.view(np.uint32).any() and not so.view(np.uint32).any() and not ko.any() and (io == -1).all()
    c = HC.make(7, 300, 3, thr=-INF, dirty=False)
    bo, so, ko, io, k = c.host()
    coords, score, cls = c.dense()
    assert k == 300 and io.tolist() == list(range(300)) and (bo == coords).all() and (so == score).all() and (ko == cls).all()
    # the tails over a poisoned buffer, nothing beyond N, and the optional index output
    c = HC.make(8, 64, 3, thr=0.25, hot=0.2, dirty=False)
    d = capi.HeadDesc.from_buffer_copy(c.desc())
    d.head = c.raw.ctypes.data
    bo, so = np.full((66, 4), np.float32(-77.0)), np.full((66,), np.float32(-77.0))
    ko, io = np.full((66,), 12345, np.int32), np.full((66,), 12345, np.int32)
    co = C.c_int32(999)
    capi.check(lib.cvgs_head_decode_host(C.byref(d), bo[1:].ctypes.data, so[1:].ctypes.data, ko[1:].ctypes.data, io[1:].ctypes.data, C.addressof(co)))
    k = co.value
    assert 0 < k < 64 and not bo[1 + k:65].view(np.uint32).any() and not so[1 + k:65].view(np.uint32).any() and not ko[1 + k:65].any() and (io[1 + k:65] == -1).all()
    assert (bo[0] == -77).all() and (bo[65] == -77).all() and so[0] == so[65] == -77 and ko[0] == ko[65] == io[0] == io[65] == 12345
    capi.check(lib.cvgs_head_decode_host(C.byref(d), bo[1:].ctypes.data, so[1:].ctypes.data, ko[1:].ctypes.data, None, C.addressof(co)))
    assert co.value == k


# ---- composition with cvgs_boxes_select -----------------------------------------------------------------------------------------------------
def test_select_over_the_decoders_outputs_equals_select_over_the_dense_arrays(lib, seeded):
    """cvgs_boxes_select_host over (boxes_out, scores_out, classes_out, count_out) and over the model's dense per-candidate arrays, same
    threshold: identical boxes, scores and count; the index arrays are related through the decoder's index_out."""
    kept_total = 0
    for c in seeded[::2] + [HC.make(90, 900, 80, M.BF16, "AN", hot=0.3)]:
        thr = max(c.thr, -1e30)
        bo, so, ko, io, k = c.host()
        coords, score, cls = c.dense()

        def select(boxes, scores, classes, count):
            d = cvgs.box_select_desc((640, 640), None, None, c.n, None, None, None, thr, 0.5, 256, 64, cvgs.CAND_CXCYWH_F32, count=None)
            return cvgs.boxes_select_host(d, boxes, scores, classes, count)
        # (the decoder ran with c.thr; with thr = -inf select's own threshold -1e30 drops the -inf scores on both sides alike)
        a = select(bo, so, ko, k)
        b = select(coords, score, cls, None)
        assert a[1] == b[1] and (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[2].view(np.uint32) == b[2].view(np.uint32)).all()
        assert (io[a[3][:a[1]]] == b[3][:b[1]]).all() and (a[3][a[1]:] == -1).all()
        kept_total += a[1]
    assert kept_total > 16 * 3


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
def _good_desc():
    """A descriptor that passes with pretend device addresses (validation dereferences nothing); the buffers do not overlap."""
    return cvgs.head_desc(0x10000, cvgs.HEAD_BF16, 8400, 1, 8400, 80, 0.25, 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000)


def _refused(lib, descs, n=None, msg=b""):
    arr = (capi.HeadDesc * len(descs))(*descs)
    rc = lib.cvgs_head_decode(arr, len(descs) if n is None else n, None)
    assert rc == capi.ERR_INVALID, (rc, lib.cvgs_last_error())
    assert msg in lib.cvgs_last_error(), lib.cvgs_last_error()


REFUSALS = [  # (field, value, message)
    ("struct_size", 8, b"size mismatch"),
    ("flags", 1, b"flags must be 0"),
    ("reserved", 1, b"reserved must be 0"),
    ("elem_type", 3, b"bad elem_type"),
    ("elem_type", -1, b"bad elem_type"),
    ("max_candidates", 0, b"max_candidates must be in [1, 65535]"),
    ("max_candidates", 65536, b"max_candidates must be in [1, 65535]"),
    ("head", None, b"head is null"),
    ("cand_stride", 0, b"cand_stride must be at least 1"),
    ("attr_stride", 0, b"attr_stride must be at least 1"),
    ("attr_stride", -8400, b"attr_stride must be at least 1"),
    ("num_classes", 0, b"num_classes must be in [1, 4096]"),
    ("num_classes", 4097, b"num_classes must be in [1, 4096]"),
    ("box_attr", -1, b"box_attr"),
    ("box_attr", 8189, b"box_attr"),
    ("obj_attr", -2, b"obj_attr"),
    ("obj_attr", 8192, b"obj_attr"),
    ("class_attr", -1, b"class_attr"),
    ("class_attr", 8192 - 79, b"class_attr"),
    ("score_threshold", NAN, b"score_threshold is NaN"),
    ("scratch", None, b"scratch is null"),
    ("boxes_out", None, b"boxes_out is null"),
    ("scores_out", None, b"scores_out is null"),
    ("classes_out", None, b"classes_out is null"),
    ("count_out", None, b"count_out is null"),
    ("head", 0x10001, b"alignment of its element type"),
    ("scratch", 0x100004, b"scratch needs 8-byte"),
    ("boxes_out", 0x200002, b"scratch needs 8-byte"),
    ("scores_out", 0x300001, b"scratch needs 8-byte"),
    ("classes_out", 0x400002, b"scratch needs 8-byte"),
    ("index_out", 0x600003, b"scratch needs 8-byte"),
    ("count_out", 0x500002, b"scratch needs 8-byte"),
    # overlaps inside one descriptor: scratch is 1024 + 8 * 8400 bytes, boxes_out 134400, the other arrays 33600
    ("boxes_out", 0x100000 + 68000, b"overlap"),
    ("scores_out", 0x200000 + 134396, b"overlap"),
    ("classes_out", 0x300000 + 33596, b"overlap"),
    ("index_out", 0x400000 + 33596, b"overlap"),
    ("count_out", 0x600000 + 33596, b"overlap"),
]


def test_struct_scratch_size_and_the_host_entrys_checks(lib):
    d = _good_desc()
    assert C.sizeof(capi.HeadDesc) == 104
    assert lib.cvgs_head_decode_scratch_bytes(8400) == 1024 + 8 * 8400 and lib.cvgs_head_decode_scratch_bytes(1) == 1032
    assert lib.cvgs_head_decode_scratch_bytes(65535) == 1024 + 8 * 65535
    for bad in (0, -1, 65536):
        assert lib.cvgs_head_decode_scratch_bytes(bad) == 0 and cvgs.head_decode_scratch_bytes(bad) == 0
    d.struct_size = 8  # the host entry takes the same descriptor and runs the same checks
    assert lib.cvgs_head_decode_host(C.byref(d), 8, 8, 8, None, 8) == capi.ERR_INVALID and b"size mismatch" in lib.cvgs_last_error()
    e = _good_desc()
    e.score_threshold = -INF  # allowed; 0x10000 + 2 is aligned for a 16-bit head but not for fp32
    e.head = 0x10002
    e.elem_type = cvgs.HEAD_F32
    _refused(lib, [e], msg=b"alignment of its element type")


@pytest.mark.parametrize("field,value,msg", REFUSALS, ids=["%s=%s" % (f, v) for f, v, _ in REFUSALS])
def test_refusals(lib, field, value, msg):
    d = _good_desc()
    setattr(d, field, value)
    _refused(lib, [d], msg=msg)


def test_refusals_of_the_call(lib):
    d = _good_desc()
    assert lib.cvgs_head_decode(None, 1, None) == capi.ERR_INVALID and b"null descriptors" in lib.cvgs_last_error()
    _refused(lib, [d], n=0, msg=b"n must be in [1, 16]")
    many = []
    for k in range(17):
        e = _good_desc()
        for f in ("scratch", "boxes_out", "scores_out", "classes_out", "index_out", "count_out"):
            setattr(e, f, getattr(e, f) + k * 0x1000000)
        many.append(e)
    _refused(lib, many, msg=b"n must be in [1, 16]")
    _refused(lib, [d, _good_desc()], msg=b"overlap")  # two frames of one call share their buffers
    for args in ((None, 8, 8, 8, None, 8), (C.byref(d), None, 8, 8, None, 8), (C.byref(d), 8, None, 8, None, 8), (C.byref(d), 8, 8, None, None, 8),
                 (C.byref(d), 8, 8, 8, None, None)):
        assert lib.cvgs_head_decode_host(*args) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()


# ---- the C++ facade and the shared text -----------------------------------------------------------------------------------------------------
def test_facade_lowers_to_the_same_descriptor_bytes():
    """cvGS::DeviceHeadDecode (tests/cpp/headdecode_desc.cpp) compiles against the facade without a GPU and describes a call with the
    bytes the Python binding writes for the same arguments; feed() describes the selector the binding describes."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CPP, "bin/headdecode_desc"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CPP, "bin", "headdecode_desc")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines())
    assert got["desc"] == bytes(_good_desc()).hex()
    rows = cvgs.head_desc(0x10000, cvgs.HEAD_F32, 1000, 10, 1, 3, 0.5, 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, None, 2, 7, 6)
    assert got["rows"] == bytes(rows).hex()
    sel = cvgs.box_select_desc((1920, 1080), 0x200000, 0x300000, 8400, 0x700000, 0x800000, 0x800400, 0.25, 0.5, 1024, 50, cvgs.CAND_CXCYWH_F32, 4, 1,
                               0x400000, 1, 0x500000)
    assert got["select"] == bytes(sel).hex()


def test_extension_header_with_the_head_struct_is_plain_c99(tmp_path):
    src = tmp_path / "ext.c"
    src.write_text('#include "include/cvgs_hip_ext.h"\n'
                   'int main(void) { cvgs_head_desc d; d.struct_size = (uint32_t)sizeof d; return d.struct_size == 104 ? 0 : 1; }\n')
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + ROOT, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_shared_head_text_under_sanitizers(lib, seeded, tmp_path):
    """tests/cpp/head_text_asan.cpp: the text the kernels and the host entry share (csrc/cvgs_geometry.h), compiled into a stand-alone
    program with -fsanitize=address,undefined and the engine's -ffp-contract=off, driven the way the kernels drive it (groups of lanes and
    a butterfly for the best class, tile counts, the prefix over tiles, packed positions and tails into buffers of exactly N slots) over
    the seeded cases and two larger ones: equal to the host entry, no report."""
    exe = tmp_path / "head_text_asan"
    cxx = next(shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c))
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
             "-Werror"]
    if "clang" not in os.path.basename(cxx):  # gcc: the sanitizers' runtimes inside the program, as clang links them (nothing to load first)
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + [os.path.join(CPP, "head_text_asan.cpp"), "-o", str(exe)], check=True)
    cases = seeded + [HC.make(61, 1300, 80, M.F16, "AN", hot=0.5), HC.make(62, 1025, 257, M.F32, "NA", obj=True, thr=-INF)]
    path = tmp_path / "cases.txt"
    HC.text_file(cases, str(path))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "%d cases, 0 bad" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
