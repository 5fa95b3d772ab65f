"""What the ten detector-side entry points (csrc/cvgs_detect.cpp) refuse, as one deterministic case list, and the answers of the commit
that had them in cvgs_api.cpp: tests/golden/detect_refusals.json (tests/test_detect_refusals.py replays the list and requires equality).

Per stage: the good descriptor of the stage's own CPU test (pretend, non-overlapping addresses: validation dereferences nothing), every
single defect of that test's tables, every unordered pair of them applied together in table order (the pairs pin the ORDER of the checks),
and the defects of the call (null array, n = 0, n = max + 1, two frames sharing their buffers).

No call of this file can reach a launch or a dereference, by construction:
- a device entry point gets [d, guard]: descriptor 0 is checked first, and the guard is refused whenever d is not.  Two guards with two
  texts ("size mismatch", "flags must be 0") tell "d passed its checks" from "d has that defect".  A d that passes (the good descriptor,
  an overlap defect, a pair whose defects cancel) is then sent as [d, d], whose outputs overlap whatever they are; the boxes stage has no
  overlap test, so there the answer is the marker PASSES and nothing more is called.
- a host twin dereferences, so it gets only descriptors whose defects lie in fields it reads; the fields it ignores keep their good values,
  so the device probe above answers with a check both run.  Only if that probe refuses is the twin called; otherwise the answer is PASSES.

Left out of the host twins (asserted by the test): every case with a defect in a field the twin ignores, and the defects of the call.
  cvgs_warp_table_build_host  LEFT_OUT = 67    cvgs_boxes_select_host  LEFT_OUT = 536
  cvgs_head_decode_host       LEFT_OUT = 474   cvgs_points_gather_host LEFT_OUT = 2
cvgs_plane_tables_from_boxes has no twin (cvgs_plane_table_build serves chains and is not part of this file's subject).

The same route records what the four host twins WRITE for twin_cases() (real, small host inputs), which tests/cpp/detect_asan.cpp
compares with what cvgs_detect.cpp writes into heap buffers of exactly the contract's size.

Record:  python -m tests.detect_refusal_cases --record tests/golden/detect_refusals.json   (in a tree whose library is the one to record)"""
import base64
import ctypes as C
import hashlib
import itertools
import json
import os
import sys
import zlib

from cvgpuspeedup_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_refusals.json")
PASSES = (0, "PASSES: not called any further")
LEFT_OUT = {"cvgs_warp_table_build_host": 67, "cvgs_boxes_select_host": 536, "cvgs_head_decode_host": 474, "cvgs_points_gather_host": 2}
FAR = 0x7000000  # pretend outputs of a host twin, never reached


class Defect:
    def __init__(self, name, apply, fields):
        self.name, self.apply, self.fields = name, apply, fields  # fields: the descriptor fields set (None: found by Stage)


def _field_defects(rows):
    out = []
    for f, v, _ in rows:
        if callable(f):
            out.append(Defect("xform:%s" % v, f, ("xform",)))
        else:
            out.append(Defect("%s=%s" % (f, v), (lambda d, f=f, v=v: setattr(d, f, v)), (f,)))
    return out


def _xform_defects(rows):
    def put(i, v):
        def apply(d):
            d.xform[i] = v
        return apply
    return [Defect("xform[%d]=%s" % (i, v), put(i, v), ("xform",)) for i, v in rows]


class Stage:
    def __init__(self, entry, desc_type, good, defects, max_frames, out_fields, ignored=(), twin=None, twin_args=None):
        self.entry, self.desc_type, self.good, self.defects, self.max_frames = entry, desc_type, good, defects, max_frames
        self.out_fields, self.ignored, self.twin, self.twin_args = out_fields, set(ignored), twin, twin_args
        self.has_overlap_test = bool(out_fields)
        for x in defects:  # a defect given as a function: the fields it sets are those whose bytes it changes in the good descriptor
            if x.fields is None:
                a, b = good(), good()
                x.apply(b)
                at = lambda d, f: bytes(d)[getattr(desc_type, f).offset:getattr(desc_type, f).offset + getattr(desc_type, f).size]
                x.fields = tuple(f[0] for f in desc_type._fields_ if at(a, f[0]) != at(b, f[0]))
                assert x.fields, x.name


def stages():
    from tests import test_box_select as TS
    from tests import test_boxes as TB
    from tests import test_head_decode as TH
    from tests import test_point_gather as TG
    from tests import test_warp_points as TW
    lam = lambda rows, fields=None: [Defect(r[0], r[1], fields) for r in rows]
    boxes = Stage("cvgs_plane_tables_from_boxes", capi.BoxTableDesc, TB._desc, lam(TB.BAD), capi.MAX_CHAINS, ())
    boxes_nv = Stage("cvgs_plane_tables_from_boxes", capi.BoxTableDesc, lambda: TB._desc(frame=TB._nv12(), **TB.NV), lam(TB.BAD_NV12) + lam(TB.BAD), capi.MAX_CHAINS, ())
    boxes_nv.tag = "nv12"
    warp = Stage("cvgs_warp_tables_from_points", capi.WarpTableDesc, TW._desc, lam(TW.BAD) + lam(TW.BAD_DEVICE_ONLY), 16, ("table_out",),
                 ("table_out",), "cvgs_warp_table_build_host", lambda d: (C.byref(d), FAR))
    sel_out = ("scratch", "boxes_out", "count_out", "scores_out", "index_out")
    frame = [Defect("frame_width=2^24+1", lambda d: setattr(d, "frame_width", (1 << 24) + 1), ("frame_width",)),
             Defect("frame_height=2^24+1", lambda d: setattr(d, "frame_height", (1 << 24) + 1), ("frame_height",))]
    xf = _xform_defects([(0, 0.0), (0, -1.0), (0, TS.INF), (0, TS.NAN), (1, 0.0), (1, TS.INF), (1, TS.NAN), (2, TS.INF), (2, TS.NAN), (3, -TS.INF), (3, TS.NAN)])
    select = Stage("cvgs_boxes_select", capi.BoxSelectDesc, TS._good_desc, _field_defects(TS.REFUSALS) + frame + xf, 16, sel_out, sel_out,
                   "cvgs_boxes_select_host", lambda d: (C.byref(d), FAR, FAR + 0x100000, None, None))
    head_out = ("scratch", "boxes_out", "scores_out", "classes_out", "index_out", "count_out")
    head = Stage("cvgs_head_decode", capi.HeadDesc, TH._good_desc, _field_defects(TH.REFUSALS), 16, head_out, head_out,
                 "cvgs_head_decode_host", lambda d: (C.byref(d), FAR, FAR + 0x100000, FAR + 0x200000, None, FAR + 0x300000))
    gather = Stage("cvgs_points_gather", capi.PointGatherDesc, TG._good_desc, _field_defects(TG.REFUSALS), 16, ("points_out", "conf_out", "source_out"), (),
                   "cvgs_points_gather_host", lambda d: (C.byref(d), d.points_out, d.conf_out, d.source_out))  # the twin's outputs are arguments: the descriptor's
    return [boxes, boxes_nv, warp, select, head, gather]


def _combos(stage):
    """[(id, [defects])]: none, every single one, every unordered pair in table order."""
    idx = range(len(stage.defects))
    sets = [()] + [(i,) for i in idx] + list(itertools.combinations(idx, 2))
    tag = getattr(stage, "tag", "")
    return [("%s%s[%s]" % (stage.entry, ":" + tag if tag else "", " + ".join("%d:%s" % (i, stage.defects[i].name) for i in s)), [stage.defects[i] for i in s]) for s in sets]


def _build(stage, defects):
    d = stage.good()
    for x in defects:
        x.apply(d)
    return d


def _answer(lib, rc):
    return (int(rc), lib.cvgs_last_error().decode("utf-8", "replace") if rc else "")


def _call(lib, stage, descs, n=None):
    arr = (stage.desc_type * len(descs))(*descs)
    return _answer(lib, getattr(lib, stage.entry)(arr, len(descs) if n is None else n, None))


def _probe(lib, stage, d):
    """The answer of d's own checks, or None if d passes them: [d, guard] with two guards."""
    g1, g2 = stage.good(), stage.good()
    g1.struct_size, g2.flags = 0, 1
    a, b = _call(lib, stage, [d, g1]), _call(lib, stage, [d, g2])
    assert a[0] and b[0], "a guarded call was accepted"
    return a if a == b else None


def cases():
    """[(id, entry, function lib -> (code, text))], in a fixed order."""
    out = []
    for st in stages():
        def device(lib, st=st, defects=None):
            d = _build(st, defects)
            a = _probe(lib, st, d)
            if a is not None:
                return a
            return _call(lib, st, [d, d]) if st.has_overlap_test else PASSES
        for cid, defects in _combos(st):
            out.append((cid, st.entry, lambda lib, f=device, x=defects: f(lib, defects=x)))
        if getattr(st, "tag", ""):
            continue
        g = st.good()
        out.append((st.entry + "[null array]", st.entry, lambda lib, st=st: _answer(lib, getattr(lib, st.entry)(None, 1, None))))
        out.append((st.entry + "[n=0]", st.entry, lambda lib, st=st, g=g: _call(lib, st, [g], n=0)))
        out.append((st.entry + "[n=max+1]", st.entry, lambda lib, st=st, g=g: _call(lib, st, [g] * (st.max_frames + 1))))
        if st.twin:
            def twin(lib, st=st, defects=None):
                d = _build(st, defects)
                if _probe(lib, st, d) is None:
                    return PASSES
                return _answer(lib, getattr(lib, st.twin)(*st.twin_args(d)))
            for cid, defects in _combos(st):
                if any(set(x.fields) & st.ignored for x in defects):
                    continue
                out.append((cid.replace(st.entry, st.twin, 1), st.twin, lambda lib, f=twin, x=defects: f(lib, defects=x)))
            out.append((st.twin + "[null descriptor]", st.twin, lambda lib, st=st, g=g: _answer(lib, getattr(lib, st.twin)(*((None,) + tuple(st.twin_args(g))[1:])))))
    return out


def left_out(all_cases):
    """Per twin: the cases of its device entry point that it does not get."""
    n = {}
    for _, entry, _ in all_cases:
        n[entry] = n.get(entry, 0) + 1
    return {st.twin: n[st.entry] - n[st.twin] for st in stages() if st.twin}


def ids_digest(all_cases):
    return hashlib.sha256("\n".join(c[0] for c in all_cases).encode()).hexdigest()


def replay(lib, all_cases):
    return [run(lib) for _, _, run in all_cases]


# ---- the host twins' outputs: inputs for tests/cpp/detect_asan.cpp, the bytes the recorded library writes for them ------------------------
WARP_FRAME = (61, 97, 4096, 304)  # rows, cols, pretend data address, step of the CV_8UC3 frame detect_asan.cpp describes too
WARP_DSIZE = (112, 96)
SELECT_FRAME, XFORM = (640, 480), (1.5, 0.75, 2.0, -3.0)


def _bits(v):
    import numpy as np
    return int(np.float32(v).view(np.uint32))


def twin_cases():
    """[(stage, [int parameters], [input arrays], function -> [output arrays or None])]: the smallest shapes that reach every branch of
    the four host twins.  One line of detect_asan.cpp's case file each: twin_line()."""
    import numpy as np
    from cvgpuspeedup_amd import cvgs
    rng = np.random.RandomState(20261021)
    out = []
    for n_cand, max_out in ((1, 3), (4, 3), (4, 2)):  # pre_nms_k 3: 0, 1 and pre_nms_k + 1 live candidates
        for count in (None, 0, 1, -5, 70000):
            boxes = (rng.rand(n_cand, 4) * (300, 300, 90, 90) + (60, 60, 10, 10)).astype(np.float32)
            scores, classes = (0.2 + 0.8 * rng.rand(n_cand)).astype(np.float32), (np.arange(n_cand) % 2).astype(np.int32)
            d = cvgs.box_select_desc(SELECT_FRAME, None, None, n_cand, None, None, None, 0.25, 0.5, 3, max_out, cvgs.CAND_CXCYWH_F32, xform=XFORM)

            def run(d=d, a=(boxes, scores, classes, count)):
                bo, k, so, io = cvgs.boxes_select_host(d, *a)
                return [bo, np.array([k], np.int32), so, io]
            ints = [n_cand, 3, max_out, count is not None, count or 0, _bits(0.25), _bits(0.5)] + [_bits(v) for v in XFORM]
            out.append(("select", ints, [boxes, scores, classes], run))
    for n in (1, 257):
        for elem in (cvgs.HEAD_F32, cvgs.HEAD_F16, cvgs.HEAD_BF16):
            for row in (True, False):
                raw = rng.rand(n, 8).astype(np.float32) if row else rng.rand(8, n).astype(np.float32)  # box, objectness, three classes
                raw = raw if elem == cvgs.HEAD_F32 else raw.astype(np.float16) if elem == cvgs.HEAD_F16 else (raw.view(np.uint32) >> 16).astype(np.uint16)
                cs, at = (8, 1) if row else (1, n)
                d = cvgs.head_desc(None, elem, n, cs, at, 3, 0.25, None, None, None, None, None, None, 0, 5, 4)

                def run(d=d, raw=raw):
                    bo, so, ko, io, k = cvgs.head_decode_host(d, raw)
                    return [bo, so, ko, io, np.array([k], np.int32)]
                out.append(("head", [n, elem, cs, at, 0, 4, 5, 3, _bits(0.25)], [raw], run))
    for n_points in (1, 64):
        for conf in (False, True):
            for kept_count in (None, -1, 9, 2):
                step = 3 if conf else 2
                attrs = 5 + n_points * step
                raw = (rng.rand(9, attrs) * 640).astype(np.float32)
                kept, cand = np.array([0, 3, 12, 8], np.int32), np.array([8, 7, 6, -1, 4, 3, 2, 1, 0], np.int32)
                d = cvgs.point_gather_desc(None, cvgs.HEAD_F32, 9, attrs, 1, 5, step, n_points, 4, None, None, xform=XFORM, conf_offset=2 if conf else -1)

                def run(d=d, a=(raw, kept, kept_count, cand)):
                    return list(cvgs.points_gather_host(d, *a))
                ints = [9, attrs, 1, 5, step, n_points, 2 if conf else -1, 4, kept_count is not None, kept_count or 0] + [_bits(v) for v in XFORM]
                out.append(("gather", ints, [raw, kept, cand], run))
    tmpl5 = np.array([[38.25, 51.5], [73.5, 51.5], [56.0, 71.75], [41.5, 92.25], [70.75, 92.25]], np.float32)
    for fit, tmpl in ((cvgs.WARP_FIT_SIMILARITY, tmpl5), (cvgs.WARP_FIT_AFFINE3, tmpl5[:3])):
        for count in (None, -1, 6, 3):  # max_items 5
            pts = (2.0 * tmpl[None] + (30.0, 11.0) + rng.rand(5, len(tmpl), 2)).astype(np.float32)
            pts[4] = pts[4, 0]  # an item whose landmarks coincide: not valid
            frame = cvgs.GpuMat(WARP_FRAME[0], WARP_FRAME[1], cvgs.CV_8UC3, WARP_FRAME[2], WARP_FRAME[3])
            d = cvgs.warp_table_desc(frame, None, None, 5, WARP_DSIZE, tmpl.tolist(), fit, cvgs.WARP_AFFINE)

            def run(d=d, a=(pts, count)):
                table, valid = cvgs.build_warp_table_host(d, *a)
                return [np.frombuffer(table, np.uint8), np.array(valid, np.int32)]
            out.append(("warp", [fit, len(tmpl), 5, count is not None, count or 0], [tmpl, pts], run))
    return out


def twin_line(case, outputs_hex):
    hexes = lambda arrays: " ".join("-" if a is None else a.tobytes().hex() for a in arrays)
    return "%s %s # %s # %s" % (case[0], " ".join(str(int(v)) for v in case[1]), hexes(case[2]), " ".join(outputs_hex))


def twin_outputs():
    """What the loaded library's twins write, as hex per output ('-': an output that is not asked for)."""
    return [["-" if a is None else a.tobytes().hex() for a in case[3]()] for case in twin_cases()]


def recorded_twin_outputs(doc):
    return json.loads(zlib.decompress(base64.b64decode(doc["twin_outputs_zlib_b64"])))


def record(path):
    lib = capi.load_library()
    all_cases = cases()
    answers = replay(lib, all_cases)
    texts = sorted({a for a in answers})
    where = {a: i for i, a in enumerate(texts)}
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc.update({"cases": len(all_cases), "ids_sha256": ids_digest(all_cases), "answers": [list(t) for t in texts], "case_answer": [where[a] for a in answers],
                "twin_outputs_zlib_b64": base64.b64encode(zlib.compress(json.dumps(twin_outputs()).encode(), 9)).decode()})
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d distinct answers -> %s; left out of the twins: %s" % (len(all_cases), len(texts), path, left_out(all_cases)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        record(sys.argv[2])
    else:
        sys.exit(__doc__)
