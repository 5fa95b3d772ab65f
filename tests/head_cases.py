"""Seeded detector heads for cvgs_head_decode (tests/test_head_decode.py on the CPU, tests/test_zzzzzz_gpu_head_decode.py on the GPU).

A Case holds the head's storage as the library reads it -- float32, float16, or uint16 holding bfloat16 bits, in one of the layouts
below -- with the strides and attribute indices that describe it, and gives the [N, A] view the model takes.  Class scores are multiples
of 1 / 64 (exact in all three types, so ties occur), most of them below the threshold; a sprinkle of values is NaN / infinite / -0.0.

  layouts   "NA"  [N, A]: (A, 1)            "NA_pad"  rows padded by 3 elements: (A + 3, 1)       "NA_x2"  every second element: (2 A, 2)
            "AN"  [A, N]: (1, N)            "AN_pad"  channels padded by 5 elements: (1, N + 5)
"""
import numpy as np

from cvgpuspeedup_amd import cvgs
from tests import head_model as M

LAYOUTS = ("NA", "AN", "NA_pad", "AN_pad", "NA_x2")
STORAGE = {M.F32: np.float32, M.F16: np.float16, M.BF16: np.uint16}


def to_storage(values, elem):
    """float32 values -> the head's element type (bfloat16 by truncation: the model and the library both read what is stored)."""
    values = np.asarray(values, np.float32)
    if elem == M.F32:
        return values.copy()
    if elem == M.F16:
        with np.errstate(all="ignore"):
            return values.astype(np.float16)
    return (values.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


class Case:
    def __init__(self, values, elem, layout, num_classes, thr, obj, lead=0):
        """values: float32 [N, A] with A = lead + 4 + (1 if obj) + num_classes: `lead` unused attributes, the box, the objectness, the classes."""
        self.n, self.a = values.shape
        self.elem, self.layout, self.num_classes, self.thr = elem, layout, num_classes, thr
        self.box_attr, self.obj_attr, self.class_attr = lead, (lead + 4 if obj else -1), lead + 4 + (1 if obj else 0)
        assert self.a == self.class_attr + num_classes
        n, a = self.n, self.a
        st = to_storage(values, elem)
        if layout in ("NA", "NA_pad"):
            self.cand_stride, self.attr_stride = a + (3 if layout == "NA_pad" else 0), 1
            self.raw = to_storage(np.full((n, self.cand_stride), np.nan, np.float32), elem)  # (padding: NaN bits, never read)
            self.raw[:, :a] = st
        elif layout == "NA_x2":
            self.cand_stride, self.attr_stride = 2 * a, 2
            self.raw = to_storage(np.full((n, 2 * a), np.nan, np.float32), elem)
            self.raw[:, ::2] = st
        else:
            self.cand_stride, self.attr_stride = 1, n + (5 if layout == "AN_pad" else 0)
            self.raw = to_storage(np.full((a, self.attr_stride), np.nan, np.float32), elem)
            self.raw[:, :n] = st.T
        self.raw = np.ascontiguousarray(self.raw)

    def view(self):
        """The [N, A] view of the storage through the two strides."""
        isz = self.raw.itemsize
        return np.lib.stride_tricks.as_strided(self.raw.reshape(-1), (self.n, self.a), (self.cand_stride * isz, self.attr_stride * isz), writeable=False)

    def desc(self, **ptrs):
        """The descriptor without addresses (cvgs.head_decode_host fills the head in), or with the device ones given."""
        return cvgs.head_desc(ptrs.get("head"), self.elem, self.n, self.cand_stride, self.attr_stride, self.num_classes, self.thr, ptrs.get("scratch"),
                              ptrs.get("boxes_out"), ptrs.get("scores_out"), ptrs.get("classes_out"), ptrs.get("count_out"), ptrs.get("index_out"),
                              self.box_attr, self.class_attr, self.obj_attr)

    def host(self):
        """cvgs_head_decode_host on this case: (boxes_out, scores_out, classes_out, index_out, count)."""
        return cvgs.head_decode_host(self.desc(), self.raw)

    def model(self):
        return M.decode(self.view(), self.elem, self.box_attr, self.obj_attr, self.class_attr, self.num_classes, self.thr)

    def dense(self):
        return M.dense(self.view(), self.elem, self.box_attr, self.obj_attr, self.class_attr, self.num_classes)


def same(a, b):
    """Byte equality of two result tuples."""
    return ((a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2] == b[2]).all()
            and (a[3] == b[3]).all() and a[4] == b[4])


def values(seed, n, num_classes, obj=False, lead=0, hot=0.04, dirty=True, extent=640.0):
    """float32 [N, A]: boxes (cx, cy, w, h) inside `extent`, class scores k / 64 -- below 0.25 except for a fraction `hot` of the candidates,
    whose winning class is drawn uniformly -- and objectness k / 16."""
    rng = np.random.default_rng(seed)
    a = lead + 4 + (1 if obj else 0) + num_classes
    v = np.zeros((n, a), np.float32)
    v[:, :lead] = rng.uniform(-1, 1, (n, lead))
    v[:, lead:lead + 2] = rng.uniform(0, extent, (n, 2))
    v[:, lead + 2:lead + 4] = rng.uniform(extent / 40, extent / 4, (n, 2))
    c0 = lead + 4 + (1 if obj else 0)
    v[:, c0:] = rng.integers(0, 12, (n, num_classes)) / 64.0
    is_hot = rng.uniform(0, 1, n) < hot
    win = rng.integers(0, num_classes, n)
    level = rng.integers(20, 65, n) / 64.0
    rows = np.flatnonzero(is_hot)
    v[rows, c0 + win[rows]] = level[rows]
    tie = rows[::3]  # a third of the hot candidates carry their top score twice
    v[tie, c0 + (win[tie] + 1 + rng.integers(0, num_classes, len(tie))) % num_classes] = level[tie]
    if obj:
        v[:, lead + 4] = rng.integers(4, 17, n) / 16.0
    if dirty and n >= 40:
        pick = rng.permutation(n)
        v[pick[0], lead] = np.nan                       # a NaN coordinate under a hot score
        v[pick[0], c0] = 1.0
        v[pick[1], c0 + num_classes - 1] = np.nan       # a NaN class score
        v[pick[2], c0:] = np.nan                        # every class score NaN
        v[pick[3], c0] = np.inf
        v[pick[4], c0:] = -0.0
        v[pick[5], lead + 3] = np.inf                   # an infinite size passes through
        v[pick[5], c0 + num_classes // 2] = 0.875
        if obj:
            v[pick[6], lead + 4] = np.nan
            v[pick[6], c0] = 1.0
            v[pick[3], lead + 4] = 0.0                  # inf * 0
            v[pick[7], lead + 4] = -0.0
    return v


def make(seed, n=300, num_classes=3, elem=M.F32, layout="NA", obj=False, thr=0.25, lead=0, hot=0.04, dirty=True):
    return Case(values(seed, n, num_classes, obj, lead, hot, dirty), elem, layout, num_classes, thr, obj, lead)


def seeded_cases():
    """The cases the host entry, the model and the stand-alone text program all run: every element type x layout x objectness, C in
    {1, 2, 80}, N around the tile, three thresholds."""
    out = []
    seed = 500
    for elem in (M.F32, M.F16, M.BF16):
        for layout in LAYOUTS:
            for obj in (False, True):
                seed += 1
                out.append(make(seed, (260, 517, 97)[seed % 3] + seed % 5, (1, 2, 80)[(seed // 2) % 3], elem, layout, obj, thr=(0.25, 0.5, -np.inf, 0.0)[seed % 4],
                                lead=(0, 2)[seed % 2], hot=(0.04, 0.3)[seed % 2]))
    return out


def text_file(cases, path):
    """The cases, widened by the MODEL, and the host entry's outputs for tests/cpp/head_text_asan.cpp: unsigned integers, floats as bit
    patterns.  (The program drives step 2 onwards; the element types' widening is held to the model by the host-entry comparison.)"""
    lines = [str(len(cases))]
    for c in cases:
        w = M.widen(c.view(), c.elem).view(np.uint32)
        lines.append(" ".join(str(v) for v in (c.n, c.a, c.box_attr, c.obj_attr + 1, c.class_attr, c.num_classes, int(np.float32(c.thr).view(np.uint32)))))
        lines.extend(" ".join(str(v) for v in row) for row in w)
        bo, so, ko, io, k = c.host()
        lines.append(str(k))
        bu, su, iu = bo.view(np.uint32), so.view(np.uint32), io.view(np.uint32)
        lines.extend("%d %d %d %d %d %d %d" % (bu[j, 0], bu[j, 1], bu[j, 2], bu[j, 3], su[j], ko[j], iu[j]) for j in range(c.n))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
