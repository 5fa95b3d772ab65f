"""Seeded landmark heads and kept lists for cvgs_points_gather (tests/test_point_gather.py on the CPU,
tests/test_zzzzzzzzz_gpu_point_gather.py on the GPU).

A Case holds the head's storage as the library reads it -- float32, float16, or uint16 holding bfloat16 bits, in one of the layouts of
tests/head_cases.py -- whose candidates carry `lead` unused attributes, a box, a score and n_points landmarks of point_step attributes
each (x, y and, with a confidence, one more at conf_offset), and the index lists a decode + select pair would leave behind:

  cand_index  (optional) decode's index_out: ascending raw indices of `members` candidates, -1 behind them
  kept_index  select's index_out: distinct indices into the compacted list (or raw ones without cand_index), -1 behind the kept rows
  kept_count  None, or any int32 (the library clamps it)

Hostile entries sit INSIDE the live range: -1, max_candidates, INT32_MAX and INT32_MIN in kept_index and in the cand_index slots kept
rows point at, and a kept index that points behind decode's count (a stale row).  The landmarks of kept candidates include NaN, +-inf,
-0.0 and fp16 subnormals.
"""
import numpy as np

from cvgpuspeedup_amd import cvgs
from tests import head_cases as HC
from tests import point_gather_model as M

LAYOUTS = ("NA", "AN", "NA_pad", "AN_pad")
STEPS = ((2, -1), (3, -1), (3, 2), (4, 3))  # (point_step, conf_offset)
N_POINTS = (1, 2, 5, 16, 17, 64)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
# (sx, sy, ox, oy): the identity; powers of two with integer offsets (exact on integer landmarks); and scales / offsets under which the
# float32 product is inexact, so that multiply-then-add differs from a fused product-sum (tests/test_point_gather.py asserts that it does)
XFORMS = ((1.0, 1.0, 0.0, 0.0), (2.0, 0.5, 3.0, -7.0), (1.6180340051651, 0.7071067690849304, 13.369999885559082, -4.199999809265137))
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 2.0 ** -24, 1023 * 2.0 ** -24, -(2.0 ** -24))


def lay_out(values, elem, layout):
    """float32 [N, A] -> (storage, cand_stride, attr_stride); padding holds NaN bits and is never read."""
    n, a = values.shape
    st = HC.to_storage(values, elem)
    if layout in ("NA", "NA_pad"):
        cs, as_ = a + (3 if layout == "NA_pad" else 0), 1
        raw = HC.to_storage(np.full((n, cs), np.nan, np.float32), elem)
        raw[:, :a] = st
    else:
        cs, as_ = 1, n + (5 if layout == "AN_pad" else 0)
        raw = HC.to_storage(np.full((a, as_), np.nan, np.float32), elem)
        raw[:, :n] = st.T
    return np.ascontiguousarray(raw), cs, as_


class Case:
    def __init__(self, values, elem, layout, lead, n_points, step, conf_offset, max_out, kept_index, kept_count=None, cand_index=None, xform=XFORMS[0]):
        self.n, self.a = values.shape
        self.elem, self.layout, self.n_points, self.point_step, self.conf_offset = elem, layout, n_points, step, conf_offset
        self.point_attr = lead + 5
        assert self.a >= self.point_attr + n_points * step
        self.max_out, self.kept_count, self.xform = max_out, kept_count, tuple(float(np.float32(v)) for v in xform)
        self.kept_index = np.ascontiguousarray(kept_index, np.int32)
        self.cand_index = None if cand_index is None else np.ascontiguousarray(cand_index, np.int32)
        assert self.kept_index.shape == (max_out,) and (self.cand_index is None or self.cand_index.shape == (self.n,))
        self.raw, self.cand_stride, self.attr_stride = lay_out(values, elem, layout)

    @property
    def items(self):
        return self.max_out * self.n_points

    def view(self):
        """The [N, A] view of the storage through the two strides."""
        isz = self.raw.itemsize
        return np.lib.stride_tricks.as_strided(self.raw.reshape(-1), (self.n, self.a), (self.cand_stride * isz, self.attr_stride * isz), writeable=False)

    def desc(self, **ptrs):
        """The descriptor without addresses (cvgs.points_gather_host fills the inputs in), or with the device ones given."""
        return cvgs.point_gather_desc(ptrs.get("head"), self.elem, self.n, self.cand_stride, self.attr_stride, self.point_attr, self.point_step,
                                      self.n_points, self.max_out, ptrs.get("kept_index"), ptrs.get("points_out"), ptrs.get("kept_count"),
                                      ptrs.get("cand_index"), self.xform, self.conf_offset, ptrs.get("conf_out"), ptrs.get("source_out"))

    def host(self):
        """cvgs_points_gather_host on this case: (points, conf or None, source)."""
        return cvgs.points_gather_host(self.desc(), self.raw, self.kept_index, self.kept_count, self.cand_index)

    def model(self):
        return M.gather(self.view(), self.elem, self.point_attr, self.point_step, self.n_points, self.conf_offset, self.max_out, self.kept_index,
                        self.kept_count, self.cand_index, self.xform)


def same(got, want):
    """Byte equality of a (points, conf, source) result with another, or with the model's bit arrays."""
    def bits(a):
        return None if a is None else np.ascontiguousarray(a).view(np.uint32)
    return ((bits(got[0]) == bits(want[0])).all() and (got[1] is None) == (want[1] is None) and (got[1] is None or (bits(got[1]) == bits(want[1])).all())
            and (np.asarray(got[2], np.int32) == np.asarray(want[2], np.int32)).all())


def make(seed, n=120, n_points=5, elem=M.F32, layout="NA", step=2, conf_offset=-1, max_out=8, kept_count="kept", with_cand=True, lead=0, xform=XFORMS[2],
         hostile=True, special=True, integer=False):
    """One seeded case.  kept_count: "kept" = the number of kept rows, or any value for the descriptor (None: no count)."""
    rng = np.random.default_rng(seed)
    a = lead + 5 + n_points * step + seed % 2  # (an unused trailing attribute on odd seeds)
    v = rng.uniform(-20.0, 660.0, (n, a)).astype(np.float32)
    if integer:  # exact in all three element types
        v = rng.integers(-20, 251, (n, a)).astype(np.float32)
    v[:, lead + 4] = rng.integers(0, 65, n) / 64.0
    if conf_offset != -1:
        v[:, lead + 5 + conf_offset::step][:, :n_points] = rng.integers(0, 65, (n, n_points)) / 64.0
    members = max(1, min(n, (2 * n) // 3))
    kept = min(max_out, members, max(1, (3 * max_out) // 4)) if max_out > 1 else 1
    if with_cand:
        cand = np.full(n, -1, np.int64)
        cand[:members] = np.sort(rng.choice(n, members, replace=False))
        ki = np.full(max_out, -1, np.int64)
        ki[:kept] = rng.choice(members, kept, replace=False)
    else:
        cand = None
        ki = np.full(max_out, -1, np.int64)
        ki[:kept] = rng.choice(n, kept, replace=False)
    src = ki[:kept] if cand is None else cand[ki[:kept]]
    if special:  # the landmarks of kept candidates: one special value each, as far as they go
        cols = lead + 5 + step * rng.integers(0, n_points, len(SPECIALS)) + rng.integers(0, 2, len(SPECIALS))
        for r, (c, s) in enumerate(zip(cols, SPECIALS)):
            v[src[r % kept], c] = s
    if hostile and kept >= 6:
        bad = (-1, n, INT32_MAX, INT32_MIN)
        rows = rng.permutation(kept)
        for r, b in zip(rows[:4], bad):
            ki[r] = b
        if cand is not None:
            for r, b in zip(rows[4:8], bad):  # the slots the next kept rows point at
                cand[ki[r]] = b
            if members < n and kept >= 9:
                ki[rows[8]] = members + (n - members) // 2  # behind decode's count: cand_index holds -1 there
    count = kept if isinstance(kept_count, str) else kept_count
    return Case(v, elem, layout, lead, n_points, step, conf_offset, max_out, ki, count, cand, xform)


def kept_counts(max_out):
    return (None, 0, 1, max_out, max_out + 7, -3)


def seeded_cases():
    """Every element type x layout x (point_step, confidence) x cand_index on / off: 96 cases, with n_points, max_out, kept_count and the
    xform cycling through their values."""
    out = []
    k = 0
    for elem in (M.F32, M.F16, M.BF16):
        for layout in LAYOUTS:
            for step, conf_offset in STEPS:
                for with_cand in (False, True):
                    max_out = (13, 1, 8, 50, 21)[k % 5]
                    out.append(make(3000 + k, (97, 120, 64)[k % 3] + k % 7, N_POINTS[k % 6], elem, layout, step, conf_offset, max_out,
                                    (("kept",) + kept_counts(max_out))[(k // 2) % 7], with_cand, lead=(0, 2)[(k // 3) % 2], xform=XFORMS[(k // 5) % 3]))
                    k += 1
    return out


def text_file(cases, path):
    """The cases as the library reads them and the host entry's outputs for tests/cpp/gather_text_asan.cpp: unsigned integers, floats and
    negative indices as 32-bit patterns."""
    def u32(a):
        return np.ascontiguousarray(a).view(np.uint32).reshape(-1)
    lines = [str(len(cases))]
    for c in cases:
        xf = np.asarray(c.xform, np.float32).view(np.uint32)
        has_count = c.kept_count is not None
        count = int(np.int32(c.kept_count).view(np.uint32)) if has_count else 0
        lines.append(" ".join(str(int(v)) for v in (c.elem, c.n, c.cand_stride, c.attr_stride, c.point_attr, c.point_step, c.n_points, c.conf_offset + 1, c.max_out,
                                                    int(has_count), count, int(c.cand_index is not None), xf[0], xf[1], xf[2], xf[3], c.raw.size)))
        raw = c.raw.reshape(-1)
        lines.append(" ".join(map(str, (u32(raw) if c.elem == M.F32 else raw.view(np.uint16)).tolist())))
        lines.append(" ".join(map(str, u32(c.kept_index).tolist())))
        if c.cand_index is not None:
            lines.append(" ".join(map(str, u32(c.cand_index).tolist())))
        po, co, so = c.host()
        lines.append(" ".join(map(str, u32(po).tolist())))
        if co is not None:
            lines.append(" ".join(map(str, u32(co).tolist())))
        lines.append(" ".join(map(str, u32(so).tolist())))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
