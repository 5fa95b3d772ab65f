"""A model of cvgs_points_gather's contract (include/cvgs_hip_ext.h) that does not call the library and shares no code with
csrc/cvgs_geometry.h: whole-array numpy.

  widen    through integer views: bf16 is shifted into the top half of a uint32; fp16 is taken apart into sign, exponent and mantissa --
           normals re-biased, inf / NaN with the mantissa shifted up, subnormals as the exact float32 product mantissa * 2^-24.
  gather   validity as whole-array comparisons in int64 (so no index wraps), rows by fancy indexing with the failed indices replaced by 0
           before they are used, the mapping as ONE float32 multiplication followed by ONE float32 addition, NaN results replaced by the
           bit pattern 0x7fc00000, invalid rows filled afterwards.

`attrs` is the [max_candidates, A] view of the head's storage (any strides): float32, float16, or uint16 holding bfloat16 bits.
"""
import numpy as np

F32, F16, BF16 = 0, 1, 2
NAN_BITS = np.uint32(0x7FC00000)


def widen(raw, elem):
    raw = np.ascontiguousarray(raw)
    if elem == F32:
        assert raw.dtype == np.float32
        return raw.copy()
    h = raw.view(np.uint16).astype(np.uint32)
    if elem == BF16:
        return (h << np.uint32(16)).view(np.float32)
    s, e, m = (h & np.uint32(0x8000)) << np.uint32(16), (h >> np.uint32(10)) & np.uint32(31), h & np.uint32(0x3FF)
    normal = s | ((e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(13))
    special = s | np.uint32(0x7F800000) | (m << np.uint32(13))
    sub = s | (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)  # exact: m < 2^10
    return np.where(e == 31, special, np.where(e == 0, sub, normal)).astype(np.uint32).view(np.float32)


def live_rows(kept_count, max_out):
    return max_out if kept_count is None else min(max(int(kept_count), 0), max_out)


def sources(max_candidates, max_out, kept_index, kept_count, cand_index):
    """int64 [max_out]: the raw candidate of every row, -1 for an invalid one."""
    j = np.arange(max_out)
    k = np.asarray(kept_index[:max_out], np.int64)
    ok = (j < live_rows(kept_count, max_out)) & (k >= 0) & (k < max_candidates)
    c = np.where(ok, k, 0)
    if cand_index is not None:
        m = np.asarray(cand_index, np.int64)[c]
        ok &= (m >= 0) & (m < max_candidates)
        c = np.where(ok, m, 0)
    return np.where(ok, c, -1)


def map_axis(v, s, o):
    with np.errstate(all="ignore"):
        r = (v * np.float32(s)).astype(np.float32)
        r = (r + np.float32(o)).astype(np.float32)
    bits = r.view(np.uint32).copy()
    bits[np.isnan(r)] = NAN_BITS
    return bits


def gather(attrs, elem, point_attr, point_step, n_points, conf_offset, max_out, kept_index, kept_count, cand_index, xform):
    """(points uint32 bits [max_out, n_points, 2], conf uint32 bits [max_out, n_points] or None, source int32 [max_out])."""
    src = sources(attrs.shape[0], max_out, kept_index, kept_count, cand_index)
    valid = src >= 0
    rows = widen(np.asarray(attrs)[np.where(valid, src, 0)], elem)  # [max_out, A]
    xa = point_attr + point_step * np.arange(n_points)
    pts = np.empty((max_out, n_points, 2), np.uint32)
    pts[:, :, 0] = map_axis(rows[:, xa], xform[0], xform[2])
    pts[:, :, 1] = map_axis(rows[:, xa + 1], xform[1], xform[3])
    pts[~valid] = NAN_BITS
    conf = None
    if conf_offset != -1:
        conf = np.ascontiguousarray(rows[:, xa + conf_offset]).view(np.uint32).copy()
        conf[~valid] = 0
    return pts, conf, src.astype(np.int32)


def exact_f64(values, xform):
    """The exact mapping of float64 landmarks [..., 2] (for inputs whose products and sums are exact in float32)."""
    out = np.asarray(values, np.float64).copy()
    out[..., 0] = out[..., 0] * float(xform[0]) + float(xform[2])
    out[..., 1] = out[..., 1] * float(xform[1]) + float(xform[3])
    return out
