"""Two models of cvgs_boxes_select's contract (include/cvgs_hip_ext.h), neither of which calls the library:

  select_f32   an independent restatement of the contract: np.float32 scalars (every operation rounded once, in the written order) and
               plain Python loops.  The host entry and the kernels must equal it byte for byte.
  select_f64   the same selection in exact arithmetic: float64 coordinates, and the textbook predicate inter / uni > thr.  On inputs whose
               fp32 operations are all exact (integer coordinates in a frame <= 4096^2, thresholds k / 4) it must select the same boxes.

Both take dense views: boxes [n, 4], scores [n], classes [n] or None (numpy slices of a strided head are fine), count or None, and a
Params.  Both return (boxes_out [max_out, 4], kept, scores_out [max_out], index_out [max_out]) with the documented tails.
"""
from collections import namedtuple

import numpy as np

XYXY, CXCYWH = 0, 1
Params = namedtuple("Params", "fmt W H score_thr iou_thr pre_k max_out xform")
F = np.float32


def params(W, H, score_thr, iou_thr, pre_k, max_out, fmt=XYXY, xform=(1.0, 1.0, 0.0, 0.0)):
    return Params(fmt, W, H, score_thr, iou_thr, pre_k, max_out, tuple(xform))


def live_count(count, n):
    return n if count is None else min(max(int(count), 0), n)


# ---- the fp32 restatement ------------------------------------------------------------------------------------------------------------
def _clamp32(v, e):
    v = v if v > F(0.0) else F(0.0)  # -0.0 and NaN give +0.0
    return v if v < e else e


def prepare32(p, c, score):
    """Steps 2-5: the clamped (xa, ya, xb, yb) of a member, or None."""
    c0, c1, c2, c3 = (F(v) for v in c)
    score = F(score)
    if np.isnan(score) or not score >= F(p.score_thr) or np.isnan(c0) or np.isnan(c1) or np.isnan(c2) or np.isnan(c3):
        return None
    sx, sy, ox, oy = (F(v) for v in p.xform)
    with np.errstate(all="ignore"):
        if p.fmt == CXCYWH:
            hw = c2 * F(0.5)
            hh = c3 * F(0.5)
            xa, xb, ya, yb = c0 - hw, c0 + hw, c1 - hh, c1 + hh
        else:
            xa, ya, xb, yb = c0, c1, c2, c3
        xa = xa * sx
        xa = xa + ox
        xb = xb * sx
        xb = xb + ox
        ya = ya * sy
        ya = ya + oy
        yb = yb * sy
        yb = yb + oy
    xa, xb = _clamp32(xa, F(p.W)), _clamp32(xb, F(p.W))
    ya, yb = _clamp32(ya, F(p.H)), _clamp32(yb, F(p.H))
    if not (xb > xa and yb > ya):
        return None
    return (xa, ya, xb, yb)


def suppresses32(j, i, thr):
    """Step 7: kept box j suppresses box i (tuples of np.float32)."""
    iw = min(i[2], j[2]) - max(i[0], j[0])
    ih = min(i[3], j[3]) - max(i[1], j[1])
    if not (iw > F(0.0) and ih > F(0.0)):
        return False
    inter = iw * ih
    area_i = (i[2] - i[0]) * (i[3] - i[1])
    area_j = (j[2] - j[0]) * (j[3] - j[1])
    uni = (area_i + area_j) - inter
    return bool(inter > F(thr) * uni)


# ---- the exact model -----------------------------------------------------------------------------------------------------------------
def prepare64(p, c, score):
    c = [float(v) for v in c]
    score = float(score)
    if np.isnan(score) or not score >= float(F(p.score_thr)) or any(np.isnan(v) for v in c):
        return None
    sx, sy, ox, oy = (float(F(v)) for v in p.xform)
    if p.fmt == CXCYWH:
        xa, xb, ya, yb = c[0] - c[2] / 2, c[0] + c[2] / 2, c[1] - c[3] / 2, c[1] + c[3] / 2
    else:
        xa, ya, xb, yb = c
    xa, xb, ya, yb = xa * sx + ox, xb * sx + ox, ya * sy + oy, yb * sy + oy
    xa, xb = min(max(xa, 0.0), float(p.W)), min(max(xb, 0.0), float(p.W))
    ya, yb = min(max(ya, 0.0), float(p.H)), min(max(yb, 0.0), float(p.H))
    if not (xb > xa and yb > ya):
        return None
    return (xa, ya, xb, yb)


def suppresses64(j, i, thr):
    iw = min(i[2], j[2]) - max(i[0], j[0])
    ih = min(i[3], j[3]) - max(i[1], j[1])
    if not (iw > 0.0 and ih > 0.0):
        return False
    inter = iw * ih
    uni = (i[2] - i[0]) * (i[3] - i[1]) + (j[2] - j[0]) * (j[3] - j[1]) - inter
    return inter / uni > float(F(thr))


# ---- steps 1 and 6-8, shared by the two (integers and comparisons only) --------------------------------------------------------------------
def _select(p, boxes, scores, classes, count, prepare, suppresses):
    n = len(scores)
    members = []
    for i in range(live_count(count, n)):
        b = prepare(p, boxes[i], scores[i])
        if b is not None:
            members.append((i, b))
    # score descending, equal scores by lower index: Python's sort is stable and members are in index order
    members.sort(key=lambda m: -float(scores[m[0]]))
    work = members[:p.pre_k]
    kept = []
    for i, b in work:
        if len(kept) == p.max_out:
            break
        if not any((classes is None or int(classes[j]) == int(classes[i])) and suppresses(bj, b, p.iou_thr) for j, bj in kept):
            kept.append((i, b))
    boxes_out = np.zeros((p.max_out, 4), np.float32)
    scores_out = np.zeros((p.max_out,), np.float32)
    index_out = np.full((p.max_out,), -1, np.int32)
    for k, (i, b) in enumerate(kept):
        boxes_out[k] = b
        scores_out[k] = scores[i]
        index_out[k] = i
    return boxes_out, len(kept), scores_out, index_out


def select_f32(p, boxes, scores, classes=None, count=None):
    return _select(p, boxes, scores, classes, count, prepare32, suppresses32)


def select_f64(p, boxes, scores, classes=None, count=None):
    return _select(p, boxes, scores, classes, count, prepare64, suppresses64)
