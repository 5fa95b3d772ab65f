"""A model of cvgs_head_decode's contract (include/cvgs_hip_ext.h) that does not call the library and shares no code with
csrc/cvgs_geometry.h: whole-array numpy.

  widen    fp16 through np.float16, bf16 through a 16-bit shift into the top half of a float32, fp32 as it is.
  decode   the best class as "the first index of the maximum over the non-NaN entries" -- where the contract's starting value (-inf, 0)
           stands in front of the entries: a candidate whose maximum is -inf (or that has no non-NaN entry) keeps class 0 and best = -inf --
           the score as ONE np.float32 multiplication, membership as two whole-array comparisons, compaction by boolean indexing.

`attrs` is the [N, A] view of the head's storage (any strides): float32, float16, or uint16 holding bfloat16 bits.
"""
import numpy as np

F32, F16, BF16 = 0, 1, 2


def widen(raw, elem):
    raw = np.ascontiguousarray(raw)
    if elem == F32:
        assert raw.dtype == np.float32
        return raw.copy()
    if elem == F16:
        return raw.view(np.float16).astype(np.float32)
    assert raw.dtype == np.uint16
    return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)


def dense(attrs, elem, box_attr, obj_attr, class_attr, num_classes):
    """Steps 1-3 for every candidate: (coords float32 [N, 4], score float32 [N], cls int32 [N])."""
    w = widen(attrs, elem)
    n = w.shape[0]
    cls_scores = w[:, class_attr:class_attr + num_classes]
    valid = ~np.isnan(cls_scores)
    top = np.where(valid, cls_scores, -np.inf).max(axis=1)                      # the maximum over the non-NaN entries (-inf without one)
    first = np.argmax(valid & (cls_scores == top[:, None]), axis=1)             # its first index
    wins = top > -np.inf                                                        # (-inf never beats the starting value)
    cls = np.where(wins, first, 0).astype(np.int32)
    best = np.where(wins, cls_scores[np.arange(n), first], np.float32(-np.inf)).astype(np.float32)  # the winner's bits (-0.0 stays -0.0)
    score = best
    if obj_attr >= 0:
        with np.errstate(all="ignore"):
            score = (w[:, obj_attr] * best).astype(np.float32)
    return np.ascontiguousarray(w[:, box_attr:box_attr + 4]), score, cls


def decode(attrs, elem, box_attr, obj_attr, class_attr, num_classes, thr):
    """(boxes_out [N, 4], scores_out [N], classes_out [N], index_out [N], count) with the documented tails."""
    coords, score, cls = dense(attrs, elem, box_attr, obj_attr, class_attr, num_classes)
    n = len(score)
    with np.errstate(all="ignore"):
        member = (score >= np.float32(thr)) & ~np.isnan(coords).any(axis=1)
    idx = np.flatnonzero(member)
    k = len(idx)
    bo, so = np.zeros((n, 4), np.float32), np.zeros((n,), np.float32)
    ko, io = np.zeros((n,), np.int32), np.full((n,), -1, np.int32)
    bo[:k], so[:k], ko[:k], io[:k] = coords[idx], score[idx], cls[idx], idx
    return bo, so, ko, io, k
