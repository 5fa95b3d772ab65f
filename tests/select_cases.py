"""Seeded candidate sets for cvgs_boxes_select (tests/test_box_select.py on the CPU, tests/test_zzzzz_gpu_box_select.py on the GPU).

A Case holds the detector head as the library reads it -- dense arrays, or ONE interleaved float32 [n, 6] tensor (box, score, class as
int32 bits) read in place -- the dense views the models take, and the Params.  Candidates come in clusters (so that suppression has work to
do), scores are quantised (so that ties occur), and a sprinkle of them is NaN / infinite / empty / outside the frame."""
import numpy as np

from cvgpuspeedup_amd import cvgs
from tests import select_model as M


class Case:
    def __init__(self, p, boxes, scores, classes, count, head=None):
        self.p, self.boxes, self.scores, self.classes, self.count, self.head = p, boxes, scores, classes, count, head
        self.n = len(scores)

    def strides(self):
        """(box_stride, score_stride, class_stride) in elements."""
        return (6, 6, 6) if self.head is not None else (4, 1, 1)

    def desc(self, **ptrs):
        """The descriptor without addresses (cvgs.boxes_select_host fills the inputs in), or with the device ones given."""
        p = self.p
        bs, ss, cs = self.strides()
        return cvgs.box_select_desc((p.W, p.H), ptrs.get("boxes"), ptrs.get("scores"), self.n, ptrs.get("scratch"), ptrs.get("boxes_out"), ptrs.get("count_out"),
                                    p.score_thr, p.iou_thr, p.pre_k, p.max_out, p.fmt, bs, ss, ptrs.get("classes"), cs, ptrs.get("count"), p.xform,
                                    ptrs.get("scores_out"), ptrs.get("index_out"))

    def host(self):
        """cvgs_boxes_select_host on this case: (boxes_out, kept, scores_out, index_out)."""
        return cvgs.boxes_select_host(self.desc(), self.boxes, self.scores, self.classes, self.count)

    def model(self, f64=False):
        return (M.select_f64 if f64 else M.select_f32)(self.p, self.boxes, self.scores, self.classes, self.count)


def same(a, b):
    """Byte equality of two result tuples."""
    return (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and a[1] == b[1] and (a[2].view(np.uint32) == b[2].view(np.uint32)).all() and (a[3] == b[3]).all()


def make(seed, n=300, fmt=M.XYXY, interleaved=False, with_classes=False, xform=(1.0, 1.0, 0.0, 0.0), W=640, H=480, score_thr=0.3, iou_thr=0.5,
         pre_k=128, max_out=40, count=None, integer=False, dirty=True, n_classes=3):
    rng = np.random.default_rng(seed)
    k = max(n // 12, 1)
    centres = rng.uniform([0, 0], [W, H], (k, 2))
    sizes = rng.uniform(min(W, H) / 30, min(W, H) / 4, (k, 2))
    which = rng.integers(0, k, n)
    jitter = min(W, H) / 80
    cx = centres[which, 0] + rng.normal(0, jitter, n)
    cy = centres[which, 1] + rng.normal(0, jitter, n)
    w = sizes[which, 0] * rng.uniform(0.8, 1.25, n)
    h = sizes[which, 1] * rng.uniform(0.8, 1.25, n)
    xa, ya, xb, yb = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    if integer:
        xa, ya = np.floor(xa), np.floor(ya)
        xb, yb = xa + np.maximum(np.round(w), 1), ya + np.maximum(np.round(h), 1)
    # frame -> detector coordinates
    sx, sy, ox, oy = xform
    xa, xb, ya, yb = (xa - ox) / sx, (xb - ox) / sx, (ya - oy) / sy, (yb - oy) / sy
    if fmt == M.CXCYWH:
        b = np.stack([(xa + xb) / 2, (ya + yb) / 2, xb - xa, yb - ya], axis=1)
    else:
        b = np.stack([xa, ya, xb, yb], axis=1)
    boxes = b.astype(np.float32)
    scores = (np.round(rng.uniform(0, 1, n) * 64) / 64).astype(np.float32)  # 65 levels: ties among a few hundred candidates
    if dirty and n >= 40:
        pick = rng.permutation(n)
        boxes[pick[0], 0] = np.nan
        boxes[pick[1], 3] = np.nan
        scores[pick[2]] = np.nan
        boxes[pick[3]] = (np.inf, 0, np.inf, 10) if fmt == M.XYXY else (np.inf, 5, np.inf, 10)   # CXCYWH: inf - inf inside step 3
        boxes[pick[4]] = (-np.inf, -np.inf, np.inf, np.inf) if fmt == M.XYXY else (0, 0, np.inf, np.inf)
        boxes[pick[5], 2:] = (boxes[pick[5], 0], boxes[pick[5], 1]) if fmt == M.XYXY else (0, 0)   # empty
        boxes[pick[6]] = (-5000, -5000, -4000, -4000) if fmt == M.XYXY else (-5000, -5000, 10, 10)  # outside
        scores[pick[7]] = np.inf
        scores[pick[8]] = -0.0
        scores[pick[9]] = 0.0
        scores[pick[3]] = scores[pick[4]] = 1.0
    classes = rng.integers(0, n_classes, n).astype(np.int32) if with_classes else None
    p = M.params(W, H, score_thr, iou_thr, pre_k, max_out, fmt, xform)
    if not interleaved:
        return Case(p, boxes, scores, classes, count)
    head = np.zeros((n, 6), np.float32)
    head[:, :4], head[:, 4] = boxes, scores
    ih = head.view(np.int32)
    ih[:, 5] = classes if with_classes else 0x7fc00000  # (unused: NaN bits)
    return Case(p, head[:, :4], head[:, 4], ih[:, 5] if with_classes else None, count, head)


def seeded_cases():
    """The cases the host entry, the restatement and the stand-alone text program all run."""
    out = []
    seed = 100
    for fmt in (M.XYXY, M.CXCYWH):
        for interleaved in (False, True):
            for with_classes in (False, True):
                for xform in ((1.0, 1.0, 0.0, 0.0), (3.0, 3.0, 0.0, -420.0), (0.3333333, 0.75, 13.5, -7.25)):
                    seed += 1
                    out.append(make(seed, 260 + seed % 7, fmt, interleaved, with_classes, xform, W=1920 if xform[0] == 3.0 else 640,
                                    H=1080 if xform[0] == 3.0 else 480, count=(None, 200, 1000)[seed % 3], pre_k=(128, 64, 1024)[seed % 3],
                                    max_out=(40, 64, 17)[seed % 3], iou_thr=(0.5, 0.45, 0.3)[seed % 3]))
    return out


def text_file(cases, path):
    """The cases and the host entry's outputs for tests/cpp/select_text_asan.cpp: unsigned integers, floats as bit patterns."""
    def bits(v):
        return int(np.float32(v).view(np.uint32))
    lines = [str(len(cases))]
    for c in cases:
        p = c.p
        lines.append(" ".join(str(v) for v in [p.fmt, p.W, p.H, bits(p.score_thr), bits(p.iou_thr), p.pre_k, p.max_out] + [bits(v) for v in p.xform] +
                              [c.n, M.live_count(c.count, c.n), int(c.classes is not None)]))
        bu = np.ascontiguousarray(c.boxes).view(np.uint32)
        su = np.ascontiguousarray(c.scores).view(np.uint32)
        cu = np.ascontiguousarray(c.classes).view(np.uint32) if c.classes is not None else np.zeros(c.n, np.uint32)
        for i in range(c.n):
            lines.append("%d %d %d %d %d %d" % (bu[i, 0], bu[i, 1], bu[i, 2], bu[i, 3], su[i], cu[i]))
        bo, kept, so, io = c.host()
        lines.append(str(kept))
        for k in range(p.max_out):
            u = bo[k].view(np.uint32)
            lines.append("%d %d %d %d %d %d" % (u[0], u[1], u[2], u[3], so[k:k + 1].view(np.uint32)[0], io[k:k + 1].view(np.uint32)[0]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
