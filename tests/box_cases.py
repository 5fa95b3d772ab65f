"""An independent model of the box rule of cvgs_plane_tables_from_boxes, and the cases the tests share.

Written from the text of include/cvgs_hip_ext.h (integer / float32 numpy), not from the engine's sources and not through cvgs.py:

  XYXY_F32  (xa, ya, xb, yb) float32, xb / yb exclusive: any NaN -> invalid; l = (int)floor(min(max(xa, 0), W)), r = (int)ceil(min(max(xb, 0), W)),
            t / b the same with H (the clamp first: +-inf and huge values never reach the conversion).
  XYWH_I32  (x, y, w, h) int32: w <= 0 or h <= 0 -> invalid; l = clamp(x, 0, W), r = clamp(x + w, 0, W) with the sum in 64 bits.
  4:2:0     l, t down to even; r, b up to even, then clamped to W / H (both even).
  valid iff r > l and b > t (after the snapping) and the index is below the count clamped to [0, max_boxes].

rect() answers (l, t, w, h) or None.  Nothing here knows the plane table's layout beyond what the header documents.
"""
import numpy as np

XYXY_F32, XYWH_I32 = 0, 1
INVALID_RECT = (0, 0, 0, 0)
F = np.float32


def _axis_f32(a, b, extent):
    e = F(extent)
    lo = np.floor(np.minimum(np.maximum(F(a), F(0)), e))
    hi = np.ceil(np.minimum(np.maximum(F(b), F(0)), e))
    return int(lo), int(hi)


def _axis_i32(o, n, extent):
    o, n = int(o), int(n)  # Python integers: the sum cannot overflow
    return min(max(o, 0), extent), min(max(o + n, 0), extent)


def rect(box, fmt, W, H, yuv420=False):
    """(l, t, w, h) of one box clamped into a W x H frame, or None for an invalid box."""
    if fmt == XYXY_F32:
        xa, ya, xb, yb = (F(v) for v in box)
        if any(np.isnan(v) for v in (xa, ya, xb, yb)):
            return None
        l, r = _axis_f32(xa, xb, W)
        t, b = _axis_f32(ya, yb, H)
    else:
        x, y, w, h = (int(v) for v in box)
        if w <= 0 or h <= 0:
            return None
        l, r = _axis_i32(x, w, W)
        t, b = _axis_i32(y, h, H)
    if yuv420:
        assert W % 2 == 0 and H % 2 == 0
        l, t = l - (l & 1), t - (t & 1)
        r, b = min(r + (r & 1), W), min(b + (b & 1), H)
    if r > l and b > t:
        return (l, t, r - l, b - t)
    return None


def apply_count(all_rects, count):
    """The count rule on a list of per-box results: entries at or beyond the count (None = all; clamped to [0, len]) are invalid."""
    n = len(all_rects)
    live = n if count is None else min(max(int(count), 0), n)
    return list(all_rects[:live]) + [None] * (n - live)


def rects(boxes, fmt, W, H, count=None, yuv420=False):
    """One entry per box: (l, t, w, h) or None; entries at or beyond the count (clamped to [0, len(boxes)]) are None."""
    return apply_count([rect(b, fmt, W, H, yuv420) for b in boxes], count)


# ---- hand-pinned cases: (box, expected rect or None) for a W x H = 257 x 131 frame -----------------------------------------------
W0, H0 = 257, 131
NAN, INF = float("nan"), float("inf")
PINNED_XYXY = [
    # entirely outside, one per side
    ((-50.0, 10.0, -1.0, 40.0), None), ((257.0, 10.0, 300.0, 40.0), None), ((10.0, -30.0, 40.0, -0.5), None), ((10.0, 131.0, 40.0, 500.0), None),
    # straddling each edge
    ((-5.5, 10.0, 20.0, 40.0), (0, 10, 20, 30)), ((250.0, 10.0, 300.0, 40.0), (250, 10, 7, 30)),
    ((10.0, -7.0, 40.0, 12.0), (10, 0, 30, 12)), ((10.0, 120.0, 40.0, 999.0), (10, 120, 30, 11)),
    # zero and negative extents
    ((30.0, 30.0, 30.0, 60.0), None), ((30.0, 30.0, 60.0, 30.0), None), ((60.0, 30.0, 30.0, 60.0), None), ((30.0, 60.0, 60.0, 30.0), None),
    # NaN in each slot
    ((NAN, 1.0, 20.0, 20.0), None), ((1.0, NAN, 20.0, 20.0), None), ((1.0, 1.0, NAN, 20.0), None), ((1.0, 1.0, 20.0, NAN), None),
    # +-inf, +-1e30
    ((-INF, -INF, INF, INF), (0, 0, 257, 131)), ((INF, 0.0, INF, 10.0), None), ((-INF, 5.0, -INF, 10.0), None),
    ((-1e30, -1e30, 1e30, 1e30), (0, 0, 257, 131)), ((1e30, 0.0, 2e30, 10.0), None), ((3.0, -1e30, 9.0, 1e30), (3, 0, 6, 131)),
    # fractional edges: 10.0 / 10.000001 / 9.999999 as the left edge (floor) and as the right edge (ceil)
    ((10.0, 0.0, 20.0, 5.0), (10, 0, 10, 5)), ((10.000001, 0.0, 20.0, 5.0), (10, 0, 10, 5)), ((9.999999, 0.0, 20.0, 5.0), (9, 0, 11, 5)),
    ((0.0, 0.0, 10.0, 5.0), (0, 0, 10, 5)), ((0.0, 0.0, 10.000001, 5.0), (0, 0, 11, 5)), ((0.0, 0.0, 9.999999, 5.0), (0, 0, 10, 5)),
    # a sub-pixel box is one pixel; reversed sub-pixel edges inside one pixel still cover it (the rule is r > l after floor / ceil)
    ((10.25, 7.5, 10.75, 7.75), (10, 7, 1, 1)), ((10.75, 7.0, 10.25, 8.0), (10, 7, 1, 1)),
    # the whole frame, the last pixel
    ((0.0, 0.0, 257.0, 131.0), (0, 0, 257, 131)), ((256.0, 130.0, 257.0, 131.0), (256, 130, 1, 1)),
]
I32_MAX, I32_MIN = 2**31 - 1, -2**31
PINNED_XYWH = [
    ((-50, 10, 49, 30), None), ((257, 10, 40, 30), None), ((10, -30, 30, 30), None), ((10, 131, 30, 30), None),
    ((-5, 10, 25, 30), (0, 10, 20, 30)), ((250, 10, 50, 30), (250, 10, 7, 30)), ((10, -7, 30, 19), (10, 0, 30, 12)), ((10, 120, 30, 900), (10, 120, 30, 11)),
    ((30, 30, 0, 30), None), ((30, 30, 30, 0), None), ((30, 30, -5, 30), None), ((30, 30, 30, -5), None), ((30, 30, I32_MIN, 4), None),
    # x + w beyond int32: the 64-bit sum clamps to the frame instead of wrapping negative
    ((100, 50, I32_MAX, I32_MAX), (100, 50, 157, 81)), ((I32_MAX, 0, I32_MAX, 10), None), ((I32_MIN, I32_MIN, I32_MAX, I32_MAX), None),
    ((I32_MIN, 0, I32_MAX, 10), None), ((-1, -1, I32_MAX, I32_MAX), (0, 0, 257, 131)),
    ((0, 0, 257, 131), (0, 0, 257, 131)), ((256, 130, 1, 1), (256, 130, 1, 1)), ((0, 0, 1, 1), (0, 0, 1, 1)),
]
# 4:2:0 snapping on a 130 x 66 surface: odd origins go down, odd ends go up, the last column / row stay inside
WY, HY = 130, 66
PINNED_420_XYWH = [
    ((3, 5, 4, 4), (2, 4, 6, 6)), ((3, 5, 1, 1), (2, 4, 2, 2)), ((129, 65, 1, 1), (128, 64, 2, 2)), ((129, 65, 50, 50), (128, 64, 2, 2)),
    ((0, 0, 130, 66), (0, 0, 130, 66)), ((2, 4, 6, 6), (2, 4, 6, 6)), ((130, 0, 4, 4), None), ((1, 1, 128, 64), (0, 0, 130, 66)),
]
PINNED_420_XYXY = [
    ((3.5, 5.5, 6.5, 8.5), (2, 4, 6, 6)), ((129.0, 65.0, 130.0, 66.0), (128, 64, 2, 2)), ((128.5, 64.5, 500.0, 500.0), (128, 64, 2, 2)),
    ((4.0, 4.0, 4.0, 9.0), None), ((5.0, 5.0, 5.5, 5.5), (4, 4, 2, 2)), ((NAN, 0.0, 4.0, 4.0), None),
]


def boxes_array(boxes, fmt):
    return np.array(boxes, dtype=np.float32 if fmt == XYXY_F32 else np.int64).astype(np.float32 if fmt == XYXY_F32 else np.int32).reshape(-1, 4)


def covering_boxes(fmt, W, H, n_random=1600, seed=11):
    """Boxes that together cover every width 1..W and every height 1..H at least once, a random remainder (a third of it clipped or
    invalid), and the pinned cases of the format -- about 2,000 boxes.  Returns an array [n, 4] of the format's dtype."""
    rng = np.random.default_rng(seed)
    out = []
    for w in range(1, W + 1):  # every width, the height walking through 1..H
        h = (w - 1) % H + 1
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    for h in range(1, H + 1):
        w = (h * 7 - 1) % W + 1
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    for _ in range(n_random):
        x, y = int(rng.integers(-40, W + 20)), int(rng.integers(-30, H + 20))
        w, h = int(rng.integers(-3, W)), int(rng.integers(-3, H))
        out.append((x, y, w, h))
    if fmt == XYWH_I32:
        arr = np.array(out, dtype=np.int32)
        pinned = boxes_array([b for b, _ in PINNED_XYWH], fmt)
    else:
        arr = np.array([(x, y, x + w, y + h) for x, y, w, h in out], dtype=np.float32)
        frac = rng.random((len(out), 4), dtype=np.float32) * F(0.98) + F(0.01)
        arr[W + H:] += (frac[W + H:] - F(0.5))  # the random remainder gets fractional edges; the covering boxes stay exact
        pinned = boxes_array([b for b, _ in PINNED_XYXY], fmt)
    return np.concatenate([arr, pinned], axis=0)
