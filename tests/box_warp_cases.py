"""The cases of cvgs_warp_tables_from_boxes' tests, shared by the CPU tests (tests/test_box_warp.py) and the GPU tests
(tests/test_zzzzzzzzzzz_gpu_box_warp.py): the frame, the configurations and the box sets.  Pure numpy; nothing here calls the library."""
import itertools

import numpy as np

W, H, STEP = 97, 61, 304            # the frame: CV_8UC3, padded rows
FRAME_DATA = 0x7F0012345600         # a pretend device address for the host entry (never dereferenced)
STRETCH, EXPAND = 0, 1
TARGETS = ((1, 1), (8, 6), (192, 256), (256, 192))
SCALES = ((1.0, 1.0), (1.25, 1.25))
PADS = ((0.0, 0.0), (3.5, 3.5))
FLT_MAX = float(np.finfo(np.float32).max)


def configs():
    """[(shape, dsize, scale, pad)]: both shapes x four targets x two scales x two pads, and two with unequal axes."""
    out = list(itertools.product((STRETCH, EXPAND), TARGETS, SCALES, PADS))
    return out + [(EXPAND, (192, 256), (1.25, 1.5), (0.0, 7.25)), (STRETCH, (8, 6), (0.5, 2.0), (1.0, 0.0))]


def integer_boxes():
    return np.array([(10, 5, 40, 50), (0, 0, W, H), (3, 7, 4, 8), (20, 20, 84, 52), (96, 60, 97, 61), (0, 0, 1, 1), (5, 5, 13, 11)], np.float32)


def half_pixel_boxes():
    return np.array([(10.5, 5.5, 40.5, 50.5), (0.5, 0.5, 96.5, 60.5), (3.25, 7.75, 4.5, 8.125), (-0.5, -0.5, 0.5, 0.5), (30.5, 2.0, 31.0, 59.5)], np.float32)


def random_boxes(n=400, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-40, 140, (n, 2))
    s = np.exp(rng.uniform(np.log(0.01), np.log(400), (n, 2)))
    return np.concatenate([a, a + s], axis=1).astype(np.float32)


def outside_boxes():
    """Wholly outside each side and corner, partly outside each side, larger than the frame."""
    return np.array([(-50, 10, -20, 40), (120, 10, 150, 40), (10, -60, 40, -30), (10, 80, 40, 120), (-30, -30, -5, -5), (100, 70, 130, 90),
                     (-10, 10, 20, 40), (80, 10, 110, 40), (10, -10, 40, 20), (10, 40, 40, 70), (-5, -5, 8, 8), (90, 55, 105, 70),
                     (-20, -20, 120, 80), (-1000, -1000, 1000, 1000), (-3, 20, 100, 30), (40, -300, 50, 300)], np.float32)


def tie_boxes():
    """t1 == t2 for at least one configuration each: the box already has the target's aspect ratio."""
    return np.array([(10, 5, 106, 133), (1, 2, 9, 8), (4, 4, 20, 20), (0, 0, 128, 96), (2.5, 3.5, 50.5, 67.5), (-6, -8, 0, 0)], np.float32)


def degenerate_boxes():
    """Zero area and inverted on either axis."""
    return np.array([(10, 5, 10, 50), (10, 5, 40, 5), (10, 5, 10, 5), (40, 5, 10, 50), (10, 50, 40, 5), (40, 50, 10, 5), (0, 0, 0, 0),
                     (-0.0, 3, 0.0, 9)], np.float32)


def nonfinite_boxes():
    """NaN, +inf and -inf in each slot of an otherwise good box."""
    out = []
    for slot in range(4):
        for v in (np.nan, np.inf, -np.inf):
            b = [10.0, 5.0, 40.0, 50.0]
            b[slot] = v
            out.append(b)
    return np.array(out, np.float32)


def huge_boxes():
    """Values near FLT_MAX: finite doubles whose narrowing overflows (invalid), their neighbours that just fit (valid), and a valid item whose
    boxes_out overflows to inf (the contract narrows boxes_out without a test)."""
    m = FLT_MAX
    return np.array([(-m, 0, m, 10), (0, -m, 10, m), (-m, -m, m, m), (m / 2, 0, m, 10), (0, 1e38, 10, 3.3e38), (-3e38, 0, 3e38, 10),
                     (1e38, 0, 3.4e38, 10), (-m, 0, -m / 2, 10), (0, 0, 1e30, 1e-30), (0, 0, 1e-30, 1e30), (1e37, 1e37, 1.00001e37, 1.00001e37)], np.float32)


def all_boxes():
    return np.concatenate([integer_boxes(), half_pixel_boxes(), random_boxes(), outside_boxes(), tie_boxes(), degenerate_boxes(), nonfinite_boxes(),
                           huge_boxes()])


def counts(n):
    """(label, count): NULL, 0, mid-range, max, beyond max_items, negative."""
    return [("null", None), ("zero", 0), ("one", 1), ("mid", n // 2), ("max-1", n - 1), ("max", n), ("beyond", n + 5), ("negative", -3)]
