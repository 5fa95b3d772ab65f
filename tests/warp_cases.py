"""Warp test inputs shared by the CPU and GPU tests: the point sets of the reference's warp test
(tests/warping/test_warping_opencv.cu:47-48,140-153) and an independent float64 restatement of the warp."""
import numpy as np

# (src points, dst points) of the reference's perspective tests
REF_POINT_SETS = [
    ([(56, 65), (368, 52), (28, 387), (389, 390)], [(0, 0), (300, 0), (0, 300), (300, 300)]),
    ([(50, 50), (400, 50), (50, 400), (400, 400)], [(0, 0), (300, 0), (0, 300), (300, 300)]),
    ([(30, 30), (350, 30), (30, 350), (350, 350)], [(0, 0), (250, 0), (0, 250), (250, 250)]),
    ([(70, 70), (370, 70), (70, 370), (370, 370)], [(0, 0), (280, 0), (0, 280), (280, 280)]),
    ([(20, 20), (320, 20), (20, 320), (320, 320)], [(0, 0), (200, 0), (0, 200), (200, 200)]),
]


def get_perspective_transform(src, dst):
    """cv::getPerspectiveTransform: the 3x3 H with H*(x,y,1) ~ (u,v,1) for the four point pairs (h22 = 1)."""
    a = np.zeros((8, 8))
    b = np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        a[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        a[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    h = np.linalg.solve(a, b)
    return np.append(h, 1.0).reshape(3, 3)


def warp_f64(img, inv, dsize, perspective):
    """The float64 restatement of the warp: a thin caller of the independent model (tests/f64_model.py: zero outside, bilinear inside with
    the right/bottom taps clamped to the last column/row, coordinates in float64 from the fp32-narrowed inverse matrix).
    Returns (values [y][x][c], inside, sx, sy)."""
    from types import SimpleNamespace

    from tests import f64_model as F
    img = np.asarray(img)
    cn = 1 if img.ndim == 2 else img.shape[2]
    depth = {np.dtype(np.uint8): F.DEPTH_8U, np.dtype(np.uint16): F.DEPTH_16U, np.dtype(np.int16): F.DEPTH_16S, np.dtype(np.float32): F.DEPTH_32F}[img.dtype]
    rd = SimpleNamespace(dsize=(int(dsize[0]), int(dsize[1])), src_type=depth + ((cn - 1) << 3))
    val, _, (sx, sy, inside) = F._warp_plane(rd, F.View(img), list(np.asarray(inv, np.float64).reshape(-1)), bool(perspective), F.SPEC)
    return val.v, inside, sx, sy
