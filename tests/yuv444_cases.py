"""Planar 4:4:4 surfaces (I444) for the tests: surface builders and the COMPOSED oracle value.

The CPU oracle knows the 4:2:0 layouts only.  It converts (Y, U, V) per tap and blends fp32 taps with one shared function, so the
expected bits of a 4:4:4 chain are composed from two oracle runs (the method of tests/yuv422_cases.py):
  1. the surface's samples are laid out as an NV12 surface of 2H x 2W luma whose luma sample [2y][2x] is Y[y][x] and whose chroma
     sample [y][x] is (U, V)[y][x]; the oracle's per-pixel NV12 read (same range / primaries / alpha, no program) into an fp32
     image, even rows and even columns kept: E[y][x] is what the 4:4:4 read stage delivers for pixel (x, y);
  2. the chain under test with its read replaced by a per-pixel read / bilinear resize of E (CV_32FC3 / C4; crops: views of E).
tests/test_yuv444.py pins the method on pictures whose chroma is constant in 2 x 2 blocks, where the oracle's direct NV12 answer
exists, and holds E and its resize to the float64 model."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H

I444 = 7  # cvgs_yuv_layout (capi.YUV_I444)


class Surf:
    """A w x h picture as three planes Y, U, V inside ONE byte buffer:
        guard | lead | Y rows (step apart) ... U rows, uv bytes behind Y ... V rows, uv bytes behind U ... | guard
    step >= w and uv >= (h - 1) * step + w are free (odd values, no common factor); `lead` shifts the data pointer's alignment."""

    def __init__(self, w, h, seed, step=None, uv=None, guard=0, lead=0, planes=None):
        self.w, self.h = int(w), int(h)
        self.step = int(step) if step is not None else self.w
        self.uv = int(uv) if uv is not None else self.h * self.step
        assert self.step >= self.w and self.uv >= (self.h - 1) * self.step + self.w
        self.origin = int(guard) + int(lead)
        self.buf = np.zeros(self.origin + 2 * self.uv + (self.h - 1) * self.step + self.w + int(guard), np.uint8)
        self.planes = planes if planes is not None else tuple(H.random_u8((self.h, self.w), seed + k) for k in range(3))
        idx = self.origin + (np.arange(3)[:, None, None] * self.uv + np.arange(self.h)[None, :, None] * self.step + np.arange(self.w)[None, None, :])
        self.sample_index = idx.reshape(-1)
        self.buf[self.sample_index] = np.stack(self.planes).reshape(-1)

    def fill_rest(self, pattern):
        """Every byte that is no sample -- row padding, the gaps between the planes, the guard bands -- takes `pattern` (an array of
        the buffer's length)."""
        keep = self.buf[self.sample_index].copy()
        self.buf[:] = pattern
        self.buf[self.sample_index] = keep

    def mat(self, base, owner):
        m = cvgs.GpuMat(self.h, self.w, cvgs.CV_8UC1, base + self.origin, self.step, owner=owner)
        m.uv_offset = self.uv
        return m


def wrap_array(s):
    return s.mat(s.buf.ctypes.data, s.buf)


def tensor_wrapper(surfs, dev):
    """Uploads the surfaces' buffers; returns wrap(surf) -> luma view on the device, and the tensors."""
    import torch
    ts = {id(s): torch.from_numpy(s.buf).to(dev) for s in surfs}
    return (lambda s: s.mat(ts[id(s)].data_ptr(), ts[id(s)])), ts


def nv12_of(y, u, v):
    """The NV12 surface of step 1 above: (3H, 2W) u8 -- 2H luma rows with Y at the even rows and columns, then H chroma rows of W
    interleaved (U, V) pairs."""
    h, w = y.shape
    nv = np.zeros((3 * h, 2 * w), np.uint8)
    nv[0:2 * h:2, 0::2] = y
    nv[2 * h:, 0::2] = u
    nv[2 * h:, 1::2] = v
    return nv


def read_stage_value(oracle, y, u, v, color_range, primaries, alpha):
    """E: (H, W, 3|4) fp32, the value the read stage delivers per pixel for Y[y][x], U[y][x], V[y][x]."""
    h, w = y.shape
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    nv = nv12_of(y, u, v)
    out = np.zeros((2 * h, 2 * w, cn), np.float32)
    luma = cvgs.GpuMat(2 * h, 2 * w, cvgs.CV_8UC1, nv.ctypes.data, nv.strides[0], owner=nv)
    oracle.execute(cvgs.lower([cvgs.read_nv12(luma, None, color_range, primaries, alpha), cvgs.write(f, cvgs.GpuMat.from_array(out, f))]))
    return np.ascontiguousarray(out[0::2, 0::2])


def composed_ops(ops, views_of):
    """ops with the YUV read replaced by the same read of the fp32 image(s) E.  views_of(mat) -> (E, x, y): the E of the surface
    `mat` views and the view's origin inside it."""
    rd = ops[0]
    cn = 4 if rd.yuv[2] else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    mats = []
    for m in rd.mats:
        e, x, y = views_of(m)
        assert e.shape[2] == cn and y + m.rows <= e.shape[0] and x + m.cols <= e.shape[1]
        mats.append(cvgs.GpuMat(m.rows, m.cols, f, e.ctypes.data + y * e.strides[0] + x * cn * 4, e.strides[0], owner=e))
    kind = capi.READ_PIXEL if rd.dsize is None else capi.READ_RESIZE_LINEAR
    rd2 = cvgs.ReadIOp(kind, f, mats, rd.used_planes, rd.dsize, rd.ar, rd.background)
    return [rd2] + list(ops[1:])


class Expect:
    """Composed oracle values for chains over a set of host surfaces (Surf).  The read stage works pixel by pixel, so the E of a
    view is computed from the view's own samples; it is computed once per view and conversion."""

    def __init__(self, oracle, surfs):
        self.oracle, self.surfs = oracle, list(surfs)
        self.cache = {}

    def views_of(self, rd):
        def find(m):
            for i, s in enumerate(self.surfs):
                first = s.buf.ctypes.data + s.origin
                if first <= m.data < first + (s.h - 1) * s.step + s.w:
                    assert m.step == s.step and m.uv_offset == s.uv
                    y, x = divmod(m.data - first, s.step)
                    assert x + m.cols <= s.w and y + m.rows <= s.h
                    key = (i, rd.yuv, x, y, m.cols, m.rows)
                    if key not in self.cache:
                        crop = [np.ascontiguousarray(p[y:y + m.rows, x:x + m.cols]) for p in s.planes]
                        self.cache[key] = read_stage_value(self.oracle, *crop, rd.yuv[0], rd.yuv[1], bool(rd.yuv[2]))
                    return self.cache[key], 0, 0
            raise AssertionError("a source view outside every surface")
        return find

    def run(self, ops):
        """ops: the 4:4:4 chain over host buffers (wrap_array views), its write stage on a host array.  Executes the composed chain."""
        assert ops[0].yuv_layout == I444
        self.oracle.execute(cvgs.lower(composed_ops(ops, self.views_of(ops[0]))))
