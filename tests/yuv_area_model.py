"""Two numpy models of the INTER_AREA read of 4:2:0 decoder surfaces (CVGS_READ_NV12_RESIZE_AREA), written from the arithmetic contract in
include/cvgs_hip.h.  Neither calls the library for a pixel: the library only supplies the plane GEOMETRY (fx, fy and the aspect-ratio window,
cvgs.build_plane_table) and the chain's own operands.

  * yuv_area_plane_f32: the fp32 restatement -- np.float32 arithmetic in the written order: the luma axis of tests/area_model.py
    (axis_taps_f32), its chroma twin (chroma_axis_taps_f32), the AREA loop nest over the luma codes and over the chroma pairs, ONE conversion
    of the three means.  The kernels are held to it BIT FOR BIT (tests/test_gpu_yuv_area.py).
  * yuv_area_plane_f64: the INDEPENDENT float64 model, built from existing pieces only -- every luma pixel of the view converted to RGB with
    tests/f64_model.yuv_taps + convert_yuv (nearest chroma in surface coordinates), then area_model.area_plane_f64 over the RGB picture.
    It shares neither the chroma axis nor the order "average, then convert" with the restatement.

Both share the chain tail of tests/area_model.py (apply_program, store_bits) and one case list (the GPU test's)."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as A
from tests import f64_model as F

F32 = np.float32

# ---- the case list: one 98 x 62 surface per layout, the targets of tests/area_model.py, crops at even origins -----------------------------
SRC_W, SRC_H = 98, 62
TARGETS = A.TARGETS                # (16, 8), (33, 7)
NARROW_TARGET = A.NARROW_TARGET    # (1, 8)
LAYOUTS = {"NV12": capi.YUV_NV12, "NV21": capi.YUV_NV21, "P010": capi.YUV_P010}
CROPS = (  # (x, y, w, h)
    (0, 0, 98, 62),     # the whole surface
    (4, 6, 2, 2),
    (6, 2, 2, 40),
    (2, 8, 40, 2),
    (10, 10, 16, 8),    # identity for 16 x 8
    (20, 30, 33, 7),    # identity for 33 x 7 (odd width and height)
    (2, 4, 1, 8),       # identity for 1 x 8
    (30, 20, 7, 5),     # both axes non-shrinking (for both targets)
    (2, 40, 90, 6),     # x shrinks, y does not
    (10, 12, 38, 19),   # 2.375x (16 x 8), odd height
    (8, 4, 32, 16),     # exactly 2x (16 x 8)
    (2, 2, 48, 24),     # exactly 3x (16 x 8)
    (10, 2, 66, 14),    # exactly 2x (33 x 7)
    (12, 14, 39, 19),   # odd width and height
    (56, 38, 42, 24),   # touches the right and the bottom edge
)
EVEN_CROPS = tuple(c for c in CROPS if not (c[2] | c[3]) & 1)  # what the bilinear NV12 kind takes too


def make_surface(layout, seed=0x8A2E):
    """The (62 * 3 / 2) x 98 surface of a layout: 62 luma rows, then 31 rows of interleaved chroma pairs; seeded random plus a ramp.
    NV12 / NV21: uint8.  P010: uint16, the 10-bit code in the high bits and RANDOM low 6 bits (which the read must ignore)."""
    rng = np.random.default_rng(seed + layout)
    rows = SRC_H * 3 // 2
    ramp = np.arange(SRC_W)[None, :] * 3 + np.arange(rows)[:, None] * 5
    if layout == capi.YUV_P010:
        code = (rng.integers(0, 800, (rows, SRC_W)) + ramp % 224).astype(np.uint16)
        return np.ascontiguousarray((code << 6) | rng.integers(0, 64, (rows, SRC_W)).astype(np.uint16))
    return np.ascontiguousarray((rng.integers(0, 200, (rows, SRC_W)) + ramp % 56).astype(np.uint8))


def surface_type(layout):
    return cvgs.make_type(capi.DEPTH_16U if layout == capi.YUV_P010 else capi.DEPTH_8U, 1)


def luma_mat(surface, layout, data=None):
    """The luma view (62 rows; the chroma plane follows it) of a surface held in a numpy array -- or at the device address `data`."""
    return cvgs.GpuMat(SRC_H, SRC_W, surface_type(layout), surface.ctypes.data if data is None else data, surface.strides[0], owner=surface)


# ---- the fp32 restatement --------------------------------------------------------------------------------------------------------------
def _box_taps(a, b, n):
    """The taps of the footprints [a, b) over n samples (the shrinking rule of the contract, for the luma or the chroma grid)."""
    i0 = np.minimum(np.floor(a).astype(np.int64), n - 1)
    i1 = np.maximum(np.minimum(np.ceil(b).astype(np.int64), n), i0 + 1)
    cnt = i1 - i0
    J = int(cnt.max())
    n_out = a.shape[0]
    idx, wt, live, W = np.zeros((n_out, J), np.int64), np.zeros((n_out, J), F32), np.zeros((n_out, J), bool), np.zeros(n_out, F32)
    single = b <= a
    for j in range(J):
        i = i0 + j
        w = (np.minimum((i + 1).astype(F32), b) - np.maximum(i.astype(F32), a)).astype(F32)
        w = np.where(single, F32(1.0), w).astype(F32)
        lv = j < cnt
        idx[:, j] = np.where(lv, i, i0)
        wt[:, j] = w
        live[:, j] = lv
        W = np.where(lv, (W + w).astype(F32), W).astype(F32)
    return idx, wt, live, W


def chroma_axis_taps_f32(n_out, f, n):
    """The chroma twin of area_model.axis_taps_f32(n_out, f, n): (idx, wt, live, W) over the nc = (n + 1) >> 1 chroma samples."""
    f = F32(f)
    if not f > F32(1.0):
        idx, wt, live, W = A.axis_taps_f32(n_out, f, n)  # the luma pair and its weights; idx[:, 1] is min(i0 + 1, n - 1) already
        return idx >> 1, wt, live, W
    t = np.arange(n_out, dtype=np.int64)
    a = t.astype(F32) * f
    b = np.minimum((t + 1).astype(F32) * f, F32(n)).astype(F32)
    return _box_taps((a * F32(0.5)).astype(F32), (b * F32(0.5)).astype(F32), (n + 1) >> 1)


def _nest(v, ty, tx):
    """The AREA loop nest over v (rows, cols, k) float32 with the taps ty, tx = (idx, wt, live, W): (ny, nx, k) means."""
    (iy, wy, ly, Wy), (ix, wx, lx, Wx) = ty, tx
    ny, nx, k = iy.shape[0], ix.shape[0], v.shape[2]
    acc = np.zeros((ny, nx, k), F32)
    for jj in range(iy.shape[1]):
        rows = v[iy[:, jj]]
        row = np.zeros((ny, nx, k), F32)
        for ii in range(ix.shape[1]):
            term = (rows[:, ix[:, ii], :] * wx[None, :, ii, None]).astype(F32)
            row = np.where(lx[None, :, ii, None], (row + term).astype(F32), row)
        acc = np.where(ly[:, jj, None, None], (acc + (row * wy[:, jj, None, None]).astype(F32)).astype(F32), acc)
    inv = (F32(1.0) / (Wx[None, :] * Wy[:, None]).astype(F32)).astype(F32)
    return (acc * inv[:, :, None]).astype(F32)


# (rv, gu, gv, bu) as the engine holds them: 6-decimal fp32 literals of the derivation from the standards' luma weights
# (tests/test_independent_pins.py re-derives every set in float64); keyed by (range, ten_bit), then by primaries
_MATRIX = {
    (capi.YUV_FULL, False): {capi.BT601: (1.402, -0.344136, -0.714136, 1.772), capi.BT709: (1.5748, -0.187324, -0.468124, 1.8556),
                             capi.BT2020: (1.4746, -0.164553, -0.571353, 1.8814)},
    (capi.YUV_LIMITED, False): {capi.BT601: (1.596027, -0.391762, -0.812968, 2.017232), capi.BT709: (1.792741, -0.213249, -0.532909, 2.112402),
                                capi.BT2020: (1.678674, -0.187326, -0.650424, 2.141772)},
    (capi.YUV_LIMITED, True): {capi.BT601: (1.600721, -0.392915, -0.815359, 2.023165), capi.BT709: (1.798014, -0.213876, -0.534477, 2.118615),
                               capi.BT2020: (1.683611, -0.187877, -0.652337, 2.148072)},
}
_MATRIX[(capi.YUV_FULL, True)] = _MATRIX[(capi.YUV_FULL, False)]  # full range: no scale, the same coefficients on 10-bit codes
_LUMA = {(capi.YUV_FULL, False): (0.0, 1.0), (capi.YUV_FULL, True): (0.0, 1.0), (capi.YUV_LIMITED, False): (16.0, 1.164383),
         (capi.YUV_LIMITED, True): (64.0, 1.167808)}


def yuv_literals(color_range, primaries, ten_bit):
    """(ysub, yscale, rv, gu, gv, bu, csub, amax) as float32: the literals of the bilinear NV12 kind's conversion."""
    k = _LUMA[(color_range, ten_bit)] + _MATRIX[(color_range, ten_bit)][primaries] + ((512.0, 1023.0) if ten_bit else (128.0, 255.0))
    return tuple(F32(c) for c in k)


def convert_f32(Y, U, V, color_range, primaries, ten_bit, alpha):
    """The bilinear NV12 kind's per-tap conversion on float32 arrays, every operation rounded once."""
    ysub, yscale, rv, gu, gv, bu, csub, amax = yuv_literals(color_range, primaries, ten_bit)
    cb, cr = (U - csub).astype(F32), (V - csub).astype(F32)
    yv = ((Y - ysub).astype(F32) * yscale).astype(F32)
    r = (yv + (rv * cr).astype(F32)).astype(F32)
    g = ((yv + (gu * cb).astype(F32)).astype(F32) + (gv * cr).astype(F32)).astype(F32)
    b = (yv + (bu * cb).astype(F32)).astype(F32)
    chans = [r, g, b] + ([np.full_like(r, amax)] if alpha else [])
    return np.stack(chans, -1)


def view_codes(surface, layout, crop):
    """(luma codes (h, w, 1), chroma codes (ceil(h/2), ceil(w/2), 2) in (U, V) order) of a crop at an even origin, float32."""
    x, y, w, h = crop
    assert not (x | y) & 1
    nch, ncw = (h + 1) // 2, (w + 1) // 2
    luma = surface[y:y + h, x:x + w]
    pairs = surface[SRC_H + y // 2:SRC_H + y // 2 + nch, x:x + 2 * ncw].reshape(nch, ncw, 2)
    if layout == capi.YUV_P010:
        luma, pairs = luma >> 6, pairs >> 6
    if layout == capi.YUV_NV21:
        pairs = pairs[..., ::-1]
    return luma.astype(F32)[..., None], pairs.astype(F32)


def yuv_area_plane_f32(surface, layout, crop, P, dst_w, dst_h, bg, yuv):
    """One plane: (dst_h, dst_w, 3 | 4) float32; outside the window the background.  yuv = (range, primaries, alpha)."""
    color_range, primaries, alpha = yuv
    cn = 4 if alpha else 3
    out = np.empty((dst_h, dst_w, cn), F32)
    out[:] = np.asarray(bg[:cn], F32)
    x1, y1, x2, y2 = P["x1"], P["y1"], P["x2"], P["y2"]
    if x2 < x1 or y2 < y1:
        return out
    assert crop[2] == P["w"] and crop[3] == P["h"]
    luma, pairs = view_codes(surface, layout, crop)
    nx, ny = x2 - x1 + 1, y2 - y1 + 1
    Ym = _nest(luma, A.axis_taps_f32(ny, P["fy"], P["h"]), A.axis_taps_f32(nx, P["fx"], P["w"]))
    Cm = _nest(pairs, chroma_axis_taps_f32(ny, P["fy"], P["h"]), chroma_axis_taps_f32(nx, P["fx"], P["w"]))
    out[y1:y2 + 1, x1:x2 + 1, :] = convert_f32(Ym[..., 0], Cm[..., 0], Cm[..., 1], color_range, primaries, layout == capi.YUV_P010, alpha)
    return out


# ---- the independent float64 model -----------------------------------------------------------------------------------------------------
def yuv_area_plane_f64(surface, layout, crop, P, dst_w, dst_h, bg, yuv):
    color_range, primaries, alpha = yuv
    x, y, w, h = crop
    view = F.View(surface, x, y, w, h, luma_h=SRC_H)
    ty, tx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rgb = F.convert_yuv(F.yuv_taps(view, layout, ty, tx), 0.0, color_range, primaries, layout == capi.YUV_P010, bool(alpha)).v
    return A.area_plane_f64(rgb, P, dst_w, dst_h, bg)


# ---- a whole chain -----------------------------------------------------------------------------------------------------------------------
def yuv_area_chain(plane_fn, surface, layout, crops, params, dsize, used, bg, yuv, ops, dtype):
    """(batch, dst_h, dst_w, cn_out): every plane through plane_fn, planes >= used take the default value, then the program on everything."""
    dst_w, dst_h = dsize
    cn = 4 if yuv[2] else 3
    planes = []
    for z, crop in enumerate(crops):
        if z < used:
            planes.append(plane_fn(surface, layout, crop, params[z], dst_w, dst_h, bg, yuv).astype(dtype))
        else:
            p = np.empty((dst_h, dst_w, cn), dtype)
            p[:] = np.asarray(bg[:cn], F32).astype(dtype)
            planes.append(p)
    return A.apply_program(np.stack(planes), ops)
