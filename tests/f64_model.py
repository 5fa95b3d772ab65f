"""An independent float64 model of every read and pointwise stage, with a DERIVED error bound per output element.

Written from the published definitions -- OpenCV-CUDA's resize_linear (no half-pixel offset, floor, +1 tap clamped to the last
column / row, weights from the unclamped neighbour), the BT.601 / BT.709 / BT.2020 luma weights (Kr, Kb), the FOURCC layouts (NV12,
NV21, I420, YV12, P010, YUYV, UYVY, I444), cv::saturate_cast (round to nearest even, clamp, NaN -> 0) and IEEE binary16 / bfloat16 rounding --
and NOT from oracle/cvgs_oracle.c.  Nothing here imports oracle/ or the product package: the iop objects the tests build are read by
attribute only, and the numeric codes below are those of the public C header (include/cvgs_hip.h).

evaluate(iops, views) -> Result: for every output element a value v and an absolute bound b (float64, logical order [plane][y][x][c]).

Two fp32 quantities are part of the operation's DEFINITION and are reproduced exactly: the scale float32(1 / (dst / src)) and the source
coordinate float32(i) * scale (one fp32 product).  Taps, weights and sums are float64.

The bound is carried forward with u = 2^-24:
  * every fp32 operation of the specified evaluation adds u * |result| to the propagated bound of its inputs (Val.mul / add / div);
  * the bilinear sum adds K_BILINEAR * u * sum |w_i p_i| with K_BILINEAR = 7, counted from the specified order
    acc = p00*w00; acc += p10*w10; acc += p01*w01; acc += p11*w11 with w = wx * wy, wx = float(x2) - sx (or sx - float(x1)):
    2 (one rounding in each 1-D weight difference) + 1 (the weight product) + 1 (the tap product) + 3 (the additions; the first term
    passes through all three);
  * the 6-decimal coefficient literals of the YCbCr matrices add half a unit of their last digit (0.5e-6) times |chroma| (|luma| for
    the luma scale), and u * |coefficient| for the literal's own narrowing to fp32;
  * warps add the coordinate term: the fp32 coordinate differs from the float64 one by at most
    delta = K_COORD * u * (|m0 x| + |m1 y| + |m2|), K_COORD = 3 (a product and two additions at most on every term), divided through
    for perspective (first order, inflated by 2^-10 for the remainder); bilinear interpolation is continuous across integer
    coordinates, so the value moves by at most delta_x * max|d/dx| + delta_y * max|d/dy| over the 3x3 cells around the tap.  Only the
    source BORDER is a discontinuity (zero against a value): pixels within delta of it are reported in Result.excluded.

Acceptance (Result.check): a float output g passes iff |g - v| <= b + one output-format rounding of (|v| + b); an integer output passes
iff g lies in [sat(r(v - b)), sat(r(v + b))], r = round-to-nearest-even (saturating cast) or truncation (fk::Cast).

Every defining choice is a named switch (SPEC) that defaults to the specification; tests/test_model_vs_oracle.py flips each one and
shows that the oracle then falls outside the bound somewhere on its grid."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
K_BILINEAR = 7
K_COORD = 3
LITERAL_HALF_DIGIT = 0.5e-6

# include/cvgs_hip.h
DEPTH_8U, DEPTH_8S, DEPTH_16U, DEPTH_16S, DEPTH_32S, DEPTH_32F, DEPTH_64F, DEPTH_16F = range(8)
FLAG_BF16 = 0x1000
DEPTH_16BF = DEPTH_16F | FLAG_BF16
READ_PIXEL, READ_RESIZE, READ_YUV, READ_YUV_RESIZE, READ_WARP_AFFINE, READ_WARP_PERSPECTIVE = range(6)
PRESERVE_AR, IGNORE_AR, PRESERVE_AR_RN_EVEN, PRESERVE_AR_LEFT = 0, 1, 2, 3
FULL, LIMITED = 0, 1
NV12, NV21, I420, YV12, P010, YUYV, UYVY, I444 = range(8)
BT601, BT709, BT2020 = 0, 1, 2
(OP_NOP, OP_CAST, OP_MUL, OP_ADD, OP_SUB, OP_DIV, OP_REORDER, OP_ADD_ALPHA, OP_DROP_ALPHA, OP_GRAY, OP_CAST_TRUNC) = range(11)
WRITE_PIXEL_2D, WRITE_PIXEL_3D, WRITE_SPLIT, WRITE_T_SPLIT = 0, 1, 2, 3

LUMA_WEIGHTS = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}  # (Kr, Kb) of the recommendations
INT_RANGE = {DEPTH_8U: (0, 255), DEPTH_8S: (-128, 127), DEPTH_16U: (0, 65535), DEPTH_16S: (-32768, 32767),
             DEPTH_32S: (-2 ** 31, 2 ** 31 - 1)}
FLOAT_FORMAT = {DEPTH_32F: (24, -126), DEPTH_16F: (11, -14), DEPTH_16BF: (8, -126)}  # (precision bits, minimum normal exponent)

# Every defining choice; False = the specification.
SPEC = {
    "half_pixel_centres": False,        # source coordinate (i + 0.5) * scale - 0.5 instead of i * scale
    "weights_from_clamped": False,      # weights from the clamped +1 neighbour instead of the unclamped one
    "chroma_rounds_up": False,          # chroma sample index (x + 1) / 2 instead of x / 2
    "chroma_from_crop_origin": False,   # chroma indexed from the crop's own origin against the surface's chroma plane
    "uv_swapped": False,                # U and V exchanged
    "yuyv_uyvy_swapped": False,         # YUYV read as UYVY and the reverse
    "blend_before_convert": False,      # luma blended, chroma taken once from the first tap, converted once (see _resize_plane)
    "limited_as_full": False,           # limited range treated as full range
    "bt601_for_bt709": False,           # BT.601 weights where BT.709 is asked for
    "saturate_truncates": False,        # the saturating cast truncates instead of rounding to nearest even
    "ar_extent_truncated": False,       # PRESERVE_AR: fitted extent truncated instead of rounded
    "warp_border_replicate": False,     # warp: outside pixels replicate the border instead of being zero
    "coefficient_digit_off": False,     # the sixth decimal of every chroma coefficient off by one
    "i444_chroma_subsampled": False,    # I444 chroma taken at (x / 2, y / 2), the 4:2:0 index, instead of the luma's own (x, y)
}


def switches(**flipped):
    s = dict(SPEC)
    for k, v in flipped.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def half_ulp(x, depth):
    """Half a unit in the last place of |x| in the float format of `depth`: the largest error of one rounding to nearest."""
    p, emin = FLOAT_FORMAT[depth]
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.where(ax > 0, np.maximum(e, emin), emin)
    return np.ldexp(1.0, (e - p).astype(np.int64))


def rne_float(x, depth):
    """x (float64) rounded to nearest even in the float format of `depth`, overflow to infinity, subnormals kept (IEEE 754)."""
    p, emin = FLOAT_FORMAT[depth]
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    e = np.floor(np.log2(np.where((ax > 0) & np.isfinite(ax), ax, 1.0)))
    q = np.ldexp(1.0, (np.maximum(e, emin) - (p - 1)).astype(np.int64))  # one unit in the last place
    r = np.rint(x / q) * q                                                 # np.rint: ties to even; x / q is exact (power of two)
    emax = {DEPTH_32F: 127, DEPTH_16F: 15, DEPTH_16BF: 127}[depth]
    big = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    r = np.where(np.abs(r) > big, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def widen(arr, depth):
    """Source samples as float64, exactly.  CV_16BF sources are uint16 bit patterns."""
    if depth == DEPTH_16BF:
        return (np.ascontiguousarray(arr).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.asarray(arr).astype(np.float64)


class View:
    """A crop (x, y, w, h) of a surface held in a numpy array.  Plain images: (H, W[, C]).  4:2:0 surfaces: the whole (luma_h * 3 / 2, W)
    array with `luma_h` luma rows.  Packed 4:2:2: (H, W, 2).  Planar 4:4:4: the three planes stacked, (3, H, W), with x, y, w, h given.
    A padded pitch is a crop of a wider array."""

    def __init__(self, arr, x=0, y=0, w=None, h=None, luma_h=None):
        self.arr, self.x, self.y, self.luma_h = arr, int(x), int(y), luma_h
        full_h = luma_h if luma_h is not None else arr.shape[0]
        self.w = int(w) if w is not None else arr.shape[1] - self.x
        self.h = int(h) if h is not None else full_h - self.y


class Val:
    """Values with bounds, float64 (..., C).  depth: the type the chain carries.  `pending`: a rounding to a 16-bit float format that has
    not been charged to b yet (charged by the next stage, or by the acceptance as the output format's one rounding)."""

    def __init__(self, v, b, depth, pending=None):
        self.v, self.b, self.depth, self.pending = np.asarray(v, np.float64), np.asarray(b, np.float64) + np.zeros_like(v), depth, pending

    def settle(self):
        if self.pending is not None:
            self.b = self.b + half_ulp(np.abs(self.v) + self.b, self.pending)
            self.pending = None
        return self

    def mul(self, c, literal_error=0.0, narrowing=False):
        """fp32 product with a constant c: one rounding, plus what c itself may be off by."""
        c = np.asarray(c, np.float64)
        v = self.v * c
        cerr = literal_error + (U * np.abs(c) if narrowing else 0.0)
        return Val(v, self.b * (np.abs(c) + cerr) + cerr * np.abs(self.v) + U * (np.abs(v) + self.b * np.abs(c)), self.depth)

    def add(self, o, sign=1.0):
        ov, ob = (o.v, o.b) if isinstance(o, Val) else (np.asarray(o, np.float64), 0.0)
        v = self.v + sign * ov
        bb = self.b + ob
        return Val(v, bb + U * (np.abs(v) + bb), self.depth)

    def div(self, c):
        c = np.asarray(c, np.float64)
        v = self.v / c
        bb = self.b / np.abs(c)
        return Val(v, bb + U * (np.abs(v) + bb), self.depth)


# ---- colour ---------------------------------------------------------------------------------------------------------------------------
def yuv_matrix(color_range, primaries, ten_bit, sw=SPEC):
    """(ysub, yscale, rv, gu, gv, bu, csub, amax) in float64 from Kr / Kb: R = Y' + 2(1-Kr) Cr, B = Y' + 2(1-Kb) Cb,
    G = Y' - 2 Kb (1-Kb) / Kg Cb - 2 Kr (1-Kr) / Kg Cr, Kg = 1 - Kr - Kb; limited range: luma (Y - 16) * 255/219, chroma * 255/224 on
    8-bit codes, (Y - 64) * 1023/876 and * 1023/896 on 10-bit codes."""
    if sw["bt601_for_bt709"] and primaries == BT709:
        primaries = BT601
    if sw["limited_as_full"]:
        color_range = FULL
    kr, kb = LUMA_WEIGHTS[primaries]
    kg = 1.0 - kr - kb
    m = np.array([2.0 * (1.0 - kr), -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg, 2.0 * (1.0 - kb)])
    ysub, yscale = 0.0, 1.0
    if color_range == LIMITED:
        top = 1023.0 if ten_bit else 255.0
        ysub = 64.0 if ten_bit else 16.0
        yscale = top / (876.0 if ten_bit else 219.0)
        m = m * (top / (896.0 if ten_bit else 224.0))
    if sw["coefficient_digit_off"]:
        m = m + np.sign(m) * 1e-6
    return (ysub, yscale) + tuple(m) + ((512.0, 1023.0) if ten_bit else (128.0, 255.0))


def convert_yuv(yuv, yuv_b, color_range, primaries, ten_bit, alpha, sw=SPEC):
    """(..., 3) Y, U, V codes -> RGB(A) Val.  Subtractions of the offsets are exact on codes; each coefficient product and each
    sum is one fp32 operation of the specified evaluation yv = (Y - ysub) * yscale; R = yv + rv cr; G = (yv + gu cb) + gv cr;
    B = yv + bu cb."""
    ysub, yscale, rv, gu, gv, bu, csub, amax = yuv_matrix(color_range, primaries, ten_bit, sw)
    lit = LITERAL_HALF_DIGIT
    y = Val(yuv[..., 0] - ysub, yuv_b[..., 0] if np.ndim(yuv_b) else yuv_b, DEPTH_32F)
    cb = Val(yuv[..., 1] - csub, yuv_b[..., 1] if np.ndim(yuv_b) else yuv_b, DEPTH_32F)
    cr = Val(yuv[..., 2] - csub, yuv_b[..., 2] if np.ndim(yuv_b) else yuv_b, DEPTH_32F)
    yv = y.mul(yscale, lit, True) if yscale != 1.0 else y
    r = yv.add(cr.mul(rv, lit, True))
    g = yv.add(cb.mul(gu, lit, True)).add(cr.mul(gv, lit, True))
    b = yv.add(cb.mul(bu, lit, True))
    chans = [r, g, b] + ([Val(np.full_like(r.v, amax), 0.0, DEPTH_32F)] if alpha else [])
    return Val(np.stack([c.v for c in chans], -1), np.stack([c.b for c in chans], -1), DEPTH_32F)


def yuv_taps(view, layout, ty, tx, sw=SPEC):
    """Y, U, V codes (float64, (..., 3)) of the crop's pixels (ty, tx).  Chroma of a pixel is the sample of its 2x2 block (4:2:0) or of
    its horizontal pair (4:2:2) in SURFACE coordinates; 4:4:4 has one chroma sample per pixel, at the luma's own coordinates."""
    a = view.arr
    if sw["yuyv_uyvy_swapped"] and layout in (YUYV, UYVY):
        layout = UYVY if layout == YUYV else YUYV
    sy, sx = view.y + ty, view.x + tx
    cy, cx = (ty, tx) if sw["chroma_from_crop_origin"] else (sy, sx)
    if layout in (YUYV, UYVY):
        yi, ci = (0, 1) if layout == YUYV else (1, 0)
        px = (cx + 1) // 2 if sw["chroma_rounds_up"] else cx // 2
        px = np.minimum(px, a.shape[1] // 2 - 1)
        row = sy if not sw["chroma_from_crop_origin"] else cy
        y_, u_, v_ = a[sy, sx, yi], a[row, 2 * px, ci], a[row, 2 * px + 1, ci]
    elif layout == I444:
        px, py = (cx // 2, cy // 2) if sw["i444_chroma_subsampled"] else (cx, cy)
        y_, u_, v_ = a[0, sy, sx], a[1, py, px], a[2, py, px]
    else:
        H, W = view.luma_h, a.shape[1]
        if sw["chroma_rounds_up"]:
            px, py = np.minimum((cx + 1) // 2, W // 2 - 1), np.minimum((cy + 1) // 2, H // 2 - 1)
        else:
            px, py = cx // 2, cy // 2
        y_ = a[sy, sx]
        if layout in (NV12, NV21, P010):
            first, second = a[H + py, 2 * px], a[H + py, 2 * px + 1]
            u_, v_ = (second, first) if layout == NV21 else (first, second)
        else:  # planar chroma: the U plane then the V plane (YV12: V then U), (W/2) x (H/2) samples each, packed behind the luma
            flat = np.ascontiguousarray(a[H:]).reshape(-1)
            first, second = flat[py * (W // 2) + px], flat[(H // 2) * (W // 2) + py * (W // 2) + px]
            u_, v_ = (second, first) if layout == YV12 else (first, second)
        if layout == P010:
            y_, u_, v_ = y_ >> 6, u_ >> 6, v_ >> 6
    if sw["uv_swapped"]:
        u_, v_ = v_, u_
    y_, u_, v_ = np.broadcast_arrays(y_, u_, v_)
    return np.stack([y_, u_, v_], -1).astype(np.float64)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def exact_window(sw_, sh, dw, dh, ar, truncate=False):
    """The aspect-ratio window in exact arithmetic: scale by height, fall back to width when it does not fit, extents
    rounded half away from zero (RN_EVEN: then down to even), centred (LEFT: x = 0).  Returns (x1, y1, x2, y2, margin)
    where margin = distance of the rounded quantity from the nearest .5 tie.  truncate=True: the rule the reference's own test spells on
    its OpenCV side; the two differ on the sizes listed in tests/golden/ar_extent_differences.json, which holds the product to ROUND."""
    def rnd(q):
        return (int(q) if truncate else int(q + Fraction(1, 2))), abs((q - int(q)) - Fraction(1, 2))
    tw, m = rnd(Fraction(dh * sw_, sh))
    th = dh
    if ar == PRESERVE_AR_RN_EVEN:
        tw -= tw % 2
    if tw > dw:
        tw = dw
        th, m = rnd(Fraction(dw * sh, sw_))
        if ar == PRESERVE_AR_RN_EVEN:
            th -= th % 2
    tw, th = max(tw, 1), max(th, 1)
    x1 = 0 if ar == PRESERVE_AR_LEFT else (dw - tw) // 2
    y1 = (dh - th) // 2
    return x1, y1, x1 + tw - 1, y1 + th - 1, float(m)


def resize_coords(n_out, n_src, sw=SPEC):
    """Source coordinates of n_out destination samples over n_src source samples: float32(i) * float32(1 / (n_out / n_src)), the
    product rounded once to fp32 -- returned as float64."""
    scale = np.float32(1.0 / (float(n_out) / float(n_src)))
    i = np.arange(n_out, dtype=np.float32)
    if sw["half_pixel_centres"]:
        return np.maximum((i.astype(np.float64) + 0.5) * float(scale) - 0.5, 0.0)
    return (i * scale).astype(np.float64)


def bilinear(tap, sx, sy, w, h, sw=SPEC):
    """sum of the four taps at (floor, floor + 1 clamped); sx, sy broadcast against each other.  tap(ty, tx) -> Val of (..., C).
    Returns the Val of the blend, its bound being the taps' own bounds blended plus K_BILINEAR * u * sum |w p|."""
    x1, y1 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    ax, ay = sx - x1, sy - y1
    wx = (1.0 - ax, ax)
    wy = (1.0 - ay, ay)
    if sw["weights_from_clamped"]:
        wx, wy = (x2 - sx, ax), (y2 - sy, ay)
    v = b = mag = 0.0
    for (yy, wyy) in ((y1, wy[0]), (y2, wy[1])):
        for (xx, wxx) in ((x1, wx[0]), (x2, wx[1])):
            t = tap(yy, xx)
            wgt = (wyy * wxx)[..., None]
            v = v + t.v * wgt
            b = b + t.b * np.abs(wgt)
            mag = mag + (np.abs(t.v) + t.b) * np.abs(wgt)
    return Val(v, b + K_BILINEAR * U * mag, DEPTH_32F)


def _plain_tap(view, depth):
    a = view.arr.reshape(view.arr.shape[0], view.arr.shape[1], -1)
    img = widen(a[view.y:view.y + view.h, view.x:view.x + view.w], depth)
    return img, (lambda ty, tx: Val(img[ty, tx], 0.0, DEPTH_32F))


def _background(rd, cn, shape):
    return Val(np.broadcast_to(f32(list(rd.background)[:cn]), shape + (cn,)).copy(), 0.0, DEPTH_32F)


def _resize_plane(rd, view, is_yuv, layout, sw):
    dw, dh = rd.dsize
    cn = (4 if rd.yuv[2] else 3) if is_yuv else type_cn(rd.src_type)
    if rd.ar == IGNORE_AR:
        x1, y1, x2, y2 = 0, 0, dw - 1, dh - 1
    else:
        x1, y1, x2, y2, _ = exact_window(view.w, view.h, dw, dh, rd.ar, sw["ar_extent_truncated"])
    tw, th = x2 - x1 + 1, y2 - y1 + 1
    sx, sy = resize_coords(tw, view.w, sw)[None, :], resize_coords(th, view.h, sw)[:, None]
    if is_yuv:
        args = (rd.yuv[0], rd.yuv[1], layout == P010, bool(rd.yuv[2]), sw)
        tap = lambda ty, tx: convert_yuv(yuv_taps(view, layout, ty, tx, sw), 0.0, *args)  # noqa: E731  convert each tap, then blend
        if sw["blend_before_convert"]:
            # the mistake this switch stands for: the luma plane is interpolated, the chroma is sited once (the first tap's sample)
            # and the blend is converted once.  (Blending the four taps' own Y, U, V and converting afterwards is algebraically the
            # SAME value -- the conversion is affine and the weights sum to one -- so that order differs by rounding only.)
            raw = lambda ty, tx: Val(yuv_taps(view, layout, ty, tx, sw)[..., :1], 0.0, DEPTH_32F)  # noqa: E731
            luma = bilinear(raw, sx, sy, view.w, view.h, sw)
            first = yuv_taps(view, layout, np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64), sw)
            inner = convert_yuv(np.concatenate([luma.v, first[..., 1:]], -1), np.concatenate([luma.b, 0 * first[..., 1:]], -1), *args)
        else:
            inner = bilinear(tap, sx, sy, view.w, view.h, sw)
    else:
        _, tap = _plain_tap(view, depth_of(rd.src_type))
        inner = bilinear(tap, sx, sy, view.w, view.h, sw)
    out = _background(rd, cn, (dh, dw))
    out.v[y1:y2 + 1, x1:x2 + 1] = inner.v
    out.b[y1:y2 + 1, x1:x2 + 1] = inner.b
    return out


def _neighbourhood_max(d, rows, cols):
    """max of d over a window of `rows` x `cols` cells starting one cell up / left of each position (edges replicated)."""
    p = np.pad(d, ((1, rows - 2), (1, cols - 2), (0, 0)), mode="edge")
    out = np.zeros_like(d)
    for i in range(rows):
        for j in range(cols):
            out = np.maximum(out, p[i:i + d.shape[0], j:j + d.shape[1]])
    return out


def _warp_plane(rd, view, m, persp, sw):
    """Warp of one plane: coordinates in float64 from the fp32-narrowed inverse matrix m (9 values), zero outside the source."""
    dw, dh = rd.dsize
    img, tap = _plain_tap(view, depth_of(rd.src_type))
    h, w, cn = img.shape
    m = f32(m)
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)

    def row(k):
        val = m[k] * xs + m[k + 1] * ys + m[k + 2]
        return val, K_COORD * U * (np.abs(m[k] * xs) + np.abs(m[k + 1] * ys) + np.abs(m[k + 2]))
    sx, dx = row(0)
    sy, dy = row(3)
    if persp:
        den, dd = row(6)
        sx, sy = sx / den, sy / den
        grow = 1.0 + 2.0 ** -10
        dx = ((dx + np.abs(sx) * dd) / np.abs(den)) * grow + U * np.abs(sx)
        dy = ((dy + np.abs(sy) * dd) / np.abs(den)) * grow + U * np.abs(sy)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    near = ((np.abs(sx) <= dx) | (np.abs(sx - w) <= dx) | (np.abs(sy) <= dy) | (np.abs(sy - h) <= dy))
    excluded = near & (sx >= -dx) & (sx <= w + dx) & (sy >= -dy) & (sy <= h + dy)
    if sw["warp_border_replicate"]:
        take, cx, cy = np.ones_like(inside), np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    else:
        take, cx, cy = inside, np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    val = bilinear(tap, cx, cy, w, h, sw)
    # the value term of the coordinate error: the steepest horizontal / vertical step of the 3x3 cells around the tap
    gx = np.zeros_like(img)
    gy = np.zeros_like(img)
    gx[:, :-1] = np.abs(img[:, 1:] - img[:, :-1])
    gy[:-1, :] = np.abs(img[1:, :] - img[:-1, :])
    gx, gy = _neighbourhood_max(gx, 4, 3), _neighbourhood_max(gy, 3, 4)
    x1, y1 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    b = val.b + dx[..., None] * gx[y1, x1] + dy[..., None] * gy[y1, x1]
    t = take[..., None]
    return Val(np.where(t, val.v, 0.0), np.where(t, b, 0.0), DEPTH_32F), excluded, (sx, sy, inside)


# ---- types ----------------------------------------------------------------------------------------------------------------------------
def type_cn(t):
    return ((t >> 3) & 63) + 1


def depth_of(t):
    return DEPTH_16BF if (t & 7) == DEPTH_16F and (t & FLAG_BF16) else (t & 7)


def _cast(x, dst, truncating, sw):
    src = x.depth
    if dst == src:
        return x
    if dst in (DEPTH_16F, DEPTH_16BF):
        x = x.settle()
        return Val(x.v, x.b, dst, pending=dst)
    x = x.settle()
    if dst == DEPTH_32F:
        if src in (DEPTH_32S, DEPTH_64F):
            return Val(x.v, x.b + U * (np.abs(x.v) + x.b), dst)
        return Val(x.v, x.b, dst)  # 8- and 16-bit integers and 16-bit floats widen exactly
    if dst == DEPTH_64F:
        if src == DEPTH_32F:
            return Val(x.v, x.b, dst)  # every fp32 value is a double: exact, no bound added (64F ARITHMETIC: tests/exact_model.py)
        raise NotImplementedError("CV_64F chains are held by the exact model: tests/exact_model.py")
    lo, hi = INT_RANGE[dst]
    if src in INT_RANGE:
        a, c = np.clip(x.v - x.b, lo, hi), np.clip(x.v + x.b, lo, hi)
    else:
        r = np.trunc if (truncating or sw["saturate_truncates"]) else np.rint  # np.rint: ties to even
        nan = np.isnan(x.v)
        a = np.clip(r(np.where(nan, 0.0, x.v - x.b)), lo, hi)
        c = np.clip(r(np.where(nan, 0.0, x.v + x.b)), lo, hi)
    return Val((a + c) / 2.0, (c - a) / 2.0, dst)


def _reorder(x, aux, n):
    idx = [(aux >> (2 * c)) & 3 for c in range(n)]
    return Val(x.v[..., idx], x.b[..., idx], x.depth)


def apply_op(x, opcode, aux, operand, sw=SPEC):
    if opcode == OP_NOP:
        return x
    if opcode in (OP_CAST, OP_CAST_TRUNC):
        return _cast(x, aux, opcode == OP_CAST_TRUNC, sw)
    if opcode in (OP_REORDER, OP_DROP_ALPHA):
        return _reorder(x, aux, x.v.shape[-1] if opcode == OP_REORDER else 3)
    if opcode == OP_ADD_ALPHA:
        y = _reorder(x, aux, 3)
        a = np.full(y.v.shape[:-1] + (1,), float(np.float32(operand[0])))
        return Val(np.concatenate([y.v, a], -1), np.concatenate([y.b, 0 * a], -1), x.depth)
    x = x.settle()
    if opcode == OP_GRAY:  # CCIR 601 luma (r * 0.299 + g * 0.587) + b * 0.114 on the named channels, constants narrowed to fp32
        if x.depth not in (DEPTH_32F, DEPTH_8U, DEPTH_16U):
            raise NotImplementedError
        ch = [Val(x.v[..., (aux >> (2 * k)) & 3], x.b[..., (aux >> (2 * k)) & 3], DEPTH_32F) for k in range(3)]
        lum = ch[0].mul(f32(0.299)).add(ch[1].mul(f32(0.587))).add(ch[2].mul(f32(0.114)))
        out = Val(lum.v[..., None], lum.b[..., None], DEPTH_32F)
        return out if x.depth == DEPTH_32F else _cast(out, x.depth, False, SPEC)
    if x.depth != DEPTH_32F:
        raise NotImplementedError("arithmetic on integer-typed values is held by the exact model: tests/exact_model.py")
    c = f32(list(operand)[:x.v.shape[-1]])  # the scalar narrowed double -> float, part of the definition
    if opcode == OP_MUL:
        return x.mul(c)
    if opcode == OP_ADD:
        return x.add(c)
    if opcode == OP_SUB:
        return x.add(c, -1.0)
    if opcode == OP_DIV:
        return x.div(c)
    raise NotImplementedError(opcode)


class Result:
    def __init__(self, val, excluded):
        self.v, self.b, self.depth, self.pending = val.v, val.b, val.depth, val.pending
        self.excluded = excluded  # bool [plane][y][x] (warps only: within delta of the source border) or None

    def logical(self, got, write_kind):
        """A written output (any shape, memory order of the write kind) as [plane][y][x][c]: packed pixels, NCHW (split), CNHW (splitT)."""
        n, h, w, c = self.v.shape
        got = np.asarray(got)
        if write_kind == WRITE_SPLIT:
            return got.reshape(n, c, h, w).transpose(0, 2, 3, 1)
        if write_kind == WRITE_T_SPLIT:
            return got.reshape(c, n, h, w).transpose(1, 2, 3, 0)
        return got.reshape(n, h, w, c)

    def check(self, got):
        """got: [plane][y][x][c] in the output's own number format (16-bit floats widened to float64 by the caller).
        Returns (ok, ratio): ok per element (excluded pixels count as ok), ratio = |g - v| / tolerance."""
        g = np.asarray(got, np.float64)
        if self.depth in INT_RANGE:
            tol = self.b + 0.5
            ok = np.abs(g - self.v) <= self.b  # v, b are the centre and half-width of [sat(r(v - b)), sat(r(v + b))]
        else:
            fmt = self.depth if self.depth in FLOAT_FORMAT else DEPTH_32F
            tol = self.b + half_ulp(np.abs(self.v) + self.b, fmt)
            ok = np.abs(g - self.v) <= tol
        ratio = np.abs(g - self.v) / tol
        if self.excluded is not None:
            ok = ok | self.excluded[..., None]
            ratio = np.where(self.excluded[..., None], 0.0, ratio)
        return ok, ratio


def evaluate(iops, views, sw=SPEC):
    """iops: [read, pointwise..., write] as the tests build them; views: one View per plane of the read (the same memory the chain reads)."""
    rd = iops[0]
    n = rd.batch
    used = min(rd.used_planes, n)
    layout = getattr(rd, "yuv_layout", 0)
    planes, excl = [], None
    if rd.kind == READ_PIXEL:
        for z in range(n):
            a = views[z].arr.reshape(views[z].arr.shape[0], views[z].arr.shape[1], -1)
            d = depth_of(rd.src_type)
            planes.append(Val(widen(a[views[z].y:views[z].y + views[z].h, views[z].x:views[z].x + views[z].w], d), 0.0, d))
    elif rd.kind == READ_YUV:
        for z in range(n):
            ty, tx = np.mgrid[0:views[z].h, 0:views[z].w]
            planes.append(convert_yuv(yuv_taps(views[z], layout, ty, tx, sw), 0.0, rd.yuv[0], rd.yuv[1], layout == P010, bool(rd.yuv[2]), sw))
    elif rd.kind in (READ_RESIZE, READ_YUV_RESIZE):
        cn = (4 if rd.yuv[2] else 3) if rd.kind == READ_YUV_RESIZE else type_cn(rd.src_type)
        for z in range(n):
            planes.append(_resize_plane(rd, views[z], rd.kind == READ_YUV_RESIZE, layout, sw) if z < used
                          else _background(rd, cn, (rd.dsize[1], rd.dsize[0])))
    else:
        cn = type_cn(rd.src_type)
        excl = np.zeros((n, rd.dsize[1], rd.dsize[0]), bool)
        for z in range(n):
            if z < used:
                p, excl[z], _ = _warp_plane(rd, views[z], rd.warp[9 * z:9 * z + 9], rd.kind == READ_WARP_PERSPECTIVE, sw)
                planes.append(p)
            else:
                planes.append(_background(rd, cn, (rd.dsize[1], rd.dsize[0])))
    x = Val(np.stack([p.v for p in planes]), np.stack([p.b for p in planes]), planes[0].depth)
    for iop in iops[1:-1]:
        for opcode, aux, operand in iop.ops:
            x = apply_op(x, opcode, aux, operand, sw)
    return Result(x, excl)
