"""CVGS_WRITE_NV12 (include/cvgs_hip.h) twice over, for tests/test_nv12_write.py and tests/test_gpu_nv12_write.py:

 * write_f32: a numpy fp32 restatement of the contract -- the header's operations in the header's order, every one rounded once to
   float32, the header's 6-decimal literals.  The kernels must store these bytes, bit for bit.
 * write_f64: an independent float64 model -- constants taken from the standards' luma weights with exact division, nothing rounded
   before the final byte.  It says how far the fp32 contract is from the real conversion (tests/test_nv12_write.py).

Both take the float R, G, B picture that reaches the write stage ([H, W, 3], H and W even) and return (luma [H, W], chroma [H/2, W])
as uint8, chroma interleaved in the layout's order."""
import numpy as np

FULL, LIMITED = 0, 1
BT601, BT709, BT2020 = 0, 1, 2
NV12, NV21 = 0, 1

# the standards' luma weights (Kr, Kb); Kg = 1 - Kr - Kb
WEIGHTS = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}
# the literals of yuv_write_matrix (csrc/k_nv12_write.hip) and of the header: kr, kg, kb, cu, cv
LITERALS = {BT601: (0.299, 0.587, 0.114, 0.564334, 0.713267),
            BT709: (0.2126, 0.7152, 0.0722, 0.538909, 0.635001),
            BT2020: (0.2627, 0.678, 0.0593, 0.531519, 0.67815)}
SY, SC = 0.858824, 0.878431  # 219 / 255, 224 / 255
PAIRS = [(r, p) for r in (FULL, LIMITED) for p in (BT601, BT709, BT2020)]


def derived(primaries):
    """(kr, kg, kb, cu, cv) in float64 from the luma weights."""
    kr, kb = WEIGHTS[primaries]
    return kr, 1.0 - kr - kb, kb, 0.5 / (1.0 - kb), 0.5 / (1.0 - kr)


def to_u8(v):
    """The CVGS_OP_CAST-to-8U rule: round to nearest even, saturate to 0..255, NaN -> 0."""
    v = np.asarray(v)
    r = np.rint(v)
    r = np.where(np.isnan(v), 0, r)
    return np.clip(r, 0, 255).astype(np.uint8)


def _interleave(ub, vb, layout):
    h2, w2 = ub.shape
    out = np.empty((h2, 2 * w2), np.uint8)
    out[:, 0::2] = ub if layout == NV12 else vb
    out[:, 1::2] = vb if layout == NV12 else ub
    return out


def yuv_f32(rgb, color_range, primaries):
    """The float Y, U, V planes of the contract, fp32."""
    f = np.float32
    rgb = np.asarray(rgb, np.float32)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    kr, kg, kb, cu, cv = (f(v) for v in LITERALS[primaries])
    with np.errstate(all="ignore"):
        y = (kr * R + kg * G) + kb * B
        cb = (B - y) * cu
        cr = (R - y) * cv
        if color_range == LIMITED:
            return y * f(SY) + f(16.0), cb * f(SC) + f(128.0), cr * f(SC) + f(128.0)
        return y, cb + f(128.0), cr + f(128.0)


def block_mean_f32(c):
    """The float chroma sample of every 2 x 2 block of a float32 plane [H, W]: top row, bottom row, then the quarter."""
    assert c.dtype == np.float32
    with np.errstate(all="ignore"):
        m = ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * np.float32(0.25)
    assert m.dtype == np.float32
    return m


def write_f32(rgb, color_range, primaries, layout=NV12):
    Y, U, V = yuv_f32(rgb, color_range, primaries)
    assert Y.dtype == np.float32 and U.dtype == np.float32 and Y.shape[0] % 2 == 0 and Y.shape[1] % 2 == 0
    return to_u8(Y), _interleave(to_u8(block_mean_f32(U)), to_u8(block_mean_f32(V)), layout)


def yuv_f64(rgb, color_range, primaries):
    """The float64 model's values in front of the final rounding: (Y [H, W], U [H/2, W/2], V [H/2, W/2])."""
    rgb = np.asarray(rgb, np.float64)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    kr, kg, kb, cu, cv = derived(primaries)
    y = kr * R + kg * G + kb * B
    cb, cr = (B - y) * cu, (R - y) * cv
    if color_range == LIMITED:
        Y, U, V = y * (219.0 / 255.0) + 16.0, cb * (224.0 / 255.0) + 128.0, cr * (224.0 / 255.0) + 128.0
    else:
        Y, U, V = y, cb + 128.0, cr + 128.0
    ub = (U[0::2, 0::2] + U[0::2, 1::2] + U[1::2, 0::2] + U[1::2, 1::2]) / 4.0
    vb = (V[0::2, 0::2] + V[0::2, 1::2] + V[1::2, 0::2] + V[1::2, 1::2]) / 4.0
    return Y, ub, vb


def write_f64(rgb, color_range, primaries, layout=NV12):
    Y, ub, vb = yuv_f64(rgb, color_range, primaries)
    return to_u8(Y), _interleave(to_u8(ub), to_u8(vb), layout)


def surface_image(luma, chroma, step, uv_offset, total, fill):
    """The bytes of a surface buffer of `total` bytes that held `fill` everywhere before the write: luma rows at y * step, chroma rows at
    uv_offset + y * step, the row padding and everything else untouched."""
    h, w = luma.shape
    buf = np.full(total, fill, np.uint8)
    for y in range(h):
        buf[y * step:y * step + w] = luma[y]
    for y in range(h // 2):
        buf[uv_offset + y * step:uv_offset + y * step + w] = chroma[y]
    return buf


def random_surface(w, h, seed):
    """An NV12 surface [3h/2, w] whose luma and chroma both hold every code 0..255 (w * h >= 512), seeded."""
    rng = np.random.RandomState(seed)
    s = rng.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    assert w * h >= 512 and w * (h // 2) >= 256
    s[:h].reshape(-1)[rng.permutation(w * h)[:256]] = np.arange(256, dtype=np.uint8)
    s[h:].reshape(-1)[rng.permutation(w * (h // 2))[:256]] = np.arange(256, dtype=np.uint8)
    return s
