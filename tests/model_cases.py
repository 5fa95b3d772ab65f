"""The case grid of the float64 model (tests/f64_model.py), shared by tests/test_model_vs_oracle.py (CPU oracle) and
tests/test_gpu_model.py (kernels).  A case is a function of a backend B that builds the chain on B's memory and returns
(iops, views): the iop list and one f64_model.View per plane over the SAME numpy data.  Inputs are seeded and non-constant; ramps and a
chroma-only checkerboard stand where random noise would hide a siting error."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import helpers as H
from tests import warp_cases as WC

NP_OF_DEPTH = {cvgs.CV_8U: np.uint8, cvgs.CV_16U: np.uint16, cvgs.CV_16S: np.int16, cvgs.CV_32F: np.float32, cvgs.CV_16F: np.float16,
               cvgs.CV_32S: np.int32, cvgs.CV_8S: np.int8}
BG = [17.25, 99.5, 3.0, 200.0]


def np_dtype(cv_type):
    if capi.type_is_bf16(cv_type):
        return np.uint16
    return NP_OF_DEPTH[capi.type_depth(cv_type)]


class HostBackend:
    """Chains over numpy memory, for the CPU oracle.  The oracle knows neither bfloat16 nor packed 4:2:2: bf16_twin=True builds the
    fp32 twin of a CV_16BF chain (bf16 sources widened exactly, the final conversion left to the caller, as tests/test_gpu_bf16.py does);
    packed 4:2:2 chains go through tests/yuv422_cases.Expect."""
    device = False

    def __init__(self, bf16_twin=True):
        self.twin, self.sources, self.outs, self.rounded_to_bf16 = bf16_twin, [], [], False

    def T(self, cv_type):
        return (cv_type & ~capi.TYPE_FLAG_BF16 & ~7) | cvgs.CV_32F if (self.twin and capi.type_is_bf16(cv_type)) else cv_type

    def src(self, arr, cv_type):
        if self.twin and capi.type_is_bf16(cv_type):
            arr = np.ascontiguousarray((arr.astype(np.uint32) << 16).view(np.float32))
        self.sources.append(arr)
        return cvgs.GpuMat.from_array(arr, self.T(cv_type))

    def out(self, shape, cv_type):
        a = np.zeros(shape, np_dtype(self.T(cv_type)))
        self.outs.append(a)
        return cvgs.GpuMat.from_array(a, self.T(cv_type))

    def to16(self, f_type, h_type):
        if self.twin and capi.type_is_bf16(h_type):
            self.rounded_to_bf16 = True
            return []
        return [cvgs.convertTo(f_type, h_type)]

    def result(self):
        return self.outs[0]


class DeviceBackend:
    """Chains over device memory; every output sits between canary bands that must come back untouched."""
    device = True
    GUARD = 4096

    def __init__(self):
        self.keep, self.outs, self.sources = [], [], []

    def T(self, cv_type):
        return cv_type

    def src(self, arr, cv_type):
        import torch
        a = np.ascontiguousarray(arr)
        self.sources.append(a)
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        self.keep.append(t)
        return cvgs.GpuMat(a.shape[0], a.shape[1], cv_type, t.data_ptr(), a.strides[0], owner=t)

    def out(self, shape, cv_type):
        import torch
        a = np.zeros(shape, np_dtype(cv_type))
        big = torch.full((a.nbytes + 2 * self.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        big[self.GUARD:self.GUARD + a.nbytes].zero_()
        self.outs.append((big, a))
        return cvgs.GpuMat(shape[0], shape[1], cv_type, big.data_ptr() + self.GUARD, a.strides[0], owner=big)

    def to16(self, f_type, h_type):
        return [cvgs.convertTo(f_type, h_type)]

    def result(self):
        big, a = self.outs[0]
        g = big.cpu().numpy()
        assert (g[:self.GUARD] == 0xA5).all() and (g[-self.GUARD:] == 0xA5).all(), "store outside the output"
        return g[self.GUARD:-self.GUARD].view(a.dtype).reshape(a.shape)


def widen_output(got, cv_type):
    """An output array in its own number format as float64 (CV_16BF: uint16 bit patterns)."""
    return F.widen(got, F.depth_of(cv_type))


# ---- sources --------------------------------------------------------------------------------------------------------------------------
def random_src(shape, depth, seed):
    if depth == cvgs.CV_8U:
        return H.random_u8(shape, seed)
    w = H.random_u16(shape, seed)
    if depth == cvgs.CV_16U:
        return w
    if depth == cvgs.CV_16S:
        return w.view(np.int16)
    f = ((w.astype(np.float32) - 32768.0) / np.float32(37.0)).astype(np.float32)
    if depth == cvgs.CV_32F:
        return f
    if depth == cvgs.CV_16F:
        return f.astype(np.float16)
    if depth == capi.DEPTH_16BF:
        return (np.ascontiguousarray(f).view(np.uint32) >> 16).astype(np.uint16)
    raise ValueError(depth)


def src_type(depth, cn):
    return (cvgs.make_type(cvgs.CV_16F, cn) | capi.TYPE_FLAG_BF16) if depth == capi.DEPTH_16BF else cvgs.make_type(depth, cn)


def pattern(shape, kind, seed):
    """u8 plane: random, a horizontal or vertical ramp (every sample differs from its neighbour along the ramp), or a checkerboard."""
    h, w = shape
    if kind == "random":
        return H.random_u8(shape, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "ramp_h":
        return ((xx * 5 + 3) % 256).astype(np.uint8)
    if kind == "ramp_v":
        return ((yy * 7 + 1) % 256).astype(np.uint8)
    return np.where((xx + yy) % 2 == 0, 40, 220).astype(np.uint8)


def yuv_surface(layout, w, h, seed, kind="random", pitch=0):
    """A picture (w x h, both even) as one surface array.  kind: random | ramp_h | ramp_v | chroma_checker (flat luma, chroma planes a
    checkerboard: only the chroma siting shows)."""
    ck = "checker" if kind == "chroma_checker" else kind
    y = np.full((h, w), 120, np.uint8) if kind == "chroma_checker" else pattern((h, w), kind, seed)
    if layout in (capi.YUV_YUYV, capi.YUV_UYVY):
        u, v = pattern((h, w // 2), ck, seed + 1), pattern((h, w // 2), ck, seed + 2)[:, ::-1].copy()
        s = np.zeros((h, w + pitch, 2), np.uint8)
        s[..., :] = 77
        yi, ci = (0, 1) if layout == capi.YUV_YUYV else (1, 0)
        s[:, :w, yi] = y
        s[:, 0:w:2, ci] = u
        s[:, 1:w:2, ci] = v
        return s
    u, v = pattern((h // 2, w // 2), ck, seed + 1), pattern((h // 2, w // 2), ck, seed + 2)[:, ::-1].copy()
    s = np.full((h + h // 2, w + pitch), 77, np.uint8)
    s[:h, :w] = y
    if layout in (capi.YUV_NV12, capi.YUV_NV21, capi.YUV_P010):
        a, b = (v, u) if layout == capi.YUV_NV21 else (u, v)
        s[h:, 0:w:2] = a
        s[h:, 1:w:2] = b
        if layout == capi.YUV_P010:  # 10-bit codes in the high bits of 16-bit samples
            extra = H.random_u8(s.shape, seed + 3).astype(np.uint16) & 3
            s = ((s.astype(np.uint16) << 2) | extra) << 6
    else:
        assert pitch == 0
        first, second = (u, v) if layout == capi.YUV_I420 else (v, u)
        s[h:].reshape(-1)[:(h // 2) * (w // 2)] = first.reshape(-1)
        s[h:].reshape(-1)[(h // 2) * (w // 2):] = second.reshape(-1)
    return s


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
def normalise(cn, swap=True):
    """the headline chain: swap, x, -, / """
    f = cvgs.make_type(cvgs.CV_32F, cn)
    ops = []
    if swap and cn >= 3:
        ops.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f))
    return ops + [cvgs.multiply(f, [H.K1_ALPHA] * cn), cvgs.subtract(f, H.K1_SUB[cn] if cn in H.K1_SUB else [0.4] * cn),
                  cvgs.divide(f, H.K1_DIV[cn] if cn in H.K1_DIV else [0.25] * cn)]


ARITH_MUL, ARITH_ADD = [0.9, 0.8, 0.7, 0.6], [3.5, 2.25, 1.75, 0.5]  # tail="arith": stays inside 0..255 on u8 sources (integer outputs do not saturate flat)


def resize_case(depth, cn, frame_hw, crops, dst, ar=cvgs.IGNORE_AR, used=None, tail="none", write="split", seed=1, out16=None, out_int=None, table=False,
                pitch_pad=3):
    """tail: none | normalise (swap, x, -, /) | mul_sub_div (x, -, /) | arith (x, +) | interp (x, +, -, x, /: no canonical form).
    write: split | splitT | packed | planes2d (separate pitched fp32 planes, pitch_pad elements wider than the target).
    out_int: a packed integer output of that depth (the saturating cast folds into the store).  table: on a device backend the planes
    travel as a resident device table (cvgs_plane_table_build) instead of in the kernel arguments."""
    def build(B):
        st = src_type(depth, cn)
        frame = random_src((frame_hw[0], frame_hw[1], cn), depth, seed)
        m = B.src(frame, st)
        frame = B.sources[-1]  # (the oracle's fp32 twin of a bf16 source: the same values, widened)
        f = cvgs.make_type(cvgs.CV_32F, cn)
        n = len(crops)
        rd = cvgs.resize(B.T(st), cvgs.INTER_LINEAR, [m.roi(*c) for c in crops], dst, n if used is None else used, BG[:cn], ar)
        if table and B.device:
            import torch
            t = torch.frombuffer(bytearray(cvgs.build_plane_table(rd)), dtype=torch.uint8).cuda()
            B.keep.append(t)
            rd.table = t.data_ptr()
        if tail == "normalise":
            ops = normalise(cn)
        elif tail == "mul_sub_div":
            ops = normalise(cn, swap=False)
        elif tail == "arith":
            ops = [cvgs.multiply(f, ARITH_MUL[:cn]), cvgs.add(f, ARITH_ADD[:cn])]
        elif tail == "interp":
            ops = [cvgs.multiply(f, ARITH_MUL[:cn]), cvgs.add(f, ARITH_ADD[:cn]), cvgs.subtract(f, [0.4] * cn), cvgs.multiply(f, [1.25] * cn), cvgs.divide(f, [0.25] * cn)]
        else:
            assert tail == "none", tail
            ops = []
        ot = f
        if out16 is not None:
            ot = src_type(out16, cn)
            ops += B.to16(f, ot)
        if out_int is not None:
            ot = cvgs.make_type(out_int, cn)
            ops += [cvgs.convertTo(f, ot)]
        o1 = cvgs.make_type(capi.type_depth(ot), 1) | (ot & capi.TYPE_FLAG_BF16)
        if write == "split":
            wr = cvgs.split(B.T(ot), B.out((n, cn * dst[0] * dst[1]), o1), dst)
        elif write == "splitT":
            o = B.out((n, cn * dst[0] * dst[1]), o1)
            wr = cvgs.splitT(B.T(ot), o.data, dst[0], dst[1], n, keep=o)
        elif write == "planes2d":
            o = B.out((n * cn * dst[1], dst[0] + pitch_pad), cvgs.CV_32FC1)
            planes = [[cvgs.GpuMat(dst[1], dst[0], cvgs.CV_32FC1, o.data + ((z * cn + k) * dst[1]) * o.step, o.step, owner=o) for k in range(cn)] for z in range(n)]
            wr = cvgs.split(f, planes if n > 1 else planes[0])
        else:
            wr = cvgs.write(B.T(ot), B.out((n, dst[0] * dst[1], cn), ot), dst)
        return [rd] + ops + [wr], [F.View(frame, *c) for c in crops]
    return build


def yuv_case(layout, rng, prim, alpha, dst, crop=None, kind="random", pitch=0, w=48, h=32, tail="none", seed=7):
    def build(B):
        s = yuv_surface(layout, w, h, seed, kind, pitch)
        cn = 4 if alpha else 3
        f = cvgs.make_type(cvgs.CV_32F, cn)
        x, y, cw, chh = crop if crop is not None else (0, 0, w, h)
        if layout in (capi.YUV_YUYV, capi.YUV_UYVY):
            m = B.src(s, cvgs.make_type(cvgs.CV_8U, 2))
            mat = m.yuv422_roi(x, y, cw, chh) if (crop is not None or pitch) else m
            view = F.View(s, x, y, cw, chh)
        else:
            t = cvgs.CV_16UC1 if layout == capi.YUV_P010 else cvgs.CV_8UC1
            m = B.src(s, t)
            luma = cvgs.GpuMat(h, s.shape[1], t, m.data, m.step, owner=m.owner)
            mat = luma.nv12_roi(x, y, cw, chh) if (crop is not None or pitch) else luma
            view = F.View(s, x, y, cw, chh, luma_h=h)
        rd = cvgs.read_nv12(mat, dst, rng, prim, alpha, layout)
        ops = normalise(cn) if tail == "normalise" else []
        if dst is None:
            wr = cvgs.write(f, B.out((chh, cw, cn), f))
        else:
            wr = cvgs.split(f, B.out((1, cn * dst[0] * dst[1]), cvgs.CV_32FC1), dst)
        return [rd] + ops + [wr], [view]
    build.layout422 = layout if layout in (capi.YUV_YUYV, capi.YUV_UYVY) else None
    return build


def yuv444_case(rng, prim, alpha, dst, crop=None, kind="random", w=48, h=32, tail="none", seed=7):
    """Planar 4:4:4 (I444): three w x h planes behind one another; a crop (any origin, odd ones included) is also what a padded pitch is.
    The oracle's value is composed (tests/yuv444_cases.Expect) from B.surfs444."""
    def build(B):
        from tests import yuv444_cases as Y444
        ck = "checker" if kind == "chroma_checker" else kind
        y = np.full((h, w), 120, np.uint8) if kind == "chroma_checker" else pattern((h, w), kind, seed)
        u, v = pattern((h, w), ck, seed + 1), pattern((h, w), ck, seed + 2)[:, ::-1].copy()
        surf = Y444.Surf(w, h, seed, planes=(y, u, v))
        cn = 4 if alpha else 3
        f = cvgs.make_type(cvgs.CV_32F, cn)
        x, y0, cw, chh = crop if crop is not None else (0, 0, w, h)
        m = B.src(surf.buf.reshape(3 * h, w), cvgs.CV_8UC1)
        luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, m.data, m.step, owner=m.owner)
        luma.uv_offset = h * m.step
        B.surfs444 = [surf]
        rd = cvgs.read_yuv444(luma.yuv444_roi(x, y0, cw, chh), dst, rng, prim, alpha)
        ops = normalise(cn) if tail == "normalise" else []
        if dst is None:
            wr = cvgs.write(f, B.out((chh, cw, cn), f))
        else:
            wr = cvgs.split(f, B.out((1, cn * dst[0] * dst[1]), cvgs.CV_32FC1), dst)
        return [rd] + ops + [wr], [F.View(np.stack([y, u, v]), x, y0, cw, chh)]
    build.layout422 = None
    build.layout444 = True
    return build


def affine_matrix(angle_deg, scale, tx, ty, centre):
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = centre
    return [[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]]


def warp_case(kind, transforms, src_hw, dsize, cn=3, used=None, default=None, tail="none", seed=20, to_u8=False):
    def build(B):
        n = len(transforms)
        st = cvgs.make_type(cvgs.CV_8U, cn)
        f = cvgs.make_type(cvgs.CV_32F, cn)
        srcs = [H.random_u8((src_hw[0], src_hw[1], cn), seed + i) for i in range(n)]
        mats = [B.src(s, st) for s in srcs]
        rd = cvgs.warp(kind, st, mats if n > 1 else mats[0], transforms if n > 1 else transforms[0], dsize, used, default)
        ops = normalise(cn) if tail == "normalise" else []
        ot = f
        if to_u8:
            ops, ot = ops + [cvgs.cast(f, st)], st
        wr = cvgs.write(ot, B.out((n, dsize[0] * dsize[1], cn), ot), dsize)
        return [rd] + ops + [wr], [F.View(s) for s in srcs]
    return build


def pointwise_case(depth, cn, hw, stages, out_type, seed=5, special=None, write="packed"):
    """per-pixel read -> stages(in_type) -> write"""
    def build(B):
        st = src_type(depth, cn)
        a = random_src((hw[0], hw[1], cn), depth, seed)
        if special is not None:
            a = a.copy()
            a.reshape(-1)[:special.size] = special
        m = B.src(a, st)
        a = B.sources[-1]
        ops = stages(B, B.T(st))
        ot = B.T(out_type)
        if write == "split":
            o = B.out((1, cn * hw[0] * hw[1]), cvgs.make_type(capi.type_depth(out_type), 1) | (out_type & capi.TYPE_FLAG_BF16))
            wr = cvgs.split_tensor(ot, o.data, hw[1], hw[0], 1, keep=o)
        else:
            wr = cvgs.write(ot, B.out((hw[0], hw[1], type_cn(out_type)), out_type))
        return [cvgs.ReadIOp(capi.READ_PIXEL, B.T(st), [m], 1)] + ops + [wr], [F.View(a)]
    return build


def type_cn(t):
    return capi.type_cn(t)


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
CASES = {}   # name -> (family, build, expected kernel-name prefix on the fast path or None)


def add(name, family, build, kernel=None):
    assert name not in CASES, name
    CASES[name] = (family, build, kernel)


DEPTH_NAMES = {cvgs.CV_8U: "8u", cvgs.CV_16U: "16u", cvgs.CV_16S: "16s", cvgs.CV_32F: "32f", cvgs.CV_16F: "16f", capi.DEPTH_16BF: "16bf"}
# crops of a 97 x 61 frame: origins and sizes odd and even in x and y, 1x1, 1xN, Nx1, 2x2, touching the last row / column
CROPS = [(0, 0, 97, 61), (3, 5, 30, 20), (4, 7, 31, 21), (5, 6, 21, 40), (10, 11, 1, 1), (11, 2, 1, 33), (2, 13, 35, 1), (6, 9, 2, 2),
         (60, 30, 37, 31), (96, 60, 1, 1), (8, 8, 80, 50)]
FRAME = (61, 97)

for _d in (cvgs.CV_8U, cvgs.CV_16U, cvgs.CV_16S, cvgs.CV_32F, cvgs.CV_16F, capi.DEPTH_16BF):
    for _cn in (1, 2, 3, 4):
        # (24, 16): up-scaling for the small crops, down-scaling by non-integer factors for the large ones
        add("k1_%sc%d" % (DEPTH_NAMES[_d], _cn), "K1 " + DEPTH_NAMES[_d], resize_case(_d, _cn, FRAME, CROPS, (24, 16), seed=10 + _cn),
            "k1_" if _d in (cvgs.CV_8U, cvgs.CV_16U, cvgs.CV_16S) and _cn in (3, 4) else None)
add("k1_8uc3_up", "K1 8u", resize_case(cvgs.CV_8U, 3, FRAME, [(3, 5, 9, 7), (60, 30, 37, 31)], (64, 128), tail="normalise", seed=3), "k1_u8c3_swap_mul_sub_div")
add("k1_8uc3_down", "K1 8u", resize_case(cvgs.CV_8U, 3, (300, 500), [(1, 3, 499, 297), (17, 20, 333, 211)], (64, 128), tail="normalise", seed=4),
    "k1_u8c3_swap_mul_sub_div")
for _ar, _nm in ((cvgs.PRESERVE_AR, "ar"), (cvgs.PRESERVE_AR_RN_EVEN, "ar_even"), (cvgs.PRESERVE_AR_LEFT, "ar_left")):
    # extents away from .5 ties (tests/test_independent_pins.py covers the window itself); both fit directions, a 1-pixel source
    add("k1_8uc3_" + _nm, "K1 8u", resize_case(cvgs.CV_8U, 3, FRAME, [(3, 5, 30, 20), (4, 7, 13, 41), (5, 6, 21, 40), (10, 11, 1, 1), (2, 2, 90, 11)],
                                                (40, 24), ar=_ar, seed=6), "k1_")
    add("k1_32fc1_" + _nm, "K1 32f", resize_case(cvgs.CV_32F, 1, FRAME, [(3, 5, 30, 20), (4, 7, 13, 41)], (40, 24), ar=_ar, seed=7))
add("k1_8uc3_used", "K1 8u", resize_case(cvgs.CV_8U, 3, FRAME, CROPS[:6], (24, 16), used=4, tail="normalise", seed=8), "k1_")
add("k1_16uc4_used_splitT", "K1 16u", resize_case(cvgs.CV_16U, 4, FRAME, CROPS[:5], (24, 16), used=3, write="splitT", seed=9), "k1_")
add("k1_8uc3_packed", "K1 8u", resize_case(cvgs.CV_8U, 3, FRAME, CROPS[:4], (24, 16), write="packed", seed=11))
add("store_k1_f16", "stores", resize_case(cvgs.CV_8U, 3, FRAME, CROPS, (24, 16), tail="normalise", out16=cvgs.CV_16F, seed=12), "k1_")
add("store_k1_bf16", "stores", resize_case(cvgs.CV_8U, 3, FRAME, CROPS, (24, 16), tail="normalise", out16=capi.DEPTH_16BF, seed=13), "k1_")
add("store_k1_c4_bf16_splitT", "stores", resize_case(cvgs.CV_8U, 4, FRAME, CROPS[:5], (24, 16), tail="normalise", out16=capi.DEPTH_16BF, write="splitT", seed=14),
    "k1_")

LAYOUT_NAMES = {capi.YUV_NV12: "nv12", capi.YUV_NV21: "nv21", capi.YUV_I420: "i420", capi.YUV_YV12: "yv12", capi.YUV_P010: "p010",
                capi.YUV_YUYV: "yuyv", capi.YUV_UYVY: "uyvy"}
for _l, _ln in LAYOUT_NAMES.items():
    _is422 = _l in (capi.YUV_YUYV, capi.YUV_UYVY)
    _fast = "k_yuv422_resize" if _is422 else "k4_nv12_resize"
    for _r in (capi.YUV_FULL, capi.YUV_LIMITED):
        for _p in (capi.BT601, capi.BT709, capi.BT2020):
            for _a in (False, True):
                _tag = "%s_r%d_p%d_a%d" % (_ln, _r, _p, int(_a))
                add("yuv_px_" + _tag, "YUV " + _ln, yuv_case(_l, _r, _p, _a, None, seed=30 + _p))
                add("yuv_rs_" + _tag, "YUV " + _ln, yuv_case(_l, _r, _p, _a, (29, 19), seed=40 + _p), None if _a else _fast)
    for _k in ("ramp_h", "ramp_v", "chroma_checker"):
        add("yuv_rs_%s_%s" % (_ln, _k), "YUV " + _ln, yuv_case(_l, capi.YUV_LIMITED, capi.BT709, False, (37, 23), kind=_k), _fast)
        add("yuv_px_%s_%s" % (_ln, _k), "YUV " + _ln, yuv_case(_l, capi.YUV_FULL, capi.BT601, False, None, kind=_k))
    add("yuv_up_%s" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_LIMITED, capi.BT601, False, (64, 128), tail="normalise", w=16, h=12), _fast)
    if _is422:  # crops at odd y, odd sizes (x stays on a pixel pair), a padded pitch
        add("yuv_rs_%s_crop_odd_y" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_LIMITED, capi.BT709, False, (21, 13), crop=(4, 5, 31, 17), kind="chroma_checker"), _fast)
        add("yuv_px_%s_crop_odd_y" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_FULL, capi.BT601, True, None, crop=(10, 3, 21, 9)))
        add("yuv_rs_%s_pitch" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_FULL, capi.BT2020, False, (21, 13), pitch=10), _fast)
    elif _l in (capi.YUV_NV12, capi.YUV_NV21, capi.YUV_P010):  # 4:2:0 crops sit on 2x2 blocks; planar chroma cannot be cropped
        add("yuv_rs_%s_crop" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_LIMITED, capi.BT709, False, (21, 13), crop=(6, 12, 30, 18), kind="chroma_checker"), _fast)
        add("yuv_px_%s_crop" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_FULL, capi.BT601, True, None, crop=(10, 4, 22, 10)))
        add("yuv_rs_%s_pitch" % _ln, "YUV " + _ln, yuv_case(_l, capi.YUV_FULL, capi.BT2020, False, (21, 13), pitch=16), _fast)

# planar 4:4:4: a conversion of each range, the siting patterns (a chroma checkerboard shows an index taken from the 4:2:0 rule), crops at odd
# origins (which is also what a padded pitch is), up-scaling into the headline chain
add("yuv_px_i444_r0_p0_a0", "YUV i444", yuv444_case(capi.YUV_FULL, capi.BT601, False, None, seed=30))
add("yuv_rs_i444_r1_p1_a0", "YUV i444", yuv444_case(capi.YUV_LIMITED, capi.BT709, False, (29, 19), seed=41), "k_yuv444_resize")
add("yuv_rs_i444_r1_p2_a1", "YUV i444", yuv444_case(capi.YUV_LIMITED, capi.BT2020, True, (29, 19), seed=42))
add("yuv_px_i444_chroma_checker", "YUV i444", yuv444_case(capi.YUV_FULL, capi.BT601, False, None, kind="chroma_checker"))
add("yuv_rs_i444_ramp_h", "YUV i444", yuv444_case(capi.YUV_LIMITED, capi.BT709, False, (37, 23), kind="ramp_h"), "k_yuv444_resize")
add("yuv_up_i444", "YUV i444", yuv444_case(capi.YUV_LIMITED, capi.BT601, False, (64, 128), tail="normalise", w=16, h=12), "k_yuv444_resize")
add("yuv_rs_i444_crop_odd", "YUV i444", yuv444_case(capi.YUV_LIMITED, capi.BT709, False, (21, 13), crop=(5, 3, 31, 17), kind="chroma_checker"), "k_yuv444_resize")
add("yuv_px_i444_crop_odd", "YUV i444", yuv444_case(capi.YUV_FULL, capi.BT601, True, None, crop=(11, 3, 21, 9)))

_AFF = affine_matrix(17.0, 1.31, 3.37, -2.21, (60, 45))
add("warp_affine", "warp", warp_case(cvgs.WARP_AFFINE, [_AFF], (90, 120), (110, 100)))
add("warp_affine_norm", "warp", warp_case(cvgs.WARP_AFFINE, [_AFF], (90, 120), (64, 48), tail="normalise"), "warp_affine_u8c3")
add("warp_affine_c1_u8", "warp", warp_case(cvgs.WARP_AFFINE, [affine_matrix(-31.0, 0.77, 0.4, 5.13, (40, 40))], (80, 80), (70, 90), cn=1, to_u8=True))
for _i in range(5):
    add("warp_persp_%d" % _i, "warp", warp_case(cvgs.WARP_PERSPECTIVE, [WC.get_perspective_transform(*WC.REF_POINT_SETS[_i])], (430, 470), (470, 430), seed=20 + _i))
_PM = WC.get_perspective_transform([(5, 5), (70, 8), (3, 50), (75, 55)], [(0, 0), (80, 0), (0, 60), (80, 60)])
add("warp_batch_default", "warp", warp_case(cvgs.WARP_PERSPECTIVE, [_PM] * 4, (60, 80), (80, 60), used=2, default=[7.0, 8.0, 9.0], tail="normalise", seed=40),
    "warp_perspective_u8c3")

_F3 = cvgs.CV_32FC3


def _convert_sat(B, st):  # 8U -> (x 3.1 - 260) -> 8U: saturates at both ends
    return [cvgs.convertTo(st, st, 3.1, -260.0)]


def _convert_u16(B, st):
    return [cvgs.convertTo(st, cvgs.make_type(cvgs.CV_16U, 3), 700.5, -70000.25)]


def _to_f16(B, st):
    return [cvgs.convertTo(st, _F3, 1.0 / 255.0, -0.25)] + B.to16(_F3, cvgs.CV_16FC3)


def _to_bf16(B, st):
    return [cvgs.convertTo(st, _F3, 1.0 / 255.0, -0.25)] + B.to16(_F3, cvgs.CV_16BFC3)


def _slow_div(B, st):  # a divisor with an all-ones significand (the fast division's guard refuses it) and a huge one
    return [cvgs.convertTo(st, _F3), cvgs.divide(_F3, [float(np.float32(1.9999999)), 3.0e25, -0.3])]


def _gray(B, st):
    return [cvgs.cvtColor(cvgs.COLOR_RGB2GRAY, st, cvgs.CV_8UC1)]


def _alpha(B, st):
    return [cvgs.cvtColor(cvgs.COLOR_BGR2RGBA, st, cvgs.CV_8UC4), cvgs.convertTo(cvgs.CV_8UC4, cvgs.CV_32FC4, 0.5, 1.0), cvgs.cvtColor(cvgs.COLOR_RGBA2BGR, cvgs.CV_32FC4, _F3)]


def _norm(B, st):
    return [cvgs.convertTo(st, _F3)] + normalise(3)


_SPECIAL = np.array([-1e9, -300.7, -1.5, -0.5, -0.49999997, 0.0, 0.5, 0.49999997, 1.5, 2.5, 254.5, 255.5, 300.2, 7e4, 1e9, np.nan], np.float32)


def _sat_f32(B, st):
    return [cvgs.convertTo(st, cvgs.CV_8UC1)]


def _trunc_f32(B, st):
    return [cvgs.cast(st, cvgs.CV_16SC1)]


add("chain_normalise", "chains", pointwise_case(cvgs.CV_8U, 3, (45, 67), _norm, _F3), "pointwise")
add("chain_convert_saturates", "chains", pointwise_case(cvgs.CV_8U, 3, (45, 67), _convert_sat, cvgs.CV_8UC3), "pointwise")
add("chain_convert_u16", "chains", pointwise_case(cvgs.CV_8U, 3, (33, 50), _convert_u16, cvgs.make_type(cvgs.CV_16U, 3)))
add("chain_slow_divisor", "chains", pointwise_case(cvgs.CV_8U, 3, (45, 67), _slow_div, _F3))
add("chain_gray", "chains", pointwise_case(cvgs.CV_8U, 3, (45, 64), _gray, cvgs.CV_8UC1))
add("chain_alpha", "chains", pointwise_case(cvgs.CV_8U, 3, (45, 67), _alpha, _F3))
add("chain_sat_f32", "chains", pointwise_case(cvgs.CV_32F, 1, (16, 64), _sat_f32, cvgs.CV_8UC1, special=_SPECIAL))
add("chain_trunc_f32", "chains", pointwise_case(cvgs.CV_32F, 1, (16, 64), _trunc_f32, cvgs.CV_16SC1, special=_SPECIAL))
add("store_px_f16", "stores", pointwise_case(cvgs.CV_8U, 3, (45, 67), _to_f16, cvgs.CV_16FC3), "pointwise")
add("store_px_bf16", "stores", pointwise_case(cvgs.CV_8U, 3, (45, 67), _to_bf16, cvgs.CV_16BFC3), "pointwise")
add("store_px_bf16_split", "stores", pointwise_case(cvgs.CV_8U, 3, (45, 67), _to_bf16, cvgs.CV_16BFC3, write="split"), "pointwise")
