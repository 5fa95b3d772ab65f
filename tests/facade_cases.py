"""The case table of the C++ facade check (tests/cpp/facade_model.cpp): name -> (input builder, Python spelling, near-miss spellings).

tests/cpp/facade_model.cpp builds every chain of this table in the facade's OWN spelling (cvGS:: templates, cv::Size, cv::Scalar, cv::Rect,
cv::Mat, std::array<GpuMat, N>) over the raw inputs written from here, and runs it on the CPU oracle or on the GPU.  The Python spelling of
the same chain returns (iops, views) like the builders of tests/model_cases.py, for the float64 model (tests/f64_model.py) alone: the model
reads the iop objects by attribute and the views as numpy arrays, so nothing of the facade's lowering reaches the expected values.

A near-miss is the Python spelling of a plausible mis-lowering (Scalar channels reversed, Size transposed, the neighbouring colour code, the
next AspectRatio mode, alpha and beta exchanged, another range / primaries / layout, the warp matrix read column-major, usedPlanes +- 1):
tests/test_facade_model.py shows that the facade's output falls outside the bound of every one of them, i.e. that the inputs can tell.

Every Scalar has distinct, non-symmetric channel values, every Size is non-square, every image is non-constant.  Shapes are the model
grid's: frame 97 x 61, destinations (24, 16) / (29, 19) / (40, 24), YUV surfaces 48 x 32, warps <= 120 x 90.

Left out, with the reason: the warp overload with per-plane destination sizes (std::array<cv::Size, BATCH>): f64_model.evaluate gives every
plane of a read one size, so tests/model_cases.warp_case cannot express it; arithmetic on integer-typed pixels (multiply<CV_8UC3> ...): outside
the model (tests/test_gpu_int_arith.py holds it to the oracle); the executeOperations overloads that prepend a read or append a write (they need a
stream, which the oracle leg has not): their read and write are the ones spelled out here."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import model_cases as MC
from tests import warp_cases as WC

GUARD = 4096          # canary bytes in front of and behind every output (the program's constant)
CANARY = 0xA5
FRAME = MC.FRAME      # (61, 97): rows, cols
PX_HW = (45, 67)      # pointwise images
YUV_W, YUV_H = 48, 32
BG = [17.25, 99.5, 3.0, 200.0]
MULV = [0.00392156862745098, 0.0078125, 0.015625, 0.0625]
SUBV = [0.485, 0.456, 0.406, 0.3]
DIVV = [0.229, 0.224, 0.225, 0.25]
ADDV = [1.5, -2.25, 3.125, -0.75]
FKV = [1.25, 0.5, 2.75]
AR_CROPS = [(3, 5, 30, 20), (4, 7, 13, 41), (5, 6, 21, 40), (10, 11, 1, 1), (2, 2, 90, 11)]   # the k1_8uc3_ar* crops of model_cases.py
ROI_CROPS = [(3, 5, 30, 20), (4, 7, 31, 21), (60, 30, 37, 31), (8, 8, 80, 50)]


class Case:
    def __init__(self, family, inputs, spell, near, oracle, kernel):
        self.family, self.inputs, self.spell, self.near, self.oracle, self.kernel = family, inputs, spell, near, oracle, kernel


CASES = {}  # name -> Case, in the order of the C++ table


def add(name, family, inputs, spell, near, oracle=True, kernel=None):
    """oracle=False: the CPU oracle does not know the chain (packed 4:2:2, planar 4:4:4, bfloat16): the GPU leg alone runs it.
    kernel: the fast kernel's name prefix that the Python twin in model_cases.py names for this shape of chain."""
    assert name not in CASES and near, name
    CASES[name] = Case(family, inputs, spell, near, oracle, kernel)


def _f(cn):
    return cvgs.make_type(cvgs.CV_32F, cn)


def _one(t):
    return cvgs.make_type(capi.type_depth(t), 1) | (t & capi.TYPE_FLAG_BF16)


def _write(B, kind, ot, n, dst):
    """the write stage and its (dense) output: only its kind, type and sizes matter to the model"""
    w, h = dst
    cn = capi.type_cn(ot)
    if kind == "split":       # split<O>(GpuMat, Size) and split<O>(RawPtr<_3D>)
        return cvgs.split(ot, B.out((n, cn * w * h), _one(ot)), dst)
    if kind == "splitT":      # splitT<O>(RawPtr<T3D>)
        o = B.out((n, cn * w * h), _one(ot))
        return cvgs.splitT(ot, o.data, w, h, n, keep=o)
    if kind == "split2d":     # split<O>(vector<GpuMat>) and split<O>(array<vector<GpuMat>, N>)
        planes = [[B.out((h, w), _one(ot)) for _ in range(cn)] for _ in range(n)]
        return cvgs.split(ot, planes if n > 1 else planes[0])
    if kind == "write2d":     # write<O>(GpuMat)
        return cvgs.write(ot, B.out((h, w, cn), ot))
    assert kind == "write3d"  # write<O>(GpuMat, Size) and write(Tensor)
    return cvgs.write(ot, B.out((n, w * h), ot), dst)


def logical_kind(kind):
    """The program writes the planes of a SplitWrite<_2D> densely behind one another, [image][channel][y][x]: the tensor split's order."""
    return capi.WRITE_TENSOR_SPLIT if kind == capi.WRITE_SPLIT_2D else kind


def _tail(cn, p):
    """swap, x, -, / with the case's scalars (`rev`: every Scalar's channels reversed; `order`: subtract before multiply)"""
    f = _f(cn)
    pick = (lambda v: v[:cn][::-1]) if p.get("rev") else (lambda v: v[:cn])
    ops = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f)] if cn >= 3 else []
    mul, sub, div = cvgs.multiply(f, pick(MULV)), cvgs.subtract(f, pick(SUBV)), cvgs.divide(f, pick(DIVV))
    return ops + ([sub, mul, div] if p.get("order") else [mul, sub, div])


def _swap_planes(cn):
    return [cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, _f(cn))]


def transposed(size):
    return (size[1], size[0])


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
def frame_inputs(depth, cn, seed, hw=FRAME):
    return lambda: [MC.random_src((hw[0], hw[1], cn), depth, seed)]


def resize_spell(depth, cn, **base):
    def spell(B, arrs, **kw):
        p = dict(crops=None, dst=(24, 16), ar=cvgs.IGNORE_AR, used=None, bg=None, tail=False, write="split", fx=0.0, fy=0.0, planes_swapped=False)
        p.update(base)
        p.update(kw)
        st = MC.src_type(depth, cn)
        m = B.src(arrs[0], st)
        if p["crops"] is None:   # resize<T, INTER>(GpuMat, dsize, fx, fy)
            rd = cvgs.resize(st, cvgs.INTER_LINEAR, m, p["dst"], fx=p["fx"], fy=p["fy"])
            views, n = [F.View(arrs[0])], 1
        else:
            crops = [tuple(int(v) for v in c) for c in p["crops"]]
            n = len(crops)
            rd = cvgs.resize(st, cvgs.INTER_LINEAR, [m.roi(*c) for c in crops], p["dst"], n if p["used"] is None else p["used"], p["bg"], p["ar"])
            views = [F.View(arrs[0], *c) for c in crops]
        ops = _tail(cn, p) if p["tail"] else []
        if p["planes_swapped"]:
            ops += _swap_planes(cn)
        return [rd] + ops + [_write(B, p["write"], _f(cn), n, rd.dsize)], views
    return spell


_T = [("Size transposed", dict(dst=(16, 24)))]
add("resize_single_dsize_8uc3", "resize", frame_inputs(cvgs.CV_8U, 3, 101), resize_spell(cvgs.CV_8U, 3, dst=(29, 19), write="write2d"),
    [("Size transposed", dict(dst=(19, 29)))])
add("resize_single_fxfy_8uc1", "resize", frame_inputs(cvgs.CV_8U, 1, 102), resize_spell(cvgs.CV_8U, 1, dst=(0, 0), fx=0.4, fy=0.3, write="write2d"),
    [("fx and fy exchanged", dict(fx=0.3, fy=0.4))])
add("resize_batch_roi_8uc3", "resize", frame_inputs(cvgs.CV_8U, 3, 103), resize_spell(cvgs.CV_8U, 3, crops=ROI_CROPS, tail=True), _T + [
    ("Scalars reversed", dict(rev=True)), ("subtract before multiply", dict(order=True))], kernel="k1_")
add("resize_batch_crop2d_16uc3", "resize", frame_inputs(cvgs.CV_16U, 3, 104),
    resize_spell(cvgs.CV_16U, 3, crops=[(3.7, 5.2, 30.9, 20.5), (60.99, 30.5, 36.2, 30.9), (8.5, 8.5, 80.5, 50.5)]), _T + [
        ("Rect2d rounded, not truncated", dict(crops=[(4, 5, 31, 20), (61, 30, 36, 31), (8, 8, 80, 50)]))], kernel="k1_")
add("resize_batch_used_bg_8uc4", "resize", frame_inputs(cvgs.CV_8U, 4, 105),
    resize_spell(cvgs.CV_8U, 4, crops=MC.CROPS[1:6], used=3, bg=BG, write="splitT"),
    [("usedPlanes - 1", dict(used=2)), ("usedPlanes + 1", dict(used=4)), ("background reversed", dict(bg=BG[::-1])),
     ("background not per channel", dict(bg=[BG[0]] * 4))], kernel="k1_")
for _ar, _nm, _next in ((cvgs.PRESERVE_AR, "preserve", cvgs.IGNORE_AR), (cvgs.IGNORE_AR, "ignore", cvgs.PRESERVE_AR_RN_EVEN),
                        (cvgs.PRESERVE_AR_RN_EVEN, "rn_even", cvgs.PRESERVE_AR_LEFT), (cvgs.PRESERVE_AR_LEFT, "left", cvgs.PRESERVE_AR)):
    add("resize_ar_%s_8uc3" % _nm, "resize", frame_inputs(cvgs.CV_8U, 3, 106), resize_spell(cvgs.CV_8U, 3, crops=AR_CROPS, dst=(40, 24), ar=_ar, bg=BG),
        [("the next AspectRatio", dict(ar=_next)), ("Size transposed", dict(dst=(24, 40)))] +
        ([] if _ar == cvgs.IGNORE_AR else [("background reversed", dict(bg=BG[:3][::-1]))]), kernel="k1_")  # (IGNORE_AR pads nothing)
for _d, _nm in ((cvgs.CV_8U, "8uc1"), (cvgs.CV_16S, "16sc1"), (cvgs.CV_32F, "32fc1")):
    add("resize_batch_%s" % _nm, "resize", frame_inputs(_d, 1, 107), resize_spell(_d, 1, crops=ROI_CROPS[:3], write="write3d"), _T)


# ---- per-pixel chains -----------------------------------------------------------------------------------------------------------------
def px_spell(depth, cn, stages, out_type, write="write2d", hw=PX_HW):
    def spell(B, arrs, **kw):
        st = MC.src_type(depth, cn)
        m = B.src(arrs[0], st)
        rd = cvgs.ReadIOp(capi.READ_PIXEL, st, [m], 1)
        return [rd] + stages(st, **kw) + [_write(B, write, out_type, 1, (hw[1], hw[0]))], [F.View(arrs[0])]
    return spell


def _convert(out_type, alpha=None, beta=None):
    def stages(st, exchanged=False, alpha_as_beta=False, normalised=False):
        if normalised:  # the mistake "convertTo() to float scales to 0..1"
            return [cvgs.convertTo(st, out_type, 1.0 / 255.0)]
        if alpha_as_beta:
            return [cvgs.convertTo(st, out_type, 1.0, alpha)]
        a, b = (beta, alpha) if exchanged else (alpha, beta)
        return [cvgs.convertTo(st, out_type, a, b)]
    return stages


_X = [("alpha and beta exchanged", dict(exchanged=True))]
_U3, _F3 = cvgs.CV_8UC3, cvgs.CV_32FC3
add("convert_plain_8u_32f", "convertTo", frame_inputs(cvgs.CV_8U, 3, 110, PX_HW), px_spell(cvgs.CV_8U, 3, _convert(_F3), _F3),
    [("scaled to 0..1", dict(normalised=True))])
add("convert_alpha_8u_32f", "convertTo", frame_inputs(cvgs.CV_8U, 3, 111, PX_HW), px_spell(cvgs.CV_8U, 3, _convert(_F3, 0.25), _F3),
    [("alpha taken as beta", dict(alpha_as_beta=True))])
add("convert_alpha_beta_8u_32f", "convertTo", frame_inputs(cvgs.CV_8U, 3, 112, PX_HW), px_spell(cvgs.CV_8U, 3, _convert(_F3, 1.0 / 255.0, -0.25), _F3), _X)
add("convert_saturates_8u_8u", "convertTo", frame_inputs(cvgs.CV_8U, 3, 113, PX_HW), px_spell(cvgs.CV_8U, 3, _convert(_U3, 3.1, -260.0), _U3), _X,
    kernel="pointwise")
add("convert_8u_16u", "convertTo", frame_inputs(cvgs.CV_8U, 3, 114, PX_HW),
    px_spell(cvgs.CV_8U, 3, _convert(cvgs.CV_16UC3, 700.5, -70000.25), cvgs.CV_16UC3), _X)
add("convert_8u_16f", "convertTo", frame_inputs(cvgs.CV_8U, 3, 115, PX_HW),
    px_spell(cvgs.CV_8U, 3, _convert(cvgs.CV_16FC3, 1.0 / 255.0, -0.25), cvgs.CV_16FC3), _X)
add("convert_8u_16bf", "convertTo", frame_inputs(cvgs.CV_8U, 3, 116, PX_HW),
    px_spell(cvgs.CV_8U, 3, _convert(cvgs.CV_16BFC3, 1.0 / 255.0, -0.25), cvgs.CV_16BFC3), _X, oracle=False)
# the reference README's spelling: convertTo<CV_8UC3, CV_32FC3>() behind the batched resize (the facade elides the redundant cast), `substract`
add("convert_readme_redundant_cast", "convertTo", frame_inputs(cvgs.CV_8U, 3, 117), resize_spell(cvgs.CV_8U, 3, crops=ROI_CROPS, tail=True, dst=(29, 19)),
    [("Scalars reversed", dict(rev=True)), ("Size transposed", dict(dst=(19, 29)))], kernel="k1_")


def _arith(cn):
    def stages(st, rev=False, operands_exchanged=False):
        pick = (lambda v: v[1:cn + 1] if cn == 1 else v[:cn][::-1]) if rev else (lambda v: v[:cn])
        f = _f(cn)
        ops = [cvgs.divide(f, pick(DIVV)), cvgs.add(f, pick(ADDV)), cvgs.multiply(f, pick(MULV)), cvgs.subtract(f, pick(SUBV))]
        return [ops[1], ops[0], ops[3], ops[2]] if operands_exchanged else ops
    return stages


for _cn in (1, 3, 4):  # / + x - : not the reference's x - / order, so the order of the stages matters
    add("arith_32fc%d" % _cn, "arithmetic", frame_inputs(cvgs.CV_32F, _cn, 120 + _cn, PX_HW), px_spell(cvgs.CV_32F, _cn, _arith(_cn), _f(_cn)),
        [("Scalar channels reversed" if _cn > 1 else "the next channel's value", dict(rev=True)), ("neighbouring stages exchanged", dict(operands_exchanged=True))])

# every colour code cv2cuda_types.h lists: (name, code, channels in, channels out, the neighbouring code or None = "no conversion at all")
COLOR_CODES = [("bgr2bgra", cvgs.COLOR_BGR2BGRA, 3, 4, cvgs.COLOR_BGR2RGBA), ("bgra2bgr", cvgs.COLOR_BGRA2BGR, 4, 3, cvgs.COLOR_BGRA2RGB),
               ("bgr2rgba", cvgs.COLOR_BGR2RGBA, 3, 4, cvgs.COLOR_BGR2BGRA), ("bgra2rgb", cvgs.COLOR_BGRA2RGB, 4, 3, cvgs.COLOR_BGRA2BGR),
               ("bgr2rgb", cvgs.COLOR_BGR2RGB, 3, 3, None), ("bgra2rgba", cvgs.COLOR_BGRA2RGBA, 4, 4, None),
               ("bgr2gray", cvgs.COLOR_BGR2GRAY, 3, 1, cvgs.COLOR_RGB2GRAY), ("rgb2gray", cvgs.COLOR_RGB2GRAY, 3, 1, cvgs.COLOR_BGR2GRAY),
               ("bgra2gray", cvgs.COLOR_BGRA2GRAY, 4, 1, cvgs.COLOR_RGBA2GRAY), ("rgba2gray", cvgs.COLOR_RGBA2GRAY, 4, 1, cvgs.COLOR_BGRA2GRAY)]


def _cvt(code, depth, icn, ocn, neighbour):
    def stages(st, near=False):
        ot = cvgs.make_type(depth, ocn)
        if near and neighbour is None:
            return [cvgs.PointwiseIOp(st, ot, [])]
        return [cvgs.cvtColor(neighbour if near else code, st, ot)]
    return stages


for _nm, _code, _icn, _ocn, _nb in COLOR_CODES:
    for _d, _dn in ((cvgs.CV_8U, "8u"), (cvgs.CV_32F, "32f")):
        add("cvt_%s_%s" % (_nm, _dn), "cvtColor", frame_inputs(_d, _icn, 130 + _code, PX_HW),
            px_spell(_d, _icn, _cvt(_code, _d, _icn, _ocn, _nb), cvgs.make_type(_d, _ocn)), [("the neighbouring colour code", dict(near=True))])

# ---- writes ---------------------------------------------------------------------------------------------------------------------------
_PS = [("planes in reversed order", dict(planes_swapped=True))]
add("write_split_vector", "writes", frame_inputs(cvgs.CV_8U, 3, 140), resize_spell(cvgs.CV_8U, 3, dst=(29, 19), write="split2d"),
    _PS + [("Size transposed", dict(dst=(19, 29)))])
add("write_split_array_of_vectors", "writes", frame_inputs(cvgs.CV_8U, 4, 141), resize_spell(cvgs.CV_8U, 4, crops=ROI_CROPS[:2], write="split2d"), _PS + _T)
add("write_split_rawptr3d", "writes", frame_inputs(cvgs.CV_8U, 3, 142), resize_spell(cvgs.CV_8U, 3, crops=ROI_CROPS[:3], write="split"), _PS + _T)
add("write_tensor", "writes", frame_inputs(cvgs.CV_8U, 3, 143), resize_spell(cvgs.CV_8U, 3, crops=ROI_CROPS[:3], write="write3d", dst=(29, 19)),
    _PS + [("Size transposed", dict(dst=(19, 29)))])


# ---- warps ----------------------------------------------------------------------------------------------------------------------------
def column_major(m):
    """the matrix a reader gets who takes the row-major doubles for column-major ones"""
    m = np.asarray(m, np.float64)
    return m.reshape(-1).reshape(m.shape[1], m.shape[0]).T.copy()


def warp_inputs(transforms, src_hw, cn, seed):
    from tests import helpers as H
    return lambda: [H.random_u8((src_hw[0], src_hw[1], cn), seed + i) for i in range(len(transforms))] + [np.ascontiguousarray(t, np.float64) for t in transforms]


def warp_spell(kind, n, dsize, cn=3, **base):
    def spell(B, arrs, **kw):
        p = dict(used=None, default=None, tail=False, colmajor=False, forward=False, dsize=dsize)
        p.update(base)
        p.update(kw)
        st = cvgs.make_type(cvgs.CV_8U, cn)
        mats = [B.src(a, st) for a in arrs[:n]]
        tr = [column_major(t) if p["colmajor"] else np.asarray(t) for t in arrs[n:]]
        if p["forward"]:  # the mistake "the matrix is handed on without being inverted" = inverted twice
            tr = [np.array(cvgs.invert_affine(t) if kind == cvgs.WARP_AFFINE else cvgs.invert_3x3(t)) for t in tr]
        rd = cvgs.warp(kind, st, mats if n > 1 else mats[0], [t.tolist() for t in tr] if n > 1 else tr[0].tolist(), p["dsize"], p["used"], p["default"])
        ops = _tail(cn, p) if p["tail"] else []
        return [rd] + ops + [_write(B, "write3d", _f(cn), n, p["dsize"])], [F.View(a) for a in arrs[:n]]
    return spell


_WN = [("matrix read column-major", dict(colmajor=True)), ("matrix not inverted", dict(forward=True))]
AFFINES = [MC.affine_matrix(17.0, 1.31, 3.37, -2.21, (60, 45)), MC.affine_matrix(-31.0, 0.77, 0.4, 5.13, (55, 40)), MC.affine_matrix(48.0, 1.6, -4.3, 2.9, (62, 47))]
_PM = WC.get_perspective_transform([(5, 5), (70, 8), (3, 50), (75, 55)], [(0, 0), (80, 0), (0, 60), (80, 60)])
_PM2 = WC.get_perspective_transform([(9, 4), (66, 11), (6, 53), (72, 49)], [(0, 0), (80, 0), (0, 60), (80, 60)])
add("warp_affine_single", "warp", warp_inputs(AFFINES[:1], (90, 120), 3, 150), warp_spell(cvgs.WARP_AFFINE, 1, (110, 100)), _WN + [("Size transposed", dict(dsize=(100, 110)))])
add("warp_perspective_single", "warp", warp_inputs([_PM], (60, 80), 3, 151), warp_spell(cvgs.WARP_PERSPECTIVE, 1, (80, 60)), _WN + [("Size transposed", dict(dsize=(60, 80)))])
add("warp_affine_batch", "warp", warp_inputs(AFFINES, (90, 120), 3, 152), warp_spell(cvgs.WARP_AFFINE, 3, (64, 48), tail=True),
    _WN + [("Scalars reversed", dict(rev=True))], kernel="warp_affine_u8c3")
add("warp_perspective_batch_used_default", "warp", warp_inputs([_PM, _PM2, _PM, _PM2], (60, 80), 3, 153),
    warp_spell(cvgs.WARP_PERSPECTIVE, 4, (80, 60), used=2, default=[7.0, 8.0, 9.0], tail=True),
    _WN + [("usedPlanes - 1", dict(used=1)), ("usedPlanes + 1", dict(used=3)), ("default value reversed", dict(default=[9.0, 8.0, 7.0]))], kernel="warp_perspective_u8c3")

# ---- YUV surfaces ---------------------------------------------------------------------------------------------------------------------
I444 = capi.YUV_I444
LAYOUTS = [("nv12", capi.YUV_NV12), ("p010", capi.YUV_P010), ("yuy2", capi.YUV_YUYV), ("uyvy", capi.YUV_UYVY), ("yuv444", I444)]


def yuv_inputs(layout, seed, kind="random"):
    def make():
        if layout != I444:
            return [MC.yuv_surface(layout, YUV_W, YUV_H, seed, kind)]
        ck = "checker" if kind == "chroma_checker" else kind
        y = np.full((YUV_H, YUV_W), 120, np.uint8) if kind == "chroma_checker" else MC.pattern((YUV_H, YUV_W), kind, seed)
        u, v = MC.pattern((YUV_H, YUV_W), ck, seed + 1), MC.pattern((YUV_H, YUV_W), ck, seed + 2)[:, ::-1].copy()
        return [np.concatenate([y, u, v])]
    return make


def yuv_spell(layout, **base):
    def spell(B, arrs, **kw):
        p = dict(rng=capi.YUV_FULL, prim=capi.BT709, alpha=False, swap=False, dst=None, crops=None, ar=cvgs.IGNORE_AR, bg=None, layout=layout, write=None,
                 to_u8=False)
        p.update(base)
        p.update(kw)
        s, L, w, h = arrs[0], p["layout"], YUV_W, YUV_H
        cn = 4 if p["alpha"] else 3
        f = _f(cn)
        if L in (capi.YUV_YUYV, capi.YUV_UYVY):
            roi = B.src(s, cvgs.make_type(cvgs.CV_8U, 2)).yuv422_roi
            view = lambda c: F.View(s, *c)  # noqa: E731
        elif L == I444:
            m = B.src(s, cvgs.CV_8UC1)
            luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, m.data, m.step, owner=m.owner)
            luma.uv_offset = h * m.step
            roi = luma.yuv444_roi
            view = lambda c: F.View(s.reshape(3, h, w), *c)  # noqa: E731
        else:
            t = cvgs.CV_16UC1 if L == capi.YUV_P010 else cvgs.CV_8UC1
            m = B.src(s, t)
            roi = cvgs.GpuMat(h, w, t, m.data, m.step, owner=m.owner).nv12_roi
            view = lambda c: F.View(s, *c, luma_h=h)  # noqa: E731
        crops = p["crops"] or [(0, 0, w, h)]
        mats = [roi(*c) for c in crops]
        rd = cvgs.read_nv12(mats if len(mats) > 1 else mats[0], p["dst"], p["rng"], p["prim"], p["alpha"], L)
        rd.ar = p["ar"]
        if p["bg"] is not None:  # given in the IOp's channel order; it enters the chain in front of the R <-> B swap
            bg = list(p["bg"]) + [0.0] * (4 - len(p["bg"]))
            rd.background = [bg[2], bg[1], bg[0], bg[3]] if p["swap"] else bg
        ops = _swap_planes(cn) if p["swap"] else []
        ot = f
        if p["to_u8"]:
            ot = cvgs.make_type(cvgs.CV_8U, cn)
            ops = [cvgs.convertTo(f, ot), cvgs.cvtColor(cvgs.COLOR_RGBA2BGRA, ot)]
        out_size = p["dst"] if p["dst"] is not None else (crops[0][2], crops[0][3])
        kind = p["write"] or ("write2d" if (p["dst"] is None and len(crops) == 1) else "split")
        return [rd] + ops + [_write(B, kind, ot, len(crops), out_size)], [view(c) for c in crops]
    return spell


YUV_CROPS = {False: [(6, 12, 30, 18), (10, 4, 22, 10)], True: [(6, 13, 31, 17), (10, 3, 21, 9)]}   # 4:2:0: on 2x2 blocks; others: even x only / any
YUV_CROPS_PX = {False: [(6, 12, 22, 10), (10, 4, 22, 10)], True: [(6, 13, 21, 9), (10, 3, 21, 9)]}  # per-pixel batches: one size
for _ln, _l in LAYOUTS:
    _free = _l in (capi.YUV_YUYV, capi.YUV_UYVY, I444)
    _oracle = not _free
    _fast = {capi.YUV_YUYV: "k_yuv422_resize", capi.YUV_UYVY: "k_yuv422_resize", I444: "k_yuv444_resize"}.get(_l, "k4_nv12_resize")
    _other = {capi.YUV_YUYV: capi.YUV_UYVY, capi.YUV_UYVY: capi.YUV_YUYV}.get(_l)
    _lay = [("the other packed layout", dict(layout=_other))] if _other is not None else []
    if _l == I444:
        _crops = [(5, 3, 31, 17), (11, 3, 21, 9)]
        _crops_px = [(5, 3, 21, 9), (11, 4, 21, 9)]
    else:
        _crops, _crops_px = YUV_CROPS[_free], YUV_CROPS_PX[_free]
    add("yuv_%s_px" % _ln, "YUV " + _ln, yuv_inputs(_l, 160, "chroma_checker"), yuv_spell(_l, rng=capi.YUV_FULL, prim=capi.BT601),
        [("BT.709 for BT.601", dict(prim=capi.BT709)), ("B and R exchanged", dict(swap=True))] + _lay, oracle=_oracle)
    add("yuv_%s_rs" % _ln, "YUV " + _ln, yuv_inputs(_l, 161), yuv_spell(_l, rng=capi.YUV_LIMITED, prim=capi.BT709, swap=True, dst=(29, 19)),
        [("full for limited range", dict(rng=capi.YUV_FULL)), ("RGB for BGR", dict(swap=False)), ("Size transposed", dict(dst=(19, 29)))] + _lay,
        oracle=_oracle, kernel=_fast)
    add("yuv_%s_crops_letterbox" % _ln, "YUV " + _ln, yuv_inputs(_l, 162),
        yuv_spell(_l, rng=capi.YUV_LIMITED, prim=capi.BT2020, alpha=True, swap=True, dst=(40, 24), crops=_crops, ar=cvgs.PRESERVE_AR, bg=BG),
        [("background reversed", dict(bg=BG[::-1])), ("background behind the swap", dict(bg=[BG[2], BG[1], BG[0], BG[3]])),
         ("BT.709 for BT.2020", dict(prim=capi.BT709)), ("the next AspectRatio", dict(ar=cvgs.IGNORE_AR))], oracle=_oracle)
    add("yuv_%s_crops_px" % _ln, "YUV " + _ln, yuv_inputs(_l, 163), yuv_spell(_l, rng=capi.YUV_FULL, prim=capi.BT2020, alpha=True, crops=_crops_px, write="write3d"),
        [("BT.601 for BT.2020", dict(prim=capi.BT601)), ("limited for full range", dict(rng=capi.YUV_LIMITED)), ("crops exchanged", dict(crops=_crops_px[::-1]))],
        oracle=_oracle)


# ---- the fk:: spellings of the facade tests -------------------------------------------------------------------------------------------
def _fk_stages(st, rev=False):
    v = FKV[::-1] if rev else FKV
    return [cvgs.convertTo(st, _F3), cvgs.multiply(_F3, v), cvgs.convertTo(_F3, _U3)]


add("fk_read_mul_saturate", "fk", frame_inputs(cvgs.CV_8U, 3, 170, PX_HW), px_spell(cvgs.CV_8U, 3, _fk_stages, _U3), [("operand reversed", dict(rev=True))])
add("fk_resize_over_fused_nv12", "fk", yuv_inputs(capi.YUV_NV12, 171),
    yuv_spell(capi.YUV_NV12, rng=capi.YUV_FULL, prim=capi.BT709, alpha=True, dst=(29, 19), to_u8=True, write="write2d"),
    [("limited for full range", dict(rng=capi.YUV_LIMITED)), ("Size transposed", dict(dst=(19, 29)))])


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def write_inputs(directory):
    """<dir>/<case>.in<k>: the raw bytes of every input array of every case; returns {name: arrays}"""
    import os
    arrays = {}
    for name, case in CASES.items():
        arrays[name] = [np.ascontiguousarray(a) for a in case.inputs()]
        for k, a in enumerate(arrays[name]):
            a.tofile(os.path.join(directory, "%s.in%d" % (name, k)))
    return arrays


def read_output(directory, name):
    """The program's <case>.out: four int64 (guard, rows, row bytes, pitch), then guard + rows * pitch + guard bytes.  Asserts that the
    canary bands -- in front, behind, and the padding of every pitched row -- are untouched; returns the dense payload bytes."""
    import os
    raw = np.fromfile(os.path.join(directory, name + ".out"), np.uint8)
    guard, rows, row_bytes, pitch = (int(v) for v in raw[:32].view(np.int64))
    body = raw[32:]
    assert guard == GUARD and pitch >= row_bytes and body.size == 2 * guard + rows * pitch, (name, guard, rows, row_bytes, pitch, body.size)
    assert (body[:guard] == CANARY).all() and (body[body.size - guard:] == CANARY).all(), "%s: store outside the output" % name
    grid = body[guard:guard + rows * pitch].reshape(rows, pitch)
    assert (grid[:, row_bytes:] == CANARY).all(), "%s: store into the padding of a pitched row" % name
    return np.ascontiguousarray(grid[:, :row_bytes]).reshape(-1)


def model_of(name, arrays, **variant):
    """(model Result, iops) of a case's Python spelling (or of a near-miss of it) over the case's inputs"""
    iops, views = CASES[name].spell(MC.HostBackend(bf16_twin=False), arrays, **variant)
    return F.evaluate(iops, views), iops


def held(res, iops, payload):
    """(ok, ratio) of the program's payload bytes against a model Result; a payload of another size is outside every bound"""
    dst_type = iops[-1].dst_type
    got = payload.view(MC.np_dtype(dst_type))
    if got.size != res.v.size:
        return np.zeros(1, bool), np.full(1, np.inf)
    return res.check(res.logical(MC.widen_output(got, dst_type), logical_kind(iops[-1].kind)))
