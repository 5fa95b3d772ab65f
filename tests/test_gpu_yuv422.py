"""Packed 4:2:2 surfaces (YUYV / UYVY: capture cards, V4L2 cameras, 4:2:2 JPEG decoders) through the fused resize kernels of
k_yuv422.hip and the pointwise source kind SD_YUV422, mirroring tests/test_gpu_k4_planar.py.  Every case is compared bit for bit
(0 ULP) with the composed oracle value (tests/yuv422_cases.py; the method is pinned on the CPU by tests/test_yuv422.py) AND with the
interpreted kernel (CVGS_CHAIN_FORCE_GENERIC), with the kernel name asserted."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import yuv422_cases as Y

pytestmark = pytest.mark.gpu

F3, U3 = cvgs.CV_32FC3, cvgs.CV_8UC3
NORM = lambda f, cn=3: [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.subtract(f, [0.485, 0.456, 0.406, 0.5][:cn]), cvgs.divide(f, [0.229, 0.224, 0.225, 0.25][:cn])]
TORCH_DT = {np.float32: "float32", np.uint8: "uint8", np.float16: "float16"}


def run_both(oracle, build, surfs, layout, shp, np_dt, ot, want_prefix="k_yuv422_resize", bf16=False, check_generic=True):
    """build(wrap, out) -> ops, wrap(surface array) -> CV_8UC2 GpuMat.  Fast path and interpreted path vs the composed oracle value."""
    import torch
    dev = torch.device("cuda:0")
    ref = np.zeros(shp, np.float32 if bf16 else np_dt)
    ref_ot = cvgs.make_type(cvgs.DEPTH_32F, cvgs.type_cn(ot)) if bf16 else ot
    exp = Y.Expect(oracle, surfs, layout)
    with np.errstate(all="ignore"):
        exp.run(build(Y.wrap_array, cvgs.GpuMat.from_array(ref, ref_ot)) if not bf16 else build(Y.wrap_array, cvgs.GpuMat.from_array(ref, ref_ot), True))
    ts = {id(s): torch.from_numpy(s).to(dev) for s in surfs}
    gt = torch.zeros(shp, dtype=torch.bfloat16 if bf16 else getattr(torch, TORCH_DT[np_dt]), device=dev)
    ops = build(lambda a: Y.wrap_tensor(ts[id(a)]), cvgs.GpuMat.from_tensor(gt, ot))
    name = cvgs.kernel_name(*ops)
    assert name.startswith(want_prefix), name
    get = (lambda: gt.float().cpu().numpy()) if bf16 else (lambda: gt.cpu().numpy())
    if bf16:  # the oracle ran the chain up to the cast in fp32: round it to bf16 (nearest even) the way the store does
        ref = torch.from_numpy(ref).to(torch.bfloat16).float().numpy()
    cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    assert ref.any()
    H.assert_bit_exact(get(), ref, "fast path %s" % name)
    if check_generic:
        gt.zero_()
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=capi.CHAIN_FORCE_GENERIC)
        torch.cuda.synchronize()
        H.assert_bit_exact(get(), ref, "interpreted")
    return ref, name


SHAPES = [((640, 360), (213, 120)), ((640, 360), (64, 128)), ((1920, 1080), (1280, 720)), ((322, 198), (70, 66)), ((64, 36), (200, 150)),
          ((6, 4), (9, 7)), ((4, 4), (64, 3)), ((130, 2), (65, 5)),
          # single-pair rows, odd widths (crops of a wider surface), a last-pair clamp, odd heights, up-scaling
          ((1, 1), (5, 4)), ((2, 3), (70, 9)), ((3, 5), (64, 64)), ((5, 7), (33, 20)), ((5, 3), (3, 2)), ((127, 33), (300, 100))]


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prog", ["bgr_norm", "rgb_norm", "plain", "u8"])
def test_stretch(oracle, layout, shape, prog):
    (w, h), dst = shape
    surf = Y.random_surface(w + 2 + (w & 1), h + 1, 9000 + w + h, layout)
    f = F3

    def build(wrap, out):
        rd = cvgs.read_yuv422(wrap(surf).yuv422_roi(2, 1, w, h), dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        if prog == "bgr_norm":
            return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) + [cvgs.split(f, out, dst)]
        if prog == "rgb_norm":
            return [rd] + NORM(f) + [cvgs.split(f, out, dst)]
        if prog == "plain":
            return [rd, cvgs.multiply(f, [0.5, 0.25, 2.0]), cvgs.split(f, out, dst)]
        return [rd, cvgs.convertTo(f, U3), cvgs.write(U3, out)]

    if prog == "u8":
        shp, dt, ot = (dst[1], dst[0], 3), np.uint8, U3
    else:
        shp, dt, ot = (1, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1
    want = {"bgr_norm": "k_yuv422_resize_swap_mul_sub_div", "rgb_norm": "k_yuv422_resize_mul_sub_div", "plain": "k_yuv422_resize_arith",
            "u8": "k_yuv422_resize_u8c3"}[prog]
    _, name = run_both(oracle, build, [surf], layout, shp, dt, ot, want)
    assert name == want


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("ar", [cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])
@pytest.mark.parametrize("shape", [((640, 360), (64, 64)), ((360, 640), (96, 64)), ((1920, 1080), (640, 640)), ((322, 198), (70, 70)), ((3, 9), (40, 30))])
@pytest.mark.parametrize("prog", ["rgb_norm", "bgr_norm", "u8_batch"])
def test_letterbox_and_default_planes(oracle, layout, ar, shape, prog):
    (w, h), dst = shape
    we = w + (w & 1)
    s0, s1 = Y.random_surface(we, h, 9100 + w, layout), Y.random_surface(we, h, 9200 + w, layout)
    f, n = F3, 3

    def build(wrap, out):
        mats = [wrap(s).yuv422_roi(0, 0, w, h) for s in (s0, s1, s0)]
        rd = cvgs.read_yuv422(mats, dst, capi.YUV_LIMITED, capi.BT601, False, layout=layout)
        rd.ar = ar
        rd.background = cvgs._scalar([114.0, 100.5, 7.25])
        rd.used_planes = 2
        if prog == "rgb_norm":
            return [rd] + NORM(f) + [cvgs.split(f, out, dst)]
        if prog == "bgr_norm":
            return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) + [cvgs.split(f, out, dst)]
        return [rd, cvgs.convertTo(f, U3), cvgs.write(U3, out, dst)]

    if prog == "u8_batch":
        shp, dt, ot = (n, dst[0] * dst[1], 3), np.uint8, U3
    else:
        shp, dt, ot = (n, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1
    run_both(oracle, build, [s0, s1], layout, shp, dt, ot)


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("range_", [capi.YUV_FULL, capi.YUV_LIMITED])
@pytest.mark.parametrize("prim", [capi.BT601, capi.BT709, capi.BT2020])
@pytest.mark.parametrize("alpha", [False, True])
def test_ranges_primaries_alpha(oracle, layout, range_, prim, alpha):
    w, h, dst = 322, 198, (101, 77)
    surf = Y.random_surface(w, h, 9300, layout)
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)

    def build(wrap, out):
        return [cvgs.read_yuv422(wrap(surf), dst, range_, prim, alpha, layout=layout), cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn]), cvgs.split(f, out, dst)]

    run_both(oracle, build, [surf], layout, (1, cn * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1)


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("shape", [((640, 360), (224, 224)), ((5, 3), (70, 20))])
def test_fp16_tensor(oracle, layout, shape):
    (w, h), dst = shape
    surf = Y.random_surface(w + (w & 1), h, 9400, layout)
    f = F3

    def build(wrap, out):
        rd = cvgs.read_yuv422(wrap(surf).yuv422_roi(0, 0, w, h), dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) + [cvgs.convertTo(f, cvgs.CV_16FC3), cvgs.split(cvgs.CV_16FC3, out, dst)]

    run_both(oracle, build, [surf], layout, (1, 3 * dst[0] * dst[1]), np.float16, cvgs.CV_16FC1, "k_yuv422_resize_swap_mul_sub_div_f16")


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("prog,want", [("bgr_norm", "k_yuv422_resize_swap_mul_sub_div_bf16"), ("plain", "k_yuv422_resize_arith_bf16")])
def test_bf16_tensor(oracle, layout, prog, want):
    """CV_16BF hand-off tensors: the fp32 chain's value rounded to bf16 (nearest even) by the store."""
    w, h, dst = 640, 360, (128, 64)
    surf = Y.random_surface(w, h, 9450, layout)
    f = F3

    def build(wrap, out, fp32_reference=False):
        rd = cvgs.read_yuv422(wrap(surf), dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) if prog == "bgr_norm" else [cvgs.multiply(f, [0.5, 0.25, 2.0])]
        if fp32_reference:
            return [rd] + mid + [cvgs.split(f, out, dst)]
        return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, dst)]

    _, name = run_both(oracle, build, [surf], layout, (1, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_16BFC1, want, bf16=True)
    assert name == want


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("n", [70, 330])
def test_many_planes(oracle, layout, n):
    """More planes than the small argument block holds (65-320: the 16 KB block) and more than any block holds (> 320: a staged table)."""
    w, h, dst = 96, 64, (40, 24)
    surfs = [Y.random_surface(w, h, 9500 + i, layout) for i in range(4)]
    f = F3

    def build(wrap, out):
        mats = [wrap(surfs[i % 4]).yuv422_roi(2 * (i % 5), i % 7, w - 10 - (i % 3), h - 8) for i in range(n)]
        rd = cvgs.read_yuv422(mats, dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) + [cvgs.split(f, out, dst)]

    run_both(oracle, build, surfs, layout, (n, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1)


def crops_4k(n, seed):
    """n crops of a 3840 x 2160 surface: even x, odd and even y, odd and even widths."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        w, h = int(rng.randint(40, 400)), int(rng.randint(60, 500))
        x, y = 2 * int(rng.randint(0, (3840 - w) // 2)), int(rng.randint(0, 2160 - h))
        out.append((x, y | (i & 1) if (y | 1) + h <= 2160 else y, w, h))
    return out


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("target", ["fp32", "fp16", "bf16"])
def test_fifty_crops_of_a_4k_surface(oracle, layout, target):
    surf = Y.random_surface(3840, 2160, 9600, layout)
    crops, dst, f = crops_4k(50, 11), (64, 128), F3
    assert any(c[2] & 1 for c in crops) and any(c[1] & 1 for c in crops)

    def build(wrap, out, fp32_reference=False):
        rd = cvgs.read_yuv422([wrap(surf).yuv422_roi(*c) for c in crops], dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])]
        if target == "fp32" or fp32_reference:
            return [rd] + mid + [cvgs.split(f, out, dst)]
        t = cvgs.CV_16FC3 if target == "fp16" else cvgs.CV_16BFC3
        return [rd] + mid + [cvgs.convertTo(f, t), cvgs.split(t, out, dst)]

    shp = (50, 3 * dst[0] * dst[1])
    if target == "bf16":
        run_both(oracle, build, [surf], layout, shp, np.float32, cvgs.CV_16BFC1, "k_yuv422_resize_swap_mul_sub_div_bf16", bf16=True)
    elif target == "fp16":
        run_both(oracle, build, [surf], layout, shp, np.float16, cvgs.CV_16FC1, "k_yuv422_resize_swap_mul_sub_div_f16")
    else:
        run_both(oracle, build, [surf], layout, shp, np.float32, cvgs.CV_32FC1, "k_yuv422_resize_swap_mul_sub_div")


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("shape", [((1920, 1080), (640, 360)), ((322, 198), (70, 66)), ((64, 36), (200, 150)), ((5, 4), (63, 7))])
@pytest.mark.parametrize("spelling", ["cast", "cast_then_reorder", "reorder_then_cast", "scale"])
@pytest.mark.parametrize("cn", [3, 4])
def test_u8_image_outputs(oracle, layout, shape, spelling, cn):
    (w, h), dst = shape
    surf = Y.random_surface(w + (w & 1), h, 9700 + w, layout)
    f, u = cvgs.make_type(cvgs.DEPTH_32F, cn), cvgs.make_type(cvgs.DEPTH_8U, cn)
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA

    def build(wrap, out):
        rd = cvgs.read_yuv422(wrap(surf).yuv422_roi(0, 0, w, h), dst, capi.YUV_FULL, capi.BT709, cn == 4, layout=layout)
        mid = {"cast": [cvgs.convertTo(f, u)], "cast_then_reorder": [cvgs.convertTo(f, u), cvgs.cvtColor(swap, u)],
               "reorder_then_cast": [cvgs.cvtColor(swap, f), cvgs.convertTo(f, u)], "scale": [cvgs.convertTo(f, u, 1.4, -30.0)]}[spelling]
        return [rd] + mid + [cvgs.write(u, out)]

    tag = "u8c%d" % cn
    want = {"cast": "k_yuv422_resize_" + tag, "cast_then_reorder": "k_yuv422_resize_swap_" + tag, "reorder_then_cast": "k_yuv422_resize_swap_" + tag,
            "scale": "k_yuv422_resize_interp_" + tag}[spelling]
    ref, name = run_both(oracle, build, [surf], layout, (dst[1], dst[0], cn), np.uint8, u, want)
    assert name == want
    if cn == 4:
        assert (ref[..., 3] == 255).all()


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("shape", [((1920, 1080), (640, 360)), ((322, 198), (70, 66)), ((5, 4), (63, 7))])
@pytest.mark.parametrize("cn", [3, 4])
@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("half", [False, True])
def test_packed_float_image_outputs(oracle, layout, shape, cn, batch, half):
    (w, h), dst = shape
    surf = Y.random_surface(w + (w & 1), h, 9800 + w, layout)
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    t = cvgs.make_type(cvgs.DEPTH_16F, cn) if half else f
    n = 3 if batch else 1

    def build(wrap, out):
        view = wrap(surf).yuv422_roi(0, 0, w, h)
        rd = cvgs.read_yuv422([view] * n if batch else view, dst, capi.YUV_LIMITED, capi.BT601, cn == 4, layout=layout)
        if batch:
            rd.used_planes = 2
            rd.background = cvgs._scalar([3.0, -4.0, 17.5, 9.0][:cn] + [0.0] * (4 - cn))
        mid = [cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn])] + ([cvgs.convertTo(f, t)] if half else [])
        return [rd] + mid + [cvgs.write(t, out, dst) if batch else cvgs.write(t, out)]

    shp = (n, dst[0] * dst[1], cn) if batch else (dst[1], dst[0], cn)
    run_both(oracle, build, [surf], layout, shp, np.float16 if half else np.float32, t, "k_yuv422_resize")


ARITH = {
    "norm_then_add": (lambda f: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, [1.0, 4.0, 3.2]), cvgs.divide(f, [3.2, 0.6, 11.8]),
                                 cvgs.add(f, [0.5, 0.25, 0.125])], "k_yuv422_resize_arith"),
    "sub_div": (lambda f: [cvgs.subtract(f, [127.5] * 3), cvgs.divide(f, [58.4, 57.1, 57.4])], "k_yuv422_resize_arith"),
    "div_only": (lambda f: [cvgs.divide(f, [255.0, 127.5, 2.0])], "k_yuv422_resize_arith"),
    "swap_only": (lambda f: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)], "k_yuv422_resize_arith"),
    "nothing": (lambda f: [], "k_yuv422_resize_arith"),
    "zero_products": (lambda f: [cvgs.multiply(f, [0.0, -0.0, 1.0]), cvgs.divide(f, [3.2, 0.6, 11.8]), cvgs.add(f, [-0.0] * 3)], "k_yuv422_resize_arith"),
    "refused_divisor": (lambda f: [cvgs.divide(f, [2.0 ** 24, 0.6, float(np.float32(2.0) - np.float32(2.0 ** -23))])], "k_yuv422_resize_arith"),
    "three_linear_before_div": (lambda f: [cvgs.add(f, [1.0] * 3), cvgs.multiply(f, [0.5] * 3), cvgs.subtract(f, [0.25] * 3), cvgs.divide(f, [3.0, 7.0, 9.0])], "k_yuv422_resize_interp"),
}


@pytest.mark.parametrize("name", sorted(ARITH))
@pytest.mark.parametrize("layout,shape", [(Y.YUYV, ((640, 360), (213, 120))), (Y.UYVY, ((322, 198), (70, 66))), (Y.YUYV, ((64, 36), (200, 150)))])
def test_canonical_arithmetic_and_interpreted_programs(oracle, name, layout, shape):
    (w, h), dst = shape
    stages, want = ARITH[name]
    surf = Y.random_surface(w, h, 9900 + w, layout)
    yi = 0 if layout == Y.YUYV else 1
    surf[: h // 3, :, yi] = 16        # a black band: Y = 16 ...
    surf[: h // 3, :, 1 - yi] = 128   # ... with neutral chroma: R = G = B = 0 under the limited-range matrix (zero dividends)
    f = F3

    def build(wrap, out):
        return [cvgs.read_yuv422(wrap(surf), dst, capi.YUV_LIMITED, capi.BT601, False, layout=layout)] + stages(f) + [cvgs.split(f, out, dst)]

    _, got = run_both(oracle, build, [surf], layout, (1, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1, want)
    assert got == want


# ---- per-pixel reads (CVGS_READ_NV12 without a resize): the pointwise source kind ------------------------------------------------
@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("size", [(640, 360), (322, 99), (5, 3), (1, 1), (2, 2), (3, 1), (67, 5), (256, 4)])
@pytest.mark.parametrize("target", ["planar_f32", "planar_norm", "planar_f16", "planar_bf16", "packed_f32", "packed_f16", "packed_u8", "alpha_packed"])
def test_pointwise_targets(oracle, layout, size, target):
    w, h = size
    surf = Y.random_surface(w + 2 + (w & 1), h + 1, 10000 + w, layout)
    alpha = target == "alpha_packed"
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)

    def build(wrap, out, fp32_reference=False):
        rd = cvgs.read_yuv422(wrap(surf).yuv422_roi(2, 1, w, h), None, capi.YUV_LIMITED, capi.BT709, alpha, layout=layout)
        scale = cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn])
        if target == "planar_f32":
            return [rd, scale, cvgs.split(f, out, (w, h))]
        if target == "planar_norm":
            return [rd] + NORM(f) + [cvgs.split(f, out, (w, h))]
        if target == "planar_f16":
            return [rd, scale, cvgs.convertTo(f, cvgs.CV_16FC3), cvgs.split(cvgs.CV_16FC3, out, (w, h))]
        if target == "planar_bf16":
            if fp32_reference:
                return [rd, scale, cvgs.split(f, out, (w, h))]
            return [rd, scale, cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, (w, h))]
        if target in ("packed_f32", "alpha_packed"):
            return [rd, scale, cvgs.write(f, out)]
        if target == "packed_f16":
            return [rd, scale, cvgs.convertTo(f, cvgs.CV_16FC3), cvgs.write(cvgs.CV_16FC3, out)]
        if target == "packed_u8":
            return [rd, cvgs.convertTo(f, U3, 1.2, -10.0), cvgs.write(U3, out)]
        raise AssertionError(target)

    planar = target.startswith("planar")
    shp = (1, 3 * w * h) if planar else (h, w, cn)
    if target == "planar_bf16":
        run_both(oracle, build, [surf], layout, shp, np.float32, cvgs.CV_16BFC1, "pointwise4_yuv422_bf16", bf16=True)
        return
    dt = np.float16 if target.endswith("f16") else (np.uint8 if target == "packed_u8" else np.float32)
    ot = {"planar_f32": cvgs.CV_32FC1, "planar_norm": cvgs.CV_32FC1, "planar_f16": cvgs.CV_16FC1, "packed_f32": F3, "packed_f16": cvgs.CV_16FC3,
          "packed_u8": U3, "alpha_packed": cvgs.CV_32FC4}[target]
    want = "pointwise4_yuv422" + ("_f16" if target.endswith("f16") else ("_u8" if target == "packed_u8" else ""))
    _, name = run_both(oracle, build, [surf], layout, shp, dt, ot, want)
    assert name == want


@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_pointwise_batch_with_default_planes(oracle, layout):
    w, h, n = 130, 37, 4
    surfs = [Y.random_surface(w + 2, h + 3, 10100 + i, layout) for i in range(2)]
    f = F3

    def build(wrap, out):
        mats = [wrap(surfs[i % 2]).yuv422_roi(2, i, w, h) for i in range(n)]
        rd = cvgs.read_yuv422(mats, None, capi.YUV_FULL, capi.BT601, False, layout=layout)
        rd.used_planes = 3
        rd.background = cvgs._scalar([3.0, -4.0, 17.5])
        return [rd] + NORM(f) + [cvgs.split(f, out, (w, h))]

    run_both(oracle, build, surfs, layout, (n, 3 * w * h), np.float32, cvgs.CV_32FC1, "pointwise4_yuv422")


# ---- the byte order is live; 4:2:2 with pairwise equal chroma rows == the NV12 picture ----------------------------------------------------
def test_swapping_the_byte_order_changes_the_result():
    import torch
    dev = torch.device("cuda:0")
    surf = Y.random_surface(640, 360, 10200, Y.YUYV)
    st = torch.from_numpy(surf).to(dev)
    dst, f, outs = (213, 120), F3, {}
    for dsize in (dst, None):
        for layout in Y.LAYOUTS:
            shape = (1, 3 * dst[0] * dst[1]) if dsize else (1, 3 * 640 * 360)
            gt = torch.zeros(shape, dtype=torch.float32, device=dev)
            ops = [cvgs.read_yuv422(Y.wrap_tensor(st), dsize, capi.YUV_LIMITED, capi.BT709, False, layout=layout), cvgs.multiply(f, [0.5] * 3),
                   cvgs.split(f, cvgs.GpuMat.from_tensor(gt, cvgs.CV_32FC1), dsize or (640, 360))]
            cvgs.executeOperations(torch.cuda.current_stream(), *ops)
            torch.cuda.synchronize()
            outs[(dsize, layout)] = gt.cpu().numpy()
        assert (outs[(dsize, Y.YUYV)] != outs[(dsize, Y.UYVY)]).mean() > 0.5


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("dst", [(213, 120), (64, 128), (800, 500)])
def test_pairwise_equal_chroma_rows_equal_the_nv12_picture(oracle, layout, dst):
    """A 4:2:2 surface whose chroma rows 2k and 2k + 1 are equal holds the picture of an NV12 surface: same tensor, and the oracle's
    DIRECT NV12 answer is the reference here."""
    import torch
    dev = torch.device("cuda:0")
    w, h = 640, 360
    nv = H.random_u8((h * 3 // 2, w), 10300)
    y, u, v = nv[:h], nv[h:, 0::2], nv[h:, 1::2]
    surf = Y.pack(y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0), layout)
    f = F3
    prog = lambda: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f)
    ref = np.zeros((1, 3 * dst[0] * dst[1]), np.float32)
    luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, nv.ctypes.data, nv.strides[0], owner=nv)
    oracle.execute(cvgs.lower([cvgs.read_nv12(luma, dst, capi.YUV_LIMITED, capi.BT709, False)] + prog() + [cvgs.split(f, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), dst)]))
    st = torch.from_numpy(surf).to(dev)
    gt = torch.zeros(ref.shape, dtype=torch.float32, device=dev)
    ops = [cvgs.read_yuv422(Y.wrap_tensor(st), dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)] + prog() + [cvgs.split(f, cvgs.GpuMat.from_tensor(gt, cvgs.CV_32FC1), dst)]
    assert cvgs.kernel_name(*ops) == "k_yuv422_resize_swap_mul_sub_div"
    cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    H.assert_bit_exact(gt.cpu().numpy(), ref, "4:2:2 with doubled chroma rows vs the NV12 picture")


# ---- ticks: cvgs_execute_many ------------------------------------------------------------------------------------------------------------
def _tick(layout, n_cams, n_crops, dst, seed, dev, target="fp32", surf_size=(1280, 720)):
    import torch
    w, h = surf_size
    f = F3
    rng = np.random.RandomState(seed)
    surfs = [Y.random_surface(w, h, seed + 10 * i, layout) for i in range(n_cams)]
    ts = [torch.from_numpy(s).to(dev) for s in surfs]
    crops = []
    for _ in range(n_crops):
        cw, ch = int(rng.randint(9, 300)), int(rng.randint(9, 300))
        crops.append((2 * int(rng.randint(0, (w - cw) // 2)), int(rng.randint(0, h - ch)), cw, ch))
    tdt = {"fp32": torch.float32, "bf16": torch.bfloat16}[target]

    def chain(wrap, cam, out, fp32_reference=False):
        rd = cvgs.read_yuv422([wrap(cam).yuv422_roi(*c) for c in crops], dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])]
        if target == "fp32" or fp32_reference:
            return [rd] + mid + [cvgs.split(f, out, dst)]
        return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, dst)]

    outs = [torch.full((n_crops, 3 * dst[0] * dst[1]), -3.0, dtype=tdt, device=dev) for _ in range(n_cams)]
    ot = cvgs.CV_32FC1 if target == "fp32" else cvgs.CV_16BFC1
    chains = [chain(lambda i: Y.wrap_tensor(ts[i]), cam, cvgs.GpuMat.from_tensor(outs[cam], ot)) for cam in range(n_cams)]
    return surfs, ts, crops, chain, outs, chains


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("n_cams,n_crops,target", [(2, 5, "fp32"), (4, 50, "fp32"), (16, 50, "fp32"), (16, 50, "bf16"), (7, 13, "bf16")])
def test_tick_in_one_graph_node(oracle, layout, n_cams, n_crops, target):
    """2-16 surfaces' crop chains (host descriptors) as ONE cvgs_execute_many launch: captured into a graph with exactly one kernel node,
    equal to the one-by-one result and to the composed oracle value."""
    import torch
    dev = torch.device("cuda:0")
    dst = (64, 128)
    surfs, ts, crops, chain, outs, chains = _tick(layout, n_cams, n_crops, dst, 10400, dev, target)
    get = lambda t: t.float().cpu().numpy()
    one_by_one = []
    for ops in chains:
        cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    for cam in range(n_cams):
        one_by_one.append(get(outs[cam]))
        outs[cam].fill_(-3.0)
    exp = Y.Expect(oracle, surfs, layout)
    for cam in (0, n_cams - 1):
        ref = np.zeros((n_crops, 3 * dst[0] * dst[1]), np.float32)
        exp.run(chain(lambda i: Y.wrap_array(surfs[i]), cam, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), True))
        if target == "bf16":
            ref = torch.from_numpy(ref).to(torch.bfloat16).float().numpy()
        H.assert_bit_exact(one_by_one[cam], ref, "one by one, camera %d" % cam)
    from tests.test_gpu_many import _captured_kernel_nodes
    lib = capi.load_library()
    lowered = [cvgs.lower(c) for c in chains]  # (kept alive: the packed descriptors borrow their host arrays)
    packed = cvgs.pack_chains(lowered)
    assert _captured_kernel_nodes(lib, packed, n_cams, None) == 1, "one fused launch"
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        capi.check(lib.cvgs_execute_many(packed, n_cams, s.cuda_stream))
    torch.cuda.synchronize()
    assert all((get(o) == -3.0).all() for o in outs)  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for cam in range(n_cams):
        H.assert_bit_exact(get(outs[cam]), one_by_one[cam], "tick, camera %d" % cam)
    del g, packed, lowered


@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_aliased_tick_falls_back_to_sequential_launches(oracle, layout):
    """Two chains that write the SAME tensor are not independent: the tick keeps the sequential meaning (the second chain's values win)."""
    import torch
    dev = torch.device("cuda:0")
    dst = (64, 128)
    surfs, ts, crops, chain, outs, chains = _tick(layout, 2, 6, dst, 10500, dev)
    aliased = [chains[0], chain(lambda i: Y.wrap_tensor(ts[i]), 1, cvgs.GpuMat.from_tensor(outs[0], cvgs.CV_32FC1))]
    from tests.test_gpu_many import _captured_kernel_nodes
    lowered = [cvgs.lower(c) for c in aliased]  # (kept alive: the packed descriptors borrow their host arrays)
    assert _captured_kernel_nodes(capi.load_library(), cvgs.pack_chains(lowered), 2, None) == 2, "sequential launches"
    for o in outs:
        o.fill_(-3.0)
    held = cvgs.executeMany(torch.cuda.current_stream(), aliased)
    torch.cuda.synchronize()
    ref = np.zeros((6, 3 * dst[0] * dst[1]), np.float32)
    Y.Expect(oracle, surfs, layout).run(chain(lambda i: Y.wrap_array(surfs[i]), 1, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1)))
    H.assert_bit_exact(outs[0].cpu().numpy(), ref, "aliased pair: the second chain's values")
    assert (outs[1].cpu().numpy() == -3.0).all()
    del held


# ---- CircularTensor push -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("order", [cvgs.NewestFirst, cvgs.OldestFirst])
def test_circular_tensor_push(oracle, layout, resize, order):
    """Camera frames pushed into a CircularTensor through the 4:2:2 read (per-pixel and resized): the whole tensor after every update."""
    import torch
    from tests.test_gpu_circular_nv12 import _read_device
    dev = torch.device("cuda:0")
    w, h = 64, 32
    dst = (32, 16) if resize else None
    ow, oh = dst if resize else (w, h)
    f, batch = F3, 3
    ct = cvgs.CircularTensor(Y.CV_8UC2, cvgs.CV_32FC1, 3, batch, order, cvgs.Standard, ow, oh)
    history = []
    for k in range(5):
        surf = Y.random_surface(w, h, 10600 + k, layout)
        st = torch.from_numpy(surf).to(dev)
        ops = lambda m: [cvgs.read_yuv422(m, dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout), cvgs.multiply(f, [0.5, 0.25, 2.0])]
        ct.update(torch.cuda.current_stream(), *(ops(Y.wrap_tensor(st)) + [ct.write_split(f)]))
        torch.cuda.synchronize()
        ref = np.zeros((1, 3 * ow * oh), np.float32)
        Y.Expect(oracle, [surf], layout).run(ops(Y.wrap_array(surf)) + [cvgs.split(f, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (ow, oh))])
        history.insert(0, ref.reshape(-1))  # newest first
        got = _read_device(ct.data(), ct.nbytes()).view(np.float32).reshape(batch, -1)
        for age, r in enumerate(history[:batch]):
            slot = age if order == cvgs.NewestFirst else batch - 1 - age
            H.assert_bit_exact(got[slot], r, "update %d, age %d" % (k, age))
    ct.release()


# ---- seeded differential fuzz: fast kernels vs the interpreted kernel vs the composed oracle -------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_differential_fuzz(oracle, seed):
    rng = np.random.RandomState(4220 + seed)
    layout = Y.LAYOUTS[seed & 1]
    sw, sh = 2 * int(rng.randint(1, 200)), int(rng.randint(1, 200))
    surf = Y.random_surface(sw, sh, 10700 + seed, layout)
    n = int(rng.randint(1, 9))
    crops = []
    for _ in range(n):
        cw, ch = int(rng.randint(1, sw + 1)), int(rng.randint(1, sh + 1))
        crops.append((2 * int(rng.randint(0, (sw - cw) // 2 + 1)), int(rng.randint(0, sh - ch + 1)), cw, ch))
    resize = bool(rng.randint(0, 4))
    if not resize:
        crops = [(c[0], c[1], crops[0][2], crops[0][3]) for c in crops if c[0] + crops[0][2] <= sw and c[1] + crops[0][3] <= sh] or [crops[0]]
        n = len(crops)
    dst = (int(rng.randint(1, 150)), int(rng.randint(1, 100))) if resize else None
    ow, oh = dst if resize else (crops[0][2], crops[0][3])
    alpha = bool(rng.randint(0, 2))
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    range_, prim = int(rng.randint(0, 2)), int(rng.randint(0, 3))
    ar = int(rng.choice([cvgs.IGNORE_AR, cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])) if resize else cvgs.IGNORE_AR
    used = n if rng.randint(0, 3) else int(rng.randint(1, n + 1))
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA
    progs = [[], [cvgs.cvtColor(swap, f)] + NORM(f, cn), NORM(f, cn), [cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn]), cvgs.add(f, [1.0, -2.0, 0.5, 3.0][:cn])],
             [cvgs.add(f, [1.0] * cn), cvgs.multiply(f, [0.5] * cn), cvgs.subtract(f, [0.25] * cn), cvgs.divide(f, [3.0, 7.0, 9.0, 2.0][:cn])]]
    prog = progs[int(rng.randint(0, len(progs)))]
    packed = bool(rng.randint(0, 3) == 0)

    def build(wrap, out):
        rd = cvgs.read_yuv422([wrap(surf).yuv422_roi(*c) for c in crops], dst, range_, prim, alpha, layout=layout)
        rd.ar, rd.used_planes = ar, used
        rd.background = cvgs._scalar([114.0, 100.5, 7.25, 30.0][:cn] + [0.0] * (4 - cn))
        return [rd] + prog + [cvgs.write(f, out, (ow, oh)) if packed else cvgs.split(f, out, (ow, oh))]

    shp = (n, ow * oh, cn) if packed else (n, cn * ow * oh)
    ot = f if packed else cvgs.CV_32FC1
    run_both(oracle, build, [surf], layout, shp, np.float32, ot, "k_yuv422_resize" if resize else "pointwise4_yuv422")


def test_cpp_facade_program_passes():
    """cvGS::cvtColorYUY2 / cvtColorUYVY with crops -> resize -> normalize -> split (tests/cpp/test_yuv422.cpp)."""
    import os
    import subprocess
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "test_yuv422")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", cpp, "bin/test_yuv422"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- the remaining u8 image cases of tests/test_gpu_k4_planar.py: programs in front of the cast, batches with saturating backgrounds --------
@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("shape", [((640, 360), (213, 120)), ((1920, 1080), (640, 360)), ((322, 198), (64, 66)), ((322, 198), (128, 5)),
                                   ((64, 36), (200, 150)), ((3840, 2160), (1920, 1080)), ((5, 4), (63, 7))])
@pytest.mark.parametrize("prog", ["cast", "swap_cast", "scale_cast", "swap_scale_add_cast"])
@pytest.mark.parametrize("batch", [False, True])
def test_u8_image_outputs_with_programs_and_batches(oracle, layout, shape, prog, batch):
    """Camera surface -> packed u8 C3 image(s): resize -> [swap / scale in float] -> SaturateCast -> write; batches with usedPlanes < N whose
    background (300, -4, 17.5) has to saturate through the store's conversion on the windowed u8 kernels."""
    (w, h), dst = shape
    surf = Y.random_surface(w + (w & 1), h, 11000 + w, layout)
    f, u = F3, U3
    n = 3 if batch else 1

    def build(wrap, out):
        view = wrap(surf).yuv422_roi(0, 0, w, h)
        rd = cvgs.read_yuv422([view] * n if batch else view, dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
        if batch:
            rd.used_planes = 2
            rd.background = cvgs._scalar([300.0, -4.0, 17.5])
        ops = [rd]
        if prog.startswith("swap"):
            ops.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f))
        if prog == "scale_cast":
            ops.append(cvgs.convertTo(f, u, 1.7))  # saturates the bright pixels
        elif prog == "swap_scale_add_cast":
            ops.append(cvgs.convertTo(f, u, 0.75, -20.5))  # and the dark ones
        else:
            ops.append(cvgs.convertTo(f, u))
        return ops + [cvgs.write(u, out, dst) if batch else cvgs.write(u, out)]

    shp = (n, dst[0] * dst[1], 3) if batch else (dst[1], dst[0], 3)
    want = {"cast": "k_yuv422_resize_u8c3", "swap_cast": "k_yuv422_resize_swap_u8c3", "scale_cast": "k_yuv422_resize_interp_u8c3",
            "swap_scale_add_cast": "k_yuv422_resize_interp_u8c3"}[prog]
    ref, name = run_both(oracle, build, [surf], layout, shp, np.uint8, u, want)
    assert name == want
    if prog == "scale_cast" and w > 6:
        assert (ref == 255).any()
    if batch and prog == "cast":  # the default-value plane: the background through the saturating store (300 -> 255, -4 -> 0, 17.5 -> 18)
        assert (ref[2] == np.array([255, 0, 18], np.uint8)).all()


@pytest.mark.parametrize("layout", Y.LAYOUTS)
@pytest.mark.parametrize("cn", [3, 4])
@pytest.mark.parametrize("batch", [False, True])
def test_canonical_program_into_a_u8_image(oracle, layout, cn, batch):
    """Camera surface -> resize -> swap, multiply, add (brightness / contrast) -> SaturateCast -> packed u8 image: the canonical arithmetic
    program in front of the store's conversion (kernel k_yuv422_resize_arith_u8cN); batch: default-value planes whose background saturates."""
    (w, h), dst = (640, 360), (213, 120)
    surf = Y.random_surface(w, h, 11300 + cn, layout)
    f, u = cvgs.make_type(cvgs.DEPTH_32F, cn), cvgs.make_type(cvgs.DEPTH_8U, cn)
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA
    n = 3 if batch else 1

    def build(wrap, out):
        view = wrap(surf)
        rd = cvgs.read_yuv422([view] * n if batch else view, dst, capi.YUV_FULL, capi.BT709, cn == 4, layout=layout)
        if batch:
            rd.used_planes = 2
            rd.background = cvgs._scalar([300.0, -4.0, 17.5, 9.0][:cn] + [0.0] * (4 - cn))
        return [rd, cvgs.cvtColor(swap, f), cvgs.multiply(f, [1.25, 0.75, 1.1, 1.0][:cn]), cvgs.add(f, [-12.5, 20.0, 0.25, 0.0][:cn]), cvgs.convertTo(f, u),
                cvgs.write(u, out, dst) if batch else cvgs.write(u, out)]

    shp = (n, dst[0] * dst[1], cn) if batch else (dst[1], dst[0], cn)
    ref, name = run_both(oracle, build, [surf], layout, shp, np.uint8, u, "k_yuv422_resize_arith_u8c%d" % cn)
    assert name == "k_yuv422_resize_arith_u8c%d" % cn
    assert (ref == 255).any() and (ref == 0).any()


# ---- the descriptor queue does not take the layouts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_descriptor_queue_refuses_the_layouts(layout):
    """A 4:2:2 chain of the shape the queue serves for NV12 crops is refused (CVGS_ERR_UNSUPPORTED) and nothing runs: the queue's
    worker must never read a CV_8UC2 surface as NV12."""
    import torch
    dev = torch.device("cuda:0")
    surf = Y.random_surface(640, 360, 11400, layout)
    st = torch.from_numpy(surf).to(dev)
    dst, f = (64, 128), F3
    out = torch.full((4, 3 * dst[0] * dst[1]), -3.0, dtype=torch.float32, device=dev)
    crops = [(0, 0, 640, 360), (10, 20, 100, 200), (300, 100, 64, 128), (2, 2, 64, 64)]
    ops = [cvgs.read_yuv422([Y.wrap_tensor(st).yuv422_roi(*c) for c in crops], dst, capi.YUV_FULL, capi.BT601, False, layout=layout),
           cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
           cvgs.split(f, cvgs.GpuMat.from_tensor(out, cvgs.CV_32FC1), dst)]
    q = cvgs.Queue()
    try:
        with pytest.raises(capi.CvgsError) as e:
            q.submit(*ops)
        assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.CvgsError) as e:
            q.submit_on(torch.cuda.current_stream(), *ops)
        assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        q.destroy()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -3.0).all()
