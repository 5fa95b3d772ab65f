"""Planar 4:4:4 surfaces (I444: rocDecode's YUV444 output, rocJPEG's output for non-subsampled JPEGs) through the fused resize kernels of
k_yuv444.hip and the pointwise source kind SD_YUV444.  Every case is compared bit for bit (0 ULP) with the composed oracle value
(tests/yuv444_cases.py; the method is pinned on the CPU by tests/test_yuv444.py) AND with the interpreted kernel
(CVGS_CHAIN_FORCE_GENERIC), with the kernel name asserted.  Shapes are the small ones at which this kernel can go wrong: rows of one
and two pixels (the 1-byte window, the clamp of the 2-byte window), odd sizes, widths around the 64-column tile, more than one block."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import yuv444_cases as Y

pytestmark = pytest.mark.gpu

F3, U3 = cvgs.CV_32FC3, cvgs.CV_8UC3
NORM = lambda f, cn=3: [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.subtract(f, [0.485, 0.456, 0.406, 0.5][:cn]), cvgs.divide(f, [0.229, 0.224, 0.225, 0.25][:cn])]
TORCH_DT = {np.float32: "float32", np.uint8: "uint8", np.float16: "float16"}
FAMILY = "k_yuv444_resize"


def run_both(oracle, build, surfs, shp, np_dt, ot, want_prefix=FAMILY, bf16=False, check_generic=True):
    """build(wrap, out) -> ops, wrap(Surf) -> CV_8UC1 luma view with uv_offset.  Fast path and interpreted path vs the composed oracle value."""
    import torch
    dev = torch.device("cuda:0")
    ref = np.zeros(shp, np.float32 if bf16 else np_dt)
    ref_ot = cvgs.make_type(cvgs.DEPTH_32F, cvgs.type_cn(ot)) if bf16 else ot
    exp = Y.Expect(oracle, surfs)
    with np.errstate(all="ignore"):
        exp.run(build(Y.wrap_array, cvgs.GpuMat.from_array(ref, ref_ot)) if not bf16 else build(Y.wrap_array, cvgs.GpuMat.from_array(ref, ref_ot), True))
    wrap, _held = Y.tensor_wrapper(surfs, dev)
    gt = torch.zeros(shp, dtype=torch.bfloat16 if bf16 else getattr(torch, TORCH_DT[np_dt]), device=dev)
    ops = build(wrap, cvgs.GpuMat.from_tensor(gt, ot))
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


def view_of(wrap, s, w, h):
    """The w x h view at the odd origin (1, 1) of a surface made by padded(w, h, ...)."""
    return wrap(s).yuv444_roi(1, 1, w, h)


def padded(w, h, seed):
    """A surface two columns wider and two rows taller than the view, with an odd step and planes an odd distance apart."""
    step = (w + 2) | 1
    return Y.Surf(w + 2, h + 2, seed, step=step + 2, uv=(h + 2) * (step + 2) + 7)


SOURCES = [(1, 1), (2, 1), (1, 5), (3, 9), (63, 5), (64, 4), (65, 3), (67, 5), (322, 198)]
TARGETS = [(63, 5), (64, 9), (65, 3), (130, 7)]  # shrink and enlarge, across the 64-column tile
PROGRAMS = {
    "bgr_norm": (lambda f: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f), "swap_mul_sub_div"),
    "rgb_norm": (lambda f: NORM(f), "mul_sub_div"),
    "plain": (lambda f: [cvgs.multiply(f, [0.5, 0.25, 2.0])], "arith"),
    "arith": (lambda f: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, [1.0, 4.0, 3.2]), cvgs.divide(f, [3.2, 0.6, 11.8]),
                         cvgs.add(f, [0.5, 0.25, 0.125])], "arith"),
    "interp": (lambda f: [cvgs.add(f, [1.0] * 3), cvgs.multiply(f, [0.5] * 3), cvgs.subtract(f, [0.25] * 3), cvgs.divide(f, [3.0, 7.0, 9.0])], "interp"),
}


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("prog", sorted(PROGRAMS) + ["u8"])
def test_stretch(oracle, src, prog):
    w, h = src
    surf = padded(w, h, 9000 + 7 * w + h)
    f = F3
    for dst in TARGETS:
        def build(wrap, out):
            rd = cvgs.read_yuv444(view_of(wrap, surf, w, h), dst, capi.YUV_LIMITED, capi.BT709, False)
            if prog == "u8":
                return [rd, cvgs.convertTo(f, U3), cvgs.write(U3, out)]
            return [rd] + PROGRAMS[prog][0](f) + [cvgs.split(f, out, dst)]

        if prog == "u8":
            shp, dt, ot, want = (dst[1], dst[0], 3), np.uint8, U3, FAMILY + "_u8c3"
        else:
            shp, dt, ot, want = (1, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1, FAMILY + "_" + PROGRAMS[prog][1]
        _, name = run_both(oracle, build, [surf], shp, dt, ot, want)
        assert name == want, dst


# (the u8 image kinds carry their own programs)
TARGET_KINDS = [(k, p) for k in ["planar_f16", "planar_bf16", "packed_f32", "packed_f16"] for p in ["bgr_norm", "plain", "interp"]] + \
               [("u8c3_swap", "own"), ("u8c4", "own"), ("u8c4_arith", "own")]


@pytest.mark.parametrize("src", [(1, 1), (2, 1), (3, 9), (65, 3), (322, 198)])
@pytest.mark.parametrize("kind,prog", TARGET_KINDS)
def test_every_target(oracle, src, kind, prog):
    """The targets beside the planar fp32 tensor and the plain u8 image of test_stretch, for a compile-time, the canonical and the
    interpreted program."""
    w, h = src
    surf = padded(w, h, 9100 + 7 * w + h)
    alpha = kind.startswith("u8c4")
    cn = 4 if alpha else 3
    f, u = cvgs.make_type(cvgs.DEPTH_32F, cn), cvgs.make_type(cvgs.DEPTH_8U, cn)
    swap = cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA
    for dst in [(65, 3), (130, 7)]:
        def build(wrap, out, fp32_reference=False):
            rd = cvgs.read_yuv444(view_of(wrap, surf, w, h), dst, capi.YUV_LIMITED, capi.BT601, alpha)
            mid = PROGRAMS[prog][0](f) if prog != "own" else []
            if kind == "planar_f16":
                return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16FC3), cvgs.split(cvgs.CV_16FC3, out, dst)]
            if kind == "planar_bf16":
                return [rd] + mid + ([cvgs.split(f, out, dst)] if fp32_reference else [cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, dst)])
            if kind == "packed_f32":
                return [rd] + mid + [cvgs.write(f, out)]
            if kind == "packed_f16":
                return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16FC3), cvgs.write(cvgs.CV_16FC3, out)]
            if kind == "u8c3_swap":
                return [rd, cvgs.convertTo(f, u), cvgs.cvtColor(swap, u), cvgs.write(u, out)]
            if kind == "u8c4":
                return [rd, cvgs.convertTo(f, u), cvgs.write(u, out)]
            return [rd, cvgs.cvtColor(swap, f), cvgs.multiply(f, [1.25, 0.75, 1.1, 1.0]), cvgs.add(f, [-12.5, 20.0, 0.25, 0.0]), cvgs.convertTo(f, u), cvgs.write(u, out)]

        suffix = PROGRAMS[prog][1] if prog != "own" else ""
        if kind == "planar_f16":
            want = FAMILY + "_" + suffix + "_f16"
            _, name = run_both(oracle, build, [surf], (1, 3 * dst[0] * dst[1]), np.float16, cvgs.CV_16FC1, want)
        elif kind == "planar_bf16":
            want = FAMILY + "_" + suffix + "_bf16"
            _, name = run_both(oracle, build, [surf], (1, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_16BFC1, want, bf16=True)
        elif kind == "packed_f32":
            want = FAMILY + "_" + ("arith" if prog != "interp" else "interp")  # packed pixels: the canonical program, also for the normalisation
            _, name = run_both(oracle, build, [surf], (dst[1], dst[0], 3), np.float32, F3, want)
        elif kind == "packed_f16":
            _, name = run_both(oracle, build, [surf], (dst[1], dst[0], 3), np.float16, cvgs.CV_16FC3, FAMILY)
            want = name  # (the cast to fp16 stays in the program: which program class serves it is not pinned here)
        else:
            want = FAMILY + {"u8c3_swap": "_swap_u8c3", "u8c4": "_u8c4", "u8c4_arith": "_arith_u8c4"}[kind]
            ref, name = run_both(oracle, build, [surf], (dst[1], dst[0], cn), np.uint8, u, want)
            if cn == 4:
                assert (ref[..., 3] == 255).all()
        assert name == want, (dst, name)


# ---- layout freedom: crops at odd origins, odd step and plane distance, data at every residue mod 4 ----------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("dst", [None, (65, 9)])
def test_unaligned_surfaces_and_odd_crops(oracle, lead, dst):
    surf = Y.Surf(67, 21, 9200 + lead, step=71, uv=21 * 71 + 14, lead=lead)
    assert surf.step % 2 and surf.uv % 2 and surf.uv % surf.step and surf.step % 4 != 0
    crops = [(1, 1, 33, 9), (3, 5, 33, 9), (34, 12, 33, 9), (7, 2, 33, 9)] if dst is None else [(1, 1, 66, 20), (3, 5, 7, 11), (66, 20, 1, 1), (33, 0, 2, 21), (0, 7, 67, 1)]
    f = F3
    ow, oh = dst if dst else (33, 9)

    def build(wrap, out):
        m = wrap(surf)
        return [cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, capi.YUV_FULL, capi.BT2020, False)] + NORM(f) + [cvgs.split(f, out, (ow, oh))]

    import torch
    wrap, held = Y.tensor_wrapper([surf], torch.device("cuda:0"))
    assert wrap(surf).data % 4 == lead
    del held
    run_both(oracle, build, [surf], (len(crops), 3 * ow * oh), np.float32, cvgs.CV_32FC1, FAMILY + "_mul_sub_div" if dst else "pointwise4_yuv444")


# ---- options ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ar", [cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT])
@pytest.mark.parametrize("shape", [((322, 198), (70, 70)), ((3, 9), (40, 30)), ((65, 3), (64, 64)), ((1, 1), (9, 5))])
@pytest.mark.parametrize("prog", ["rgb_norm", "bgr_norm", "u8_batch"])
def test_letterbox_and_default_planes(oracle, ar, shape, prog):
    (w, h), dst = shape
    s0, s1 = padded(w, h, 9300 + w), padded(w, h, 9400 + w)
    f, n = F3, 3

    def build(wrap, out):
        rd = cvgs.read_yuv444([view_of(wrap, s, w, h) for s in (s0, s1, s0)], dst, capi.YUV_LIMITED, capi.BT601, False)
        rd.ar = ar
        rd.background = cvgs._scalar([114.0, 100.5, 7.25])
        rd.used_planes = 2
        if prog == "u8_batch":
            return [rd, cvgs.convertTo(f, U3), cvgs.write(U3, out, dst)]
        return [rd] + PROGRAMS[prog][0](f) + [cvgs.split(f, out, dst)]

    if prog == "u8_batch":
        shp, dt, ot = (n, dst[0] * dst[1], 3), np.uint8, U3
    else:
        shp, dt, ot = (n, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1
    run_both(oracle, build, [s0, s1], shp, dt, ot)


@pytest.mark.parametrize("range_", [capi.YUV_FULL, capi.YUV_LIMITED])
@pytest.mark.parametrize("prim", [capi.BT601, capi.BT709, capi.BT2020])
@pytest.mark.parametrize("alpha", [False, True])
def test_ranges_primaries_alpha(oracle, range_, prim, alpha):
    w, h, dst = 67, 5, (130, 7)
    surf = padded(w, h, 9500)
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)

    def build(wrap, out):
        return [cvgs.read_yuv444(view_of(wrap, surf, w, h), dst, range_, prim, alpha), cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn]), cvgs.split(f, out, dst)]

    run_both(oracle, build, [surf], (1, cn * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1)

    def pixels(wrap, out):
        return [cvgs.read_yuv444(view_of(wrap, surf, w, h), None, range_, prim, alpha), cvgs.multiply(f, [0.5, 0.25, 2.0, 1.5][:cn]), cvgs.split(f, out, (w, h))]

    run_both(oracle, pixels, [surf], (1, cn * w * h), np.float32, cvgs.CV_32FC1, "pointwise4_yuv444")


@pytest.mark.parametrize("n", [70, 330])
@pytest.mark.parametrize("target", ["fp32", "bf16"])
def test_many_planes(oracle, n, target):
    """More planes than the small argument block holds (65-320: the 16 KB block) and more than any block holds (> 320: a staged table)."""
    w, h, dst = 96, 64, (40, 24)
    surfs = [Y.Surf(w, h, 9600 + i, step=w + 3, uv=h * (w + 3) + 1) for i in range(4)]
    f = F3

    def build(wrap, out, fp32_reference=False):
        mats = [wrap(surfs[i % 4]).yuv444_roi(i % 5, i % 7, w - 10 - (i % 3), h - 8) for i in range(n)]
        rd = cvgs.read_yuv444(mats, dst, capi.YUV_LIMITED, capi.BT709, False)
        mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f)
        if target == "fp32" or fp32_reference:
            return [rd] + mid + [cvgs.split(f, out, dst)]
        return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, dst)]

    if target == "bf16":
        run_both(oracle, build, surfs, (n, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_16BFC1, FAMILY + "_swap_mul_sub_div_bf16", bf16=True)
    else:
        run_both(oracle, build, surfs, (n, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1, FAMILY + "_swap_mul_sub_div")


def crops_4k(n, seed):
    """n crops of a 3840 x 2160 surface: odd and even origins, widths and heights."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        w, h = int(rng.randint(40, 400)), int(rng.randint(60, 500))
        out.append((int(rng.randint(0, 3840 - w)), int(rng.randint(0, 2160 - h)), w, h))
    return out


def test_fifty_crops_of_a_4k_surface(oracle):
    """The one case at the size of the flagship workload: 50 crops of a 4K surface -> [50, 3, 128, 64] (four rows per wave, the LDS tile)."""
    surf = Y.Surf(3840, 2160, 9700)
    crops, dst, f = crops_4k(50, 11), (64, 128), F3
    assert any(c[0] & 1 for c in crops) and any(c[1] & 1 for c in crops) and any(c[2] & 1 for c in crops)

    def build(wrap, out):
        m = wrap(surf)
        rd = cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, capi.YUV_LIMITED, capi.BT709, False)
        return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]), cvgs.split(f, out, dst)]

    run_both(oracle, build, [surf], (50, 3 * dst[0] * dst[1]), np.float32, cvgs.CV_32FC1, FAMILY + "_swap_mul_sub_div")


# ---- per-pixel reads (CVGS_READ_NV12 without a resize): the pointwise source kind ------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 1), (5, 3), (67, 5), (256, 4)])
@pytest.mark.parametrize("target", ["planar_f32", "planar_norm", "planar_f16", "planar_bf16", "packed_f32", "packed_f16", "packed_u8", "alpha_packed"])
def test_pointwise_targets(oracle, size, target):
    w, h = size
    surf = padded(w, h, 10000 + w)
    alpha = target == "alpha_packed"
    cn = 4 if alpha else 3
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)

    def build(wrap, out, fp32_reference=False):
        rd = cvgs.read_yuv444(view_of(wrap, surf, w, h), None, capi.YUV_LIMITED, capi.BT709, alpha)
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
        return [rd, cvgs.convertTo(f, U3, 1.2, -10.0), cvgs.write(U3, out)]

    planar = target.startswith("planar")
    shp = (1, 3 * w * h) if planar else (h, w, cn)
    if target == "planar_bf16":
        run_both(oracle, build, [surf], shp, np.float32, cvgs.CV_16BFC1, "pointwise4_yuv444_bf16", bf16=True)
        return
    dt = np.float16 if target.endswith("f16") else (np.uint8 if target == "packed_u8" else np.float32)
    ot = {"planar_f32": cvgs.CV_32FC1, "planar_norm": cvgs.CV_32FC1, "planar_f16": cvgs.CV_16FC1, "packed_f32": F3, "packed_f16": cvgs.CV_16FC3,
          "packed_u8": U3, "alpha_packed": cvgs.CV_32FC4}[target]
    want = "pointwise4_yuv444" + ("_f16" if target.endswith("f16") else ("_u8" if target == "packed_u8" else ""))
    _, name = run_both(oracle, build, [surf], shp, dt, ot, want)
    assert name == want


@pytest.mark.parametrize("size", [(67, 5), (130, 37)])
def test_pointwise_batch_with_default_planes(oracle, size):
    w, h = size
    n = 4
    surfs = [Y.Surf(w + 3, h + 4, 10100 + i, step=w + 6, uv=(h + 4) * (w + 6) + 3) for i in range(2)]
    f = F3

    def build(wrap, out):
        mats = [wrap(surfs[i % 2]).yuv444_roi(1 + (i & 1), i, w, h) for i in range(n)]
        rd = cvgs.read_yuv444(mats, None, capi.YUV_FULL, capi.BT601, False)
        rd.used_planes = 3
        rd.background = cvgs._scalar([3.0, -4.0, 17.5])
        return [rd] + NORM(f) + [cvgs.split(f, out, (w, h))]

    run_both(oracle, build, surfs, (n, 3 * w * h), np.float32, cvgs.CV_32FC1, "pointwise4_yuv444")


# ---- no byte outside the contract influences the result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [(1, 1), (2, 1), (1, 5), (3, 9), (65, 3), (67, 5)])
def test_bytes_outside_the_planes_do_not_influence_the_result(src):
    """Row padding, the gaps between the planes and a guard band around the surface are filled with a pattern, then with its
    complement: every output -- fast resize, interpreted resize, per-pixel read -- must be identical bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    w, h = src
    surf = Y.Surf(w, h, 10200 + w, step=w + 5, uv=h * (w + 5) + 9, guard=256, lead=1)
    pattern = H.random_u8((surf.buf.size,), 10250)
    f = F3
    results = []
    for fill in (pattern, 255 - pattern):
        surf.fill_rest(fill)
        assert (surf.buf[:256] == fill[:256]).all() and (surf.buf[-256:] == fill[-256:]).all()
        wrap, held = Y.tensor_wrapper([surf], dev)
        outs = []
        for dst in TARGETS + [None]:
            ow, oh = dst if dst else (w, h)
            for flags in (0, capi.CHAIN_FORCE_GENERIC):
                gt = torch.zeros((1, 3 * ow * oh), dtype=torch.float32, device=dev)
                ops = [cvgs.read_yuv444(wrap(surf), dst, capi.YUV_LIMITED, capi.BT709, False)] + NORM(f) + [cvgs.split(f, cvgs.GpuMat.from_tensor(gt, cvgs.CV_32FC1), (ow, oh))]
                cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
                torch.cuda.synchronize()
                outs.append(gt.cpu().numpy())
        results.append(outs)
        del held
    for a, b in zip(*results):
        assert a.any()
        H.assert_bit_exact(a, b, "pattern vs complement outside the planes")


# ---- 4:4:4 with 2 x 2-replicated chroma == the NV12 picture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", [(50, 30), (200, 150), None])
def test_replicated_chroma_equals_the_nv12_picture(oracle, dst):
    """The oracle's DIRECT NV12 answer is the reference here."""
    import torch
    dev = torch.device("cuda:0")
    w, h = 96, 64
    nv = H.random_u8((h * 3 // 2, w), 10300)
    rep = lambda c: np.ascontiguousarray(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1))
    surf = Y.Surf(w, h, 0, planes=(np.ascontiguousarray(nv[:h]), rep(nv[h:, 0::2]), rep(nv[h:, 1::2])))
    f = F3
    ow, oh = dst if dst else (w, h)
    prog = lambda: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f)
    ref = np.zeros((1, 3 * ow * oh), np.float32)
    luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, nv.ctypes.data, nv.strides[0], owner=nv)
    oracle.execute(cvgs.lower([cvgs.read_nv12(luma, dst, capi.YUV_LIMITED, capi.BT709, False)] + prog() + [cvgs.split(f, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (ow, oh))]))
    wrap, held = Y.tensor_wrapper([surf], dev)
    gt = torch.zeros(ref.shape, dtype=torch.float32, device=dev)
    ops = [cvgs.read_yuv444(wrap(surf), dst, capi.YUV_LIMITED, capi.BT709, False)] + prog() + [cvgs.split(f, cvgs.GpuMat.from_tensor(gt, cvgs.CV_32FC1), (ow, oh))]
    assert cvgs.kernel_name(*ops) == (FAMILY + "_swap_mul_sub_div" if dst else "pointwise4_yuv444")
    cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    H.assert_bit_exact(gt.cpu().numpy(), ref, "4:4:4 with replicated chroma vs the NV12 picture")


def test_from_yuv444_tensor_on_the_device(oracle):
    """A [3, H, W] device tensor (a view with strides: step = stride(1), uv_offset = stride(0)) read through GpuMat.from_yuv444_tensor."""
    import torch
    dev = torch.device("cuda:0")
    w, h, dst = 67, 21, (65, 9)
    planes = tuple(H.random_u8((h, w), 10350 + k) for k in range(3))
    big = torch.zeros((3, h + 3, w + 6), dtype=torch.uint8, device=dev)
    t = big[:, 2:2 + h, 5:5 + w]
    t.copy_(torch.from_numpy(np.stack(planes)).to(dev))
    surf = Y.Surf(w, h, 0, planes=planes)
    f = F3
    ref = np.zeros((1, 3 * dst[0] * dst[1]), np.float32)
    Y.Expect(oracle, [surf]).run([cvgs.read_yuv444(Y.wrap_array(surf), dst, capi.YUV_FULL, capi.BT709, False)] + NORM(f) + [cvgs.split(f, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), dst)])
    gt = torch.zeros(ref.shape, dtype=torch.float32, device=dev)
    m = cvgs.GpuMat.from_yuv444_tensor(t)
    assert (m.step, m.uv_offset) == (w + 6, (h + 3) * (w + 6))
    cvgs.executeOperations(torch.cuda.current_stream(), *([cvgs.read_yuv444(m, dst, capi.YUV_FULL, capi.BT709, False)] + NORM(f) + [cvgs.split(f, cvgs.GpuMat.from_tensor(gt, cvgs.CV_32FC1), dst)]))
    torch.cuda.synchronize()
    H.assert_bit_exact(gt.cpu().numpy(), ref, "from_yuv444_tensor")


# ---- ticks: cvgs_execute_many ------------------------------------------------------------------------------------------------------------
def _tick(n_cams, n_crops, dst, seed, dev, target="fp32", surf_size=(640, 360)):
    import torch
    w, h = surf_size
    f = F3
    rng = np.random.RandomState(seed)
    surfs = [Y.Surf(w, h, seed + 10 * i, step=w + 1, uv=h * (w + 1) + 3) for i in range(n_cams)]
    wrap, held = Y.tensor_wrapper(surfs, dev)
    crops = []
    for _ in range(n_crops):
        cw, ch = int(rng.randint(1, 300)), int(rng.randint(1, 300))
        crops.append((int(rng.randint(0, w - cw)), int(rng.randint(0, h - ch)), cw, ch))
    tdt = {"fp32": torch.float32, "bf16": torch.bfloat16}[target]

    def chain(wr, cam, out, fp32_reference=False):
        m = wr(surfs[cam])
        rd = cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, capi.YUV_LIMITED, capi.BT709, False)
        mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])]
        if target == "fp32" or fp32_reference:
            return [rd] + mid + [cvgs.split(f, out, dst)]
        return [rd] + mid + [cvgs.convertTo(f, cvgs.CV_16BFC3), cvgs.split(cvgs.CV_16BFC3, out, dst)]

    outs = [torch.full((n_crops, 3 * dst[0] * dst[1]), -3.0, dtype=tdt, device=dev) for _ in range(n_cams)]
    ot = cvgs.CV_32FC1 if target == "fp32" else cvgs.CV_16BFC1
    chains = [chain(wrap, cam, cvgs.GpuMat.from_tensor(outs[cam], ot)) for cam in range(n_cams)]
    return surfs, (wrap, held), crops, chain, outs, chains


@pytest.mark.parametrize("n_cams,n_crops,target", [(2, 5, "fp32"), (16, 50, "fp32"), (16, 50, "bf16")])
def test_tick_in_one_graph_node(oracle, n_cams, n_crops, target):
    """2-16 surfaces' crop chains (host descriptors; the inline argument blocks) as ONE cvgs_execute_many launch: captured into a graph
    with exactly one kernel node, equal to the one-by-one result and to the composed oracle value."""
    import torch
    dev = torch.device("cuda:0")
    dst = (64, 128)
    surfs, _held, crops, chain, outs, chains = _tick(n_cams, n_crops, dst, 10400, dev, target)
    get = lambda t: t.float().cpu().numpy()
    one_by_one = []
    for ops in chains:
        cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    for cam in range(n_cams):
        one_by_one.append(get(outs[cam]))
        outs[cam].fill_(-3.0)
    exp = Y.Expect(oracle, surfs)
    for cam in (0, n_cams - 1):
        ref = np.zeros((n_crops, 3 * dst[0] * dst[1]), np.float32)
        exp.run(chain(Y.wrap_array, cam, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), True))
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


def test_aliased_tick_falls_back_to_sequential_launches(oracle):
    """Two chains that write the SAME tensor are not independent: the tick keeps the sequential meaning (the second chain's values win)."""
    import torch
    dev = torch.device("cuda:0")
    dst = (64, 128)
    surfs, (wrap, _held), crops, chain, outs, chains = _tick(2, 6, dst, 10500, dev)
    aliased = [chains[0], chain(wrap, 1, cvgs.GpuMat.from_tensor(outs[0], cvgs.CV_32FC1))]
    from tests.test_gpu_many import _captured_kernel_nodes
    lowered = [cvgs.lower(c) for c in aliased]  # (kept alive: the packed descriptors borrow their host arrays)
    assert _captured_kernel_nodes(capi.load_library(), cvgs.pack_chains(lowered), 2, None) == 2, "sequential launches"
    for o in outs:
        o.fill_(-3.0)
    held = cvgs.executeMany(torch.cuda.current_stream(), aliased)
    torch.cuda.synchronize()
    ref = np.zeros((6, 3 * dst[0] * dst[1]), np.float32)
    Y.Expect(oracle, surfs).run(chain(Y.wrap_array, 1, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1)))
    H.assert_bit_exact(outs[0].cpu().numpy(), ref, "aliased pair: the second chain's values")
    assert (outs[1].cpu().numpy() == -3.0).all()
    del held


def test_a_target_inside_another_chains_v_plane_is_not_fused(oracle):
    """Chain B's tensor lies inside chain A's V plane -- behind everything A's Y rows span: fused, B would overwrite samples A is still
    reading.  The tick must run as two launches, in order, and A's result is the one of the untouched surface."""
    import torch
    dev = torch.device("cuda:0")
    w, h, dst, f = 64, 48, (8, 4), F3
    sa, sb = Y.Surf(w, h, 10600), Y.Surf(w, h, 10610)
    wrap, held = Y.tensor_wrapper([sa, sb], dev)
    crops = [(1, 1, 30, 20), (33, 27, 31, 21)]
    n_out = 2 * 3 * dst[0] * dst[1]
    v_plane = sa.origin + 2 * sa.uv
    first = (v_plane + 4 * sa.step + 3) // 4 * 4  # a 4-byte aligned position inside the V plane
    assert first + 4 * n_out <= sa.buf.size and first >= sa.origin + (h - 1) * sa.step + w
    out_b = held[id(sa)][first:first + 4 * n_out].view(torch.float32).view(2, -1)
    out_a = torch.full((2, 3 * dst[0] * dst[1]), -3.0, dtype=torch.float32, device=dev)

    def chain(wr, s, out):
        m = wr(s)
        return [cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, capi.YUV_LIMITED, capi.BT709, False), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f)] + NORM(f) + [cvgs.split(f, out, dst)]

    chains = [chain(wrap, sa, cvgs.GpuMat.from_tensor(out_a, cvgs.CV_32FC1)), chain(wrap, sb, cvgs.GpuMat.from_tensor(out_b, cvgs.CV_32FC1))]
    from tests.test_gpu_many import _captured_kernel_nodes
    lowered = [cvgs.lower(c) for c in chains]
    assert _captured_kernel_nodes(capi.load_library(), cvgs.pack_chains(lowered), 2, None) == 2, "sequential launches"
    # (the captured graph was never launched: the surface is untouched)
    held_chains = cvgs.executeMany(torch.cuda.current_stream(), chains)
    torch.cuda.synchronize()
    ref = np.zeros((2, 3 * dst[0] * dst[1]), np.float32)
    exp = Y.Expect(oracle, [sa, sb])
    exp.run(chain(Y.wrap_array, sa, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1)))
    H.assert_bit_exact(out_a.cpu().numpy(), ref, "chain A read its V plane before chain B wrote into it")
    exp.run(chain(Y.wrap_array, sb, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1)))
    H.assert_bit_exact(out_b.cpu().numpy(), ref, "chain B")
    del held_chains


# ---- CircularTensor push -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("order", [cvgs.NewestFirst, cvgs.OldestFirst])
def test_circular_tensor_push(oracle, resize, order):
    """Frames pushed into a CircularTensor through the 4:4:4 read (per-pixel and resized): the whole tensor after every update."""
    import torch
    from tests.test_gpu_circular_nv12 import _read_device
    dev = torch.device("cuda:0")
    w, h = 67, 33
    dst = (32, 16) if resize else None
    ow, oh = dst if resize else (w, h)
    f, batch = F3, 3
    ct = cvgs.CircularTensor(cvgs.CV_8UC1, cvgs.CV_32FC1, 3, batch, order, cvgs.Standard, ow, oh)
    history = []
    for k in range(5):
        surf = Y.Surf(w, h, 10700 + k, step=w + 2, uv=h * (w + 2) + 1)
        wrap, held = Y.tensor_wrapper([surf], dev)
        ops = lambda m: [cvgs.read_yuv444(m, dst, capi.YUV_LIMITED, capi.BT709, False), cvgs.multiply(f, [0.5, 0.25, 2.0])]
        ct.update(torch.cuda.current_stream(), *(ops(wrap(surf)) + [ct.write_split(f)]))
        torch.cuda.synchronize()
        ref = np.zeros((1, 3 * ow * oh), np.float32)
        Y.Expect(oracle, [surf]).run(ops(Y.wrap_array(surf)) + [cvgs.split(f, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (ow, oh))])
        history.insert(0, ref.reshape(-1))  # newest first
        got = _read_device(ct.data(), ct.nbytes()).view(np.float32).reshape(batch, -1)
        for age, r in enumerate(history[:batch]):
            slot = age if order == cvgs.NewestFirst else batch - 1 - age
            H.assert_bit_exact(got[slot], r, "update %d, age %d" % (k, age))
        del held
    ct.release()


# ---- seeded differential fuzz: fast kernels vs the interpreted kernel vs the composed oracle -------------------------------------------------
@pytest.mark.parametrize("seed", range(32))
def test_differential_fuzz(oracle, seed):
    rng = np.random.RandomState(4440 + seed)
    sw, sh = int(rng.randint(1, 200)), int(rng.randint(1, 120))
    step = sw + int(rng.randint(0, 9))
    surf = Y.Surf(sw, sh, 10800 + seed, step=step, uv=(sh - 1) * step + sw + int(rng.randint(0, 70)), lead=int(rng.randint(0, 4)))
    n = int(rng.randint(1, 9))
    crops = []
    for _ in range(n):
        cw, ch = int(rng.randint(1, sw + 1)), int(rng.randint(1, sh + 1))
        crops.append((int(rng.randint(0, sw - cw + 1)), int(rng.randint(0, sh - ch + 1)), cw, ch))
    resize = bool(rng.randint(0, 4))
    if not resize:
        crops = [(c[0], c[1], crops[0][2], crops[0][3]) for c in crops if c[0] + crops[0][2] <= sw and c[1] + crops[0][3] <= sh] or [crops[0]]
        n = len(crops)
    dst = (int(rng.randint(1, 150)), int(rng.randint(1, 60))) if resize else None
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
        m = wrap(surf)
        rd = cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, range_, prim, alpha)
        rd.ar, rd.used_planes = ar, used
        rd.background = cvgs._scalar([114.0, 100.5, 7.25, 30.0][:cn] + [0.0] * (4 - cn))
        return [rd] + prog + [cvgs.write(f, out, (ow, oh)) if packed else cvgs.split(f, out, (ow, oh))]

    shp = (n, ow * oh, cn) if packed else (n, cn * ow * oh)
    ot = f if packed else cvgs.CV_32FC1
    run_both(oracle, build, [surf], shp, np.float32, ot, FAMILY if resize else "pointwise4_yuv444")


def test_cpp_facade_program_passes():
    """cvGS::cvtColorYUV444 with crops -> resize -> normalize -> split (tests/cpp/test_yuv444.cpp)."""
    import os
    import subprocess
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "test_yuv444")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", cpp, "bin/test_yuv444"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- the descriptor queue does not take the layout ----------------------------------------------------------------------------------------
def test_descriptor_queue_refuses_the_layout():
    """A 4:4:4 chain of the shape the queue serves for NV12 crops is refused (CVGS_ERR_UNSUPPORTED, the text it uses for 4:2:2) and
    nothing runs: the queue's worker must never read a planar 4:4:4 surface as NV12."""
    import torch
    dev = torch.device("cuda:0")
    surf = Y.Surf(640, 360, 11400)
    wrap, held = Y.tensor_wrapper([surf], dev)
    dst, f = (64, 128), F3
    out = torch.full((4, 3 * dst[0] * dst[1]), -3.0, dtype=torch.float32, device=dev)
    crops = [(0, 0, 640, 360), (10, 20, 100, 200), (300, 100, 64, 128), (2, 2, 64, 64)]
    m = wrap(surf)
    ops = [cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops], dst, capi.YUV_FULL, capi.BT601, False),
           cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
           cvgs.split(f, cvgs.GpuMat.from_tensor(out, cvgs.CV_32FC1), dst)]
    q = cvgs.Queue()
    try:
        with pytest.raises(capi.CvgsError) as e:
            q.submit(*ops)
        assert e.value.code == capi.ERR_UNSUPPORTED and "not a chain the server takes" in str(e.value)
        with pytest.raises(capi.CvgsError) as e:
            q.submit_on(torch.cuda.current_stream(), *ops)
        assert e.value.code == capi.ERR_UNSUPPORTED
    finally:
        q.destroy()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -3.0).all()
