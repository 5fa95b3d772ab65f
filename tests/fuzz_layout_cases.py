"""The generator of the layout fuzzer (tests/test_gpu_fuzz_layouts.py): seeded random VALID chains over what tests/test_gpu_fuzz._case never
draws -- packed 4:2:2 reads (YUYV / UYVY), planar 4:4:4 reads (I444), CV_16BF as the stored type and CV_16BF as the source type.  A seed space
of its own: tests/test_gpu_fuzz._case and the meaning of its seeds are untouched; only its pointwise programs (_program, which takes the
rng) are shared.  Nothing here needs torch or a GPU: tests/test_fuzz_layout_cases.py pins the generator on the CPU.

case(seed, big=False) -> Case.  Case.build(wrap_surface, wrap_out, out, bf) -> iops, after tests/test_gpu_fuzz._case and
tests/test_gpu_bf16._run:
  wrap_surface(src) -> the GpuMat of the WHOLE source `src` (one of Case.sources) in the caller's memory: src.mat(base, owner, bf) over a copy
                       of src.host(bf);
  wrap_out(out, cv_type) -> the GpuMat of the output array;
  bf = True: the chain itself (CV_16BF types, outputs held as uint16); bf = False: its fp32 TWIN for the CPU oracle, which knows no bf16 -- a
  CV_16BF source widened exactly, the final conversion to CV_16BF left out (the caller rounds with rne_bf16).
Case.expected(oracle) is the exact expected output: the oracle's answer, composed from two oracle runs for 4:2:2 / 4:4:4 reads
(tests/yuv422_cases.Expect, tests/yuv444_cases.Expect), rounded to bf16 on the host for a CV_16BF store.

Classes the product refuses by design are not drawn (every drawn chain must be served, a refusal is a failure):
  * device plane tables for the layouts drawn here: "device plane tables serve the NV12 / NV21 layouts only (P010 / I420 / YV12 / YUYV / UYVY /
    I444: host descriptors)";
  * crops of I420 / YV12 surfaces: "crops of planar-chroma (I420 / YV12) surfaces";
  * 4:2:2 views at an odd x or off a 4-byte boundary: "YUYV / UYVY surfaces need data and step that are multiples of 4";
  * arithmetic and GRAY on CV_16BF values: "arithmetic stages on CV_16BF (bf16) values (convertTo CV_32F first)" -- a bf16 source read per
    pixel is converted to CV_32F before the program."""
from math import gcd

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import yuv422_cases as Y422
from tests import yuv444_cases as Y444
from tests.test_bf16_types import rne_bf16, special_values, widen_bf16
from tests.test_gpu_chains import _random_src
from tests.test_gpu_fuzz import NAME, NP, _program

EDGE_W = [1, 2, 63, 64, 65, 127, 128, 129]  # the 64-column tile
EDGE_H = [1, 3, 4, 5]                       # the rows-per-wave groups
BIG_W = [255, 256, 257, 639, 640, 641, 1279, 1280]
WRITE_KINDS = ["write3d", "write2d_batch", "write2d", "split", "splitT", "split2d"]
FAMILIES = {1: "yuv422", 2: "yuv444", 3: "bf16_store", 4: "bf16_source"}
BF16 = capi.DEPTH_16BF
DEFAULT_N, DEFAULT_BIG_N, BIG_BASE = 480, 24, 500_000  # the default seed ranges of tests/test_gpu_fuzz_layouts.py; big seeds: BIG_BASE + i
FLAGS = [0, capi.CHAIN_FORCE_GENERIC, 0, capi.CHAIN_NO_THREAD_FUSION]  # by seed % 4
GUARD_SRC = 64  # bytes of guard band on both sides of a 4:2:2 / 4:4:4 source buffer (filled like the padding)


def bf16_type(cn):
    return cvgs.make_type(capi.DEPTH_16F, cn) | capi.TYPE_FLAG_BF16


class PlainSrc:
    """An image (h, w, cn) or a 4:2:0 surface (rows * 3 / 2, w); CV_16BF images are uint16 bit patterns."""
    kind = "plain"

    def __init__(self, arr, cv_type, luma_rows=None):
        self.arr, self.cv_type, self.luma_rows = np.ascontiguousarray(arr), cv_type, luma_rows

    def is_bf16(self):
        return capi.type_is_bf16(self.cv_type)

    def host(self, bf):
        return self.arr if (bf or not self.is_bf16()) else np.ascontiguousarray(widen_bf16(self.arr))

    def type(self, bf):
        return self.cv_type if (bf or not self.is_bf16()) else cvgs.make_type(cvgs.CV_32F, capi.type_cn(self.cv_type))

    def mat(self, base, owner, bf):
        a = self.host(bf)
        return cvgs.GpuMat(self.luma_rows or a.shape[0], a.shape[1], self.type(bf), base, a.strides[0], owner=owner)


class Surf422:
    """A w x h picture (w even) as packed pixel pairs inside ONE byte buffer:  guard | lead | rows, step apart | guard.  step >= 2 w and
    lead are multiples of 4 (validation asks for 4-byte aligned data and step, nothing more).  `s` is the (h, step / 2, 2) view of the
    rows, padding included, that tests/yuv422_cases.Expect reads."""
    kind = "yuv422"

    def __init__(self, w, h, seed, layout, step=None, lead=0, guard=GUARD_SRC):
        self.w, self.h, self.layout = int(w), int(h), layout
        self.step = int(step) if step is not None else 2 * self.w
        assert self.w % 2 == 0 and self.step % 4 == 0 and self.step >= 2 * self.w and lead % 4 == 0 and guard % 4 == 0
        self.origin = int(guard) + int(lead)
        self.buf = np.zeros(self.origin + self.h * self.step + int(guard), np.uint8)
        self.s = np.ndarray((self.h, self.step // 2, 2), np.uint8, buffer=self.buf, offset=self.origin, strides=(self.step, 2, 1))
        self.s[:, :self.w] = Y422.random_surface(self.w, self.h, seed, layout)
        self.sample_index = (self.origin + np.arange(self.h)[:, None] * self.step + np.arange(2 * self.w)[None, :]).reshape(-1)

    def fill_rest(self, pattern):
        keep = self.buf[self.sample_index].copy()
        self.buf[:] = pattern
        self.buf[self.sample_index] = keep

    def host(self, bf):
        return self.buf

    def mat(self, base, owner, bf):
        return cvgs.GpuMat(self.h, self.w, Y422.CV_8UC2, base + self.origin, self.step, owner=owner)


class Surf444(Y444.Surf):
    kind = "yuv444"

    def host(self, bf):
        return self.buf

    def mat(self, base, owner, bf=True):
        return Y444.Surf.mat(self, base, owner)


def host_wrap(bf):
    """wrap_surface over the sources' own host memory (the oracle's side; the composed-oracle helpers find their surfaces by address)."""
    def wrap(src):
        a = src.host(bf)
        return src.mat(a.ctypes.data, a, bf)
    return wrap


def rest_pattern(n, k):
    """The k-th fill of the bytes that are no sample (padding, gaps between planes, guards): never constant, different for every k."""
    return ((np.arange(n, dtype=np.int64) * (37 + 12 * k) + 11 + 90 * k) % 251 + 3 * k).astype(np.uint8)


def bf16_image(shape, rng):
    """CV_16BF bit patterns: random finite data with the classes of test_bf16_types.special_values scattered through it -- +-0, +-inf, NaN,
    subnormals, the largest and the smallest normal values (half of the scattered ones), any bf16 pattern at all (the other half)."""
    f = ((rng.integers(0, 65536, shape).astype(np.float32) - 32768.0) / np.float32(37.0)).astype(np.float32)
    a = rne_bf16(f).reshape(shape)
    classes = np.unique(rne_bf16(special_values()[-18:]))
    classes = np.concatenate([classes, np.array([0x0001, 0x007F, 0x8001, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x7FC0], np.uint16)])
    hit = rng.random(shape) < 0.03
    pick = np.where(rng.random(shape) < 0.5, classes[rng.integers(0, len(classes), shape)], rng.integers(0, 65536, shape).astype(np.uint16))
    return np.where(hit, pick, a).astype(np.uint16)


def _pick(rng, edges, hi, p=0.7):
    return int(edges[int(rng.integers(0, len(edges)))]) if rng.random() < p else int(rng.integers(1, hi + 1))


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def out_array(self, bf):
        """the zeroed output array of the chain (bf = True) or of its twin"""
        return np.zeros(self.shape, self.np_dtype if (bf or not self.bf16_store) else np.float32)

    def lowered(self, bf=True):
        """(ops, keep) of the chain over host memory"""
        out = self.out_array(bf)
        return self.build(host_wrap(bf), lambda a, t: cvgs.GpuMat.from_array(a, t), out, bf), out

    def logical(self, arr):
        """an output array (or its twin's) as [plane][y][x][c], pitch padding dropped"""
        n, (dw, dh), fc, wk = self.n, self.dsize, self.out_cn, self.write_kind
        if wk == "write3d":
            return arr.reshape(n, dh, dw, fc)
        if wk == "write2d":
            return arr[:, :dw].reshape(1, dh, dw, fc)
        if wk == "write2d_batch":
            return arr.reshape(n, dh, -1, fc)[:, :, :dw]
        if wk == "split":
            return arr.reshape(n, fc, dh, dw).transpose(0, 2, 3, 1)
        if wk == "splitT":
            return arr.reshape(fc, n, dh, dw).transpose(1, 2, 3, 0)
        return arr.reshape(n, fc, dh, -1)[..., :dw].transpose(0, 2, 3, 1)

    def expected(self, oracle):
        """The exact expected output, in the GPU output's dtype (CV_16BF: uint16 bit patterns).  case() keeps it in Case.ref."""
        ops, out = self.lowered(bf=False)
        with np.errstate(all="ignore"):
            if self.read == "yuv422":
                Y422.Expect(oracle, [s.s for s in self.sources], self.layout).run(ops)
            elif self.read == "yuv444":
                Y444.Expect(oracle, self.sources).run(ops)
            else:
                oracle.execute(cvgs.lower(ops))
        return rne_bf16(out).reshape(out.shape) if self.bf16_store else out


def case(seed, big=False):
    """The case of a seed.  A draw whose expected output is all zero says nothing (a product by 0, a saturated cast of negative values, a warp
    that misses its source): the seed's next draw is taken instead, so that every case's expected value -- computed once, here, and kept in
    Case.ref -- is non-trivial."""
    from oracle import oracle_binding
    oracle_binding.load_oracle()
    for attempt in range(16):
        c = _draw(seed, big, attempt)
        c.ref = c.expected(oracle_binding)
        if c.ref.any():
            return c
    raise AssertionError("seed %d: sixteen draws in a row with an all-zero expected value" % seed)


def _short_program(rng, cn):
    """The short arithmetic programs the fast families specialise ([swap] x - / and the like), on a CV_32F value: what brings the bf16 twins
    of K1, K4 and the fast warp into the fuzzed set (a program of _program's seldom has such a shape)."""
    f = cvgs.make_type(cvgs.CV_32F, cn)
    ops = []
    if cn >= 3 and rng.integers(0, 2):
        ops.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f))
    vals = lambda: [float(np.float32(v)) for v in rng.uniform(0.3, 3.0, cn)]  # noqa: E731
    shape = int(rng.integers(0, 4))
    if shape == 1:
        ops += [cvgs.multiply(f, vals()), cvgs.subtract(f, vals()), cvgs.divide(f, vals())]
    elif shape == 2:
        ops += [cvgs.multiply(f, vals()), cvgs.add(f, vals())]
    elif shape == 3:
        ops += [cvgs.subtract(f, vals()), cvgs.divide(f, vals())]
    return ops, cvgs.CV_32F, cn


def _draw(seed, big, attempt):
    rng = np.random.default_rng([int(seed), 0x4C41, attempt])  # (not the stream of test_gpu_fuzz._case for the same seed)
    k = 8 if big else 1
    fam = int(rng.integers(1, 5))
    if fam == 1:
        read = "yuv422"
    elif fam == 2:
        read = "yuv444"
    elif fam == 3:  # any read kind tests/test_gpu_fuzz._case draws, and the two above
        read = ["pixel", "resize", "resize", "warp", "yuv420", "yuv422", "yuv444"][int(rng.integers(0, 7))]
    else:
        read = ["pixel", "resize", "warp"][int(rng.integers(0, 3))]
    yuv = read.startswith("yuv")
    n = int(rng.integers(1, 4 if big else 6))
    used = n if rng.integers(0, 3) else int(rng.integers(0, n + 1))
    resize = bool(rng.integers(0, 2)) if yuv else read == "resize"
    if big:
        dw, dh = _pick(rng, BIG_W, 1280, 0.5), int(rng.integers(90, 721))
    else:
        dw, dh = _pick(rng, EDGE_W, 200), _pick(rng, EDGE_H, 150, 0.5)
    color = (int(rng.integers(0, 2)), int(rng.integers(0, 3)), bool(rng.integers(0, 2)))  # range, primaries, alpha
    ar = [cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_LEFT, cvgs.PRESERVE_AR_RN_EVEN][int(rng.integers(0, 4))]
    bg = [float(v) for v in rng.integers(1, 100, 4)]
    crop_mode = bool(rng.integers(0, 2))  # n crop views of ONE surface instead of n surfaces
    layout, views, sources, sdepth, scn, mats_persp, warp_sizes = None, None, [], cvgs.CV_8U, 1, None, None

    if read == "yuv422":
        layout = Y422.LAYOUTS[int(rng.integers(0, 2))]
        vw, vh = int(rng.integers(1, 300 * k if not big else 1921)), int(rng.integers(1, 60 * k if not big else 1081))

        def surf(w, h, i):  # w: the widest view; the surface holds whole pairs
            we = w + (w & 1)
            pad = 4 * int(rng.integers(0, 6)) if rng.integers(0, 2) else 0
            return Surf422(we, h, seed * 10 + 3 * i, layout, step=2 * we + pad, lead=4 * int(rng.integers(0, 4)))
        if crop_mode:
            s = surf(vw + 2 * int(rng.integers(0, 9)), vh + int(rng.integers(0, 9)), 0)
            sources, views = [s], []
            for _ in range(n):  # x and width on a pixel pair (the width's last pair is read whole when it is odd), any y, any height
                w, h = (vw, vh) if not resize else (int(rng.integers(1, vw + 1)), int(rng.integers(1, vh + 1)))
                views.append((0, 2 * int(rng.integers(0, (s.w - w) // 2 + 1)), int(rng.integers(0, s.h - h + 1)), w, h))
        else:
            sizes = [(vw, vh)] * n if not resize else [(vw, vh)] + [(int(rng.integers(1, vw + 1)), int(rng.integers(1, vh + 1))) for _ in range(n - 1)]
            sources = [surf(w, h, i) for i, (w, h) in enumerate(sizes)]
            views = [(i, 0, 0, w, h) for i, (w, h) in enumerate(sizes)]
    elif read == "yuv444":
        layout = Y444.I444
        small = [(1, 1), (2, int(rng.integers(1, 40))), (int(rng.integers(1, 40)), 1), (1, int(rng.integers(1, 40)))]
        if rng.integers(0, 4) == 0 and not big:
            vw, vh = small[int(rng.integers(0, 4))]
        else:
            vw, vh = int(rng.integers(1, 300 * k if not big else 1921)), int(rng.integers(1, 60 * k if not big else 1081))

        def surf(w, h, i):
            if rng.integers(0, 4):  # odd step and plane distance with no common factor; `lead` takes the data off every alignment
                step = (w + int(rng.integers(0, 10))) | 1
                uv = (h * step + int(rng.integers(0, 40))) | 1
                while gcd(step, uv) != 1:
                    uv += 2
            else:
                step, uv = w, h * w
            return Surf444(w, h, seed * 10 + 3 * i, step=step, uv=uv, guard=GUARD_SRC, lead=int(rng.integers(0, 4)))
        if crop_mode:
            s = surf(vw + int(rng.integers(0, 9)), vh + int(rng.integers(0, 9)), 0)
            sources, views = [s], []
            for _ in range(n):  # any origin and size, odd ones included
                w, h = (vw, vh) if not resize else (int(rng.integers(1, vw + 1)), int(rng.integers(1, vh + 1)))
                if resize and rng.integers(0, 5) == 0:
                    w, h = small[int(rng.integers(0, 4))]
                    w, h = min(w, vw), min(h, vh)
                views.append((0, int(rng.integers(0, s.w - w + 1)), int(rng.integers(0, s.h - h + 1)), w, h))
        else:
            sizes = [(vw, vh)] * n if not resize else [(vw, vh)] + [(int(rng.integers(1, vw + 1)), int(rng.integers(1, vh + 1))) for _ in range(n - 1)]
            sources = [surf(w, h, i) for i, (w, h) in enumerate(sizes)]
            views = [(i, 0, 0, w, h) for i, (w, h) in enumerate(sizes)]
    elif read == "yuv420":
        layout = int(rng.integers(0, 5))  # NV12 / NV21 / I420 / YV12 / P010
        sdepth = cvgs.CV_16U if layout == capi.YUV_P010 else cvgs.CV_8U
        sw, sh = 2 * int(rng.integers(2, 60 * k)), 2 * int(rng.integers(2, 40 * k))
        interleaved = layout in (capi.YUV_NV12, capi.YUV_NV21, capi.YUV_P010)
        crop_mode = crop_mode and resize and interleaved and n > 1  # (planar chroma cannot be cropped: see the module's docstring)
        st = cvgs.make_type(sdepth, 1)
        mk = H.random_u16 if sdepth == cvgs.CV_16U else H.random_u8
        sources = [PlainSrc(mk((sh + sh // 2, sw, 1), seed * 10 + i)[:, :, 0], st, luma_rows=sh) for i in range(1 if crop_mode else n)]
        if crop_mode:
            views = []
            for _ in range(n):
                cw, ch = 2 * int(rng.integers(1, sw // 2 + 1)), 2 * int(rng.integers(1, sh // 2 + 1))
                views.append((0, 2 * int(rng.integers(0, (sw - cw) // 2 + 1)), 2 * int(rng.integers(0, (sh - ch) // 2 + 1)), cw, ch))
        else:
            views = [(i, 0, 0, sw, sh) for i in range(n)]
        vw, vh = sw, sh
        used = n  # (as tests/test_gpu_fuzz._case: whole 4:2:0 batches)
    else:
        if fam == 4:
            sdepth = BF16
        elif rng.integers(0, 3) == 0:  # (fam 3) the source types the fast families take
            sdepth = [cvgs.CV_8U, cvgs.CV_8U, cvgs.CV_16U, cvgs.CV_16S][int(rng.integers(0, 4))]
        else:
            pool = [cvgs.CV_8U, cvgs.CV_8U, cvgs.CV_8S, cvgs.CV_16U, cvgs.CV_16S, cvgs.CV_32S, cvgs.CV_32F, cvgs.CV_16F, cvgs.CV_16F if read == "warp" else cvgs.CV_64F]
            sdepth = pool[int(rng.integers(0, 7))] if rng.integers(0, 5) else pool[int(rng.integers(7, 9))]
        scn = int(rng.integers(1, 5)) if rng.integers(0, 3) else int(rng.integers(3, 5))
        vw, vh = int(rng.integers(1, 300 * k if not big else 1921)), int(rng.integers(1, 60 * k if not big else 1081))
        st = bf16_type(scn) if sdepth == BF16 else cvgs.make_type(sdepth, scn)
        for i in range(n):
            a = bf16_image((vh, vw, scn), rng) if sdepth == BF16 else _random_src((vh, vw, scn), NAME[sdepth], seed * 10 + i)
            sources.append(PlainSrc(a, st))
        views = [(i, 0, 0, vw, vh) for i in range(n)]
    if not resize and read != "warp":
        dw, dh = views[0][3], views[0][4]
        ar = cvgs.IGNORE_AR
    if read == "warp":
        ar = cvgs.IGNORE_AR
        persp = bool(rng.integers(0, 2))
        mats_persp = []
        for _ in range(n):
            m = np.eye(3)
            m[:2, :2] += rng.uniform(-0.4, 0.4, (2, 2))
            m[:2, :2] *= rng.uniform(0.3, 2.0) * max(dw, 1) / max(vw, 1)
            m[:2, 2] = np.array([dw / 2.0, dh / 2.0]) - m[:2, :2] @ np.array([vw / 2.0, vh / 2.0]) + rng.uniform(-4, 4, 2)  # centre -> about the centre
            if persp:
                m[2, :2] = rng.uniform(-0.002, 0.002, 2) / k
            mats_persp.append(m if persp else m[:2])
        used = max(used, 1)

    # ---- program and the stored type ----
    cn0 = (4 if color[2] else 3) if yuv else scn
    pre = []
    if resize or yuv or read == "warp":
        d0 = cvgs.CV_32F
    elif sdepth == BF16:  # a bf16 value takes no arithmetic: to fp32 first (exact)
        pre, d0 = [cvgs.convertTo(bf16_type(scn), cvgs.make_type(cvgs.CV_32F, scn))], cvgs.CV_32F
    else:
        d0 = sdepth
    out16 = None
    if fam == 3:
        out16 = BF16
    elif fam == 4:
        out16 = [None, cvgs.CV_16F, BF16][int(rng.integers(0, 3))]
    short = fam == 3 and d0 == cvgs.CV_32F and rng.integers(0, 3) == 0
    while True:
        prog, fd, fc = _short_program(rng, cn0) if short else _program(rng, d0, cn0)
        if fam in (3, 4) and fd != cvgs.CV_32F:  # the program ends in fp32
            prog = prog + [cvgs.convertTo(cvgs.make_type(fd, fc), cvgs.make_type(cvgs.CV_32F, fc))]
            fd = cvgs.CV_32F
        if len(pre) + sum(len(o.ops) for o in prog) + (out16 is not None) <= capi.MAX_OPS:  # (else: the next program of the same stream)
            break
    bf16_store = out16 == BF16
    if out16 == cvgs.CV_16F:
        prog = prog + [cvgs.convertTo(cvgs.make_type(cvgs.CV_32F, fc), cvgs.make_type(cvgs.CV_16F, fc))]
        fd = cvgs.CV_16F
    np_dt = np.uint16 if bf16_store else NP[fd]

    # ---- write kind (as tests/test_gpu_fuzz._case; a CV_16BF value goes to every kind: the interpreted kernels' store serves the ones no
    # fast family takes) ----
    wkinds = ["write3d", "write2d_batch"]
    if n == 1:
        wkinds.append("write2d")
    if fc >= 2:
        wkinds += ["split", "splitT", "split2d"]
    wk = wkinds[int(rng.integers(0, len(wkinds)))]
    pitch_pad = int(rng.integers(0, 4))
    if read == "warp" and wk in ("write2d_batch", "split2d") and n > 1 and rng.integers(0, 2):
        warp_sizes = [(int(rng.integers(1, dw + 1)), int(rng.integers(1, dh + 1))) for _ in range(n)]
    shape = {"write3d": (n, dw * dh, fc), "write2d": (dh, dw + pitch_pad, fc), "write2d_batch": (n * dh, dw + pitch_pad, fc),
             "split": (n, fc * dw * dh), "splitT": (fc * n, dw * dh), "split2d": (n * fc * dh, dw + pitch_pad)}[wk]

    def T(depth_or_none, cn, bf):
        """the stored type: CV_16BFCn for the chain, CV_32FCn for the twin"""
        if bf16_store:
            return bf16_type(cn) if bf else cvgs.make_type(cvgs.CV_32F, cn)
        return cvgs.make_type(fd, cn)

    def build(wrap_surface, wrap_out, out, bf):
        whole = [wrap_surface(s) for s in sources]
        if read == "yuv422":
            mats = [whole[i].yuv422_roi(x, y, w, h) for (i, x, y, w, h) in views]
        elif read == "yuv444":
            mats = [whole[i].yuv444_roi(x, y, w, h) for (i, x, y, w, h) in views]
        elif read == "yuv420":
            mats = [whole[i].nv12_roi(x, y, w, h) if crop_mode else whole[i] for (i, x, y, w, h) in views]
        else:
            mats = whole
        if yuv:
            rd = cvgs.read_nv12(mats if n > 1 else mats[0], (dw, dh) if resize else None, color[0], color[1], color[2], layout=layout)
            rd.used_planes, rd.background = used, cvgs._scalar(bg[:cn0])
            if resize:
                rd.ar = ar
        else:
            t = sources[0].type(bf)
            if read == "pixel":
                rd = cvgs.ReadIOp(capi.READ_PIXEL, t, mats, used, None, cvgs.IGNORE_AR, bg[:scn])
            elif read == "resize":
                rd = cvgs.resize(t, cvgs.INTER_LINEAR, mats, (dw, dh), used, bg[:scn], ar)
            else:
                rd = cvgs.warp(cvgs.WARP_PERSPECTIVE if mats_persp[0].shape[0] == 3 else cvgs.WARP_AFFINE, t, mats, [m.tolist() for m in mats_persp],
                               warp_sizes or (dw, dh), used, bg[:scn])
        stages = list(prog)
        if pre:  # the twin's source is fp32 already
            stages = (pre if bf else []) + stages
        if bf16_store and bf:
            stages = stages + [cvgs.convertTo(cvgs.make_type(cvgs.CV_32F, fc), bf16_type(fc))]
        ft = T(fd, fc, bf)
        o_t = T(fd, 1, bf) if wk in ("split", "splitT", "split2d") else ft
        o = wrap_out(out, o_t)
        if wk == "write3d":
            wr = cvgs.write(ft, o, (dw, dh))
        elif wk == "write2d":
            wr = cvgs.write(ft, o.roi(0, 0, dw, dh))
        elif wk == "write2d_batch":
            zs = warp_sizes or [(dw, dh)] * n  # smaller planes sit in the top-left corner of their dh x dw slot
            wr = cvgs.write_batch(ft, [cvgs.GpuMat(zs[i][1], zs[i][0], ft, o.data + i * dh * o.step, o.step, owner=o) for i in range(n)])
        elif wk == "split":
            wr = cvgs.split(ft, o, (dw, dh))
        elif wk == "splitT":
            wr = cvgs.splitT(ft, o.data, dw, dh, n, keep=o)
        else:
            zs = warp_sizes or [(dw, dh)] * n
            planes = [[cvgs.GpuMat(zs[z][1], zs[z][0], o_t, o.data + ((z * fc + c) * dh) * o.step, o.step, owner=o) for c in range(fc)] for z in range(n)]
            wr = cvgs.split(ft, planes if n > 1 else planes[0])
        return [rd] + stages + [wr]

    src_name = "16BF" if sdepth == BF16 else NAME[sdepth]
    what = "seed %d%s %s %s%s n=%d used=%d %sC%d %dx%d->%dx%d ar=%d ops=%d %s out=%s" % (
        seed, " big" if big else "", FAMILIES[fam], read + ("" if layout is None else ":%d" % layout), " crops" if (crop_mode and yuv) else "", n, used, src_name,
        scn, vw, vh, dw, dh, ar, sum(len(o.ops) for o in prog), wk, "bf16" if bf16_store else np.dtype(np_dt).name)
    return Case(seed=seed, family=fam, read=read, resize=resize, layout=layout, sources=sources, views=views, n=n, used=used, dsize=(dw, dh),
                write_kind=wk, shape=shape, np_dtype=np_dt, bf16_store=bf16_store, bf16_source=sdepth == BF16, out_depth=BF16 if bf16_store else fd,
                out_cn=fc, crop_mode=crop_mode, warp_sizes=warp_sizes, build=build, what=what)
