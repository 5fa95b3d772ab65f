"""The case grid that holds the fast warp kernels (k_warp.hip: k_warp_fast, and its bf16 twins of k_warp_bf16.hip) to EXACT expectations at the
source borders, shared by tests/test_warp_edge_cases.py (CPU: names, coverage, the oracle, the near-misses) and tests/test_gpu_warp_edges.py (the
kernels, fast and interpreted).

Why exact.  The float64 model (tests/f64_model.py) excludes every pixel whose source coordinate lies within the coordinate error of a border, and
a plane may exclude at most 1 %.  An integer translation puts whole rows and columns of the target ON a border (13.75 % of a 20x16 target over a
13x9 source for [1 0 -3; 0 1 -2]), so the taps whose rules are the delicate ones -- sx == 0, sx == w-1 (the replicated right tap, weight 0), sx in
(w-1, w) (the replicated right tap, weight > 0), sy in (h-1, h) (the clamped bottom row) -- are exactly the ones the model must skip.  With
coefficients that fp32 holds exactly and source coordinates that are multiples of 1/2, nothing rounds anywhere: the expectation is written here
from integer indices and float64 sums of u8 * weight (weights in {0, 1/4, 1/2, 1}), the pointwise tails (x 0.5, - 16, / 4) keep every value a
multiple of 1/32 below 2^10, which fp32 and fp16 hold exactly and bf16 rounds once -- and the comparison is bit for bit.  No f64_model, oracle or
library code takes part in an exact expectation (exact_plane, apply_tail, to_store_bits).

A case is a function of a backend (tests/model_cases.HostBackend / DeviceBackend): build(B) -> (iops, views); it leaves in B.placed where the
output's samples lie in the output BUFFER (tests/colour_cases.Placed: the whole buffer is read back and every byte that is no sample must still
hold its fill).  Sources are views of byte buffers filled with a pattern that is not the image's: `src_off` bytes (0, 1, 3, 5) into an aligned
allocation, rows `src_pad` bytes apart beyond their own length.  Source samples are never 0, so that a tap taken as zero always shows.

Kernel keys.  The dry run names 40 fast kernels (2 channel counts x 2 transforms x 3 programs x 3 planar stores, and 4 packed ones); each is
compiled twice, with the plane descriptors in the kernel arguments and read from a table (more than kInlineWarp = 52 planes, or a caller-owned
device table).  A KEY is (name, descriptors from a table): 72 planar keys and 8 packed ones.

Classes.  EXACT cases carry `expected(B)`, the bytes of the output's samples; MODELLED cases (fractional coefficients) are held to F.evaluate's
bound, and the share of pixels the model excludes is at most 1 % per plane (asserted on the CPU from the model alone)."""
import collections

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import f64_model as F
from tests import model_cases as MC

EXACT, MODELLED = "exact", "modelled"
TAILS = {"swap": "swap_mul_sub_div", "plain": "mul_sub_div", "interp": "interp"}
STORES = {"f32": "", "f16": "_f16", "bf16": "_bf16"}
BG = [8.0, 24.0, 40.0, 72.0]  # planes at or beyond usedPlanes; through the tails these stay multiples of 1/32
RULES = ("spec", "right_tap_zero", "bottom_row_unclamped", "inside_up_to_w-1")  # the rule of the product and three near-misses of it

Case = collections.namedtuple("Case", "name cls kernel table family cn persp tail store write n used dsize planes src_off src_pad build expected oracle")
Plane = collections.namedtuple("Plane", "w h m seed")  # source extent, the 9 inverse coefficients (destination -> source), the image's seed
CASES = collections.OrderedDict()


def kernel_of(cn, persp, tail, store, packed):
    base = "warp_%s_u8c%d" % ("perspective" if persp else "affine", cn)
    return base + "_packed_f32" if packed else "%s_%s%s" % (base, TAILS[tail], STORES[store])


def family_of(persp, store, packed):
    return "%s %s" % ("perspective" if persp else "affine", "packed" if packed else store)


def image(pl, cn):
    """seeded u8 samples in 1..255 (no zero: a tap wrongly taken as zero changes the value wherever its weight is not 0)"""
    rng = np.random.default_rng(7000 + pl.seed)
    return rng.integers(1, 256, size=(pl.h, pl.w, cn), dtype=np.uint8)


# ---- the exact expectation -----------------------------------------------------------------------------------------------------------
def coords(pl, persp, dsize):
    """source coordinates (sx, sy) of every target pixel, exact: every case's coefficients are multiples of 1/2 (perspective: a constant third row
    that divides exactly)"""
    dw, dh = dsize
    m = [float(np.float32(v)) for v in pl.m]
    assert m == [float(v) for v in pl.m], "coefficients are fp32 values"
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    sx, sy = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
    if persp:
        den = m[6] * xs + m[7] * ys + m[8]
        sx, sy = sx / den, sy / den
    return sx, sy


def exact_plane(a, pl, persp, dsize, rule="spec"):
    """[y][x][c] float64: zero outside the source (sx < 0, sx >= w, sy < 0, sy >= h), the right tap clamped to w-1, the bottom tap to h-1.
    `rule` names the product's rule or one of three near-misses of it (RULES)."""
    h, w, _ = a.shape
    sx, sy = coords(pl, persp, dsize)
    assert (sx * 2 == np.rint(sx * 2)).all() and (sy * 2 == np.rint(sy * 2)).all(), "exact cases sit on multiples of 1/2"
    inside = (sx >= 0) & (sy >= 0) & (sy < h) & ((sx <= w - 1) if rule == "inside_up_to_w-1" else (sx < w))
    x1, y1 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x1, sy - y1
    x1c, y1c = np.clip(x1, 0, w - 1), np.clip(y1, 0, h - 1)  # (only so that the pixels outside index something; they become zero below)
    x2c, y2c = np.minimum(x1c + 1, w - 1), np.minimum(y1c + 1, h - 1)
    s = a.astype(np.float64)
    p00, p10, p01, p11 = s[y1c, x1c], s[y1c, x2c], s[y2c, x1c], s[y2c, x2c]
    if rule == "right_tap_zero":
        gone = (x1c + 1 > w - 1)[..., None]
        p10, p11 = np.where(gone, 0.0, p10), np.where(gone, 0.0, p11)
    if rule == "bottom_row_unclamped":  # the row behind the last one: not the image's (here: zero)
        gone = (y1c + 1 > h - 1)[..., None]
        p01, p11 = np.where(gone, 0.0, p01), np.where(gone, 0.0, p11)
    wx, wy = fx[..., None], fy[..., None]
    v = p00 * ((1 - wx) * (1 - wy)) + p10 * (wx * (1 - wy)) + p01 * ((1 - wx) * wy) + p11 * (wx * wy)
    return np.where(inside[..., None], v, 0.0)


def apply_tail(v, tail, cn):
    """the pointwise tails in float64; every operand and every intermediate is a dyadic rational far inside fp32's precision"""
    if tail == "swap":
        v = v[..., [2, 1, 0] + ([3] if cn == 4 else [])]
    if tail == "interp":
        return ((v - 16.0) * 0.5) / 4.0
    return (v * 0.5 - 16.0) / 4.0


def tail_ops(tail, cn):
    f = cvgs.make_type(cvgs.CV_32F, cn)
    mul, sub, div = cvgs.multiply(f, [0.5] * cn), cvgs.subtract(f, [16.0] * cn), cvgs.divide(f, [4.0] * cn)
    if tail == "swap":
        return [cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f), mul, sub, div]
    return [sub, mul, div] if tail == "interp" else [mul, sub, div]


def to_store_bits(v, store):
    """float64 values as the bits of the output's number format: fp32 and fp16 hold them exactly, bf16 rounds once"""
    assert (v * 32 == np.rint(v * 32)).all() and (np.abs(v) < 1024).all(), "multiples of 1/32 below 2^10"
    if store == "f32":
        out = v.astype(np.float32)
    elif store == "f16":
        out = v.astype(np.float16)
    else:
        r = F.rne_float(v, capi.DEPTH_16BF).astype(np.float32)
        assert (r.astype(np.float64) == F.rne_float(v, capi.DEPTH_16BF)).all()
        return (np.ascontiguousarray(r).view(np.uint32) >> 16).astype(np.uint16)
    assert (out.astype(np.float64) == v).all(), "held exactly"
    return out


def in_write_order(v, write):
    """[plane][y][x][c] in the memory order of the write kind"""
    if write == "split":
        return np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    if write == "splitT":
        return np.ascontiguousarray(v.transpose(3, 0, 1, 2))
    return np.ascontiguousarray(v)


def expected_values(case, rule="spec"):
    """[plane][y][x][c] float64 of an exact case, tail applied (the unrounded value: bf16 rounds it once, to_store_bits)"""
    dw, dh = case.dsize
    out = np.empty((case.n, dh, dw, case.cn))
    for z, pl in enumerate(case.planes):
        if z < case.used:
            out[z] = exact_plane(image(pl, case.cn), pl, case.persp, case.dsize, rule)
        else:
            out[z] = np.array(BG[:case.cn])
    return apply_tail(out, case.tail, case.cn)


def tap_facts(case):
    """which border taps the used planes of a case hold (read from its coordinates)"""
    f = collections.Counter()
    for pl in case.planes[:case.used]:
        sx, sy = coords(pl, case.persp, case.dsize)
        inside = (sx >= 0) & (sx < pl.w) & (sy >= 0) & (sy < pl.h)
        f["sx==0"] += int((inside & (sx == 0)).sum())
        f["sx==w-1"] += int((inside & (sx == pl.w - 1)).sum())
        f["sx in (w-1,w)"] += int((inside & (sx > pl.w - 1)).sum())
        f["sy==0"] += int((inside & (sy == 0)).sum())
        f["sy==h-1"] += int((inside & (sy == pl.h - 1)).sum())
        f["sy in (h-1,h)"] += int((inside & (sy > pl.h - 1)).sum())
        f["outside"] += int((~inside).sum())
        f["all outside"] += int(not inside.any())
        f["tiny c%d" % case.cn if pl.w * case.cn < 8 else "windowed c%d" % case.cn] += 1
        f["window clamped"] += int((inside & (np.floor(sx) * case.cn > pl.w * case.cn - 8)).sum()) if pl.w * case.cn >= 8 else 0
    return f


# ---- one chain ------------------------------------------------------------------------------------------------------------------------
def _type16(store, cn):
    return MC.src_type(cvgs.CV_16F if store == "f16" else capi.DEPTH_16BF, cn)


def warp_edge_case(cn, persp, tail, store, write, planes, dsize, used=None, src_off=0, src_pad=0, table=False, out_off=0, out_pad=0):
    """warp(u8 C3 / C4 sources) -> tail -> [16-bit cast] -> write.  write: split | splitT (planar tensors), packed3d (dense [n][h*w] pixels), packed2d
    (one pitched image: rows out_pad bytes apart beyond their own length, starting out_off bytes into the buffer).  table: a caller-owned device
    table of ONE frame (cvgs.build_warp_table_host, the AFFINE3 fit of points placed so that the fit is exact); otherwise host descriptors, which
    the library uploads as a table when there are more than 52."""
    n = len(planes)
    used_ = n if used is None else used
    dw, dh = dsize
    st, f = cvgs.make_type(cvgs.CV_8U, cn), cvgs.make_type(cvgs.CV_32F, cn)
    kind = cvgs.WARP_PERSPECTIVE if persp else cvgs.WARP_AFFINE
    assert write == "packed2d" or (out_off == 0 and out_pad == 0)
    assert not table or len({(p.w, p.h, p.seed) for p in planes}) == 1

    def build(B):
        mats, views, padding, by_image = [], [], [], {}
        for pl in planes:
            key = (pl.w, pl.h, pl.seed)
            if key not in by_image:  # planes that name the same image share one buffer
                a = image(pl, cn)
                row = pl.w * cn
                step = row + src_pad
                raw = K.aligned_bytes(src_off + pl.h * step + 64)
                raw[:] = K.pattern_bytes(raw.size, 3 + pl.seed % 5)
                rows2d = raw[src_off:src_off + pl.h * step].reshape(pl.h, step)
                rows2d[:, :row] = a.reshape(pl.h, row)
                m = B.src(raw.reshape(1, -1), cvgs.CV_8UC1)
                assert m.data % 256 == 0, "the source buffer itself is aligned: only src_off moves the view"
                by_image[key] = (cvgs.GpuMat(pl.h, pl.w, st, m.data + src_off, step, owner=m.owner), F.View(a))
            mats.append(by_image[key][0])
            views.append(by_image[key][1])
        flat = [float(v) for pl in planes for v in pl.m]
        if table:
            desc = cvgs.warp_table_desc(mats[0], 0, 0, n, dsize, [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], cvgs.WARP_FIT_AFFINE3, kind)
            pts = [[(pl.m[2], pl.m[5]), (pl.m[2] + pl.m[0], pl.m[5] + pl.m[3]), (pl.m[2] + pl.m[1], pl.m[5] + pl.m[4])] for pl in planes]
            tb_bytes, valid = cvgs.build_warp_table_host(desc, pts)
            assert all(valid)
            tb = np.frombuffer(bytearray(tb_bytes), np.uint8)
            fitted = tb.view(np.float32).reshape(n, 16)[:, 5:14]  # WarpPlane: data (8 bytes), w, h, step, m[9], dw, dh
            assert (fitted == np.array(flat, np.float32).reshape(n, 9)).all(), "the fit gives the case's coefficients exactly"
            if B.device:
                import torch
                t = torch.from_numpy(tb).cuda()
                B.keep.append(t)
                ptr = t.data_ptr()
            else:  # a stand-in in host memory (names only: the oracle runs no tables)
                B.sources.append(tb)
                ptr = tb.ctypes.data
            rd = cvgs.warp_table(kind, mats[0], ptr, n, dsize, used_, BG)
        else:
            ident = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]] if not persp else [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
            rd = cvgs.warp(kind, st, mats, [ident] * n, dsize, used_, BG)
            rd.warp = [v if z < used_ else 0.0 for z in range(n) for v in flat[9 * z:9 * z + 9]]  # the inverse coefficients themselves
        ops, ot = tail_ops(tail, cn), f
        if store != "f32":
            ot = _type16(store, cn)
            ops = ops + B.to16(f, ot)
        dtype = MC.np_dtype(B.T(ot))
        es = np.dtype(dtype).itemsize
        row_bytes = dw * cn * es
        if write == "packed2d":
            assert n == 1
            pitch, rows = row_bytes + out_pad, dh
        else:
            pitch, rows, row_bytes = n * dh * row_bytes, 1, n * dh * row_bytes
        nbytes = out_off + (rows - 1) * pitch + row_bytes + 64
        o = B.out((1, nbytes + 256), cvgs.CV_8UC1)
        shift = (-o.data) % 256
        filled = K.pattern_bytes(nbytes + 256, 7)
        if B.device:
            import torch
            B.outs[-1][0][B.GUARD:B.GUARD + filled.size] = torch.from_numpy(filled).cuda()
        else:
            B.outs[-1][...] = filled.reshape(1, -1)
        ptr = o.data + shift + out_off
        o1 = cvgs.make_type(capi.type_depth(B.T(ot)), 1) | (B.T(ot) & capi.TYPE_FLAG_BF16)
        if write == "split":
            wr = cvgs.split(B.T(ot), cvgs.GpuMat(n, cn * dw * dh, o1, ptr, owner=o), dsize)
        elif write == "splitT":
            wr = cvgs.splitT(B.T(ot), ptr, dw, dh, n, keep=o)
        elif write == "packed3d":
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(n, dh * dw, B.T(ot), ptr, owner=o), dsize)
        else:
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(dh, dw, B.T(ot), ptr, pitch, owner=o))
        shape = {"split": (n, cn, dh, dw), "splitT": (cn, n, dh, dw)}.get(write, (n, dh, dw, cn))
        B.placed = K.Placed(shift + out_off, pitch, row_bytes, rows, shape, dtype, filled, padding)
        return [rd] + ops + [wr], views
    return build


def add(name, cls, cn, persp, tail, store, write, planes, dsize, used=None, src_off=0, src_pad=0, table=False, **kw):
    assert name not in CASES, name
    packed = write.startswith("packed")
    n = len(planes)
    used_ = n if used is None else used
    build = warp_edge_case(cn, persp, tail, store, write, planes, dsize, used, src_off, src_pad, table, **kw)

    def expected(B):
        """the bytes of the output's samples, in B's number format (a host backend's fp32 twin of a bf16 chain: the unrounded fp32 value)"""
        v = in_write_order(expected_values(CASES[name]), write)
        twin = store == "bf16" and not B.device and B.twin
        return to_store_bits(v, "f32" if twin else store)
    CASES[name] = Case(name, cls, kernel_of(cn, persp, tail, store, packed), bool(table) or n > 52, family_of(persp, store, packed), cn, persp, tail, store,
                       write, n, used_, dsize, planes, src_off, src_pad, build, expected if cls == EXACT else None, not table)


# ---- exact matrices ---------------------------------------------------------------------------------------------------------------------
def _aff(m0, m2, m4, m5):
    return (float(m0), 0.0, float(m2), 0.0, float(m4), float(m5), 0.0, 0.0, 1.0)


def matrices(w, h, dw, dh):
    """exact inverse transforms for a w x h source and a dw x dh target, named.  Every one keeps source coordinates on multiples of 1/2."""
    return collections.OrderedDict([
        ("shift_in", _aff(1, -1, 1, -1)),                      # sx == 0 at x == 1 and sy == 0 at y == 1; column 0 and row 0 outside
        ("identity", _aff(1, 0, 1, 0)),                        # sx == w-1 and sy == h-1 inside wherever the target is larger than the source
        ("shift_last", _aff(1, w - 1, 1, h - 1)),              # the last pixel at the target's origin: sx == w-1, sy == h-1; all else outside
        ("shift_left", _aff(1, w - 2, 1, 0)),                  # the last two columns
        ("outside_right", _aff(1, w, 1, 0)),                   # the whole target outside: sx >= w
        ("outside_above", _aff(1, 0, 1, -dh)),                 # the whole target outside: sy < 0
        ("half_x", _aff(1, -0.5, 1, 0)),                       # sx on halves: sx in (w-1, w) inside; x == 0 outside
        ("half_y", _aff(1, 0, 1, -0.5)),                       # sy on halves: sy in (h-1, h) inside; y == 0 outside
        ("half_xy", _aff(1, 0.5, 1, 0.5)),                     # both; weights 1/4
        ("half_last", _aff(1, w - 1.5, 1, h - 1.5)),           # (w-1.5, h-1.5), then (w-0.5, h-0.5): the replicated tap and the clamped row together
        ("flip_x", _aff(-1, w - 1, 1, 0)),                     # sx == w-1 at x == 0, sx == 0 at x == w-1
        ("flip_y", _aff(1, 0, -1, h - 1)),
        ("half_scale", _aff(0.5, 0, 0.5, 0)),                  # scale 0.5, offset 0
        ("half_scale_off", _aff(0.5, 0.5, 0.5, 0.5)),          # scale 0.5, offset 0.5
        ("half_scale_end", _aff(0.5, w - 2, 0.5, h - 1.5)),    # scale 0.5 ending behind the last column and row
    ])


MATRIX_NAMES = list(matrices(1, 1, 1, 1))


def perspective_twin(m, m8):
    """the first two rows scaled by m8, the third row (0, 0, m8): the division is exact (m8 a power of two)"""
    return tuple(v * m8 for v in m[:6]) + (0.0, 0.0, float(m8))


def plane(w, h, dsize, which, persp, seed, m8=None):
    m = matrices(w, h, dsize[0], dsize[1])[which]
    if persp:
        m = perspective_twin(m, m8 if m8 is not None else (2.0, 0.5)[seed % 2])
    return Plane(w, h, m, seed)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
SRC_WIDTHS = {3: (1, 2, 3, 5, 13), 4: (1, 2, 3, 13)}  # C3: 1, 2 tiny, 3 the first windowed row (9 bytes); C4: 1 tiny, 2 exactly the window
SRC_HEIGHTS = (1, 2, 9)
DST_WIDTHS, DST_HEIGHTS = (1, 63, 64, 65, 130), (1, 3, 4, 5)
MANY_DSIZE = (5, 3)
PLANE_COUNTS = (1, 4, 5, 52, 53)
SRC_LAYOUTS = ((0, 0), (1, 0), (3, 7), (5, 13), (0, 24), (1, 19))  # (src_off, src_pad): dense and pitched, bases 0, 1, 3, 5 bytes into the allocation

_draw = np.random.default_rng(20240)


def _planes_for(cn, persp, n, dsize):
    """n planes: the matrices in turn from a drawn start, source extents and images drawn (seeded: the grid is the same on every machine).  What the
    grid as a whole must contain is asserted in tests/test_warp_edge_cases.py."""
    ws = SRC_WIDTHS[cn]
    start = int(_draw.integers(len(MATRIX_NAMES)))
    return [plane(ws[int(_draw.integers(len(ws)))], SRC_HEIGHTS[int(_draw.integers(3))], dsize, MATRIX_NAMES[(start + k) % len(MATRIX_NAMES)], persp,
                  int(_draw.integers(4))) for k in range(n)]


_i = 0
for _cn in (3, 4):
    for _persp in (False, True):
        _pn = "persp" if _persp else "affine"
        for _store in ("f32", "f16", "bf16"):
            for _tail in ("swap", "plain", "interp"):
                _wr = ("split", "splitT")[_i % 2]
                _off, _pad = SRC_LAYOUTS[_i % len(SRC_LAYOUTS)]
                # descriptors in the kernel arguments: few planes on the edge shapes of the target, one case per key; 52 planes on some
                _n = (1, 4, 5, 1, 4, 5, 52)[_i % 7]
                _ds = MANY_DSIZE if _n == 52 else (DST_WIDTHS[_i % 5], DST_HEIGHTS[(_i // 2) % 4])
                add("c%d_%s_%s_%s_args_n%d_%dx%d" % (_cn, _pn, _tail, _store, _n, _ds[0], _ds[1]), EXACT, _cn, _persp, _tail, _store, _wr,
                    _planes_for(_cn, _persp, _n, _ds), _ds, used=(_n - 2 if _n in (4, 52) and _i % 2 else None), src_off=_off, src_pad=_pad)
                # the border planes, on a second target shape (1 x 1 included): four planes whose border taps lie at the target's origin, so that
                # every key holds sx == 0, sx == w-1, sx in (w-1, w) and sy in (h-1, h), a tiny and a windowed row, whatever the target's size
                _ds2 = (DST_WIDTHS[(_i + 2) % 5], DST_HEIGHTS[(_i // 2 + 1) % 4])
                _border = [plane(1, 1, _ds2, "half_xy", _persp, 0), plane(13, 9, _ds2, "shift_last", _persp, 1),
                           plane(3 if _cn == 3 else 2, 2, _ds2, "identity", _persp, 2), plane(((5, 13) if _cn == 3 else (3, 13))[_i % 2], (2, 9)[_i % 2], _ds2, "half_last", _persp, 3)]
                add("c%d_%s_%s_%s_args_border_%dx%d" % (_cn, _pn, _tail, _store, _ds2[0], _ds2[1]), EXACT, _cn, _persp, _tail, _store, ("splitT", "split")[_i % 2],
                    _border, _ds2, src_off=SRC_LAYOUTS[(_i + 3) % 6][0], src_pad=SRC_LAYOUTS[(_i + 3) % 6][1])
                # descriptors from the uploaded table: 53 planes, used in {0, n-2, n} with a background
                for _used in ((None, 51)[_i % 2],) + ((0,) if _tail == "plain" else ()):
                    add("c%d_%s_%s_%s_table_n53_used%s" % (_cn, _pn, _tail, _store, "all" if _used is None else _used), EXACT, _cn, _persp, _tail, _store, _wr,
                        _planes_for(_cn, _persp, 53, MANY_DSIZE), MANY_DSIZE, used=_used, src_off=_off, src_pad=_pad)
                _i += 1
        # packed fp32 pixels: dense [n][h*w] and one pitched image with patterned padding; from the kernel arguments and from the uploaded table
        for _j, (_wr, _n, _ds) in enumerate((("packed3d", 4, (65, 5)), ("packed2d", 1, (63, 4)), ("packed3d", 53, MANY_DSIZE), ("packed2d", 1, (130, 3)))):
            _off, _pad = SRC_LAYOUTS[(_i + _j) % len(SRC_LAYOUTS)]
            _kw = dict(out_off=16, out_pad=20) if _wr == "packed2d" else {}
            _pls = [[plane(1, 1, _ds, "half_xy", _persp, 0), plane(13, 9, _ds, "shift_last", _persp, 1), plane(3 if _cn == 3 else 2, 2, _ds, "identity", _persp, 2),
                     plane(5 if _cn == 3 else 3, 2, _ds, "half_last", _persp, 3)], [plane(13, 9, _ds, "half_last", _persp, 1)], None, [plane(2, 2, _ds, "half_xy", _persp, 2)]][_j]
            add("c%d_%s_%s_n%d_%dx%d" % (_cn, _pn, _wr, _n, _ds[0], _ds[1]), EXACT, _cn, _persp, ("plain", "interp", "swap", "plain")[_j], "f32", _wr,
                _pls or _planes_for(_cn, _persp, _n, _ds), _ds, used=(51 if _n == 53 else None), src_off=_off, src_pad=_pad, **_kw)

# a caller-owned device table (CVGS_READ_FLAG_TABLE_ON_DEVICE) built with cvgs.build_warp_table_host: five planes of one 13 x 9 frame
for _cn, _persp, _store, _wr in ((3, False, "f32", "split"), (4, False, "bf16", "splitT"), (3, True, "f16", "split"), (4, True, "f32", "packed3d")):
    _names = ("shift_in", "half_last", "flip_x", "half_scale_off", "identity")
    add("c%d_%s_%s_device_table" % (_cn, "persp" if _persp else "affine", _store if _wr != "packed3d" else "packed"), EXACT, _cn, _persp, "swap", _store, _wr,
        [plane(13, 9, (65, 5), _w, False, 5) for _w in _names], (65, 5), used=3, src_off=3, src_pad=9, table=True)

# modelled cases: fractional coefficients of the size at which the model excludes next to nothing
_MA = (0.31, 0.043, -1.37, -0.027, 0.41, -0.83, 0.0, 0.0, 1.0)
_MB = (0.17, -0.021, -0.6, 0.035, 0.72, -0.9, 0.0, 0.0, 1.0)
_MP = (0.31, 0.043, -1.37, -0.027, 0.41, -0.83, 1e-3, -2e-3, 1.0)
_MQ = (0.18, -0.02, 2.1, 0.03, 0.66, -0.7, -2e-3, 1e-3, 1.0)


def _f32s(m):
    return tuple(float(np.float32(v)) for v in m)


for _cn in (3, 4):
    for _persp, _ms in ((False, (_MA, _MB)), (True, (_MP, _MQ))):
        for _k, (_tail, _store, _wr, _ds) in enumerate((("swap", "f32", "split", (20, 16)), ("plain", "f16", "splitT", (65, 5)), ("interp", "f32", "packed3d", (20, 16)))):
            _w = 13
            add("c%d_%s_%s_%s_%s_modelled" % (_cn, "persp" if _persp else "affine", _tail, _store, _wr), MODELLED, _cn, _persp, _tail, _store, _wr,
                [Plane(_w, 9, _f32s(_ms[0]), 1), Plane(_w, 9, _f32s(_ms[1]), 2)], _ds, src_off=(0, 1, 5)[_k], src_pad=(0, 11, 6)[_k])

FAMILIES = sorted({c.family for c in CASES.values()})


def cases_of(family):
    return [c for c in CASES.values() if c.family == family]


def key_of(case):
    return (case.kernel, case.table)
