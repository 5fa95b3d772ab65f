"""The case grid that holds the thread-fused pointwise kernels (k_pointwise.hip: k_pointwise4, its bf16 twins of k_pointwise_bf16.hip, and the tick
kernel k_pointwise4_many) to EXACT bytes at their store edges, shared by tests/test_pointwise_edge_cases.py (CPU: names, coverage, the oracle, the
near-misses) and tests/test_zzzzzzzz_gpu_pointwise_edges.py (the kernels, fast and interpreted).

Why exact, and why the whole buffer.  The write stage pw4_write (k_pointwise_body.hpp) picks one of five store paths on wave-uniform conditions;
a condition that is wrong sends a wave down a path that writes the right VALUES to bytes nobody reads back -- the padding of a pitched image, the
rows behind a plane's last one.  So every case reads the whole output buffer back: the samples must EQUAL the expectation and every other byte
must still hold its fill.  The expectation is float64 numpy from integer indices (expected_values): every operand of the three programs is a
power of two or a small integer and the source samples are chosen so that nothing rounds in fp32 (asserted where each value is built), fp16
holds a u8 source's results exactly and bf16 rounds once (f64_model.rne_float, that one rounding only).  No oracle, f64_model or library code
takes part in an expectation.  Source samples are never 0, so a tap taken as zero shows.

Programs (the three forms the host picks for a u8 source; every other depth runs pointwise4_<depth>):
  plain   convertTo(->32F, 0.5), subtract 16, divide 4          pointwise4_u8_cast_mul_sub_div   (v * 0.5 - 16) / 4
  cast    convertTo(->32F)                                       pointwise4_u8_cast               v
  interp  [channel swap on the source type,] cast, subtract 16,  pointwise4_u8_interp             ((v - 16) * 0.5) / 4
          multiply 0.5, divide 4                                 (the swap exists for 3 and 4 channels)

A case is a function of a backend (tests/model_cases.HostBackend / DeviceBackend): build(B) -> (iops, views); it leaves in B.placed the list of
tests/colour_cases.Placed that say where the output's samples lie in the output BUFFER (one entry; SPLIT_2D: one per pitched plane, each with its
own offset and padding).  Sources are views of one byte buffer filled with a pattern that is not the image's: `src_off` bytes into an aligned
allocation, rows `src_pad` bytes apart beyond their own length.

store_path(case) restates, from the width, the height, the pitch, the element size and the plane count alone, which branches of pw4_write the
waves of a case take, which `narrow` class the case falls in and whether it runs two rows per thread (pw4_body_rows2)."""
import collections

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import f64_model as F
from tests import model_cases as MC

PROGS = ("plain", "cast", "interp")
STORES = {"f32": "", "f16": "_f16", "bf16": "_bf16"}
WRITES = ("split", "splitT", "packed3d", "packed2d", "split2d")
BG = [8.0, 24.0, 40.0, 72.0]  # planes at or beyond `used`
RULES = ("spec", "tail_zero", "default_reads_source", "no_swap", "exchanged")  # the product's rule and four near-misses of it
DEPTHS = collections.OrderedDict([("u8", cvgs.CV_8U), ("s8", cvgs.CV_8S), ("u16", cvgs.CV_16U), ("s16", cvgs.CV_16S), ("s32", cvgs.CV_32S), ("f32", cvgs.CV_32F)])
NP = {"u8": np.uint8, "s8": np.int8, "u16": np.uint16, "s16": np.int16, "s32": np.int32, "f32": np.float32}
U8_PROG_NAMES = {"plain": "cast_mul_sub_div", "cast": "cast", "interp": "interp"}
ROWS2_PIXELS = 1 << 20  # launch_pw: one-channel planes of at least this many pixels per launch run two rows per thread

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 60, 63, 64, 65, 68, 124, 127, 128, 129, 132, 255, 256, 257, 511, 512, 513, 515)
HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 17)
MANY_SIZE = (5, 3)
PLANE_COUNTS = (1, 5, capi.KERNARG_PLANES, capi.KERNARG_PLANES + 1)
OUT_OFFS = {4: (0, 4, 8, 12), 2: (0, 2, 6, 10)}  # bytes in front of a pitched image, by element size
OUT_PADS = (0, 4, 16, 20)
SRC_LAYOUTS = ((0, 0), (1, 0), (3, 7), (5, 13), (0, 24), (1, 19))  # (src_off, src_pad) in bytes for 1-byte samples; wider ones: in elements, below

Case = collections.namedtuple("Case", "name kernel family depth cn prog store write w h n used table src_off src_pad out_off out_pad seed build expected")
Path = collections.namedtuple("Path", "narrow rows2 branches")
CASES = collections.OrderedDict()


def kernel_of(depth, prog, store):
    return "pointwise4_u8_%s%s" % (U8_PROG_NAMES[prog], STORES[store]) if depth == "u8" else "pointwise4_" + depth


def family_of(depth, store):
    return "%s %s" % (depth, store)


def elem_bytes(depth):
    return np.dtype(NP[depth]).itemsize


def src_layout(depth, k):
    """the k-th source layout in bytes: bases 0, 1, 3, 5 bytes into the allocation for 1-byte samples, 0 or one element for wider ones"""
    off, pad = SRC_LAYOUTS[k % len(SRC_LAYOUTS)]
    eb = elem_bytes(depth)
    return (off, pad) if eb == 1 else ((off & 1) * eb, pad * eb)


# ---- the exact expectation -------------------------------------------------------------------------------------------------------------
def source(case, z):
    """[y][x][c] samples of plane z in the source type, seeded, never 0: any 8- / 16-bit value, CV_32S in (-2^22, 2^22), CV_32F multiples of 1/4
    below 2^16 -- the values at which no stage of the three programs rounds in fp32"""
    rng = np.random.default_rng(9000 + 131 * case.seed + z)
    shape = (case.h, case.w, case.cn)
    lo, hi = {"u8": (1, 256), "s8": (-128, 128), "u16": (1, 65536), "s16": (-32768, 32768), "s32": (-(1 << 22) + 1, 1 << 22), "f32": (-(1 << 18) + 1, 1 << 18)}[case.depth]
    a = rng.integers(lo, hi, size=shape, dtype=np.int64)
    a = np.where(a == 0, hi - 1, a)
    if case.depth == "f32":
        return (a.astype(np.float64) / 4.0).astype(np.float32)
    return a.astype(NP[case.depth])


def _held_by_fp32(v):
    assert (v.astype(np.float32).astype(np.float64) == v).all(), "a stage's value rounds in fp32"
    return v


def apply_program(v, prog, cn, swap=True):
    """the three programs in float64; every operand is a power of two or a small integer and every intermediate is asserted to be an fp32 value"""
    v = _held_by_fp32(np.asarray(v, np.float64))
    if prog == "cast":
        return v
    if prog == "interp":
        if swap and cn >= 3:
            v = v[..., [2, 1, 0] + ([3] if cn == 4 else [])]
        return _held_by_fp32(_held_by_fp32(_held_by_fp32(v - 16.0) * 0.5) / 4.0)
    return _held_by_fp32(_held_by_fp32(_held_by_fp32(v * 0.5) - 16.0) / 4.0)


def background(case):
    """BG in the source type (CV_32S: through (int)), as float64"""
    bg = np.array(BG[:case.cn])
    return np.array([float(int(b)) for b in bg]) if case.depth == "s32" else bg


def expected_values(case, rule="spec"):
    """[plane][y][x][c] float64, program applied (unrounded: bf16 rounds it once, to_store_bits).  `rule` names the product's rule or a near-miss."""
    out = np.empty((case.n, case.h, case.w, case.cn))
    for z in range(case.n):
        if z < case.used or rule == "default_reads_source":
            a = source(case, z).astype(np.float64)
            if rule == "tail_zero" and case.w % 4:  # the pixels of the ragged last group taken as zero
                a[:, case.w & ~3:, :] = 0.0
            out[z] = a
        else:
            out[z] = background(case)
    prog = case.prog
    if rule == "exchanged" and prog != "cast":  # (v - 16) * 0.5 against v * 0.5 - 16, the swap staying where it is
        if prog == "interp" and case.cn >= 3:
            out = out[..., [2, 1, 0] + ([3] if case.cn == 4 else [])]
        return apply_program(out, "plain" if prog == "interp" else "interp", case.cn, swap=False)
    return apply_program(out, prog, case.cn, swap=rule != "no_swap")


def to_store_bits(v, store):
    """float64 values as the bits of the output's number format: fp32 holds every case's values, fp16 a u8 source's, bf16 rounds once"""
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
    """[plane][y][x][c] in the memory order of the write kind (split2d: [plane][c][y][x], one pitched plane each)"""
    if write in ("split", "split2d"):
        return np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    if write == "splitT":
        return np.ascontiguousarray(v.transpose(3, 0, 1, 2))
    return np.ascontiguousarray(v)


# ---- which branch of pw4_write a case's waves take -------------------------------------------------------------------------------------
def store_path(case):
    """Restated from W, H, the pitch, the element size and the plane count (NOT read from the library): the `narrow` class (log2 of the rows per
    wave), whether the launch runs two rows per thread, and the set of store branches its waves take."""
    W, H, cn = case.w, case.h, case.cn
    es = 4 if case.store == "f32" else 2
    narrow = 2 if W <= 64 else (1 if W <= 128 else 0)
    rows2 = cn == 1 and narrow == 0 and W * H * case.n >= ROWS2_PIXELS
    br = set()
    x4, tail = W >= 4, W % 4 != 0
    if case.write == "split2d":
        br |= ({"per-plane x4"} if x4 else set()) | ({"per-plane tail"} if tail else set())
    elif case.write in ("split", "splitT"):
        br |= ({"planar x4"} if x4 else set()) | ({"planar tail"} if tail else set())
    elif narrow == 0:
        rest = W % 256
        if W >= 256:
            br.add("full group")
        br |= ({"direct x4"} if rest >= 4 else set()) | ({"direct tail"} if rest % 4 else set())
    else:
        rpw = 1 << narrow
        pitch = W * cn * es + (case.out_pad if case.write == "packed2d" else 0)
        dense = es == 4 and pitch == W * cn * es and W % 4 == 0
        if dense and H >= rpw:
            br.add("narrow dense")
        if not dense or H % rpw:  # the last wave's rows run past h: it leaves the dense path
            br |= ({"direct x4"} if x4 else set()) | ({"direct tail"} if tail else set())
    if rows2:
        br.add("rows2")
    return Path(narrow, rows2, frozenset(br))


def takes_tick(case):
    """the shapes launch_pointwise_many takes: u8 planes, an fp32 tensor (planar or dense packed pixels), descriptors in the kernel arguments"""
    return case.depth == "u8" and case.store == "f32" and case.write in ("split", "splitT", "packed3d") and not case.table


# ---- one chain -------------------------------------------------------------------------------------------------------------------------
def program_ops(depth, prog, cn):
    st, f = cvgs.make_type(DEPTHS[depth], cn), cvgs.make_type(cvgs.CV_32F, cn)
    mul, sub, div = cvgs.multiply(f, [0.5] * cn), cvgs.subtract(f, [16.0] * cn), cvgs.divide(f, [4.0] * cn)
    if prog == "cast":
        return [cvgs.convertTo(st, f)]
    if prog == "plain":
        return [mul, sub, div] if depth == "f32" else [cvgs.convertTo(st, f, 0.5), sub, div]
    ops = []
    if cn >= 3:  # the channel permutation cvGS::cvtColor<RGB2BGR / RGBA2BGRA> lowers to, on the source type (cvtColor itself takes three depths only)
        ops.append(cvgs.PointwiseIOp(st, st, [(capi.OP_REORDER, 2 | (1 << 2) | (0 << 4) | ((3 << 6) if cn == 4 else 0), None)]))
    if depth != "f32":
        ops.append(cvgs.convertTo(st, f))
    return ops + [sub, mul, div]


def _type16(store, cn):
    return MC.src_type(cvgs.CV_16F if store == "f16" else capi.DEPTH_16BF, cn)


def _up(v, a):
    return (v + a - 1) // a * a


def pointwise_edge_case(case):
    """read(case.n planes of case.depth) -> program -> [16-bit cast] -> write.  write: split | splitT (planar tensors), packed3d (dense [n][h*w]
    pixels), packed2d (one pitched image: rows out_pad bytes apart beyond their own length), split2d (n * cn separate pitched planes, plane k
    OUT_OFFS[k] bytes behind a 16-byte boundary with OUT_PADS[k] bytes of row padding, both counted on from the case's own).  Every target starts
    out_off bytes into a 256-byte aligned buffer of patterned bytes."""
    c = case
    eb, st, f = elem_bytes(c.depth), cvgs.make_type(DEPTHS[c.depth], c.cn), cvgs.make_type(cvgs.CV_32F, c.cn)

    def build(B):
        row = c.w * c.cn * eb
        step = row + c.src_pad
        region = _up(c.src_off + c.h * step + 64, 256)
        raw = K.aligned_bytes(c.n * region)
        raw[:] = K.pattern_bytes(raw.size, 3 + c.seed % 5)
        views = []
        for z in range(c.n):
            a = source(c, z)
            raw[z * region + c.src_off:z * region + c.src_off + c.h * step].reshape(c.h, step)[:, :row] = np.ascontiguousarray(a).view(np.uint8).reshape(c.h, row)
            views.append(F.View(a))
        m = B.src(raw.reshape(1, -1), cvgs.CV_8UC1)
        assert m.data % 256 == 0, "the source buffer itself is aligned: only src_off moves the views"
        mats = [cvgs.GpuMat(c.h, c.w, st, m.data + z * region + c.src_off, step, owner=m.owner) for z in range(c.n)]
        rd = cvgs.ReadIOp(capi.READ_PIXEL, st, mats, c.used, None, cvgs.IGNORE_AR, BG)
        ops, ot = program_ops(c.depth, c.prog, c.cn), f
        if c.store != "f32":
            ot = _type16(c.store, c.cn)
            ops = ops + B.to16(f, ot)
        dtype = MC.np_dtype(B.T(ot))
        es = np.dtype(dtype).itemsize
        o1 = cvgs.make_type(capi.type_depth(B.T(ot)), 1) | (B.T(ot) & capi.TYPE_FLAG_BF16)
        # where the samples lie: (origin, pitch, row bytes, rows, shape) per piece
        if c.write == "split2d":
            offs, pieces, cur = OUT_OFFS[2 if c.store != "f32" else 4], [], 0  # (the offsets of the GPU's element size, on the fp32 twin too)
            for k in range(c.n * c.cn):
                off, pad = offs[(offs.index(c.out_off) + k) % 4], OUT_PADS[(OUT_PADS.index(c.out_pad) + k) % 4]
                pieces.append((cur + off, c.w * es + pad, c.w * es, c.h, (c.h, c.w)))
                cur = _up(cur + off + c.h * (c.w * es + pad) + 8, 16)
            nbytes = cur + 64
        else:
            row_bytes = c.w * c.cn * es
            if c.write == "packed2d":
                assert c.n == 1
                pieces = [(c.out_off, row_bytes + c.out_pad, row_bytes, c.h, (1, c.h, c.w, c.cn))]
            else:
                assert c.out_pad == 0
                shape = {"split": (c.n, c.cn, c.h, c.w), "splitT": (c.cn, c.n, c.h, c.w)}.get(c.write, (c.n, c.h, c.w, c.cn))
                pieces = [(c.out_off, c.n * c.h * row_bytes, c.n * c.h * row_bytes, 1, shape)]
            nbytes = pieces[0][0] + (pieces[0][3] - 1) * pieces[0][1] + pieces[0][2] + 64
        o = B.out((1, nbytes + 256), cvgs.CV_8UC1)
        shift = (-o.data) % 256
        filled = K.pattern_bytes(nbytes + 256, 7)
        if B.device:
            import torch
            B.outs[-1][0][B.GUARD:B.GUARD + filled.size] = torch.from_numpy(filled).cuda()
        else:
            B.outs[-1][...] = filled.reshape(1, -1)
        base = o.data + shift
        B.placed = [K.Placed(shift + p[0], p[1], p[2], p[3], p[4], dtype, filled, None) for p in pieces]
        ptr = base + pieces[0][0]
        if c.write == "split":
            wr = cvgs.split(B.T(ot), cvgs.GpuMat(c.n, c.cn * c.w * c.h, o1, ptr, owner=o), (c.w, c.h))
        elif c.write == "splitT":
            wr = cvgs.splitT(B.T(ot), ptr, c.w, c.h, c.n, keep=o)
        elif c.write == "packed3d":
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(c.n, c.h * c.w, B.T(ot), ptr, owner=o), (c.w, c.h))
        elif c.write == "packed2d":
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(c.h, c.w, B.T(ot), ptr, pieces[0][1], owner=o))
        else:
            planes = [[cvgs.GpuMat(c.h, c.w, o1, base + pieces[z * c.cn + ch][0], pieces[z * c.cn + ch][1], owner=o) for ch in range(c.cn)] for z in range(c.n)]
            wr = cvgs.split(B.T(ot), planes if c.n > 1 else planes[0])
        return [rd] + ops + [wr], views
    return build


def split_whole(placed, whole, write, n, cn):
    """(the samples in the write kind's order, indices of padding bytes that no longer hold their fill) of a whole output buffer read back;
    `placed` is the list a case's build leaves in B.placed"""
    parts = [K.split_output(p, whole) for p in placed]
    moved = parts[0][1]
    for _, m in parts[1:]:  # a byte is padding if it is no piece's sample
        moved = np.intersect1d(moved, m, assume_unique=True)
    if write != "split2d":
        return parts[0][0], moved
    return np.stack([g for g, _ in parts]).reshape((n, cn) + parts[0][0].shape), moved


def add(name, depth, cn, prog, store, write, w, h, n=1, used=None, layout=0, out_off=0, out_pad=0):
    assert name not in CASES, name
    assert store == "f32" or depth == "u8", "16-bit stores exist for u8 sources"
    assert write != "split2d" or cn >= 2, "cvGS::split needs 2 to 4 channels"
    assert write in ("packed2d", "split2d") or out_pad == 0
    used_ = n if used is None else used
    off, pad = src_layout(depth, layout)

    def expected(B):
        """the bytes of the output's samples, in B's number format (a host backend's fp32 twin of a bf16 chain: the unrounded fp32 value)"""
        v = in_write_order(expected_values(CASES[name]), write)
        return to_store_bits(v, "f32" if (store == "bf16" and not B.device and B.twin) else store)
    c = Case(name, kernel_of(depth, prog, store), family_of(depth, store), depth, cn, prog, store, write, w, h, n, used_, n > capi.KERNARG_PLANES, off, pad,
             out_off, out_pad, len(CASES), None, expected)
    CASES[name] = c._replace(build=pointwise_edge_case(c))


# ---- the grid --------------------------------------------------------------------------------------------------------------------------
FAMILY_KEYS = [(d, s) for d in DEPTHS for s in (("f32", "f16", "bf16") if d == "u8" else ("f32",))]
_NEAR = ("u8", "s16")  # the depth classes that carry the narrow dense path's named near-misses

for _f, (_d, _s) in enumerate(FAMILY_KEYS):
    _es = 4 if _s == "f32" else 2
    # every width, the writes, channel counts, programs, heights and layouts in turn (rotated per family)
    for _i, _w in enumerate(WIDTHS):
        _k = _i + 2 * _f
        _wr = WRITES[_k % 5]
        _cn = 1 + (_i + _f) % 4
        if _wr == "split2d" and _cn == 1:
            _cn = 3
        _kw = dict(out_off=OUT_OFFS[_es][_k % 4], out_pad=OUT_PADS[(_k // 2) % 4]) if _wr in ("packed2d", "split2d") else dict(out_off=(0, _es)[_k % 2])
        add("%s_%s_w%d_%s" % (_d, _s, _w, _wr), _d, _cn, PROGS[_k % 3], _s, _wr, _w, HEIGHTS[(_i + 4 * _f) % 9], layout=_k, **_kw)
    # anchors: each store branch on each family, whatever the rotation above gives it
    for _j, (_wr, _w, _h, _cn, _off, _pad) in enumerate((("packed3d", 64, 8, 3, 0, 0), ("packed3d", 128, 5, 2, 0, 0), ("packed2d", 257, 3, 4, 1, 20), ("packed3d", 515, 2, 3, 0, 0),
                                                         ("packed2d", 7, 9, 2, 3, 4), ("splitT", 7, 5, 4, 1, 0), ("split2d", 7, 4, 2, 2, 16), ("split2d", 132, 2, 4, 3, 0),
                                                         ("packed2d", 60, 17, 1, 1, 0), ("split", 513, 1, 1, 0, 0))):
        _own = PROGS[(_j + _f) % 3]
        for _p in (PROGS if _d == "u8" and _j in (0, 2, 4, 5, 6) else (_own,)):  # u8: each program is a kernel of its own, so each takes every branch
            add("%s_%s_anchor_%s_%dx%d%s" % (_d, _s, _wr, _w, _h, "" if _p == _own else "_" + _p), _d, _cn, _p, _s, _wr, _w, _h, layout=_j + _f,
                out_off=OUT_OFFS[_es][_off], out_pad=_pad)
    # planes: descriptors in the kernel arguments (5, 64) and in the uploaded table (65), `used` below the count, a tiny target
    for _j, _n in enumerate(PLANE_COUNTS[1:]):
        _wr = (("split", "packed3d", "splitT")[_f % 3], "split2d", ("packed3d", "splitT", "split")[_f % 3])[_j]  # (64 x cn pitched planes: the uploaded target table)
        add("%s_%s_n%d_%s" % (_d, _s, _n, _wr), _d, (3, 4, 2)[(_j + _f) % 3], PROGS[(_j + _f + 2) % 3], _s, _wr, MANY_SIZE[0], MANY_SIZE[1], n=_n,
            used=(_n - 2, None, _n - 3)[_j], layout=_j + 3 * _f)
    add("%s_%s_n5_interp_defaults" % (_d, _s), _d, 3 + _f % 2, "interp", _s, ("packed3d", "split")[_f % 2], 7, 2, n=5, used=2, layout=_f)

# near-misses of the narrow dense path: each one step inside the condition and one step outside it
for _d in _NEAR:
    for _j, (_w, _h) in enumerate(((64, 8), (128, 4), (60, 4), (124, 2))):
        for _pad in (0, 4, 16):  # pitch = dense, dense + 4, dense + 16
            add("%s_dense_pitch+%d_%dx%d" % (_d, _pad, _w, _h), _d, 1 + (_j + _pad // 4) % 4, PROGS[_j % 3], "f32", "packed2d", _w, _h, layout=_j, out_off=(0, 4, 8, 12)[_j], out_pad=_pad)
    for _j, _w in enumerate((63, 64, 65, 127, 128, 129)):  # both narrow limits
        add("%s_dense_limit_w%d" % (_d, _w), _d, 1 + _j % 4, PROGS[_j % 3], "f32", "packed3d", _w, 8, layout=_j + 1)
    for _j, (_w, _h) in enumerate(((64, 4), (64, 5), (64, 8), (64, 9), (128, 2), (128, 3), (128, 16), (128, 17), (8, 1), (8, 3), (4, 4), (4, 7))):  # H a multiple of the rows per wave, and H + 1
        add("%s_dense_rows_%dx%d" % (_d, _w, _h), _d, 1 + (_j + 1) % 4, PROGS[(_j + 1) % 3], "f32", ("packed3d", "packed2d")[_j % 2], _w, _h, layout=_j + 2, out_off=(0, 4)[_j % 2])
for _j, (_s, _w, _h) in enumerate((("f16", 64, 8), ("bf16", 64, 8), ("f16", 128, 4), ("bf16", 128, 4), ("f16", 60, 4), ("bf16", 124, 2))):
    add("u8_%s_dense_plane_%dx%d" % (_s, _w, _h), "u8", 1 + _j % 4, PROGS[_j % 3], _s, ("packed3d", "packed2d")[_j % 2], _w, _h, layout=_j, out_off=(0, 2)[_j % 2])  # 16-bit stores: the direct path

# two rows per thread: one-channel planes at or above 2^20 pixels (the last 8-row block partial, with and without its lower rows), one just below
add("u8_rows2_1021x1029_packed3d", "u8", 1, "plain", "f32", "packed3d", 1021, 1029, layout=1)
add("s16_rows2_1021x1029_splitT", "s16", 1, "interp", "f32", "splitT", 1021, 1029, layout=2)
add("u8_rows2_1024x1025_split", "u8", 1, "cast", "f32", "split", 1024, 1025, layout=3)
add("s16_below_rows2_1024x1023_packed3d", "s16", 1, "plain", "f32", "packed3d", 1024, 1023, layout=4)

FAMILIES = [family_of(d, s) for d, s in FAMILY_KEYS]


def cases_of(family):
    return [c for c in CASES.values() if c.family == family]
