"""The case grid that holds the standalone colour-conversion kernels (k_cvtcolor_u8.hip: k_u8_permute16, k_u8_gray16, k_f32_colour4) to the
float64 model (tests/f64_model.py), shared by tests/test_colour_cases.py (CPU: names, coverage, the oracle against the model) and
tests/test_gpu_colour_model.py (the kernels against the model).

These kernels have their own geometry: a lane owns 16 pixels (4 of CV_32F), a wave's 1024 pixels (256) travel through LDS, every global access
is a 16-byte access guarded by `off < row_bytes`, and a host predicate (launch_u8_colour16 / launch_f32_colour4) decides from widths,
pointers, pitches and operand values whether a chain takes them.  The grid therefore holds

  * tile edges: WIDTHS = one lane, the last lane exactly at the end of a tile (one lane short of it, the whole tile), a whole tile followed by
    one lane, two tiles followed by one lane; HEIGHTS around the 4 rows of a workgroup;
  * pitch: source views at a 16-byte-aligned x offset of a wider buffer, single-image outputs that are views of a wider buffer, batches into a
    dense tensor -- every byte that is no sample holds a pattern, and the GPU test reads the WHOLE output buffer back;
  * what cvGS::cvtColor cannot say: gray orders that take the `ORD == 0` kernels, alphas whose bytes differ, a third selector order;
  * ineligible neighbours: an eligible case with exactly one thing changed (REASONS), expected on the interpreted kernel.

A case is a function of a backend (tests/model_cases.HostBackend / DeviceBackend): build(B, fill=0) -> (iops, views).  The chain builder is this
module's own colour_case, not model_cases.pointwise_case: that one wraps one dense array per chain and can neither pitch a source or an output
nor offset a base pointer nor batch.  A build leaves in
B.placed where the samples of the output lie in the output buffer and what every other byte was filled with.  `fill` picks the pattern of the
SOURCE padding only: no output byte may depend on it.

Non-representable alphas.  ADD_ALPHA on an integer image with an operand that is no whole number in range is accepted by cvgs_validate.
255.5 is in range: the C conversion to the channel type truncates, the value is 255, and the model is told so (alpha_value).  300 (CV_8U), -1
and 65536 have NO value -- the conversion of an out-of-range float to an unsigned type is undefined in C and C++, the oracle's own spelling of it
included --, so there the colour channels are held to the model, the alpha channel must be one constant over the image, and the three kernel
paths must agree with one another; the CPU oracle does not run these.  pointwise4_u8_u8 stores through a saturating conversion in its body
and gave 255 / 0 where its own tail and the generic kernel give another byte, so it leaves such chains to the generic kernel
(launch_pointwise_u8u8).  All three paths of these cases therefore run the generic kernel: for them the comparison across paths checks
the dispatch (the expected kernel names), no longer two kernels against each other."""
import collections

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import helpers as H

U8, U16, F32 = cvgs.CV_8U, cvgs.CV_16U, cvgs.CV_32F
DEPTHS = (U8, U16, F32)
DN = {U8: "8u", U16: "16u", F32: "32f"}
ES = {U8: 1, U16: 2, F32: 4}
NP = {U8: np.uint8, U16: np.uint16, F32: np.float32}
WIDTHS = {U8: (16, 1008, 1024, 1040, 2064), U16: (16, 1008, 1024, 1040, 2064), F32: (4, 252, 256, 260, 516)}
HEIGHTS = (1, 3, 4, 5, 9)
# (width index, height): every width and every height twice; the widest image stays under 100 KB at 8 bytes per pixel (2064 x 5)
SHAPES = [(0, 9), (1, 5), (2, 4), (3, 3), (4, 1), (0, 4), (1, 3), (2, 1), (3, 9), (4, 5)]
FAST = {(U8, "permute"): "pointwise16_u8_permute", (U8, "gray"): "pointwise16_u8_gray", (U16, "permute"): "pointwise16_u16_permute",
        (U16, "gray"): "pointwise16_u16_gray", (F32, "permute"): "pointwise4_f32_permute", (F32, "gray"): "pointwise4_f32_gray"}
FAST_PREFIXES = ("pointwise16_", "pointwise4_f32_")
# the interpreted kernel an ineligible chain of each depth runs on by default (what cvgs.kernel_name reports for it)
FALLBACK = {U8: "pointwise4_u8_u8_interp", U16: "generic_inline8", F32: "generic_inline8"}
GENERIC, GENERIC_TABLE = "generic_inline8", "generic_table"  # under CHAIN_NO_THREAD_FUSION / CHAIN_FORCE_GENERIC, every depth
FLAGS = (("default", capi.CHAIN_DEFAULT), ("no_fusion", capi.CHAIN_NO_THREAD_FUSION), ("generic", capi.CHAIN_FORCE_GENERIC))

ID3, SWAP3, THIRD3 = 0 | (1 << 2) | (2 << 4), 2 | (1 << 2) | (0 << 4), 1 | (2 << 2) | (0 << 4)
# cvtColor codes of tests/test_gpu_chains.py's _CODES: (name, code, channels in, channels out)
PERMUTE_CODES = [("BGR2RGB", cvgs.COLOR_BGR2RGB, 3, 3), ("BGRA2RGBA", cvgs.COLOR_BGRA2RGBA, 4, 4), ("BGR2BGRA", cvgs.COLOR_BGR2BGRA, 3, 4),
                 ("BGR2RGBA", cvgs.COLOR_BGR2RGBA, 3, 4), ("BGRA2BGR", cvgs.COLOR_BGRA2BGR, 4, 3), ("RGBA2BGR", cvgs.COLOR_RGBA2BGR, 4, 3)]
GRAY_CODES = [("BGR2GRAY", cvgs.COLOR_BGR2GRAY, 3, 1), ("RGB2GRAY", cvgs.COLOR_RGB2GRAY, 3, 1), ("BGRA2GRAY", cvgs.COLOR_BGRA2GRAY, 4, 1),
              ("RGBA2GRAY", cvgs.COLOR_RGBA2GRAY, 4, 1)]
GRAY_ORDERS = [((1, 0, 2), 3), ((0, 0, 0), 3), ((2, 0, 1), 3), ((3, 1, 0), 4), ((1, 2, 3), 4)]  # ((R, G, B) channel indices, channels in)
ALPHAS = {U8: (7.0, 0.0), U16: (float(0x1234), float(0x00FF))}
ALPHAS_F32 = (-0.0, float(np.float32(3.0e38)), float(np.array([0x00000123], np.uint32).view(np.float32)[0]))  # compared as bits; the last one is a subnormal
BAD_ALPHAS = {U8: (255.5, 300.0, -1.0, 65536.0), U16: (255.5, -1.0, 65536.0)}  # (300 is a CV_16U value: eligible)
PITCHED_LAYOUTS = ("src_pitch", "out_pitch", "both_pitch")
BATCH_LAYOUTS = ("batch1", "batch2", "batch3")
REASONS = ("width+1", "width-3", "src_base+4", "src_base+8", "src_step%16=8", "out_base+8", "out_pitch%16=8", "used<batch", "device_table")
BACKGROUND = [7.0, 9.0, 11.0, 13.0]  # planes at or beyond usedPlanes

Case = collections.namedtuple("Case", "name depth template kernel generic pure reason layout w h gray_order cn oracle alpha_defined build")
Placed = collections.namedtuple("Placed", "origin pitch row_bytes rows shape dtype fill src_padding")
CASES = collections.OrderedDict()


def gray_aux(order):
    return order[0] | (order[1] << 2) | (order[2] << 4)


def pattern_bytes(n, k):
    """n bytes that are neither constant nor zero; k picks one of several patterns"""
    return ((np.arange(n, dtype=np.int64) * (37 + 2 * k) + 11 + 101 * k) % 251 + 1).astype(np.uint8)


def aligned_bytes(n, align=256):
    buf = np.empty(n + align, np.uint8)
    off = (-buf.ctypes.data) % align
    return buf[off:off + n]


def samples(depth, shape, seed, finite):
    """seeded, non-constant samples.  CV_16U: 65535 and values whose two bytes differ.  CV_32F: +-inf, -0.0, 3e38 and a quiet NaN in the first and the
    last pixels of the image (finite=False: channel permutations move bits), plain finite values otherwise."""
    if depth == U8:
        return H.random_u8(shape, seed)
    a = H.random_u16(shape, seed)
    if depth == U16:
        a = a.copy()
        a.reshape(-1)[::53] = 65535
        a.reshape(-1)[1::61] = 0x01FE
        return a
    f = ((a.astype(np.float32) - 32768.0) / np.float32(37.0)).astype(np.float32)
    if not finite:
        sp = np.array([np.inf, -np.inf, -0.0, 3.0e38, np.nan, 1.0e-40], np.float32)
        flat = f.reshape(-1)
        k = min(sp.size, flat.size // 2)
        flat[:k] = sp[:k]
        flat[flat.size - k:] = sp[:k][::-1]
    return f


# ---- one chain ----------------------------------------------------------------------------------------------------------------------
def colour_case(depth, cn, ocn, stage, w, h, seed, finite, batch=1, used=None, src_off=0, src_pad=0, out_off=0, out_pad=0, out3d=False, table=False):
    """ReadIOp(READ_PIXEL) -> stage(in_type, out_type) -> write.  Every source is a view of its own byte buffer: it starts src_off bytes into a
    row of w * cn * es + src_off + src_pad bytes.  The output is a single-image view (out3d=False: it starts out_off bytes into the buffer, rows
    out_pad bytes apart beyond their own length) or a dense [batch][h * w][ocn] tensor.  Both buffers end in 64 more bytes of padding."""
    es = ES[depth]
    it, ot = cvgs.make_type(depth, cn), cvgs.make_type(depth, ocn)
    row, orow = w * cn * es, w * ocn * es
    step, pitch = src_off + row + src_pad, orow + out_pad
    assert out3d or batch == 1

    def build(B, fill=0):
        mats, views, src_padding = [], [], []
        for z in range(batch):
            a = samples(depth, (h, w, cn), seed + 7 * z, finite)
            raw = aligned_bytes(h * step + 64)
            raw[:] = pattern_bytes(raw.size, fill + 3 * z)
            rows2d = raw[:h * step].reshape(h, step)
            rows2d[:, src_off:src_off + row] = a.view(np.uint8).reshape(h, row)
            pad = np.ones(raw.size, bool)
            pad[:h * step].reshape(h, step)[:, src_off:src_off + row] = False
            m = B.src(raw.reshape(1, -1), cvgs.CV_8UC1)
            assert m.data % 256 == 0, "the source buffer itself is aligned: only src_off moves the view"
            mats.append(cvgs.GpuMat(h, w, B.T(it), m.data + src_off, step, owner=m.owner))
            views.append(F.View(a))
            src_padding.append(pad)
        if used is not None:  # planes at or beyond usedPlanes hold the background, whatever their source holds
            for z in range(used, batch):
                views[z] = F.View(np.broadcast_to(np.array(BACKGROUND[:cn], NP[depth]), (h, w, cn)).copy())
        rd = cvgs.ReadIOp(capi.READ_PIXEL, B.T(it), mats, batch if used is None else used, None, cvgs.IGNORE_AR, BACKGROUND)
        if table:  # a resident device table; on a host backend a stand-in in host memory (names only: the oracle runs no tables)
            tb = np.frombuffer(bytearray(cvgs.build_plane_table(rd)), np.uint8)
            rd.dsize = (w, h)  # (a device table states the plane extent)
            if B.device:
                import torch
                t = torch.from_numpy(tb).cuda()
                B.keep.append(t)
                rd.table = t.data_ptr()
            else:
                B.sources.append(tb)
                rd.table = tb.ctypes.data
        rows = batch * h
        nbytes = out_off + (rows - 1) * pitch + orow + 64
        o = B.out((1, nbytes + 256), cvgs.CV_8UC1)
        shift = (-o.data) % 256
        filled = pattern_bytes(nbytes + 256, 7)
        if B.device:
            import torch
            big = B.outs[-1][0]
            big[B.GUARD:B.GUARD + filled.size] = torch.from_numpy(filled).cuda()
        else:
            B.outs[-1][...] = filled.reshape(1, -1)
        ptr = o.data + shift + out_off
        if out3d:
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(batch, h * w, B.T(ot), ptr, h * orow, owner=o), (w, h))
        else:
            wr = cvgs.write(B.T(ot), cvgs.GpuMat(h, w, B.T(ot), ptr, pitch, owner=o))
        B.placed = Placed(shift + out_off, pitch, orow, rows, (batch, h, w, ocn), NP[depth], filled, src_padding)
        return [rd, stage(B.T(it), B.T(ot)), wr], views
    return build


def split_output(placed, whole):
    """(samples [plane][y][x][c], indices of padding bytes that no longer hold their fill) of a whole output buffer read back"""
    whole = np.ascontiguousarray(whole).reshape(-1).view(np.uint8)
    idx = placed.origin + np.arange(placed.rows)[:, None] * placed.pitch + np.arange(placed.row_bytes)[None, :]
    got = whole[idx.reshape(-1)].view(placed.dtype).reshape(placed.shape)
    moved = whole != placed.fill
    moved[idx.reshape(-1)] = False
    return got, np.flatnonzero(moved)


def alpha_value(depth, alpha):
    """the value of ADD_ALPHA's operand in the channel type, None where it has none (see the module docstring)"""
    if depth == F32:
        return alpha
    return float(int(alpha)) if 0.0 <= alpha <= (255.0 if depth == U8 else 65535.0) else None


def compare(case, res, got):
    """(ok, ratio, text) of the output samples against a model Result.  Pure moves: the model's bound is zero and the samples equal its value bit for
    bit (CV_32F by bit pattern, NaN at the same positions); gray: Result.check's own bound."""
    v = res.v
    if case.pure:
        assert (res.b == 0).all(), case.name
        if not case.alpha_defined:  # no value for the alpha channel: one constant, the colour channels exact
            if not (got[..., 3] == got[0, 0, 0, 3]).all():
                return False, np.inf, "the alpha channel is not one constant"
            v, got = v[..., :3], got[..., :3]
        want = v.astype(got.dtype)
        if got.dtype == np.float32:
            gn, wn = np.isnan(got), np.isnan(want)
            same = (gn == wn) & (gn | (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)))
        else:
            same = got == want
        bad = int((~same).sum())
        where = np.unravel_index(int(np.argmin(same)), same.shape) if bad else None
        return bad == 0, 0.0 if bad == 0 else np.inf, "%d of %d elements differ from the model, first at %r" % (bad, same.size, where)
    ok, ratio = res.check(got.astype(np.float64))
    worst = float(np.nanmax(ratio))
    return bool(ok.all()), worst, "%d of %d elements outside the bound, worst ratio %.3f at %r" % (
        int((~ok).sum()), ok.size, worst, np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


def model_of(case, iops, views):
    """the model's answer; an ADD_ALPHA operand enters as its value in the channel type"""
    op, aux, operand = iops[1].ops[0]
    if op == capi.OP_ADD_ALPHA and case.depth != F32:
        a = alpha_value(case.depth, operand[0])
        iops = [iops[0], cvgs.PointwiseIOp(iops[1].in_type, iops[1].out_type, [(op, aux, [0.0 if a is None else a] * 4)]), iops[2]]
    return F.evaluate(iops, views)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def _stage(op, aux, operand=None):
    return lambda it, ot: cvgs.PointwiseIOp(it, ot, [(op, aux, operand)])


def _cvt(code):
    return lambda it, ot: cvgs.cvtColor(code, it, ot)


def add(name, depth, template, cn, ocn, stage, shape, seed, kernel=None, reason=None, layout="dense", gray_order=None, oracle=True, alpha_defined=True, **kw):
    assert name not in CASES, name
    w, h = WIDTHS[depth][shape[0]], shape[1]
    if "w" in kw:
        w = kw.pop("w")
    pure = template == "permute"
    finite = not pure
    generic = GENERIC_TABLE if kw.get("table") else GENERIC
    kernel = kernel if kernel is not None else (FAST[(depth, template)] if reason is None else (generic if kw.get("table") and depth != U8 else FALLBACK[depth]))
    CASES[name] = Case(name, depth, template, kernel, generic, pure, reason, layout, w, h, gray_order, cn, oracle, alpha_defined,
                       colour_case(depth, cn, ocn, stage, w, h, seed, finite, **kw))


_LAYOUT_ARGS = {"dense": {}, "src_pitch": dict(src_off=32, src_pad=48), "out_pitch": dict(out_off=32, out_pad=48),
                "both_pitch": dict(src_off=16, src_pad=16, out_off=16, out_pad=32),
                "batch1": dict(batch=1, out3d=True), "batch2": dict(batch=2, out3d=True), "batch3": dict(batch=3, out3d=True, src_off=16, src_pad=32)}
# an eligible chain in buffers wide enough for one more pixel, so that the neighbour changes nothing but what its name says
_ROOM = dict(src_off=16, src_pad=64, out_off=16, out_pad=64)
_NEIGHBOURS = {"src_base+4": dict(_ROOM, src_off=20, src_pad=60), "src_base+8": dict(_ROOM, src_off=24, src_pad=56), "src_step%16=8": dict(_ROOM, src_pad=72),
               "out_base+8": dict(_ROOM, out_off=24), "out_pitch%16=8": dict(_ROOM, out_pad=72)}

_seed = 1000
for _d in DEPTHS:
    _n = DN[_d]
    # the ten cvtColor codes over the ten shapes, dense
    for _t, _codes in (("permute", PERMUTE_CODES), ("gray", GRAY_CODES)):
        for _i, _shape in enumerate(SHAPES):
            _cname, _code, _cn, _ocn = _codes[_i % len(_codes)]
            _seed += 1
            add("%s_%s_%dx%d" % (_n, _cname, WIDTHS[_d][_shape[0]], _shape[1]), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed)
    # gray orders cvtColor cannot say: the ORD == 0 kernels of CV_8U / CV_16U at every width; CV_32F falls back
    for _i, (_order, _cn) in enumerate(GRAY_ORDERS):
        for _shape in ((SHAPES[_i], SHAPES[_i + 5]) if _d != F32 else (SHAPES[2],)):
            _seed += 1
            add("%s_gray_%d%d%d_c%d_%dx%d" % ((_n,) + _order + (_cn, WIDTHS[_d][_shape[0]], _shape[1])), _d, "gray", _cn, 1, _stage(capi.OP_GRAY, gray_aux(_order)), _shape,
                _seed, reason="gray_order" if _d == F32 else None, gray_order=_order)
    # alphas whose bytes differ (CV_32F: bit patterns)
    _alphas = ALPHAS[_d] if _d != F32 else ALPHAS_F32
    for _i, _a in enumerate(_alphas):
        _seed += 1
        add("%s_add_alpha_%d" % (_n, _i), _d, "permute", 3, 4, _stage(capi.OP_ADD_ALPHA, (ID3, SWAP3)[_i % 2], [_a] * 4), SHAPES[3 + _i], _seed)
    # a third selector order
    _seed += 2
    add("%s_add_alpha_third_order" % _n, _d, "permute", 3, 4, _stage(capi.OP_ADD_ALPHA, THIRD3, [1.0] * 4), SHAPES[2], _seed, reason="selector")
    add("%s_drop_alpha_third_order" % _n, _d, "permute", 4, 3, _stage(capi.OP_DROP_ALPHA, THIRD3), SHAPES[2], _seed + 1, reason="selector")
    # layouts, for each template
    for _t, _codes in (("permute", PERMUTE_CODES), ("gray", GRAY_CODES)):
        for _i, _layout in enumerate(PITCHED_LAYOUTS + BATCH_LAYOUTS):
            _cname, _code, _cn, _ocn = _codes[(_i + 1) % len(_codes)]
            _seed += 1
            add("%s_%s_%s" % (_n, _cname, _layout), _d, _t, _cn, _ocn, _cvt(_code), SHAPES[(3 * _i + 1) % 10], _seed, layout=_layout, **_LAYOUT_ARGS[_layout])
    # ineligible neighbours, for each template: the eligible chain, then one thing changed
    for _t, (_cname, _code, _cn, _ocn) in (("permute", PERMUTE_CODES[3]), ("gray", GRAY_CODES[2])):
        _shape = SHAPES[3]
        _w = WIDTHS[_d][_shape[0]]
        _seed += 1
        add("%s_%s_eligible_base" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, layout="both_pitch", **_ROOM)
        add("%s_%s_width+1" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, reason="width+1", w=_w + 1,
            **dict(_ROOM, src_pad=64 - _cn * ES[_d], out_pad=64 - _ocn * ES[_d]))
        add("%s_%s_width-3" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, reason="width-3", w=_w - 3,
            **dict(_ROOM, src_pad=64 + 3 * _cn * ES[_d], out_pad=64 + 3 * _ocn * ES[_d]))
        for _r, _kw in _NEIGHBOURS.items():
            add("%s_%s_%s" % (_n, _cname, _r), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, reason=_r, **_kw)
        _seed += 1
        add("%s_%s_batch3_base" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, layout="batch3", batch=3, out3d=True)
        add("%s_%s_used2of3" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, reason="used<batch", batch=3, used=2, out3d=True)
        add("%s_%s_device_table" % (_n, _cname), _d, _t, _cn, _ocn, _cvt(_code), _shape, _seed, reason="device_table", batch=3, out3d=True, table=True, oracle=False)
    if _d != F32:  # alphas that are no whole number in range
        for _a in BAD_ALPHAS[_d]:
            _seed += 1
            # (the generic kernel at every depth: pointwise4_u8_u8, whose store saturates, does not take these)
            add("%s_add_alpha_%g" % (_n, _a), _d, "permute", 3, 4, _stage(capi.OP_ADD_ALPHA, ID3, [_a] * 4), SHAPES[3], _seed, kernel=GENERIC, reason="alpha",
                oracle=alpha_value(_d, _a) is not None, alpha_defined=alpha_value(_d, _a) is not None)

FAMILIES = [(d, t) for d in DEPTHS for t in ("permute", "gray")]


def family_name(depth, template):
    return "%s %s" % (DN[depth], template)


def cases_of(depth, template, eligible):
    return [c for c in CASES.values() if c.depth == depth and c.template == template and (c.reason is None) == eligible]
