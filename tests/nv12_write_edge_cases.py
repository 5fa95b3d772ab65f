"""The branches of the CVGS_WRITE_NV12 kernels (csrc/k_nv12_write.hip) that tests/test_gpu_nv12_write.py never executes: aspect-ratio windows,
every read layout, the store's conversion edge, targets inside a larger surface, the remaining source shapes and a mixed tick.  Expected bytes
are always nv12_write_model.write_f32 applied to the CPU oracle's CV_32FC3 picture of the same read and program (the special-value cases: to a
picture written out by hand); every byte of every buffer is compared -- guard bands, row padding, the gap between the planes -- and every case
asserts its kernel name; wherever the fast kernel is dispatched the chain also runs with CHAIN_FORCE_GENERIC.

This module defines NO test item.  all_cases() is ONE table with two users: tests/test_nv12_write_edge_cases.py walks it without a GPU (Ctx
with device None: every chain is lowered over host memory, validated, its dispatch asked as a dry run, its expected picture kept), and
tests/test_zz_gpu_write_nv12_edges.py runs it on the GPU (Ctx with a device: tests/test_gpu_nv12_write.run).

The source is the 96 x 64 NV12 surface of tests/test_gpu_nv12_write.py; every other layout holds THE SAME PICTURE (I420 / YV12: the chroma
de-interleaved; P010: the codes times 4; YUYV / UYVY: every chroma row twice; I444: every chroma sample four times), so a full-resolution
read written back with the read's range and primaries must return the surface: asserted on the model in every such case.  Targets: 34 x 14,
14 x 34, 16 x 8, four 34 x 14 quadrants of one 68 x 28, one 260 x 4.

The cases, and the branch each one executes:
  window <in> ar <mode>            a.  Nv12wCol::take, in_y, the x - P.x1 / y - P.y1 rebasing (fast) and the x >= P.x1 && ... branch (interpreted):
                                       7 crops -> 34 x 14 (pillarbox) and 14 x 34 (letterbox); NV12 and NV21 in; the three PRESERVE_AR modes
  window across column 256         a.  260 x 4: a window of columns 2..257 -- both 256-column tiles of the fast kernel hold picture and background
  window, default-value plane      a.  used_planes < batch beside windowed planes: `live` false in both kernels
  window behind a program          a.  the interpreted kernel: the background goes through the program
  window, 8UC3 crops               a.  load_px taps behind the window test; a 97 x 1 crop into 260 x 4 (rows 0..2 of 4: a block half background)
  device table with a window       b.  NPL == 0 (r.table) with PRESERVE_AR entries written on the device, an empty box: both kernels
  <layout> full resolution         c.  nv12_px's branch of the layout behind !r.is_resize; P010 behind multiply(0.25)
  <layout> resized                 c.  nv12_px's branch of the layout under nv12w_read_tap (crops where the layout has them; I444 with alpha dropped)
  store conversion <range>         d.  nv12w_u8: ties to even, saturation on both sides, -0, +-inf, NaN, +-3e9 in Y and in the chroma mean
  four quadrants of one surface    e.  nv12_roi targets; nv12w_u32u / nv12w_u16u at a base = 2 (mod 4); neighbours untouched: both kernels
  odd step, odd base               e.  every store of both kernels at odd addresses
  70 windowed planes               e.  the staged table (source and target descriptors) with windows
  8UC4 crops, BGRA2RGB             f.  r.cn == 4 taps, alpha dropped by the program
  CV_16F / CV_16BF per-pixel       f.  load_px at depth 16F / 16BF with depth0 = r.depth in front of the program's cast
  8UC3 device table                f.  a pixel-frame table chain, as dispatched and forced generic
  mixed tick                       g.  cvgs_execute_many: a windowed write chain, a K1 tensor chain, a second write chain
An 8UC1 source through GRAY2RGB is NOT here: the engine has no stage that makes three channels of one (cvtColor refuses COLOR_GRAY2BGR,
tests/test_abi.py pins that), so no chain leads from CV_8UC1 to the CV_32FC3 value the write takes.
An NV12 crop of the 96-wide surface cannot fill 260 columns (its window is at most 4 / 2 * 96 = 192 wide), so the 260 x 4 case reads the same
bytes as a 192 x 32 surface: a 128 x 2 crop of it gives the window 2..257."""
import ctypes as C
import struct

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import nv12_write_model as M
from tests import test_gpu_nv12_write as W
from tests import yuv422_cases as Y422
from tests import yuv444_cases as Y444
from tests.test_p010 import p010_surface

F3, F4 = cvgs.CV_32FC3, cvgs.CV_32FC4
FAST, INTERP = "nv12w_nv12_resize", "nv12w_interp"
ARS = {"PRESERVE_AR": cvgs.PRESERVE_AR, "PRESERVE_AR_RN_EVEN": cvgs.PRESERVE_AR_RN_EVEN, "PRESERVE_AR_LEFT": cvgs.PRESERVE_AR_LEFT}
BG = [200.0, 30.0, 90.0, 0.0]   # a non-zero three-channel background
CROPS = W.CROPS                  # 7 even crops of the 96 x 64 surface, a 2 x 2 one among them
PILLAR, LETTER = (34, 14), (14, 34)
REGION = (10, 2, 34, 14)         # the part of the picture the full-resolution reads take
CROPS3 = [(0, 0, 97, 61), (11, 13, 38, 19), (56, 38, 41, 23), (3, 5, 10, 6), (60, 1, 17, 50)]  # of the 97 x 61 pixel frames
LAYOUTS = {"NV21": capi.YUV_NV21, "I420": capi.YUV_I420, "YV12": capi.YUV_YV12, "P010": capi.YUV_P010, "YUYV": capi.YUV_YUYV,
           "UYVY": capi.YUV_UYVY, "I444": capi.YUV_I444}
N_CASES = 34


class Ctx:
    """Where a case runs.  device set: on the GPU, through W.run.  device None: dry -- the chain over host memory is lowered and validated,
    the dispatch answers its kernel name, and the expected picture is kept in `log` for the CPU test."""

    def __init__(self, device, lib, oracle):
        self.device, self.lib, self.oracle, self.dry, self.log = device, lib, oracle, device is None, []

    def surface(self, w, h, gap=0, step=None, lead=0):
        return W.Surface("cpu" if self.dry else self.device, w, h, gap, step, lead)

    def run(self, what, make_read, mid, dsize, batch, out=(M.FULL, M.BT709, M.NV12), gap=0, kernel=None, rgb=None, make_outs=None, windowed=False):
        """W.run's arguments; `kernel` is mandatory.  The fast kernel never runs alone."""
        assert kernel in (FAST, INTERP)
        both = kernel == FAST
        if not self.dry:
            return W.run(self.device, self.oracle, what, make_read, mid, dsize, batch, out, gap, kernel, both, rgb, make_outs)
        if rgb is None:
            rgb = W.oracle_rgb(self.oracle, make_read(False), mid, dsize, batch)
        want = [M.write_f32(rgb[z], *out) for z in range(batch)]
        mats = make_outs()[0] if make_outs else [self.surface(dsize[0], dsize[1], gap).mat for _ in range(batch)]
        for flags in ((0, capi.CHAIN_FORCE_GENERIC) if both else (0,)):
            self.lowers(what, [make_read(False)] + list(mid) + [cvgs.write_nv12(mats, *out)], INTERP if flags else kernel, flags)
        self.log.append({"what": what, "kernel": kernel, "rgb": np.array(rgb), "out": out, "windowed": windowed})
        return want

    def lowers(self, what, ops, kernel, flags=0):
        low = cvgs.lower(ops, flags)
        assert self.lib.cvgs_validate(C.byref(low.desc)) == capi.OK, (what, self.lib.cvgs_last_error().decode())
        name = cvgs.kernel_name(*ops, flags=flags)
        assert name == kernel, (what, flags, name)
        return low


# ---- the sources: one picture in every layout ----------------------------------------------------------------------------------------------------
_sources = {}


def _device_twin(device, hm, host):
    """The view `hm` of the host array, over a copy of the array on the device (None without a device)."""
    if device is None:
        return None
    import torch
    flat = host.reshape(-1).view(np.uint8)
    t = torch.from_numpy(flat).to(device)
    dm = cvgs.GpuMat(hm.rows, hm.cols, hm.cv_type, t.data_ptr() + (hm.data - flat.ctypes.data), hm.step, owner=t)
    if getattr(hm, "uv_offset", 0):
        dm.uv_offset = hm.uv_offset
    return dm


def planes_of_the_picture():
    host = W.frame(None, "NV12")[0]
    return host[:W.SH], np.ascontiguousarray(host[W.SH:, 0::2]), np.ascontiguousarray(host[W.SH:, 1::2])


def planar_420(y, u, v, first_v):
    h, w = y.shape
    a, b = (v, u) if first_v else (u, v)
    return np.concatenate([y.reshape(-1), a.reshape(-1), b.reshape(-1)]).reshape(h * 3 // 2, w)


def source(device, name):
    """(host object, host GpuMat, device GpuMat or None) of a source; made once per device."""
    if name in ("NV12", "NV21", "8UC3", "16UC3", "32FC3"):  # (NV21: the same bytes, the chroma pairs read the other way round)
        return W.frame(device, "NV12" if name == "NV21" else name)
    key = (name, str(device))
    if key in _sources:
        return _sources[key]
    y, u, v = planes_of_the_picture()
    rx, ry, rw, rh = REGION
    rng = np.random.RandomState(33)
    wrap = lambda a, rows, cols, t: cvgs.GpuMat(rows, cols, t, a.ctypes.data, a.strides[0], owner=a)
    if name == "WIDE":  # the NV12 surface's bytes as a 192 x 32 surface
        host = np.ascontiguousarray(W.frame(None, "NV12")[0]).reshape(48, 192)
        hm = wrap(host, 32, 192, cvgs.CV_8UC1)
    elif name in ("I420", "YV12"):
        host = planar_420(y, u, v, name == "YV12")
        hm = wrap(host, W.SH, W.SW, cvgs.CV_8UC1)
    elif name in ("I420_REGION", "YV12_REGION"):  # planar chroma has no crops: the region as a surface of its own
        host = planar_420(np.ascontiguousarray(y[ry:ry + rh, rx:rx + rw]), np.ascontiguousarray(u[ry // 2:(ry + rh) // 2, rx // 2:(rx + rw) // 2]),
                          np.ascontiguousarray(v[ry // 2:(ry + rh) // 2, rx // 2:(rx + rw) // 2]), name == "YV12_REGION")
        hm = wrap(host, rh, rw, cvgs.CV_8UC1)
    elif name == "P010":
        host = p010_surface(W.SW, W.SH, 0, codes=(y.astype(np.uint16) * 4, u.astype(np.uint16) * 4, v.astype(np.uint16) * 4))[0]
        hm = wrap(host, W.SH, W.SW, cvgs.CV_16UC1)
    elif name in ("YUYV", "UYVY"):
        host = Y422.pack(y, np.repeat(u, 2, 0), np.repeat(v, 2, 0), LAYOUTS[name])
        hm = Y422.wrap_array(host)
    elif name == "I444":
        surf = Y444.Surf(W.SW, W.SH, 0, planes=(y, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1)))
        _sources[key] = (surf, Y444.wrap_array(surf), _device_twin(device, Y444.wrap_array(surf), surf.buf))
        return _sources[key]
    elif name == "8UC4":
        host = rng.randint(0, 256, (61, 97 * 4)).astype(np.uint8)
        hm = wrap(host, 61, 97, cvgs.CV_8UC4)
    elif name == "16FC3":  # 0..255 in steps the half format holds
        host = (rng.rand(14, 34 * 3) * 255.0).astype(np.float16).view(np.uint16)
        hm = wrap(host, 14, 34, cvgs.CV_16FC3)
    elif name == "16BFC3":  # bfloat16: the high half of a float32
        host = ((rng.rand(14, 34 * 3) * 255.0).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        hm = wrap(host, 14, 34, cvgs.CV_16BFC3)
    else:
        raise KeyError(name)
    _sources[key] = (host, hm, _device_twin(device, hm, host))
    return _sources[key]


def mats_of(ctx, name):
    """pick(on_device) -> the source's GpuMat"""
    _, hm, dm = source(ctx.device, name)
    return lambda dev: dm if dev else hm


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
def windows(rd):
    """[(x1, y1, x2, y2)] of a read's planes, from the library's plane geometry."""
    raw = cvgs.build_plane_table(rd)
    return [struct.unpack_from("<QiiiffiiiiI", raw, 48 * z)[6:10] for z in range(rd.batch)]


def window_read(mat, crops, dsize, ar, layout=capi.YUV_NV12, rng=M.LIMITED, prim=M.BT601, used=None, bg=BG):
    rd = W.nv12_read([mat.nv12_roi(*c) for c in crops], dsize, rng, prim, layout, used, bg)
    rd.ar = ar
    return rd


def window_set():
    """{(mode, dsize): windows} of the 7 crops: what the window cases run, for the geometry assertions."""
    hm = W.frame(None, "NV12")[1]
    return {(mode, d): windows(window_read(hm, CROPS, d, ar)) for mode, ar in ARS.items() for d in (PILLAR, LETTER)}


def assert_window_coverage(ws):
    """The conditions the issue sets on the set of windows."""
    flat = [(w, d) for (_, d), lst in ws.items() for w in lst]
    assert any(w[0] & 1 for w, _ in flat) and any(w[0] > 0 and not w[0] & 1 for w, _ in flat), "odd and even x1"
    assert any(w[1] & 1 for w, _ in flat), "odd y1"
    assert any(w[2] & 1 and w[2] < d[0] - 1 for w, d in flat), "an odd last column inside the surface"
    assert {w[0] % 4 for w, _ in flat if w[0] > 0} >= {1, 2, 3}, "a left edge strictly inside a lane's 4 columns, every remainder"
    assert any(w[0] > 0 for w, d in flat if d == PILLAR) and any(w[1] > 0 for w, d in flat if d == LETTER), "pillarbox and letterbox"
    assert all(0 <= w[0] <= w[2] < d[0] and 0 <= w[1] <= w[3] < d[1] for w, d in flat)


# ---- a. windows ------------------------------------------------------------------------------------------------------------------------------
def case_window(ctx, layout_in, mode, out):
    pick = mats_of(ctx, "NV12")
    for d in (PILLAR, LETTER):
        mk = lambda dev: window_read(pick(dev), CROPS, d, ARS[mode], layout_in)
        ws = windows(mk(False))
        assert any(w != (0, 0, d[0] - 1, d[1] - 1) for w in ws)
        ctx.run("window layout %d %s -> %dx%d" % (layout_in, mode, d[0], d[1]), mk, [], d, len(CROPS), out, kernel=FAST, windowed=True)


def case_window_across_256(ctx):
    pick = mats_of(ctx, "WIDE")
    crops = [(10, 4, 128, 2), (0, 0, 192, 32)]
    mk = lambda dev: window_read(pick(dev), crops, (260, 4), cvgs.PRESERVE_AR)
    ws = windows(mk(False))
    assert ws[0] == (2, 0, 257, 3) and ws[1][0] > 0 and ws[1][2] < 256, ws  # one window across column 256, one inside the first tile
    ctx.run("window across column 256", mk, [], (260, 4), 2, (M.LIMITED, M.BT709, M.NV12), kernel=FAST, windowed=True)


def case_window_default_plane(ctx):
    pick = mats_of(ctx, "NV12")
    mk = lambda dev: window_read(pick(dev), CROPS[:3], PILLAR, cvgs.PRESERVE_AR, used=2)
    want = ctx.run("window, default-value plane", mk, [], PILLAR, 3, (M.FULL, M.BT601, M.NV21), kernel=FAST, windowed=True)
    l, c = M.write_f32(np.broadcast_to(np.array(BG[:3], np.float32), (14, 34, 3)), M.FULL, M.BT601, M.NV21)
    assert (want[2][0] == l).all() and (want[2][1] == c).all()
    assert (want[0][0][:, :6] == l[:, :6]).all() and not (want[0][0] == l).all()  # the bars of a windowed plane are that value too


def case_window_program(ctx):
    pick = mats_of(ctx, "NV12")
    mid = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, F3), cvgs.multiply(F3, [0.5, 1.0, 1.25]), cvgs.add(F3, [-12.5, 3.0, 20.0])]
    for d in (PILLAR, LETTER):
        mk = lambda dev: window_read(pick(dev), CROPS, d, cvgs.PRESERVE_AR, used=6)
        want = ctx.run("window behind a program -> %dx%d" % d, mk, mid, d, len(CROPS), (M.LIMITED, M.BT2020, M.NV12), kernel=INTERP, windowed=True)
        through = np.array([BG[2] * 0.5 - 12.5, BG[1] + 3.0, BG[0] * 1.25 + 20.0], np.float32)  # the background, swapped, scaled, shifted
        l, c = M.write_f32(np.broadcast_to(through, (d[1], d[0], 3)), M.LIMITED, M.BT2020)
        assert (want[6][0] == l).all() and (want[6][1] == c).all()


def case_window_8uc3(ctx):
    pick = mats_of(ctx, "8UC3")
    for d in (PILLAR, LETTER):
        for mode in ("PRESERVE_AR", "PRESERVE_AR_RN_EVEN"):
            mk = lambda dev: cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [pick(dev).roi(*c) for c in CROPS3], d, None, BG, ARS[mode])
            assert any(w[0] & 1 or w[1] & 1 for w in windows(mk(False)))
            ctx.run("window, 8UC3 crops %s -> %dx%d" % (mode, d[0], d[1]), mk, [], d, len(CROPS3), (M.FULL, M.BT709, M.NV12), kernel=INTERP, windowed=True)
    mk = lambda dev: cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [pick(dev).roi(0, 7, 97, 1)], (260, 4), None, BG, cvgs.PRESERVE_AR)
    assert windows(mk(False)) == [(0, 0, 259, 2)]
    ctx.run("window, 8UC3 97 x 1 -> 260x4", mk, [], (260, 4), 1, (M.LIMITED, M.BT601, M.NV21), kernel=INTERP, windowed=True)


# ---- b. / f. device tables -------------------------------------------------------------------------------------------------------------------
def _box_table(ctx, frame_mat, rects, dsize, ar, kind):
    """(table, rects the builder reports): written by cvgs_plane_tables_from_boxes on the device; dry: a host buffer nobody reads, and the
    boxes themselves (they lie inside the frame, 4:2:0 ones at even coordinates)."""
    if ctx.dry:
        buf = np.zeros((len(rects), 48), np.uint8)
        return buf.ctypes.data, np.array(rects, np.int32), buf
    import torch
    boxes = torch.tensor(rects, dtype=torch.int32, device=ctx.device)
    table = torch.zeros((len(rects), 48), dtype=torch.uint8, device=ctx.device)
    rects_out = torch.zeros((len(rects), 4), dtype=torch.int32, device=ctx.device)
    cvgs.plane_tables_from_boxes(torch.cuda.current_stream(), [cvgs.box_table_desc(frame_mat, boxes, table, len(rects), dsize, ar, cvgs.BOX_XYWH_I32, None,
                                                                                   rects_out, kind)])
    torch.cuda.synchronize()
    return table, rects_out.cpu().numpy(), (boxes, table)


def case_device_table_window(ctx):
    _, hm, dm = source(ctx.device, "NV12")
    rects = [(0, 0, 96, 64), (2, 4, 40, 30), (6, 8, 0, 10), (50, 20, 46, 44), (0, 32, 96, 32)]  # XYWH, even; the third is empty: invalid
    valid = [0, 1, 3, 4]
    yuv = (M.LIMITED, M.BT601, 0)
    for d in (PILLAR, LETTER):
        table, got, keep = _box_table(ctx, hm if ctx.dry else dm, rects, d, cvgs.PRESERVE_AR, capi.READ_NV12_RESIZE_LINEAR)
        for i in valid:
            assert tuple(got[i]) == rects[i], (i, got[i])
        views = [tuple(int(v) for v in got[i]) for i in valid]  # the oracle reads the rectangles the builder reports
        rgb4 = W.oracle_rgb(ctx.oracle, window_read(hm, views, d, cvgs.PRESERVE_AR), [], d, len(valid))
        rgb = np.stack([rgb4[0], rgb4[1], np.broadcast_to(np.array(BG[:3], np.float32), (d[1], d[0], 3)), rgb4[2], rgb4[3]])
        assert any(w != (0, 0, d[0] - 1, d[1] - 1) for w in windows(window_read(hm, views, d, cvgs.PRESERVE_AR)))
        mk = lambda dev: cvgs.resize_boxes(dm if dev else hm, table, len(rects), d, BG, cvgs.PRESERVE_AR, yuv=yuv)
        ctx.run("device table with a window -> %dx%d" % d, mk, [], d, len(rects), (M.FULL, M.BT709, M.NV12), kernel=FAST, rgb=rgb, windowed=True)
        del keep


def case_device_table_8uc3(ctx):
    _, hm, dm = source(ctx.device, "8UC3")
    rects = [CROPS3[1], CROPS3[2], (5, 5, 0, 0), CROPS3[4]]
    valid = [0, 1, 3]
    table, got, keep = _box_table(ctx, hm if ctx.dry else dm, rects, PILLAR, cvgs.PRESERVE_AR, capi.READ_RESIZE_LINEAR)
    for i in valid:
        assert tuple(got[i]) == rects[i], (i, got[i])
    rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [hm.roi(*(int(v) for v in got[i])) for i in valid], PILLAR, None, BG, cvgs.PRESERVE_AR)
    rgb3 = W.oracle_rgb(ctx.oracle, rd, [], PILLAR, 3)
    rgb = np.stack([rgb3[0], rgb3[1], np.broadcast_to(np.array(BG[:3], np.float32), (14, 34, 3)), rgb3[2]])
    mk = lambda dev: cvgs.resize_boxes(dm if dev else hm, table, len(rects), PILLAR, BG, cvgs.PRESERVE_AR)
    for flags in (0, capi.CHAIN_FORCE_GENERIC):  # as dispatched and forced generic: the interpreted kernel both times
        if ctx.dry:
            ctx.lowers("8UC3 device table", [mk(False), cvgs.write_nv12([ctx.surface(34, 14).mat for _ in rects])], INTERP, flags)
            continue
        import torch
        outs = [ctx.surface(34, 14) for _ in rects]
        ops = [mk(True), cvgs.write_nv12([o.mat for o in outs], M.LIMITED, M.BT709, M.NV12)]
        assert cvgs.kernel_name(*ops, flags=flags) == INTERP
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
        torch.cuda.synchronize()
        for z, o in enumerate(outs):
            o.check(*M.write_f32(rgb[z], M.LIMITED, M.BT709, M.NV12), "8UC3 device table, plane %d, flags %d" % (z, flags))
    if ctx.dry:
        ctx.log.append({"what": "8UC3 device table", "kernel": INTERP, "rgb": rgb, "out": (M.LIMITED, M.BT709, M.NV12), "windowed": True})
    del keep


# ---- c. every layout -------------------------------------------------------------------------------------------------------------------------
def _view(m, name, rect):
    if name in ("YUYV", "UYVY"):
        return m.yuv422_roi(*rect)
    if name == "I444":
        return m.yuv444_roi(*rect)
    return m.nv12_roi(*rect)


def _composed_rgb(ctx, name, read, mid, dsize, batch):
    """The oracle knows the 4:2:0 layouts: a 4:2:2 / 4:4:4 read is composed of two of its runs (tests/yuv422_cases.py, tests/yuv444_cases.py)."""
    if name not in ("YUYV", "UYVY", "I444"):
        return None
    w, h = dsize
    ref = np.zeros((batch, h * w * 3), np.float32)
    ops = [read] + list(mid) + [cvgs.write(F3, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (w, h))]
    host = source(None, name)[0]
    (Y444.Expect(ctx.oracle, [host]) if name == "I444" else Y422.Expect(ctx.oracle, [host], LAYOUTS[name])).run(ops)
    return ref.reshape(batch, h, w, 3)


def case_layout_full(ctx, name, rng, prim):
    """The region of the picture read at full resolution in `name` and written with the same range and primaries: the NV12 surface's region."""
    planar = name in ("I420", "YV12")
    src = name + "_REGION" if planar else name
    host_mat = source(None, src)[1]
    pick = mats_of(ctx, src)
    view = (lambda m: m) if planar else (lambda m: _view(m, name, REGION))
    mid = [cvgs.multiply(F3, [0.25] * 3)] if name == "P010" else []
    lay_out = M.NV21 if name == "NV21" else M.NV12
    mk = lambda dev: cvgs.read_nv12(view(pick(dev)), None, rng, prim, alpha=False, layout=LAYOUTS[name])
    rgb = _composed_rgb(ctx, name, cvgs.read_nv12(view(host_mat), None, rng, prim, alpha=False, layout=LAYOUTS[name]), mid, PILLAR, 1)
    want = ctx.run("%s full resolution" % name, mk, mid, PILLAR, 1, (rng, prim, lay_out), kernel=INTERP, rgb=rgb)
    host = W.frame(None, "NV12")[0]
    x, y, w, h = REGION
    assert (want[0][0] == host[y:y + h, x:x + w]).all() and (want[0][1] == host[W.SH + y // 2:W.SH + (y + h) // 2, x:x + w]).all(), \
        "%s: the restatement does not return the surface" % name


def case_layout_resized(ctx, name, rng, prim, out):
    planar = name in ("I420", "YV12")
    alpha = name == "I444"  # alpha=True with RGBA2RGB once
    pick = mats_of(ctx, name)
    hm = source(None, name)[1]
    crops = [(0, 0, 96, 64)] if planar else [(0, 0, 96, 64), (2, 4, 40, 30), (50, 20, 46, 44)]
    views = (lambda m: [m]) if planar else (lambda m: [_view(m, name, c) for c in crops])
    mid = ([cvgs.cvtColor(cvgs.COLOR_RGBA2RGB, F4, F3)] if alpha else []) + ([cvgs.multiply(F3, [0.25] * 3)] if name == "P010" else [])
    mk = lambda dev: cvgs.read_nv12(views(pick(dev)), PILLAR, rng, prim, alpha=alpha, layout=LAYOUTS[name])
    rgb = _composed_rgb(ctx, name, cvgs.read_nv12(views(hm), PILLAR, rng, prim, alpha=alpha, layout=LAYOUTS[name]), mid, PILLAR, len(crops))
    if name == "NV21":  # (without a program this chain is the fast kernel's, which the window cases run)
        mid = [cvgs.multiply(F3, [1.0, 0.5, 1.0])]
    ctx.run("%s resized" % name, mk, mid, PILLAR, len(crops), out, kernel=INTERP, rgb=rgb)


# ---- d. the store's conversion ----------------------------------------------------------------------------------------------------------------
def _solve(f, lo, hi, target):
    """The float32 t in [lo, hi] with f(t) == target, f non-decreasing: bisection for the smallest t with f(t) >= target."""
    lo, hi = np.float32(lo), np.float32(hi)
    assert f(lo) < target <= f(hi), (f(lo), target, f(hi))
    while True:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2.0)
        if mid == lo or mid == hi:
            break
        if f(mid) >= target:
            hi = mid
        else:
            lo = mid
    assert f(hi) == target, (target, f(hi))
    return hi


def special_picture(rng, prim):
    """([8, 16, 3] float32 picture of 8 x 4 blocks, [(plane, row, column, check)]): pixels solved in fp32 with the model's functions so that
    Y (a pixel) or the U / V mean (a block) lands on the value `check` describes.  plane 0: Y[row][column]; 1, 2: the U / V mean of block
    [row][column].  check is a float32 to hit exactly (sign included), or one of "neg", "big", "+inf", "-inf", "nan", ">2^31", "<-2^31"."""
    f = np.float32
    state = np.random.RandomState(7)
    pic = (state.rand(8, 16, 3) * 200.0 + 20.0).astype(np.float32)
    sc = M.SC if rng == M.LIMITED else 1.0
    sy = M.SY if rng == M.LIMITED else 1.0
    y0 = 16.0 if rng == M.LIMITED else 0.0
    checks = []
    ties = lambda ks: [t for k in ks for t in (np.nextafter(f(k + 0.5), f(-1e9)), f(k + 0.5), np.nextafter(f(k + 0.5), f(1e9)))]

    def y_of(px):
        return M.yuv_f32(np.array(px, np.float32).reshape(1, 1, 3), rng, prim)[0][0, 0]

    def mean_of(block, plane):
        return M.block_mean_f32(M.yuv_f32(block, rng, prim)[plane])[0, 0]

    # Y: one pixel per target, R = G = g, B solved (the weight of B is the smallest: every float32 near the target is reached)
    y_targets = ties((0, 1, 100, 101, 254, 255) if rng == M.FULL else (16, 17, 100, 101, 234, 235))
    pixels = [(r, c) for r in range(0, 2) for c in range(16)]  # the top two rows: blocks [0][0..7]
    for (r, c), t in zip(pixels, y_targets):
        g = (float(t) - y0) / sy
        b = _solve(lambda v: y_of([g, g, v]), g - 40.0, g + 40.0, t)
        pic[r, c] = [g, g, b]
        checks.append((0, r, c, t))
    rest = pixels[len(y_targets):]
    plain = [("neg", [-100.0, -90.5, -120.0]), ("big", [300.0, 290.5, 310.0]), (">2^31", [3e9, 3e9, 3e9]), ("<-2^31", [-3e9, -3e9, -3e9])]
    if rng == M.FULL:
        plain.append((f(-0.0), [-0.0, -0.0, -0.0]))
    for (r, c), (check, px) in zip(rest, plain):
        pic[r, c] = px
        checks.append((0, r, c, check))
    # the chroma means: blocks of rows 1..3; three pixels fixed around the target, the fourth solved (U: B varies, V: R varies)
    blocks = [(r, c) for r in range(1, 4) for c in range(8)]
    todo = [(1, t) for t in ties((100, 101, 254))] + [(2, t) for t in ties((100, 101))]
    for (br, bc), (plane, t) in zip(blocks, todo):
        d = 2.0 * (float(t) - 128.0) / sc   # (c, c, c + d): U = 128 + sc * d / 2; (c + d, c, c): V likewise
        base = 128.0 - d / 2.0
        blk = np.zeros((2, 2, 3), np.float32)
        for i, off in enumerate((3.1, -5.7, 2.2, 0.0)):
            px = [base, base, base]
            px[2 if plane == 1 else 0] = base + d + off
            blk[i // 2, i % 2] = px
        ch = 2 if plane == 1 else 0

        def mean_with(v, blk=blk, ch=ch, plane=plane):
            b2 = blk.copy()
            b2[1, 1, ch] = v
            return mean_of(b2, plane)
        blk[1, 1, ch] = _solve(mean_with, base + d - 60.0, base + d + 60.0, t)
        pic[2 * br:2 * br + 2, 2 * bc:2 * bc + 2] = blk
        checks.append((plane, br, bc, t))
    # (pixels of the block, value, [(plane, check)]): saturation fills the block, the non-finite and the huge values sit in single pixels
    every, big = [(0, 0), (0, 1), (1, 0), (1, 1)], 4e10
    special = [(every, [255.0, 255.0, -200.0], [(1, "neg")]), (every, [0.0, 0.0, 400.0], [(1, "big")]), (every, [-200.0, 255.0, 255.0], [(2, "neg")]),
               (every, [400.0, 0.0, 0.0], [(2, "big")]),
               ([(0, 1)], [np.inf, 10.0, 20.0], [(1, "-inf"), (2, "nan")]),   # R = +inf: Y = +inf, U = -inf, V = NaN
               ([(1, 0)], [10.0, 20.0, -np.inf], [(1, "nan"), (2, "+inf")]),  # B = -inf: Y = -inf, U = NaN, V = +inf
               ([(1, 1)], [10.0, np.nan, 20.0], [(1, "nan"), (2, "nan")]),    # G = NaN: everything NaN
               ([(0, 0)], [0.0, 0.0, big], [(1, ">2^31"), (2, ">2^31")]),     # (with the next line: two pixels of one block)
               ([(1, 1)], [0.0, 0.0, -big], [(1, "<-2^31"), (2, "<-2^31")])]
    for (br, bc), (where, val, found) in zip(blocks[len(todo):], special):
        for py, px in where:
            pic[2 * br + py, 2 * bc + px] = val
        if abs(val[2]) == big:
            pic[2 * br + 1 - where[0][0], 2 * bc + where[0][1]] = [val[2], 0.0, 0.0]
        checks += [(plane, br, bc, check) for plane, check in found]
    assert len(todo) + len(special) <= len(blocks) and len(y_targets) + len(plain) <= len(pixels)
    return pic, checks


def assert_special_picture(pic, checks, rng, prim):
    """On the CPU, with the model's functions: the picture really produces the stated floats.  Returns how many were checked."""
    Y, U, V = M.yuv_f32(pic, rng, prim)
    planes = (Y, M.block_mean_f32(U), M.block_mean_f32(V))
    for plane, r, c, check in checks:
        v = planes[plane][r, c]
        ok = {"neg": lambda: v < 0 and v > -2.0 ** 31, "big": lambda: 255.5 < v < 2.0 ** 31, "+inf": lambda: v == np.inf, "-inf": lambda: v == -np.inf,
              "nan": lambda: np.isnan(v), ">2^31": lambda: np.isfinite(v) and v > 2.0 ** 31, "<-2^31": lambda: np.isfinite(v) and v < -2.0 ** 31}
        if isinstance(check, str):
            assert ok[check](), (plane, r, c, check, v)
        else:
            assert v == check and np.signbit(v) == np.signbit(check) and v.dtype == np.float32, (plane, r, c, check, v)
    return len(checks)


_special = {}


def case_store_conversion(ctx, rng, prim, layout):
    if (rng, prim) not in _special:
        _special[(rng, prim)] = special_picture(rng, prim)
    pic, checks = _special[(rng, prim)]
    assert assert_special_picture(pic, checks, rng, prim) >= 40
    key = ("special", rng, prim, str(ctx.device))
    if key not in _sources:
        hm = cvgs.GpuMat(8, 16, F3, pic.ctypes.data, pic.strides[0], owner=pic)
        _sources[key] = (hm, _device_twin(ctx.device, hm, pic))
    hm, dm = _sources[key]
    mk = lambda dev: cvgs.ReadIOp(capi.READ_PIXEL, F3, [dm if dev else hm], 1)
    with np.errstate(all="ignore"):
        want = ctx.run("store conversion range %d" % rng, mk, [], (16, 8), 1, (rng, prim, layout), kernel=INTERP, rgb=pic[None])
    luma = want[0][0]
    for plane, r, c, check in checks:  # the bytes the rule gives for the stated floats
        if plane == 0 and not isinstance(check, str):
            k = float(check) - 0.5
            byte = int(np.clip(np.rint(np.float64(check)), 0, 255))
            assert luma[r, c] == byte, (r, c, check, luma[r, c])
            if k == int(k) and 0 <= k < 255:
                assert luma[r, c] == (k if int(k) % 2 == 0 else k + 1)  # the tie itself goes to the even code


# ---- e. placement ----------------------------------------------------------------------------------------------------------------------------
def case_quadrants(ctx):
    pick = mats_of(ctx, "NV12")
    origins = [(0, 0), (34, 0), (0, 14), (34, 14)]
    mk = lambda dev: window_read(pick(dev), CROPS[:4], PILLAR, cvgs.PRESERVE_AR)

    def make_outs():
        parent = ctx.surface(68, 28)
        mats = [parent.mat.nv12_roi(x, y, 34, 14) for x, y in origins]
        assert [m.data % 4 for m in mats] == [0, 2, 0, 2] and all(m.step == 92 for m in mats)

        def check(want, label):
            luma = np.block([[want[0][0], want[1][0]], [want[2][0], want[3][0]]])
            chroma = np.block([[want[0][1], want[1][1]], [want[2][1], want[3][1]]])
            parent.check(luma, chroma, label)
        return mats, check
    ctx.run("four quadrants of one surface", mk, [], PILLAR, 4, (M.LIMITED, M.BT709, M.NV12), kernel=FAST, make_outs=make_outs, windowed=True)
    mid = [cvgs.multiply(F3, [1.0, 0.75, 1.0])]
    ctx.run("four quadrants of one surface, interpreted", mk, mid, PILLAR, 4, (M.FULL, M.BT601, M.NV21), kernel=INTERP, make_outs=make_outs)


def case_odd_step(ctx):
    pick = mats_of(ctx, "NV12")
    mk = lambda dev: window_read(pick(dev), [CROPS[1]], PILLAR, cvgs.PRESERVE_AR)

    def make_outs():
        s = ctx.surface(34, 14, step=47, lead=1)
        assert s.mat.data % 2 == 1 and s.mat.step % 2 == 1
        return [s.mat], lambda want, label: s.check(want[0][0], want[0][1], label)
    ctx.run("odd step, odd base", mk, [], PILLAR, 1, (M.LIMITED, M.BT601, M.NV12), kernel=FAST, make_outs=make_outs, windowed=True)
    mk = lambda dev: window_read(pick(dev), [CROPS[6]], LETTER, cvgs.PRESERVE_AR_RN_EVEN)

    def make_outs2():
        s = ctx.surface(14, 34, step=15, lead=1)
        return [s.mat], lambda want, label: s.check(want[0][0], want[0][1], label)
    ctx.run("odd step, odd base, 14x34", mk, [], LETTER, 1, (M.FULL, M.BT709, M.NV21), kernel=FAST, make_outs=make_outs2, windowed=True)


def case_batch_70_windows(ctx):
    pick = mats_of(ctx, "NV12")
    crops = [CROPS[i % len(CROPS)] for i in range(70)]
    mk = lambda dev: window_read(pick(dev), crops, PILLAR, cvgs.PRESERVE_AR)
    ctx.run("70 windowed planes", mk, [], PILLAR, 70, (M.LIMITED, M.BT709, M.NV12), kernel=FAST, windowed=True)


# ---- f. other sources ------------------------------------------------------------------------------------------------------------------------
def case_8uc4(ctx):
    pick = mats_of(ctx, "8UC4")
    mk = lambda dev: cvgs.resize(cvgs.CV_8UC4, cvgs.INTER_LINEAR, [pick(dev).roi(*c) for c in CROPS3], PILLAR)
    ctx.run("8UC4 crops, BGRA2RGB", mk, [cvgs.cvtColor(cvgs.COLOR_BGRA2RGB, F4, F3)], PILLAR, len(CROPS3), (M.LIMITED, M.BT601, M.NV12), kernel=INTERP)


def case_half_sources(ctx):
    for name, t in (("16FC3", cvgs.CV_16FC3), ("16BFC3", cvgs.CV_16BFC3)):
        pick = mats_of(ctx, name)
        mk = lambda dev: cvgs.ReadIOp(capi.READ_PIXEL, t, [pick(dev)], 1)
        rgb = None
        if name == "16BFC3":  # the oracle knows nothing of bf16 (tests/test_gpu_bf16.py): it reads the source's exact widening, its fp32 twin
            wide = (source(None, name)[0].astype(np.uint32) << 16).view(np.float32)
            rgb = W.oracle_rgb(ctx.oracle, cvgs.ReadIOp(capi.READ_PIXEL, F3, [cvgs.GpuMat(14, 34, F3, wide.ctypes.data, wide.strides[0], owner=wide)], 1), [], PILLAR, 1)
            assert (rgb[0].reshape(14, -1) == wide).all() and wide.min() >= 0.0 and wide.max() > 200.0
        ctx.run("%s per-pixel read" % name, mk, [cvgs.convertTo(t, F3)], PILLAR, 1, (M.FULL, M.BT709, M.NV12 if name == "16FC3" else M.NV21), kernel=INTERP,
                rgb=rgb)


# ---- g. a mixed tick -------------------------------------------------------------------------------------------------------------------------
def case_mixed_tick(ctx):
    """cvgs_execute_many over [a windowed write chain, a K1 tensor chain, a second write chain]: every output bit-exact against its own single
    launch and against the model (the tensor: the oracle)."""
    import torch
    dev = "cpu" if ctx.dry else ctx.device
    nv, f8 = mats_of(ctx, "NV12"), mats_of(ctx, "8UC3")
    host_nv, host_f8 = source(None, "NV12")[1], source(None, "8UC3")[1]
    out_a, out_c = (M.LIMITED, M.BT709, M.NV21), (M.FULL, M.BT601, M.NV12)
    mid_c = [cvgs.multiply(F3, [0.9, 1.0, 1.1])]
    kdst, kcrops = (24, 16), CROPS3[1:4]
    ref = np.zeros((len(kcrops), 3 * kdst[0] * kdst[1]), np.float32)
    ctx.oracle.execute(cvgs.lower(H.k1_chain(host_f8, kcrops, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), kdst)))

    def chains(on_dev):
        sa, sc = [ctx.surface(*PILLAR) for _ in range(3)], [ctx.surface(*LETTER) for _ in range(2)]
        tensor = torch.full(ref.shape, -777.0, dtype=torch.float32, device=dev)
        a = [window_read(nv(on_dev), CROPS[:3], PILLAR, cvgs.PRESERVE_AR), cvgs.write_nv12([s.mat for s in sa], *out_a)]
        b = H.k1_chain(f8(on_dev), kcrops, cvgs.GpuMat.from_tensor(tensor, cvgs.CV_32FC1), kdst)
        c = [window_read(nv(on_dev), CROPS[5:7], LETTER, cvgs.PRESERVE_AR_RN_EVEN), *mid_c, cvgs.write_nv12([s.mat for s in sc], *out_c)]
        return [a, b, c], sa, sc, tensor

    rgb_a = W.oracle_rgb(ctx.oracle, window_read(host_nv, CROPS[:3], PILLAR, cvgs.PRESERVE_AR), [], PILLAR, 3)
    rgb_c = W.oracle_rgb(ctx.oracle, window_read(host_nv, CROPS[5:7], LETTER, cvgs.PRESERVE_AR_RN_EVEN), mid_c, LETTER, 2)
    if ctx.dry:
        ops, _, _, _ = chains(False)
        ctx.lowers("mixed tick, chain 0", ops[0], FAST)
        assert not cvgs.kernel_name(*ops[1]).startswith("nv12w_")
        ctx.lowers("mixed tick, chain 2", ops[2], INTERP)
        ctx.log += [{"what": "mixed tick a", "kernel": FAST, "rgb": rgb_a, "out": out_a, "windowed": True},
                    {"what": "mixed tick c", "kernel": INTERP, "rgb": rgb_c, "out": out_c, "windowed": True}]
        return
    stream = torch.cuda.current_stream()
    ops, sa, sc, tensor = chains(True)
    assert [cvgs.kernel_name(*o)[:6] == "nv12w_" for o in ops] == [True, False, True] and cvgs.kernel_name(*ops[0]) == FAST
    held = cvgs.executeMany(stream, ops)
    torch.cuda.synchronize()
    single, sa1, sc1, tensor1 = chains(True)
    for o in single:
        cvgs.executeOperations(stream, *o)
    torch.cuda.synchronize()
    for z in range(3):
        sa[z].check(*M.write_f32(rgb_a[z], *out_a), "mixed tick, chain 0 plane %d" % z)
        assert torch.equal(sa[z].t, sa1[z].t), "mixed tick, chain 0 plane %d: the tick and the single launch differ" % z
    for z in range(2):
        sc[z].check(*M.write_f32(rgb_c[z], *out_c), "mixed tick, chain 2 plane %d" % z)
        assert torch.equal(sc[z].t, sc1[z].t), "mixed tick, chain 2 plane %d: the tick and the single launch differ" % z
    H.assert_bit_exact(tensor.cpu().numpy(), ref, "mixed tick, the K1 tensor")
    H.assert_bit_exact(tensor1.cpu().numpy(), ref, "mixed tick, the K1 tensor launched alone")
    del held


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def all_cases():
    """[(label, callable(ctx))]: every case of this module, in the order they run."""
    out = []
    outs = [(M.LIMITED, M.BT709, M.NV12), (M.FULL, M.BT601, M.NV21), (M.FULL, M.BT2020, M.NV12)]
    for name, lay in (("NV12", capi.YUV_NV12), ("NV21", capi.YUV_NV21)):
        for i, mode in enumerate(ARS):
            out.append(("window %s ar %s" % (name, mode), lambda ctx, lay=lay, mode=mode, o=outs[i]: case_window(ctx, lay, mode, o)))
    out += [("window across column 256", case_window_across_256), ("window, default-value plane", case_window_default_plane),
            ("window behind a program", case_window_program), ("window, 8UC3 crops", case_window_8uc3),
            ("device table with a window", case_device_table_window)]
    pairs = dict(zip(LAYOUTS, [(M.LIMITED, M.BT601), (M.FULL, M.BT709), (M.LIMITED, M.BT2020), (M.FULL, M.BT2020), (M.FULL, M.BT601), (M.LIMITED, M.BT709),
                               (M.LIMITED, M.BT601)]))
    for i, name in enumerate(LAYOUTS):
        rng, prim = pairs[name]
        out.append(("%s full resolution" % name, lambda ctx, n=name, r=rng, p=prim: case_layout_full(ctx, n, r, p)))
        out.append(("%s resized" % name, lambda ctx, n=name, r=rng, p=prim, o=outs[i % 3]: case_layout_resized(ctx, n, r, p, o)))
    out += [("store conversion full range", lambda ctx: case_store_conversion(ctx, M.FULL, M.BT601, M.NV12)),
            ("store conversion limited range", lambda ctx: case_store_conversion(ctx, M.LIMITED, M.BT709, M.NV21)),
            ("four quadrants of one surface", case_quadrants), ("odd step, odd base", case_odd_step), ("70 windowed planes", case_batch_70_windows),
            ("8UC4 crops, BGRA2RGB", case_8uc4), ("CV_16F / CV_16BF per-pixel", case_half_sources), ("8UC3 device table", case_device_table_8uc3),
            ("mixed tick", case_mixed_tick)]
    assert len(out) == N_CASES and len({l for l, _ in out}) == N_CASES
    return out


def run_all(device, lib, oracle, subtests):
    """Every case as a subtest of ONE item, with the stop rule of tests/test_gpu_nv12_write.run_all: only a mismatch (AssertionError) lets the
    item go on to its next case; whatever else ends a case -- an error the library returns, a HIP error at the synchronisation -- ends the item,
    and nothing more is started on a card that may have faulted."""
    ctx = Ctx(device, lib, oracle)
    stopped = []
    for label, body in all_cases():
        with subtests.test(case=label):
            assert not stopped, "not started: an earlier case ended with %s" % stopped[0]
            try:
                body(ctx)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise
