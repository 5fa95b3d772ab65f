"""Warp chains (affine / perspective) of one shape in ONE cvgs_execute_many launch (csrc/k_warp.hip: k_warp_fast_many; csrc/cvgs_api.cpp:
TickFamily::warp).

Every tensor is compared BIT FOR BIT with the CPU oracle's warp over host descriptors (as tests/test_gpu_warp_points.py::_e2e takes it) and
with the same chains sent one at a time through cvgs_execute; the tensors of a tick sit side by side in one allocation with a guard band of
sentinel bytes around and between them, and the whole allocation is compared (the arena of tests/test_zzzz_gpu_area_tick.py).  Frames are
96 x 80 u8, targets 70 x 6 (two column tiles, a partial row tile) and 16 x 8: the smallest shapes at which the segment mapping can go wrong
(ragged batches, used < batch, 128 chains, both descriptor carriers).  Every read these tests cause lies inside its source view: the kernels
test 0 <= sx < w && 0 <= sy < h before any tap, and data / w / h / step of every table entry written here are a view of the frame's.

Collected behind every other module of the suite, so that it takes no existing item's place in its order."""
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from oracle import oracle_binding
from tests import test_zzzz_gpu_area_tick as T
from tests.test_bf16_types import rne_bf16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW, FH = T.FW, T.FH
BG = T.BG
ENTRY = np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")])
INVALID = [0, 0, -1, 0, 0, -1, 0, 0, 1]  # what cvgs_warp_tables_from_points writes for an item without a fit: every pixel maps outside
WHOLE = (0, 0, FW, FH)
NARROW = (40, 10, 2, 30)  # a view two pixels wide: rows of 6 / 8 bytes; C3 rows are shorter than the 8-byte window (the gather path)
NOTE_PLANES = "not fused: more host-described warp planes than the tick's argument block holds"
INLINE_PLANES = 256  # cvgs_device.h: kManyInlineWarp


def _torch():
    import torch
    return torch


def _f32(v):
    return [float(np.float32(x)) for x in v]


def _rot(deg, s, cx, cy, dsize):
    """destination -> source: rotate by deg and scale by s about the target's centre, centre to (cx, cy)"""
    a = np.deg2rad(deg)
    c, sn = s * np.cos(a), s * np.sin(a)
    ux, uy = (dsize[0] - 1) / 2.0, (dsize[1] - 1) / 2.0
    return _f32([c, -sn, cx - c * ux + sn * uy, sn, c, cy - sn * ux - c * uy, 0, 0, 1])


def _corner(dsize):
    """the identity onto the view's bottom right corner: the last tap is the last byte of the view (of the frame: of the allocation)"""
    return _f32([1, 0, FW - dsize[0], 0, 1, FH - dsize[1], 0, 0, 1])


def _persp(m, gx, gy):
    return _f32(m[:6] + [gx, gy, 1.0])


def _mats(dsize, persp, seed):
    """Five items: inside, partly outside (two of them), the corner identity, an invalid item."""
    r = np.random.default_rng(seed)
    ms = [_rot(float(r.uniform(0, 360)), float(r.uniform(0.4, 1.1)), 48, 40, dsize), _rot(30, 1.5, 2, 3, dsize), _rot(200, 0.8, 95, 70, dsize),
          _corner(dsize), _f32(INVALID)]
    if persp:
        ms = [_persp(m, 0.002 * (i + 1), -0.001 * i) if m != _f32(INVALID) else m for i, m in enumerate(ms)]
    return ms


class Tick:
    """n warp chains of one shape: chain i warps views[i][z] (a rectangle of frames[i]) by mats[i][z] into plane z of tensor i of one arena."""

    def __init__(self, device, frames, mats, dsize, persp=False, prog="swap_mul_sub_div", out="f32", used=None, bg=None, tsplit=False, views=None):
        self.device, self.frames, self.mats, self.dsize, self.persp, self.prog, self.out = device, frames, mats, dsize, persp, prog, out
        self.used, self.bg, self.tsplit = used if used is not None else [len(m) for m in mats], bg, tsplit
        self.views = views if views is not None else [[WHOLE] * len(m) for m in mats]
        self.kind = capi.READ_WARP_PERSPECTIVE if persp else capi.READ_WARP_AFFINE
        cn = frames[0].cn
        self.arena = T.Arena(device, [len(m) * cn * dsize[0] * dsize[1] * T.OUT_BYTES[out] for m in mats])
        self.keep, self._wants = [], None

    def _read(self, i, host):
        fr = self.frames[i]
        base = fr.host_mat if host else fr.dev_mat
        rd = cvgs.ReadIOp(self.kind, fr.cv_type, [base.roi(*v) for v in self.views[i]], self.used[i], self.dsize, cvgs.IGNORE_AR, self.bg)
        rd.warp, rd.warp_sizes = [v for m in self.mats[i] for v in m], None
        return rd

    def chains(self, carrier, flags=0, stated=True, sizes=None):
        """carrier "tables": a device WarpPlane table per chain, written here as cvgs_warp_tables_from_points lays it out (the chain states
        the whole frame's byte range unless stated=False); "host": host descriptors."""
        low = []
        for i, fr in enumerate(self.frames):
            if carrier == "tables":
                tab = np.zeros(len(self.mats[i]), ENTRY)
                for z, (m, v) in enumerate(zip(self.mats[i], self.views[i])):
                    roi = fr.dev_mat.roi(*v)
                    tab[z] = (roi.data, roi.cols, roi.rows, roi.step, m, self.dsize[0], self.dsize[1])
                t = _torch().from_numpy(tab.view(np.uint8).copy()).to(self.device)
                self.keep.append(t)
                rd = cvgs.warp_table(cvgs.WARP_PERSPECTIVE if self.persp else cvgs.WARP_AFFINE, fr.dev_mat, t, len(tab), self.dsize, self.used[i], self.bg)
                if not stated:
                    rd.table_hull = None
            else:
                rd = self._read(i, False)
                rd.warp_sizes = sizes
            low.append(cvgs.lower(T._chain(rd, fr.cn, self.dsize, self.prog, self.out, (self.arena.ptr(i), self.arena.t), self.tsplit), flags))
        return low

    def wants(self):
        """The CPU oracle over host descriptors (bf16: its fp32 result rounded to nearest even, as tests/test_gpu_bf16.py)."""
        if self._wants is None:
            self._wants = []
            for i, fr in enumerate(self.frames):
                n = len(self.mats[i]) * fr.cn * self.dsize[0] * self.dsize[1]
                kind = "f32" if self.out == "bf16" else self.out
                ref = np.full(n * T.OUT_BYTES[kind], 0x5D, np.uint8)
                oracle_binding.execute(cvgs.lower(T._chain(self._read(i, True), fr.cn, self.dsize, self.prog, kind, (ref.ctypes.data, ref), self.tsplit)))
                self._wants.append(rne_bf16(ref.view(np.float32)).view(np.uint8).tobytes() if self.out == "bf16" else ref.tobytes())
        return self._wants


def _fused_and_single(lib, tick, carrier, what):
    """ONE captured kernel node with a "tick: ..." note; the tick's bytes and the chain-by-chain bytes both equal the oracle's, guard bands
    included."""
    low = tick.chains(carrier)
    nodes, note = T._nodes(lib, low, tick.device)
    assert nodes == 1 and note.startswith("tick:"), (what, carrier, nodes, note)
    tick.arena.reset()
    note = T._execute_many(lib, low)
    assert note.startswith("tick:"), (what, carrier, note)
    fused = tick.arena.check(tick.wants(), "%s, %s: the tick against the oracle" % (what, carrier))
    tick.arena.reset()
    T._execute_each(lib, low)
    single = tick.arena.check(tick.wants(), "%s, %s: chain by chain against the oracle" % (what, carrier))
    assert (fused == single).all()


def _not_fused(lib, tick, low, wants, what, n, note_is=None):
    nodes, note = T._nodes(lib, low, tick.device)
    assert nodes == n, "%s: %d kernel nodes for %d chains (%s)" % (what, nodes, n, note)
    assert note.startswith("not fused:") and "no tick kernel" not in note, (what, note)
    assert note_is is None or note == note_is, (what, note)
    tick.arena.reset()
    note = T._execute_many(lib, low)
    assert note.startswith("not fused:"), (what, note)
    got = tick.arena.check(wants, what)
    tick.arena.reset()
    T._execute_each(lib, low)
    assert (tick.arena.check(wants, what + ", chain by chain") == got).all()


@pytest.fixture(scope="module")
def frames3(device):
    return [T.Frame(device, 3, 20 + s) for s in range(3)]


@pytest.fixture(scope="module")
def frames4(device):
    return [T.Frame(device, 4, 30 + s) for s in range(3)]


def _ragged(dsize, persp):
    """batches 4 / 5 / 1"""
    return [_mats(dsize, persp, 1)[:4], _mats(dsize, persp, 2), _mats(dsize, persp, 3)[:1]]


# ---- 1. one kernel node -----------------------------------------------------------------------------------------------------------------------
def test_three_warp_chains_are_one_kernel_node(device, lib, frames3):
    """Three independent same-shape affine chains with ragged batches (4 / 5 / 1) capture as exactly ONE kernel node with a "tick: ..."
    note: over device tables and with host descriptors in the kernel arguments.  (Without the warp tick kernel: three nodes, "not fused".)"""
    tick = Tick(device, frames3, _ragged((16, 8), False), (16, 8))
    for carrier in ("tables", "host"):
        low = tick.chains(carrier)
        if carrier == "tables":
            assert all(lc.desc.read.table_src_lo and lc.desc.read.table_src_hi for lc in low)
        nodes, note = T._nodes(lib, low, device)
        assert nodes == 1, "%s: %d kernel nodes (%s)" % (carrier, nodes, note)
        assert note.startswith("tick:"), note
        tick.arena.reset()
        assert T._execute_many(lib, low).startswith("tick:")
        tick.arena.check(tick.wants(), "three chains, %s" % carrier)


# ---- 2. bit-exactness -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [3, 4], ids=["c3", "c4"])
@pytest.mark.parametrize("persp", [False, True], ids=["affine", "perspective"])
def test_bit_exact_over_types_layouts_and_programs(device, lib, frames3, frames4, persp, cn):
    """fp32 / fp16 / bf16 x NCHW / CNHW x the three programs, ragged batches 4 / 5 / 1 with used < batch in the middle chain (background
    planes), invalid items, items partly outside, the corner identity whose last tap is the frame's last byte; both carriers, the 70 x 6
    target (two column tiles, a partial row tile) for the compile-time programs and 16 x 8 for the interpreted one."""
    frames = frames3 if cn == 3 else frames4
    for out in ("f32", "f16", "bf16"):
        for tsplit in (False, True):
            for prog in ("swap_mul_sub_div", "mul_sub_div", "interp"):
                dsize = (16, 8) if prog == "interp" else (70, 6)
                # (CNHW: the channel stride is the tensor's N, so the chains of one tick hold one batch -- 5 / 5 / 5 with used 5 / 3 / 1)
                mats = [_mats(dsize, persp, s) for s in (1, 2, 3)] if tsplit else _ragged(dsize, persp)
                tick = Tick(device, frames, mats, dsize, persp, prog, out, used=[5, 3, 1] if tsplit else [4, 3, 1], bg=BG, tsplit=tsplit)
                for carrier in ("tables", "host"):
                    _fused_and_single(lib, tick, carrier, "%s C%d %s %s %s" % ("persp" if persp else "affine", cn, out, "CNHW" if tsplit else "NCHW", prog))


def test_narrow_views_take_the_gather_path(device, lib, frames3, frames4):
    """Source views two pixels wide (C3: rows of 6 bytes, shorter than the 8-byte window; C4: exactly 8) beside whole frames, one view per
    plane; used_planes == 0 in one chain (nothing but background)."""
    dsize = (16, 8)
    stretch = _f32([2.0 / 16, 0, 0, 0, 30.0 / 8, 0, 0, 0, 1])  # the whole narrow view, stretched over the target
    for frames in (frames3, frames4):
        mats = [[stretch, _rot(10, 0.1, 1, 15, dsize)], [_rot(45, 1.0, 48, 40, dsize), stretch], [stretch]]
        views = [[NARROW, NARROW], [WHOLE, NARROW], [NARROW]]
        tick = Tick(device, frames, mats, dsize, bg=BG, used=[2, 2, 0], views=views)
        for carrier in ("tables", "host"):
            _fused_and_single(lib, tick, carrier, "narrow views C%d" % frames[0].cn)


# ---- 3. from landmarks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [2, 16], ids=["two_frames", "sixteen_frames"])
def test_tables_from_landmarks_feed_a_replayed_warp_tick(device, lib, n_frames):
    """cvgs_warp_tables_from_points writes the tables of all frames in ONE call; the tick over them is captured as one kernel node (behind
    the table kernel's) and replayed after the landmarks and the frames' contents changed in place: every replay equals the chains sent one
    by one over the same tables, and the replays differ."""
    torch = _torch()
    from tests import warp_point_cases as P
    dsize, items = (16, 8), 3
    tmpl = (P.TMPL5.astype(np.float64) * np.array([dsize[0] / 112.0, dsize[1] / 112.0])).astype(np.float32)
    frames = [T.Frame(device, 3, 60 + i) for i in range(n_frames)]

    def landmarks(round_):
        r = np.random.default_rng(500 + round_)
        pts = np.zeros((n_frames, items, 5, 2), np.float32)
        for f in range(n_frames):
            for i in range(items):
                a, s = r.uniform(0, 2 * np.pi), r.uniform(1.0, 3.0)
                R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
                pts[f, i] = (tmpl.astype(np.float64) - tmpl.mean(axis=0)) @ R.T + np.array([r.uniform(-5, FW + 5), r.uniform(-5, FH + 5)])
        pts[0, 1, 2, 0] = np.nan  # an item without a fit: the builder's invalid entry
        return pts

    pts_dev = torch.from_numpy(landmarks(0)).to(device)
    tables = [torch.zeros((items, 64), dtype=torch.uint8, device=device) for _ in frames]
    descs = [cvgs.warp_table_desc(fr.dev_mat, pts_dev[i], tables[i], items, dsize, tmpl) for i, fr in enumerate(frames)]
    arena = T.Arena(device, [items * 3 * dsize[0] * dsize[1] * 4] * n_frames)
    single = T.Arena(device, arena.sizes)

    def lowered(ar):
        return [cvgs.lower(T._chain(cvgs.warp_table(cvgs.WARP_AFFINE, fr.dev_mat, tables[i], items, dsize), 3, dsize, "swap_mul_sub_div", "f32", (ar.ptr(i), ar.t)))
                for i, fr in enumerate(frames)]

    low, low_single = lowered(arena), lowered(single)
    arr = cvgs.pack_chains(low)
    # the tick alone: one kernel node
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 1 and note.startswith("tick:"), (nodes, note)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    seen = []
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            cvgs.warp_tables_from_points(s, descs)
            capi.check(lib.cvgs_execute_many(arr, len(low), s.cuda_stream))
        assert lib.cvgs_last_error().decode().startswith("tick:")
        for round_ in range(3):
            arena.reset()
            g.replay()
            torch.cuda.synchronize()
            single.reset()
            T._execute_each(lib, low_single)  # (the current stream here is `side`)
            got, want = arena.bytes(), single.bytes()
            assert (got == want).all(), "replay %d: %d bytes differ from the chains sent one by one" % (round_, int((got != want).sum()))
            inv = got[arena.offsets[0]:arena.offsets[0] + arena.sizes[0]].view(np.float32).reshape(items, 3, dsize[1], dsize[0])[1]
            zero = (np.zeros(3, np.float32)[::-1] * np.float32(0.3) - np.array(T.SUB[:3], np.float32)) / np.array(T.DIV[:3], np.float32)
            assert (inv == zero[:, None, None]).all(), "the invalid item's plane is zero through the program"
            seen.append(got.copy())
            if round_ < 2:
                pts_dev.copy_(torch.from_numpy(landmarks(round_ + 1)).to(device))
                for i, fr in enumerate(frames):
                    fr.refill(100 * round_ + i)
                torch.cuda.synchronize()
    assert not (seen[0] == seen[1]).all() and not (seen[1] == seen[2]).all()


# ---- 4. chain limits --------------------------------------------------------------------------------------------------------------------------
def test_max_chains_of_one_plane_each(device, lib, frames3):
    """n = CVGS_MAX_CHAINS chains of one plane each (grid z = 128), 4 x 4 targets, both carriers: one node.  One chain more is what the
    C-ABI refuses as it always did (CVGS_ERR_INVALID, nothing enqueued)."""
    n, dsize = capi.MAX_CHAINS, (4, 4)
    r = np.random.default_rng(9)
    mats = [[_rot(float(r.uniform(0, 360)), float(r.uniform(0.5, 6.0)), float(r.uniform(0, FW)), float(r.uniform(0, FH)), dsize)] for _ in range(n + 1)]
    tick = Tick(device, [frames3[i % 3] for i in range(n)], mats[:n], dsize, prog="mul_sub_div")
    for carrier in ("tables", "host"):
        _fused_and_single(lib, tick, carrier, "128 chains")
    more = Tick(device, [frames3[i % 3] for i in range(n + 1)], mats, dsize, prog="mul_sub_div")
    low = more.chains("tables")
    more.arena.reset()
    assert lib.cvgs_execute_many(cvgs.pack_chains(low), n + 1, T._stream()) == capi.ERR_INVALID
    more.arena.check([bytes([T.SENTINEL]) * s for s in more.arena.sizes], "a refused call writes nothing")


def test_more_host_planes_than_the_argument_block_run_one_by_one(device, lib, frames3):
    """Host descriptors: 4 x 64 = 256 planes are the argument block's capacity (one node); 6 x 43 = 258 planes run chain by chain (each
    chain's planes still fit its own launch's arguments, so the six launches can be captured) with the note that says so and the same bytes.
    Over device tables the same 258 planes are one node."""
    dsize = (4, 4)
    r = np.random.default_rng(10)

    def mats(n):
        return [_rot(float(r.uniform(0, 360)), float(r.uniform(0.5, 6.0)), float(r.uniform(0, FW)), float(r.uniform(0, FH)), dsize) for _ in range(n)]

    full = Tick(device, [frames3[i % 3] for i in range(4)], [mats(INLINE_PLANES // 4) for _ in range(4)], dsize)
    _fused_and_single(lib, full, "host", "256 planes inline")
    over = Tick(device, [frames3[i % 3] for i in range(6)], [mats(43) for _ in range(6)], dsize)
    assert sum(len(m) for m in over.mats) > INLINE_PLANES
    _not_fused(lib, over, over.chains("host"), over.wants(), "258 host-described planes", 6, NOTE_PLANES)
    _fused_and_single(lib, over, "tables", "258 planes over device tables")


# ---- 5. what must not fuse still runs in order ----------------------------------------------------------------------------------------------
def test_a_chain_that_reads_its_predecessors_tensor_is_not_fused(device, lib, frames3):
    """Chain B warps (as a u8 C3 frame) the tensor chain A writes: B must see A's result, as two sequential calls would."""
    dsize, fw, fh = (16, 8), 32, 16
    mats_a, mats_b = _mats(dsize, False, 4)[:2], [_f32([1, 0, 3, 0, 1, 2, 0, 0, 1]), _rot(20, 1.2, 16, 8, dsize)]
    tick = Tick(device, frames3[:2], [mats_a, mats_b], dsize)
    want_a = Tick(device, frames3[:1], [mats_a], dsize).wants()[0]
    alias = T.Frame.__new__(T.Frame)  # B's frame: the first fh x fw x 3 bytes of A's tensor
    alias.cn, alias.cv_type = 3, cvgs.CV_8UC3
    alias.host = np.ascontiguousarray(np.frombuffer(want_a, np.uint8)[:fh * fw * 3].reshape(fh, fw, 3))
    alias.host_mat = cvgs.GpuMat.from_array(alias.host, cvgs.CV_8UC3)
    alias.dev_mat = cvgs.GpuMat(fh, fw, cvgs.CV_8UC3, tick.arena.ptr(0), fw * 3, owner=tick.arena.t)
    tick.frames = [frames3[0], alias]
    tick.views = [[WHOLE] * 2, [(0, 0, fw, fh)] * 2]
    want_b = Tick(device, [alias], [mats_b], dsize, views=[[(0, 0, fw, fh)] * 2]).wants()[0]
    for carrier in ("host", "tables"):
        _not_fused(lib, tick, tick.chains(carrier), [want_a, want_b], "B reads what A writes (%s)" % carrier, 2)


def test_what_the_warp_tick_does_not_take_runs_one_by_one(device, lib, frames3):
    """Per-plane target sizes, differing kinds / programs / target sizes / types / descriptor forms, CVGS_CHAIN_FORCE_GENERIC, packed
    writes, a 16U source, CV_64F and integer-typed arithmetic, a cast inside the program, device tables with neither hull nor vouch: n kernel
    nodes, a "not fused: ..." note that is not "no tick kernel for this read kind", and the bytes of n sequential calls."""
    dsize = (16, 8)
    mats = [_mats(dsize, False, 5)[:2], _mats(dsize, False, 6)[:2], _mats(dsize, False, 7)[:2]]
    tick = Tick(device, frames3, mats, dsize)
    _not_fused(lib, tick, tick.chains("tables", stated=False), tick.wants(), "tables, nothing stated", 3)
    _not_fused(lib, tick, tick.chains("host", flags=capi.CHAIN_FORCE_GENERIC), tick.wants(), "CHAIN_FORCE_GENERIC", 3)
    _not_fused(lib, tick, tick.chains("tables", flags=capi.CHAIN_FORCE_GENERIC), tick.wants(), "CHAIN_FORCE_GENERIC over tables", 3)
    # warp_dst_sizes that all equal the chain's size: the same bytes, but a form the tick does not read
    _not_fused(lib, tick, tick.chains("host", sizes=[dsize, dsize]), tick.wants(), "warp_dst_sizes", 3,
               "not fused: warp chains with per-plane target sizes (warp_dst_sizes)")

    def pair(a, b, what, carriers=("host", "host")):
        low = a.chains(carriers[0]) + b.chains(carriers[1])
        nodes, note = T._nodes(lib, low, device)
        assert nodes == 2 and note.startswith("not fused:") and "no tick kernel" not in note, (what, nodes, note)
        a.arena.reset()
        b.arena.reset()
        assert T._execute_many(lib, low).startswith("not fused:")
        a.arena.check(a.wants(), what + " (first)")
        b.arena.check(b.wants(), what + " (second)")

    one = Tick(device, frames3[:1], mats[:1], dsize)
    pair(one, Tick(device, frames3[1:2], [_mats(dsize, True, 6)[:2]], dsize, persp=True), "affine beside perspective")
    pair(one, Tick(device, frames3[1:2], mats[1:2], dsize, prog="mul_sub_div"), "two programs")
    pair(one, Tick(device, frames3[1:2], [_mats((70, 6), False, 6)[:2]], (70, 6)), "16 x 8 beside 70 x 6")
    pair(one, Tick(device, frames3[1:2], mats[1:2], dsize, out="f16"), "fp32 beside fp16")
    pair(one, Tick(device, frames3[1:2], mats[1:2], dsize), "host descriptors beside a device table", ("host", "tables"))

    # a 16U source: the interpreted kernel, chain by chain, both carriers
    f16u = [T.Frame(device, 3, 40 + i, capi.DEPTH_16U) for i in range(2)]
    t16 = Tick(device, f16u, mats[:2], dsize, prog="mul_sub_div")
    _not_fused(lib, t16, t16.chains("host"), t16.wants(), "16U source", 2)
    _not_fused(lib, t16, t16.chains("tables"), t16.wants(), "16U source over tables", 2)

    # programs the fast kernel does not take: a cast inside, integer-typed arithmetic, CV_64F values -- and packed pixels
    cn = 3
    f32t, u8t, f64t = cvgs.make_type(capi.DEPTH_32F, cn), cvgs.make_type(capi.DEPTH_8U, cn), cvgs.make_type(capi.DEPTH_64F, cn)
    cases = {
        "a cast inside the program": ([cvgs.multiply(f32t, T.MUL[:cn]), cvgs.convertTo(f32t, u8t), cvgs.convertTo(u8t, f32t), cvgs.subtract(f32t, T.SUB[:cn])], f32t, 4),
        "integer-typed arithmetic": ([cvgs.convertTo(f32t, u8t), cvgs.add(u8t, [1.0, 2.0, 3.0]), cvgs.convertTo(u8t, f32t)], f32t, 4),
        "CV_64F arithmetic": ([cvgs.convertTo(f32t, f64t), cvgs.multiply(f64t, T.MUL[:cn]), cvgs.convertTo(f64t, f32t)], f32t, 4),
    }
    for what, (stages, t, esz) in cases.items():
        arena = T.Arena(device, [2 * cn * dsize[0] * dsize[1] * esz] * 2)
        low, wants = [], []
        for i in range(2):
            low.append(cvgs.lower([tick._read(i, False)] + stages + [cvgs.split_tensor(t, arena.ptr(i), dsize[0], dsize[1], 2, keep=arena.t)]))
            ref = np.full(arena.sizes[i], 0x5D, np.uint8)
            oracle_binding.execute(cvgs.lower([tick._read(i, True)] + stages + [cvgs.split_tensor(t, ref.ctypes.data, dsize[0], dsize[1], 2, keep=ref)]))
            wants.append(ref.tobytes())
        holder = Tick.__new__(Tick)
        holder.device, holder.arena = device, arena
        _not_fused(lib, holder, low, wants, what, 2)

    # WRITE_PIXEL_3D: packed fp32 pixels
    arena = T.Arena(device, [2 * cn * dsize[0] * dsize[1] * 4] * 2)
    low, wants = [], []
    prog = [cvgs.multiply(f32t, T.MUL[:cn]), cvgs.subtract(f32t, T.SUB[:cn]), cvgs.divide(f32t, T.DIV[:cn])]
    for i in range(2):
        out = cvgs.GpuMat(2, cn * dsize[0] * dsize[1] * 4, cvgs.CV_8UC1, arena.ptr(i), owner=arena.t)
        low.append(cvgs.lower([tick._read(i, False)] + prog + [cvgs.write(f32t, out, dsize)]))
        nchw = np.frombuffer(Tick(device, frames3[i:i + 1], mats[i:i + 1], dsize, prog="mul_sub_div").wants()[0], np.float32).reshape(2, cn, dsize[1], dsize[0])
        wants.append(np.ascontiguousarray(nchw.transpose(0, 2, 3, 1)).tobytes())
    holder = Tick.__new__(Tick)
    holder.device, holder.arena = device, arena
    _not_fused(lib, holder, low, wants, "packed pixels (WRITE_PIXEL_3D)", 2)


# ---- 6. the C++ facade ------------------------------------------------------------------------------------------------------------------------
def test_facade_device_warps_batch_is_one_launch(lib):
    """cvGS::DeviceWarps + cvGS::ChainBatch from C++ (tests/cpp/test_warp_tick.cpp): one launch for the tick and the bytes of one
    executeOperations per chain."""
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_warp_tick")
    assert os.path.exists(exe), "%s is missing: run build() first" % exe
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_warp_tick passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
