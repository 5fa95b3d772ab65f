"""INTER_AREA crop chains of one shape in ONE cvgs_execute_many launch (csrc/k_area.hip: k_area_fast_many; csrc/cvgs_api.cpp: TickFamily::area).

Every tensor is compared BIT FOR BIT with the fp32 restatement of the contract (tests/area_model.py) and with the same chains sent one at a
time through cvgs_execute; the tensors of a tick sit side by side in one allocation with a guard band of sentinel bytes around and between
them, and the whole allocation is compared.  Frames are 96 x 80 u8, targets a few dozen pixels: the smallest shapes at which the segment
mapping can go wrong (ragged batches, used < batch, two column tiles, a partial row tile, 128 chains, every descriptor carrier).

Collected behind every other module of the suite (as tests/test_zz_gpu_area.py is), so that it takes no existing item's place in its order."""
import ctypes as C
import os

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as M

pytestmark = pytest.mark.gpu

FW, FH = 96, 80
GUARD, SENTINEL = 256, 0xA5
MUL, SUB, DIV, ADD = [0.3] * 4, [40.0, 50.0, 60.0, 70.0], [57.0, 58.0, 59.0, 61.0], [0.125, -3.0, 2.5, 1.0]
OUT_DEPTH = {"f32": capi.DEPTH_32F, "f16": capi.DEPTH_16F, "bf16": capi.DEPTH_16BF}
OUT_BYTES = {"f32": 4, "f16": 2, "bf16": 2}
BG = [11.0, 22.5, 33.0, 44.0]

ONE_PIXEL = (5, 5, 1, 1)
LAST_BYTE = (FW - 9, FH - 7, 9, 7)   # its last pixel is the frame's last byte
SHRINK_X_GROW_Y = (2, 40, 90, 4)     # for the 70 x 6 target: 90 -> 70 columns, 4 -> 6 rows
WHOLE = (0, 0, FW, FH)


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _out_type(out, cn):
    if out == "bf16":
        return cvgs.make_type(capi.DEPTH_16F, cn) | capi.TYPE_FLAG_BF16
    return cvgs.make_type(OUT_DEPTH[out], cn)


class Frame:
    """A seeded FH x FW frame: the host array, a GpuMat over it and a GpuMat over its device copy."""

    def __init__(self, device, cn, seed, depth=capi.DEPTH_8U):
        rng = np.random.default_rng(0xA7EA + seed)
        ramp = np.arange(FW)[None, :, None] * 3 + np.arange(FH)[:, None, None] * 5 + np.arange(cn)[None, None, :] * 7
        if depth == capi.DEPTH_8U:
            self.host = np.ascontiguousarray((rng.integers(0, 200, (FH, FW, cn)) + ramp % 56).astype(np.uint8))
        else:
            self.host = np.ascontiguousarray((rng.integers(0, 60000, (FH, FW, cn)) + ramp * 9).astype(np.uint16))
        self.cn, self.cv_type = cn, cvgs.make_type(depth, cn)
        self.host_mat = cvgs.GpuMat.from_array(self.host, self.cv_type)
        self.t = _torch().from_numpy(self.host.view(np.uint8).reshape(FH, -1).copy()).to(device)
        self.dev_mat = cvgs.GpuMat(FH, FW, self.cv_type, self.t.data_ptr(), self.host.strides[0], owner=self.t)

    def refill(self, seed):
        """New contents in the SAME device bytes."""
        rng = np.random.default_rng(0xB0B + seed)
        self.host[:] = rng.integers(0, 256, self.host.shape).astype(self.host.dtype)
        self.t.copy_(_torch().from_numpy(self.host.view(np.uint8).reshape(FH, -1).copy()))


class Arena:
    """The tensors of one tick side by side in one allocation, GUARD sentinel bytes in front of, between and behind them."""

    def __init__(self, device, sizes):
        self.offsets, at = [], GUARD
        for n in sizes:
            self.offsets.append(at)
            at += (n + 255) // 256 * 256 + GUARD
        self.sizes, self.total = list(sizes), at
        self.t = _torch().full((at,), SENTINEL, dtype=_torch().uint8, device=device)

    def ptr(self, i):
        return self.t.data_ptr() + self.offsets[i]

    def reset(self):
        self.t.fill_(SENTINEL)
        _torch().cuda.synchronize()

    def bytes(self):
        _torch().cuda.synchronize()
        return self.t.cpu().numpy()

    def check(self, wants, what):
        want = np.full(self.total, SENTINEL, np.uint8)
        for off, n, w in zip(self.offsets, self.sizes, wants):
            w = np.frombuffer(w, np.uint8)
            assert w.size == n, (w.size, n)
            want[off:off + n] = w
        got = self.bytes()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d bytes differ, first at arena byte %d (got %d, want %d; tensors start at %r)" % (
            what, bad.size, bad[0], got[bad[0]], want[bad[0]], self.offsets)
        return got


def _chain(read, cn, dsize, prog, out, target, tsplit=False, batch=None):
    """read -> program -> [cast] -> TensorSplit / TensorTSplit.  target: (pointer, owner)."""
    f_type = cvgs.make_type(capi.DEPTH_32F, cn)
    ops = [read]
    if prog == "swap_mul_sub_div":
        ops.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f_type))
    ops += [cvgs.multiply(f_type, MUL[:cn]), cvgs.subtract(f_type, SUB[:cn]), cvgs.divide(f_type, DIV[:cn])]
    if prog == "interp":  # one stage more than the compile-time programs
        ops.append(cvgs.add(f_type, ADD[:cn]))
    t = _out_type(out, cn)
    if out != "f32":
        ops.append(cvgs.convertTo(f_type, t))
    ptr, owner = target
    batch = read.batch if batch is None else batch
    ops.append((cvgs.splitT if tsplit else cvgs.split_tensor)(t, ptr, dsize[0], dsize[1], batch, keep=owner))
    return ops


def _expected(frame, crops, used, dsize, prog, out, ar, bg, tsplit=False, params=None):
    """The bytes the chain must store, from the fp32 restatement; the geometry is the plane table of the same read over host views."""
    cn = frame.cn
    rd = cvgs.resize(frame.cv_type, cvgs.INTER_AREA, [frame.host_mat.roi(*c) for c in crops], dsize, used, bg, ar)
    low = cvgs.lower(_chain(rd, cn, dsize, prog, out, (16, None), tsplit))
    P = params if params is not None else M.plane_params(rd)
    srcs = [frame.host[c[1]:c[1] + c[3], c[0]:c[0] + c[2]] for c in crops]
    vals, depth = M.area_chain(M.area_plane_f32, srcs, P, dsize, used, len(crops), list(low.desc.read.background), M.chain_ops(low.desc), np.float32)
    assert depth == OUT_DEPTH[out]
    vals = vals.transpose(3, 0, 1, 2) if tsplit else vals.transpose(0, 3, 1, 2)  # CNHW / NCHW
    return M.store_bits(vals, depth).tobytes()


class Tick:
    """n AREA chains of one shape: chain i reads `crop_sets[i]` of frames[i] (the first used[i] of them) into tensor i of one arena."""

    def __init__(self, device, frames, crop_sets, dsize, prog="swap_mul_sub_div", out="f32", ar=cvgs.IGNORE_AR, bg=None, used=None, tsplit=False):
        self.device, self.frames, self.crop_sets, self.dsize, self.prog, self.out = device, frames, crop_sets, dsize, prog, out
        self.ar, self.bg, self.tsplit = ar, bg, tsplit
        self.used = [len(c) for c in crop_sets] if used is None else used
        cn = frames[0].cn
        self.arena = Arena(device, [len(c) * cn * dsize[0] * dsize[1] * OUT_BYTES[out] for c in crop_sets])
        self.keep = []
        self._wants = None

    def chains(self, carrier, stated=True, flags=0):
        """The lowered chains: carrier "tables" (device plane tables, the hull stated from the host views unless stated=False) or "host"."""
        low = []
        for i, (fr, crops) in enumerate(zip(self.frames, self.crop_sets)):
            rd = cvgs.resize(fr.cv_type, cvgs.INTER_AREA, [fr.dev_mat.roi(*c) for c in crops], self.dsize, self.used[i], self.bg, self.ar)
            if carrier == "tables":
                tab = _torch().frombuffer(bytearray(cvgs.build_plane_table(rd)), dtype=_torch().uint8).to(self.device)
                self.keep.append(tab)
                rd.table = tab.data_ptr()
                if not stated:
                    rd.mats = None  # no host views at hand: the facade cannot compute a hull
            low.append(cvgs.lower(_chain(rd, fr.cn, self.dsize, self.prog, self.out, (self.arena.ptr(i), self.arena.t), self.tsplit), flags))
        return low

    def wants(self):
        if self._wants is None:
            self._wants = [_expected(fr, crops, u, self.dsize, self.prog, self.out, self.ar, self.bg, self.tsplit)
                           for fr, crops, u in zip(self.frames, self.crop_sets, self.used)]
        return self._wants


def _execute_many(lib, low):
    """One cvgs_execute_many call on the current stream; returns the note it left."""
    arr = cvgs.pack_chains(low)
    capi.check(lib.cvgs_execute_many(arr, len(low), _stream()))
    return lib.cvgs_last_error().decode()


def _execute_each(lib, low):
    for lc in low:
        capi.check(lib.cvgs_execute(C.byref(lc.desc), _stream()))


def _captured_kernel_nodes(lib, arr, n, device):
    """How many kernel launches does ONE cvgs_execute_many call enqueue?  Captured on a side stream with the HIP runtime's own capture calls
    and counted with hipGraphGetNodes.  Returns (nodes, the call's status, the note it left)."""
    torch = _torch()
    hip = C.CDLL(None)  # libamdhip64 came in with torch; its symbols are global in this process
    for name in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphGetNodes", "hipGraphDestroy"):
        if not hasattr(hip, name):
            import glob
            hip = C.CDLL(sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))[0])
            break
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 0) == 0  # hipStreamCaptureModeGlobal
    rc = lib.cvgs_execute_many(arr, n, side.cuda_stream)
    note = lib.cvgs_last_error().decode()
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
    hip.hipGraphDestroy(graph)
    return count.value, rc, note


def _nodes(lib, low, device):
    arr = cvgs.pack_chains(low)
    nodes, rc, note = _captured_kernel_nodes(lib, arr, len(low), device)
    assert rc == 0, note
    return nodes, note


def _fused_and_single(lib, tick, carrier, what, capturable=True):
    """The tick through ONE call and through one cvgs_execute per chain: both equal the restatement, so each other, guard bands included."""
    low = tick.chains(carrier)
    if capturable:
        nodes, note = _nodes(lib, low, tick.device)
        assert nodes == 1 and note.startswith("tick:"), (what, carrier, nodes, note)
    tick.arena.reset()
    note = _execute_many(lib, low)
    assert note.startswith("tick:"), (what, carrier, note)
    fused = tick.arena.check(tick.wants(), "%s, %s: the tick against the restatement" % (what, carrier))
    tick.arena.reset()
    _execute_each(lib, low)
    single = tick.arena.check(tick.wants(), "%s, %s: chain by chain against the restatement" % (what, carrier))
    assert (fused == single).all()


@pytest.fixture(scope="module")
def frames3(device):
    return [Frame(device, 3, s) for s in range(3)]


@pytest.fixture(scope="module")
def frames4(device):
    return [Frame(device, 4, 10 + s) for s in range(3)]


# ---- 1. one launch ------------------------------------------------------------------------------------------------------------------------
def test_three_area_chains_are_one_kernel_node(device, lib, frames3):
    """Three independent same-shape AREA chains capture as exactly ONE kernel node, through device tables with stated hulls and with host
    descriptors (planes in the kernel arguments); the call's note says "tick: ...".  (Before the AREA tick kernel: three nodes, "not fused".)"""
    sets = [[WHOLE, (11, 13, 38, 19)], [(8, 4, 32, 16), (1, 2, 48, 24)], [(56, 38, 40, 23), (30, 20, 7, 5)]]
    tick = Tick(device, frames3, sets, (16, 8))
    for carrier in ("tables", "host"):
        low = tick.chains(carrier)
        if carrier == "tables":
            assert all(lc.desc.read.table_src_lo and lc.desc.read.table_src_hi for lc in low)
        nodes, note = _nodes(lib, low, device)
        assert nodes == 1, "%s: %d kernel nodes (%s)" % (carrier, nodes, note)
        assert note.startswith("tick:"), note
        tick.arena.reset()
        assert _execute_many(lib, low).startswith("tick:")
        tick.arena.check(tick.wants(), "three chains, %s" % carrier)


# ---- 2. bit-exactness -----------------------------------------------------------------------------------------------------------------------
def test_ragged_batches_two_column_tiles_and_a_letterbox_window(device, lib, frames3):
    """Batches 1, 3, 2 in one tick with used_planes < batch in the middle chain; a 70 x 6 target (two column tiles, a partial row tile);
    PRESERVE_AR windows with background columns / rows; a one-pixel crop, the crop that ends on the frame's last byte, a crop that shrinks on
    x and grows on y.  C3, swap-mul-sub-div, fp32 NCHW."""
    sets = [[SHRINK_X_GROW_Y], [ONE_PIXEL, LAST_BYTE, WHOLE], [(20, 10, 30, 60), (3, 9, 40, 1)]]
    for ar in (cvgs.PRESERVE_AR, cvgs.IGNORE_AR):
        tick = Tick(device, frames3, sets, (70, 6), "swap_mul_sub_div", "f32", ar, BG, used=[1, 2, 2])
        for carrier in ("tables", "host"):
            _fused_and_single(lib, tick, carrier, "ragged 70x6 ar %d" % ar)


def test_c4_fp16_cnhw(device, lib, frames4):
    """C4, mul-sub-div, fp16 (the trailing cast inside the store), TENSOR_T_SPLIT (CNHW), a 33 x 7 target."""
    sets = [[WHOLE, ONE_PIXEL], [LAST_BYTE, (11, 13, 38, 19)], [(2, 40, 90, 6), (9, 1, 66, 14)]]
    tick = Tick(device, frames4, sets, (33, 7), "mul_sub_div", "f16", cvgs.PRESERVE_AR, BG, tsplit=True)
    for carrier in ("tables", "host"):
        _fused_and_single(lib, tick, carrier, "C4 fp16 CNHW")


def test_interpreted_program_bf16_and_fp32(device, lib, frames3, frames4):
    """One extra `add` -> the interpreted program: C3 into a bf16 NCHW tensor, C4 into fp32; batches 2, 1, 2 with a default-value plane."""
    sets = [[WHOLE, LAST_BYTE], [ONE_PIXEL], [(8, 4, 32, 16), (56, 38, 40, 23)]]
    _fused_and_single(lib, Tick(device, frames3, sets, (16, 8), "interp", "bf16", cvgs.IGNORE_AR, BG, used=[2, 1, 1]), "tables", "C3 interp bf16")
    _fused_and_single(lib, Tick(device, frames4, sets, (16, 8), "interp", "f32", cvgs.PRESERVE_AR, BG), "host", "C4 interp fp32")
    _fused_and_single(lib, Tick(device, frames4, sets, (16, 8), "swap_mul_sub_div", "bf16"), "tables", "C4 swap bf16")
    _fused_and_single(lib, Tick(device, frames3, sets, (16, 8), "mul_sub_div", "f16"), "host", "C3 mul-sub-div fp16")


def _tiny_crops(n, seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, FW - 9)), int(rng.integers(0, FH - 9)), int(rng.integers(1, 10)), int(rng.integers(1, 10))) for _ in range(n)]


def test_max_chains_of_one_plane_each(device, lib, frames3):
    """n = CVGS_MAX_CHAINS chains of one plane each (grid z = 128), 4 x 4 targets of tiny crops, both carriers."""
    n = capi.MAX_CHAINS
    crops = _tiny_crops(n, 77)
    tick = Tick(device, [frames3[i % 3] for i in range(n)], [[c] for c in crops], (4, 4), "mul_sub_div", "f32")
    for carrier in ("tables", "host"):
        _fused_and_single(lib, tick, carrier, "128 chains")


def test_large_argument_block_and_the_staged_host_table(device, lib, frames3):
    """Host descriptors: 3 x 100 planes travel in the large kernel-argument block (one captured node); 5 x 210 planes are more than 1024 in
    all and force the staged host table (eager: its pooled slot rides on the launch).  4 x 4 targets of tiny crops."""
    t300 = Tick(device, frames3, [_tiny_crops(100, 300 + i) for i in range(3)], (4, 4), "swap_mul_sub_div", "f32", used=[100, 97, 100], bg=BG)
    _fused_and_single(lib, t300, "host", "300 planes inline")
    fr = [frames3[i % 3] for i in range(5)]
    t1050 = Tick(device, fr, [_tiny_crops(210, 400 + i) for i in range(5)], (4, 4), "swap_mul_sub_div", "f32")
    low = t1050.chains("host")
    for round_ in range(2):  # twice: the second tick recycles the pooled slot of the first
        t1050.arena.reset()
        note = _execute_many(lib, low)
        assert note.startswith("tick:"), note
        t1050.arena.check(t1050.wants(), "1050 planes, staged host table, round %d" % round_)
    t1050.arena.reset()
    _execute_each(lib, low)
    t1050.arena.check(t1050.wants(), "1050 planes chain by chain")


# ---- 3. tables from device boxes -----------------------------------------------------------------------------------------------------------
def test_tables_from_device_boxes_feed_an_area_tick(device, lib, frames3):
    """cvgs_plane_tables_from_boxes (read_kind RESIZE_LINEAR, the kind it accepts) writes the tables of two frames -- one box invalid, one
    frame's count below max_boxes --; an AREA tick reads them in one launch.  Valid planes equal the host-described result, the others are
    the background run through the program."""
    torch = _torch()
    frames = frames3[:2]
    rects = [[WHOLE, (11, 13, 38, 19), (5, 7, 0, 10), LAST_BYTE], [(8, 4, 32, 16), ONE_PIXEL, (1, 2, 48, 24), (30, 20, 7, 5)]]
    counts, max_boxes, dsize = [4, 3], 4, (16, 8)
    valid = [[True, True, False, True], [True, True, True, False]]
    s = torch.cuda.current_stream()
    keep, descs, tables = [], [], []
    for fr, r, n in zip(frames, rects, counts):
        boxes = torch.tensor(r, dtype=torch.int32, device=device)
        count = torch.tensor([n], dtype=torch.int32, device=device)
        table = torch.zeros((max_boxes, 48), dtype=torch.uint8, device=device)
        keep += [boxes, count, table]
        tables.append(table)
        descs.append(cvgs.box_table_desc(fr.dev_mat, boxes, table, max_boxes, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYWH_I32, count, None, capi.READ_RESIZE_LINEAR))
    cvgs.plane_tables_from_boxes(s, descs)
    torch.cuda.synchronize()
    arena = Arena(device, [max_boxes * 3 * 16 * 8 * 4] * 2)
    low, wants = [], []
    for i, (fr, r, table) in enumerate(zip(frames, rects, tables)):
        rd = cvgs.resize_boxes(fr.dev_mat, table, max_boxes, dsize, BG, interp=cvgs.INTER_AREA)
        assert rd.kind == capi.READ_RESIZE_AREA
        low.append(cvgs.lower(_chain(rd, 3, dsize, "swap_mul_sub_div", "f32", (arena.ptr(i), arena.t))))
        good = [c for c, ok in zip(r, valid[i]) if ok]
        P = iter(M.plane_params(cvgs.resize(fr.cv_type, cvgs.INTER_AREA, [fr.host_mat.roi(*c) for c in good], dsize)))
        first = M.plane_params(cvgs.resize(fr.cv_type, cvgs.INTER_AREA, [fr.host_mat.roi(*WHOLE)], dsize))[0]
        params = [next(P) if ok else dict(first, x1=0, y1=0, x2=-1, y2=-1) for ok in valid[i]]  # the invalid entry: the empty window
        crops = [c if ok else WHOLE for c, ok in zip(r, valid[i])]
        wants.append(_expected(fr, crops, max_boxes, dsize, "swap_mul_sub_div", "f32", cvgs.IGNORE_AR, BG, params=params))
    nodes, note = _nodes(lib, low, device)
    assert nodes == 1 and note.startswith("tick:"), (nodes, note)
    arena.reset()
    assert _execute_many(lib, low).startswith("tick:")
    got = arena.check(wants, "tables from device boxes")
    bgp = (np.array(BG[:3], np.float32)[::-1] * np.float32(0.3) - np.array(SUB[:3], np.float32)) / np.array(DIV[:3], np.float32)
    for i in range(2):
        planes = got[arena.offsets[i]:arena.offsets[i] + arena.sizes[i]].view(np.float32).reshape(max_boxes, 3, 8, 16)
        for z in range(max_boxes):
            if not valid[i][z]:
                assert (planes[z] == bgp[:, None, None]).all(), "frame %d plane %d: an invalid box is all background" % (i, z)
    arena.reset()
    _execute_each(lib, low)
    arena.check(wants, "tables from device boxes, chain by chain")


# ---- 4. what must not fuse still runs in order ---------------------------------------------------------------------------------------------
def _not_fused(lib, tick, low, wants, what, n):
    nodes, note = _nodes(lib, low, tick.device)
    assert nodes == n, "%s: %d kernel nodes for %d chains (%s)" % (what, nodes, n, note)
    assert note.startswith("not fused:"), (what, note)
    tick.arena.reset()
    note = _execute_many(lib, low)
    assert note.startswith("not fused:"), (what, note)
    tick.arena.check(wants, what)


def test_a_chain_that_reads_its_predecessors_tensor_is_not_fused(device, lib, frames3):
    """Chain B reads (as a u8 C3 frame) the tensor chain A writes: the second wins, as two sequential calls would."""
    dsize, fw, fh = (16, 8), 32, 16
    crops_a, crops_b = [WHOLE, (11, 13, 38, 19)], [(0, 0, fw, fh), (3, 2, 20, 11)]
    tick = Tick(device, frames3[:2], [crops_a, crops_b], dsize)
    want_a = _expected(frames3[0], crops_a, 2, dsize, "swap_mul_sub_div", "f32", cvgs.IGNORE_AR, None)
    alias = Frame.__new__(Frame)  # B's frame: the first fh x fw x 3 bytes of A's tensor
    alias.cn, alias.cv_type = 3, cvgs.CV_8UC3
    alias.host = np.ascontiguousarray(np.frombuffer(want_a, np.uint8)[:fh * fw * 3].reshape(fh, fw, 3))
    alias.host_mat = cvgs.GpuMat.from_array(alias.host, cvgs.CV_8UC3)
    alias.dev_mat = cvgs.GpuMat(fh, fw, cvgs.CV_8UC3, tick.arena.ptr(0), fw * 3, owner=tick.arena.t)
    tick.frames = [frames3[0], alias]
    want_b = _expected(alias, crops_b, 2, dsize, "swap_mul_sub_div", "f32", cvgs.IGNORE_AR, None)
    for carrier in ("host", "tables"):
        _not_fused(lib, tick, tick.chains(carrier), [want_a, want_b], "B reads what A writes (%s)" % carrier, 2)


def test_what_the_tick_kernel_does_not_take_runs_one_by_one(device, lib, frames3):
    """Device tables with no hull and no vouch; differing target sizes; a 16U source; WRITE_PIXEL_2D_BATCH; CVGS_CHAIN_FORCE_GENERIC: n kernel
    nodes, a "not fused: ..." note, and the results of n cvgs_execute calls in order."""
    sets = [[WHOLE, (11, 13, 38, 19)], [(8, 4, 32, 16), ONE_PIXEL], [LAST_BYTE, (30, 20, 7, 5)]]
    tick = Tick(device, frames3, sets, (16, 8))
    _not_fused(lib, tick, tick.chains("tables", stated=False), tick.wants(), "tables, nothing stated", 3)
    _not_fused(lib, tick, tick.chains("host", flags=capi.CHAIN_FORCE_GENERIC), tick.wants(), "CHAIN_FORCE_GENERIC", 3)

    # differing target sizes: 16 x 8 and 33 x 7 in one call
    a, b = Tick(device, frames3[:1], sets[:1], (16, 8)), Tick(device, frames3[1:2], sets[1:2], (33, 7))
    low = a.chains("host") + b.chains("host")
    nodes, note = _nodes(lib, low, device)
    assert nodes == 2 and note.startswith("not fused:"), (nodes, note)
    a.arena.reset()
    b.arena.reset()
    assert _execute_many(lib, low).startswith("not fused:")
    a.arena.check(a.wants(), "16 x 8 beside 33 x 7")
    b.arena.check(b.wants(), "33 x 7 beside 16 x 8")

    # a 16U source: the interpreted kernel, chain by chain
    f16u = [Frame(device, 3, 40 + i, capi.DEPTH_16U) for i in range(2)]
    t16 = Tick(device, f16u, sets[:2], (16, 8), "mul_sub_div")
    _not_fused(lib, t16, t16.chains("host"), t16.wants(), "16U source", 2)

    # WRITE_PIXEL_2D_BATCH: packed fp32 pixels, one image per plane
    dsize, cn = (16, 8), 3
    f_type = cvgs.make_type(capi.DEPTH_32F, cn)
    arena = Arena(device, [2 * cn * 16 * 8 * 4] * 2)
    low, wants = [], []
    for i in range(2):
        fr, crops = frames3[i], sets[i]
        rd = cvgs.resize(fr.cv_type, cvgs.INTER_AREA, [fr.dev_mat.roi(*c) for c in crops], dsize)
        imgs = [cvgs.GpuMat(8, 16, f_type, arena.ptr(i) + z * cn * 16 * 8 * 4, 16 * cn * 4, owner=arena.t) for z in range(2)]
        low.append(cvgs.lower([rd, cvgs.multiply(f_type, MUL[:cn]), cvgs.subtract(f_type, SUB[:cn]), cvgs.divide(f_type, DIV[:cn]),
                               cvgs.write_batch(f_type, imgs)]))
        nchw = np.frombuffer(_expected(fr, crops, 2, dsize, "mul_sub_div", "f32", cvgs.IGNORE_AR, None), np.float32).reshape(2, cn, 8, 16)
        wants.append(np.ascontiguousarray(nchw.transpose(0, 2, 3, 1)).tobytes())  # packed pixels
    holder = Tick.__new__(Tick)
    holder.device, holder.arena = device, arena
    _not_fused(lib, holder, low, wants, "WRITE_PIXEL_2D_BATCH", 2)


# ---- 5. graph replay ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_area_tick_replays_on_new_frame_contents(device, lib):
    """A tick captured once and replayed: after the frames' contents change, the next replay gives the new contents' bytes -- nothing of a
    tick is resident between replays."""
    torch = _torch()
    frames = [Frame(device, 3, 90 + i) for i in range(3)]
    sets = [[WHOLE, (11, 13, 38, 19)], [(8, 4, 32, 16)], [LAST_BYTE, (2, 40, 90, 6)]]
    tick = Tick(device, frames, sets, (33, 7), "swap_mul_sub_div", "f32", cvgs.PRESERVE_AR, BG)
    low = tick.chains("tables")
    arr = cvgs.pack_chains(low)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.check(lib.cvgs_execute_many(arr, len(low), torch.cuda.current_stream().cuda_stream))
        assert lib.cvgs_last_error().decode().startswith("tick:")
        for round_ in range(3):
            tick.arena.reset()
            g.replay()
            torch.cuda.synchronize()
            tick.arena.check(tick.wants(), "replay %d" % round_)
            if round_ < 2:
                for i, fr in enumerate(frames):
                    fr.refill(10 * round_ + i)
                tick._wants = None
                torch.cuda.synchronize()
