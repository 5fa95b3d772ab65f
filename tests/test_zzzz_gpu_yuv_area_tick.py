"""INTER_AREA crop chains of NV12 / NV21 decoder surfaces in ONE cvgs_execute_many launch (csrc/k_yuv_area.hip: k_yuv_area_fast_many;
csrc/cvgs_api.cpp: TickFamily::yuv_area).

Every tensor is compared BIT FOR BIT with the fp32 restatement of the contract (tests/yuv_area_model.py) and with the same chains sent one
at a time through cvgs_execute; the tensors of a tick sit side by side in one allocation with a guard band of sentinel bytes around and
between them, and the whole allocation is compared (the arena, the node count and the tick note are tests/test_zzzz_gpu_area_tick.py's).
Surfaces are the model's 98 x 62, crops its CROPS / EVEN_CROPS (even origins: the layout's rule; odd widths and heights included), targets
16 x 8, 33 x 7 and 70 x 6 (two column tiles, a partial row tile): one lane is one pixel and nothing depends on the tile size, so these are
the smallest shapes at which the segment mapping can go wrong (ragged batches, used < batch, 128 chains, every descriptor carrier).

Collected behind every other module of the suite, so that it takes no existing item's place in its order."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as A
from tests import test_gpu_yuv_area as Y
from tests import test_zzzz_gpu_area_tick as T
from tests import yuv_area_model as M

pytestmark = pytest.mark.gpu

BG = [11.0, 22.5, 33.0, 44.0]
WHOLE = (0, 0, M.SRC_W, M.SRC_H)
SHRINK_X_GROW_Y = (2, 40, 90, 4)  # for the 70 x 6 target: 90 -> 70 columns, 4 -> 6 rows
NOTE_CAPTURE = "not fused: host descriptors beyond the kernel arguments on a capturing stream"
NOTE_NO_HULL = "not fused: chains not independent, or no hull stated (read.table_src_lo / _hi) and not vouched"


def _torch():
    import torch
    return torch


class Surface:
    """A seeded 98 x 62 surface of a layout: the host array, the luma GpuMat over it and the luma GpuMat over its device copy."""

    def __init__(self, device, name, seed):
        self.name, self.layout = name, M.LAYOUTS[name]
        self.host = M.make_surface(self.layout, seed=0x8A2E + 101 * seed)
        self.host_mat = M.luma_mat(self.host, self.layout)
        self.t = _torch().from_numpy(self.host.view(np.uint8).reshape(self.host.shape[0], -1).copy()).to(device)
        self.dev_mat = M.luma_mat(self.host, self.layout, data=self.t.data_ptr())
        self.dev_mat.owner = self.t

    def refill(self, seed):
        """New contents in the SAME device bytes."""
        rng = np.random.default_rng(0xB0B + seed)
        self.host[:] = rng.integers(0, 256, self.host.shape).astype(self.host.dtype)
        self.t.copy_(_torch().from_numpy(self.host.view(np.uint8).reshape(self.host.shape[0], -1).copy()))


def _expected(surf, crops, used, dsize, alpha, prog, out, ar=cvgs.IGNORE_AR, bg=None, tsplit=False, params=None):
    """The bytes the chain must store, from the fp32 restatement; the geometry is the plane table of the same read over host views.  The
    planes of one chain do not depend on each other, so every distinct crop is computed once."""
    cn = 4 if alpha else 3
    yuv = Y.YUV[surf.name] + (alpha,)

    def values(cs, n_used, P=None):
        rd = Y.read(surf.host_mat, surf.name, cs, dsize, alpha, ar, bg, n_used)
        low = cvgs.lower(T._chain(rd, cn, dsize, prog, out, (16, None), tsplit))
        vals, depth = M.yuv_area_chain(M.yuv_area_plane_f32, surf.host, surf.layout, cs, P if P is not None else A.plane_params(rd), dsize, n_used,
                                       list(low.desc.read.background), yuv, A.chain_ops(low.desc), np.float32)
        assert depth == T.OUT_DEPTH[out]
        return vals

    if params is not None:
        vals = values(list(crops), used, params)
    else:
        uniq = list(dict.fromkeys(crops))
        read_vals, default = values(uniq, len(uniq)), values(uniq[:1], 0)[0]
        vals = np.stack([read_vals[uniq.index(c)] if z < used else default for z, c in enumerate(crops)])
    vals = vals.transpose(3, 0, 1, 2) if tsplit else vals.transpose(0, 3, 1, 2)  # CNHW / NCHW
    return A.store_bits(vals, T.OUT_DEPTH[out]).tobytes()


class Tick:
    """n chains of one shape: chain i reads `crop_sets[i]` of surfaces[i] (the first used[i] of them) into tensor i of one arena.  It has
    what tests/test_zzzz_gpu_area_tick.py's helpers ask of a tick: device, arena, chains(carrier), wants()."""

    def __init__(self, device, surfaces, crop_sets, dsize, prog="swap_mul_sub_div", out="f32", alpha=0, ar=cvgs.IGNORE_AR, bg=None, used=None,
                 tsplit=False):
        self.device, self.surfaces, self.crop_sets, self.dsize, self.prog, self.out = device, surfaces, crop_sets, dsize, prog, out
        self.alpha, self.ar, self.bg, self.tsplit = alpha, ar, bg, tsplit
        self.used = [len(c) for c in crop_sets] if used is None else used
        self.cn = 4 if alpha else 3
        self.arena = T.Arena(device, [len(c) * self.cn * dsize[0] * dsize[1] * T.OUT_BYTES[out] for c in crop_sets])
        self.keep = []
        self._wants = None

    def chains(self, carrier, stated=True, flags=0, slots=None):
        """The lowered chains: carrier "tables" (device plane tables, the hull stated from the host views unless stated=False) or "host";
        slots[i]: the arena tensor chain i writes (its own by default)."""
        low = []
        for i, (sf, crops) in enumerate(zip(self.surfaces, self.crop_sets)):
            rd = Y.read(sf.dev_mat, sf.name, crops, self.dsize, self.alpha, self.ar, self.bg, self.used[i])
            if carrier == "tables":
                tab = _torch().frombuffer(bytearray(cvgs.build_plane_table(rd)), dtype=_torch().uint8).to(self.device)
                self.keep.append(tab)
                rd.table = tab.data_ptr()
                if not stated:
                    rd.mats = None  # no host views at hand: the facade cannot compute a hull
            slot = i if slots is None else slots[i]
            low.append(cvgs.lower(T._chain(rd, self.cn, self.dsize, self.prog, self.out, (self.arena.ptr(slot), self.arena.t), self.tsplit), flags))
        return low

    def wants(self):
        if self._wants is None:
            self._wants = [_expected(sf, crops, u, self.dsize, self.alpha, self.prog, self.out, self.ar, self.bg, self.tsplit)
                           for sf, crops, u in zip(self.surfaces, self.crop_sets, self.used)]
        return self._wants


@pytest.fixture(scope="module")
def nv12(device):
    return [Surface(device, "NV12", s) for s in range(3)]


@pytest.fixture(scope="module")
def nv21(device):
    return [Surface(device, "NV21", 10 + s) for s in range(3)]


RAGGED = [list(M.CROPS[:4]), list(M.CROPS[4:9]), [M.CROPS[13]]]  # 4 / 5 / 1 crops, odd widths and heights among them


# ---- 1. one kernel node -------------------------------------------------------------------------------------------------------------------
def test_three_nv12_area_chains_are_one_kernel_node(device, lib, nv12):
    """Three independent same-shape NV12 AREA chains with ragged batches (4 / 5 / 1 crops, host descriptors, swap-mul-sub-div, fp32)
    capture as exactly ONE kernel node and the call's note says "tick: ..."; launched eagerly they store the same bytes as one cvgs_execute
    per chain.  (Before the tick kernel of this kind: three nodes, "not fused: no tick kernel for this read kind".)"""
    tick = Tick(device, nv12, RAGGED, (16, 8))
    low = tick.chains("host")
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 1, "%d kernel nodes (%s)" % (nodes, note)
    assert note.startswith("tick:"), note
    T._fused_and_single(lib, tick, "host", "three ragged chains")


# ---- 2. kernel variants and geometry ------------------------------------------------------------------------------------------------------
def test_nv21_alpha_fp16_cnhw(device, lib, nv21):
    """NV21 with alpha (C4), mul-sub-div, fp16 (the trailing cast inside the store), TENSOR_T_SPLIT (CNHW), a 33 x 7 target."""
    sets = [[WHOLE, M.CROPS[1]], [M.CROPS[14], M.CROPS[9]], [M.CROPS[8], M.CROPS[12]]]
    tick = Tick(device, nv21, sets, (33, 7), "mul_sub_div", "f16", 1, cvgs.IGNORE_AR, BG, tsplit=True)
    for carrier in ("tables", "host"):
        T._fused_and_single(lib, tick, carrier, "NV21 C4 fp16 CNHW")


def test_interpreted_program_bf16_and_fp32_and_mul_sub_div(device, lib, nv12, nv21):
    """One extra `add` -> the interpreted program: NV12 into a bf16 NCHW tensor (a default-value plane among them), NV21 with alpha into
    fp32; mul-sub-div into fp32 and swap-mul-sub-div into bf16."""
    sets = [[WHOLE, M.CROPS[14]], [M.CROPS[1]], [M.CROPS[10], M.CROPS[13]]]
    T._fused_and_single(lib, Tick(device, nv12, sets, (16, 8), "interp", "bf16", 0, cvgs.IGNORE_AR, BG, used=[2, 1, 1]), "tables", "NV12 interp bf16")
    T._fused_and_single(lib, Tick(device, nv21, sets, (16, 8), "interp", "f32", 1, cvgs.IGNORE_AR, BG), "host", "NV21 C4 interp fp32")
    T._fused_and_single(lib, Tick(device, nv12, sets, (16, 8), "mul_sub_div", "f32"), "host", "NV12 mul-sub-div fp32")
    T._fused_and_single(lib, Tick(device, nv21, sets, (16, 8), "swap_mul_sub_div", "bf16", 1), "tables", "NV21 C4 swap bf16")


def test_unused_planes_a_letterbox_window_and_two_column_tiles(device, lib, nv12):
    """used_planes < batch with a non-zero background that runs through the program; PRESERVE_AR windows with background columns / rows;
    a 70 x 6 target (two column tiles, a partial row tile) over a view that shrinks on x and grows on y."""
    sets = [[SHRINK_X_GROW_Y], [M.CROPS[1], M.CROPS[14], WHOLE], [M.CROPS[2], M.CROPS[3]]]
    for ar in (cvgs.PRESERVE_AR, cvgs.IGNORE_AR):
        tick = Tick(device, nv12, sets, (70, 6), "swap_mul_sub_div", "f32", 0, ar, BG, used=[1, 2, 2])
        for carrier in ("tables", "host"):
            T._fused_and_single(lib, tick, carrier, "ragged 70x6 ar %d" % ar)


# ---- 3. device tables ---------------------------------------------------------------------------------------------------------------------
def test_a_table_built_on_the_host_for_the_bilinear_kind(device, lib, nv21):
    """cvgs_plane_table_build of the reads spelled NV12_RESIZE_LINEAR (even crops), copied to the device and handed to the AREA chains with
    the hull of their views stated: one kernel node, the restatement's bytes."""
    torch = _torch()
    even = list(M.EVEN_CROPS)
    sets = [even[:3], even[3:7], even[7:]]
    tick = Tick(device, nv21, sets, (33, 7), "swap_mul_sub_div", "f16")
    low, keep = [], []
    for i, (sf, crops) in enumerate(zip(nv21, sets)):
        raw = cvgs.build_plane_table(Y.read(sf.dev_mat, sf.name, crops, (33, 7), 0, interp=cvgs.INTER_LINEAR))
        keep.append(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(device))
        rd = Y.read(sf.dev_mat, sf.name, crops, (33, 7), 0)
        rd.table = keep[-1].data_ptr()
        low.append(cvgs.lower(T._chain(rd, 3, (33, 7), "swap_mul_sub_div", "f16", (tick.arena.ptr(i), tick.arena.t))))
        assert low[-1].desc.read.flags & capi.READ_FLAG_TABLE_ON_DEVICE and low[-1].desc.read.table_src_lo and low[-1].desc.read.table_src_hi
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 1 and note.startswith("tick:"), (nodes, note)
    tick.arena.reset()
    assert T._execute_many(lib, low).startswith("tick:")
    tick.arena.check(tick.wants(), "tables built for the bilinear kind")


def test_tables_from_device_boxes_stated_unstated_and_vouched(device, lib, nv12):
    """cvgs_plane_tables_from_boxes (read_kind NV12_RESIZE_LINEAR, the kind it accepts) writes the tables of two surfaces, one box invalid
    in each; an AREA tick reads them in one launch.  Valid planes equal the host-described result, the invalid ones are the background run
    through the program.  The same chains with no hull stated and no vouch run one by one with the note that says so; vouched, they are one
    node again."""
    torch = _torch()
    surfs = nv12[:2]
    rects = [[WHOLE, (10, 12, 38, 18), (4, 6, 0, 10), (56, 38, 42, 24)], [(8, 4, 32, 16), (2, 2, 48, 24), (20, 30, 32, 6), (6, 8, 10, 0)]]
    valid = [[True, True, False, True], [True, True, True, False]]
    n, dsize = 4, (16, 8)
    s = torch.cuda.current_stream()
    keep, tables, descs = [], [], []
    for sf, r in zip(surfs, rects):
        boxes = torch.tensor(r, dtype=torch.int32, device=device)
        table = torch.zeros((n, 48), dtype=torch.uint8, device=device)
        keep += [boxes, table]
        tables.append(table)
        descs.append(cvgs.box_table_desc(sf.dev_mat, boxes, table, n, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYWH_I32, None, None,
                                         capi.READ_NV12_RESIZE_LINEAR, capi.YUV_NV12))
    cvgs.plane_tables_from_boxes(s, descs)
    torch.cuda.synchronize()
    arena = T.Arena(device, [n * 3 * 16 * 8 * 4] * 2)

    def chains(hull):
        low = []
        for i, (sf, table) in enumerate(zip(surfs, tables)):
            rd = cvgs.resize_boxes(sf.dev_mat, table, n, dsize, BG, yuv=Y.YUV["NV12"] + (0,), layout=capi.YUV_NV12, interp=cvgs.INTER_AREA)
            assert rd.kind == capi.READ_NV12_RESIZE_AREA
            if hull != "stated":
                rd.table_hull = None
                rd.table_vouched = hull == "vouched"
            low.append(cvgs.lower(T._chain(rd, 3, dsize, "swap_mul_sub_div", "f32", (arena.ptr(i), arena.t))))
        return low

    wants = []
    for sf, r, ok in zip(surfs, rects, valid):
        good = [c for c, v in zip(r, ok) if v]
        P = iter(A.plane_params(Y.read(sf.host_mat, "NV12", good, dsize, 0)))
        first = A.plane_params(Y.read(sf.host_mat, "NV12", [WHOLE], dsize, 0))[0]
        params = [next(P) if v else dict(first, x1=0, y1=0, x2=-1, y2=-1) for v in ok]  # the invalid entry: the empty window
        crops = [c if v else WHOLE for c, v in zip(r, ok)]
        wants.append(_expected(sf, crops, n, dsize, 0, "swap_mul_sub_div", "f32", cvgs.IGNORE_AR, BG, params=params))
    bgp = (np.array(BG[:3], np.float32)[::-1] * np.float32(0.3) - np.array(T.SUB[:3], np.float32)) / np.array(T.DIV[:3], np.float32)
    for hull, n_nodes, start in (("stated", 1, "tick:"), ("unstated", 2, NOTE_NO_HULL), ("vouched", 1, "tick:")):
        low = chains(hull)
        nodes, note = T._nodes(lib, low, device)
        assert nodes == n_nodes and note.startswith(start), (hull, nodes, note)
        arena.reset()
        assert T._execute_many(lib, low).startswith(start)
        got = arena.check(wants, "tables from device boxes, hull %s" % hull)
        for i in range(2):
            planes = got[arena.offsets[i]:arena.offsets[i] + arena.sizes[i]].view(np.float32).reshape(n, 3, 8, 16)
            for z in range(n):
                if not valid[i][z]:
                    assert (planes[z] == bgp[:, None, None]).all(), "surface %d plane %d: an invalid box is all background" % (i, z)
    arena.reset()
    T._execute_each(lib, chains("stated"))
    arena.check(wants, "tables from device boxes, chain by chain")


# ---- 4. carriers and limits ---------------------------------------------------------------------------------------------------------------
def _tiny_crops(n, seed, distinct=None):
    """n crops of 1 .. 9 samples a side at even origins; distinct: drawn from that many different ones."""
    rng = np.random.default_rng(seed)
    some = [(2 * int(rng.integers(0, (M.SRC_W - 9) // 2)), 2 * int(rng.integers(0, (M.SRC_H - 9) // 2)), int(rng.integers(1, 10)), int(rng.integers(1, 10)))
            for _ in range(distinct or n)]
    return [some[i % len(some)] for i in range(n)]


def test_max_chains_of_one_plane_each(device, lib, nv12):
    """n = CVGS_MAX_CHAINS chains of one plane each (grid z = 128), 4 x 4 targets of tiny crops, both carriers."""
    n = capi.MAX_CHAINS
    crops = _tiny_crops(n, 77)
    tick = Tick(device, [nv12[i % 3] for i in range(n)], [[c] for c in crops], (4, 4), "mul_sub_div", "f32")
    for carrier in ("tables", "host"):
        T._fused_and_single(lib, tick, carrier, "128 chains")


def test_large_argument_block_and_the_staged_host_table(device, lib, nv12):
    """Host descriptors: 3 x 100 planes travel in the large kernel-argument block (one captured node).  17 x 61 planes are more than 1024
    in all: launched eagerly they take the staged host table (its pooled slot rides on the launch); on a capturing stream the tick is
    not fused, says why, and its 17 launches store the same bytes.  4 x 4 targets of tiny crops."""
    torch = _torch()
    t300 = Tick(device, nv12, [_tiny_crops(100, 300 + i, 20) for i in range(3)], (4, 4), "swap_mul_sub_div", "f32", used=[100, 97, 100], bg=BG)
    T._fused_and_single(lib, t300, "host", "300 planes inline")
    sf = [nv12[i % 3] for i in range(17)]
    t1037 = Tick(device, sf, [_tiny_crops(61, 400 + i % 3, 12) for i in range(17)], (4, 4), "swap_mul_sub_div", "f32")
    low = t1037.chains("host")
    for round_ in range(2):  # twice: the second tick recycles the pooled slot of the first
        t1037.arena.reset()
        note = T._execute_many(lib, low)
        assert note.startswith("tick:"), note
        t1037.arena.check(t1037.wants(), "1037 planes, staged host table, round %d" % round_)
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 17 and note == NOTE_CAPTURE, (nodes, note)
    arr = cvgs.pack_chains(low)
    side = torch.cuda.Stream()
    t1037.arena.reset()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.check(lib.cvgs_execute_many(arr, len(low), torch.cuda.current_stream().cuda_stream))
        assert lib.cvgs_last_error().decode() == NOTE_CAPTURE
        g.replay()
        torch.cuda.synchronize()
    t1037.arena.check(t1037.wants(), "1037 planes, captured chain by chain")


# ---- 5. what must not fuse still runs in order --------------------------------------------------------------------------------------------
def test_what_the_tick_kernel_does_not_take_runs_one_by_one(device, lib, nv12):
    """P010 surfaces; CVGS_CHAIN_FORCE_GENERIC; differing target sizes; a packed fp32 write; two chains that write ONE tensor: n kernel
    nodes, a "not fused: ..." note, and the results of n cvgs_execute calls in order."""
    sets = [[WHOLE, M.CROPS[9]], [M.CROPS[10], M.CROPS[1]], [M.CROPS[14], M.CROPS[7]]]
    p010 = [Surface(device, "P010", 20 + s) for s in range(2)]
    t10 = Tick(device, p010, sets[:2], (16, 8), "mul_sub_div", "f32")
    T._not_fused(lib, t10, t10.chains("host"), t10.wants(), "P010", 2)
    tick = Tick(device, nv12, sets, (16, 8))
    T._not_fused(lib, tick, tick.chains("host", flags=capi.CHAIN_FORCE_GENERIC), tick.wants(), "CHAIN_FORCE_GENERIC", 3)

    # differing target sizes: 16 x 8 and 33 x 7 in one call
    a, b = Tick(device, nv12[:1], sets[:1], (16, 8)), Tick(device, nv12[1:2], sets[1:2], (33, 7))
    low = a.chains("host") + b.chains("host")
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 2 and note.startswith("not fused:"), (nodes, note)
    a.arena.reset()
    b.arena.reset()
    assert T._execute_many(lib, low).startswith("not fused:")
    a.arena.check(a.wants(), "16 x 8 beside 33 x 7")
    b.arena.check(b.wants(), "33 x 7 beside 16 x 8")

    # WRITE_PIXEL_3D: packed fp32 pixels
    dsize, cn = (16, 8), 3
    f_type = cvgs.make_type(capi.DEPTH_32F, cn)
    arena = T.Arena(device, [2 * cn * 16 * 8 * 4] * 2)
    low, wants = [], []
    for i in range(2):
        sf, crops = nv12[i], sets[i]
        rd = Y.read(sf.dev_mat, "NV12", crops, dsize, 0)
        out = cvgs.GpuMat(2, cn * 16 * 8, cvgs.CV_32FC1, arena.ptr(i), cn * 16 * 8 * 4, owner=arena.t)
        low.append(cvgs.lower([rd, cvgs.multiply(f_type, T.MUL[:cn]), cvgs.subtract(f_type, T.SUB[:cn]), cvgs.divide(f_type, T.DIV[:cn]),
                               cvgs.write(f_type, out, dsize)]))
        assert low[-1].desc.write.kind == capi.WRITE_PIXEL_3D
        nchw = np.frombuffer(_expected(sf, crops, 2, dsize, 0, "mul_sub_div", "f32"), np.float32).reshape(2, cn, 8, 16)
        wants.append(np.ascontiguousarray(nchw.transpose(0, 2, 3, 1)).tobytes())  # packed pixels
    holder = Tick.__new__(Tick)
    holder.device, holder.arena = device, arena
    T._not_fused(lib, holder, low, wants, "packed fp32 write", 2)

    # two chains write ONE tensor: the second wins, the other tensor of the arena stays untouched
    two = Tick(device, nv12[:2], sets[:2], (16, 8))
    untouched = bytes([T.SENTINEL]) * two.arena.sizes[1]
    T._not_fused(lib, two, two.chains("host", slots=[0, 0]), [two.wants()[1], untouched], "two chains, one tensor", 2)


# ---- 6. chroma under another chain's tensor -----------------------------------------------------------------------------------------------
def test_chroma_rows_inside_another_chains_tensor_keep_the_chains_in_order(device, lib, nv12):
    """Chain B's surface is laid out with its luma rows OUTSIDE chain A's tensor and its chroma rows INSIDE it (uv_offset points there).
    With host descriptors the independence check must count the chroma rows of this read kind: the tick is not fused, and B's result is
    the one computed from the bytes A stored.  (A check that counts B's luma rows only fuses the two and lets B read what was there before.)"""
    dsize, fw, fh = (16, 8), 32, 16
    crops_a, crops_b = [WHOLE, M.CROPS[9]], [(0, 0, fw, fh), (2, 2, 20, 11)]
    size = 2 * 3 * 16 * 8 * 4
    arena = T.Arena(device, [fw * fh, size, size])  # B's luma rows, A's tensor (B's chroma rows are its first bytes), B's tensor
    want_a = _expected(nv12[0], crops_a, 2, dsize, 0, "swap_mul_sub_div", "f32")
    luma = np.random.default_rng(0xC0DE).integers(0, 256, (fh, fw)).astype(np.uint8)
    b = Surface.__new__(Surface)  # B's surface as the model reads it: the luma rows on top, the chroma rows where its 62-row layout has them
    b.name, b.layout = "NV12", capi.YUV_NV12
    b.host = np.zeros((M.SRC_H * 3 // 2, fw), np.uint8)
    b.host[:fh] = luma
    b.host[M.SRC_H:M.SRC_H + fh // 2] = np.frombuffer(want_a, np.uint8)[:fh // 2 * fw].reshape(fh // 2, fw)
    b.host_mat = cvgs.GpuMat(M.SRC_H, fw, cvgs.CV_8UC1, b.host.ctypes.data, fw, owner=b.host)
    want_b = _expected(b, crops_b, 2, dsize, 0, "swap_mul_sub_div", "f32")
    dev_b = cvgs.GpuMat(fh, fw, cvgs.CV_8UC1, arena.ptr(0), fw, owner=arena.t)
    dev_b.uv_offset = arena.ptr(1) - arena.ptr(0)
    low = [cvgs.lower(T._chain(Y.read(nv12[0].dev_mat, "NV12", crops_a, dsize, 0), 3, dsize, "swap_mul_sub_div", "f32", (arena.ptr(1), arena.t))),
           cvgs.lower(T._chain(Y.read(dev_b, "NV12", crops_b, dsize, 0), 3, dsize, "swap_mul_sub_div", "f32", (arena.ptr(2), arena.t)))]
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 2 and note == "not fused: chains not independent", (nodes, note)
    arena.reset()
    arena.t[arena.offsets[0]:arena.offsets[0] + fw * fh] = _torch().from_numpy(luma.reshape(-1)).to(device)
    assert T._execute_many(lib, low) == "not fused: chains not independent"
    arena.check([luma.tobytes(), want_a, want_b], "B's chroma rows are A's stored bytes")


# ---- 7. graph replay ----------------------------------------------------------------------------------------------------------------------
def test_a_captured_tick_over_device_tables_replays_on_new_surface_contents(device, lib):
    """A tick captured once and replayed: after the surfaces' contents change, the next replay gives the new contents' bytes -- nothing of
    a tick is resident between replays."""
    torch = _torch()
    surfs = [Surface(device, "NV12", 90 + i) for i in range(3)]
    sets = [[WHOLE, M.CROPS[9]], [M.CROPS[10]], [M.CROPS[14], M.CROPS[8]]]
    tick = Tick(device, surfs, sets, (33, 7), "swap_mul_sub_div", "f32", 0, cvgs.PRESERVE_AR, BG)
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
                for i, sf in enumerate(surfs):
                    sf.refill(10 * round_ + i)
                tick._wants = None
                torch.cuda.synchronize()
