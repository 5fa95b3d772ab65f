"""cvgs_head_decode on the GPU (include/cvgs_hip_ext.h: THE CONTRACT; csrc/k_head.hip): what the two kernels write equals
cvgs_head_decode_host byte for byte -- which tests/test_head_decode.py holds to an independent numpy model on the CPU -- with canaries on
both sides of every output and of scratch: every element type x form x objectness; N around the wave, the tile and the prefix's 256 tiles;
C around the wave; members placed none / all / first tile / last tile / exactly 256 / one per tile; ties across the 64-lane boundary;
padded strides; 16 different frames in one call; poisoned scratch; and head -> decode -> select -> tables -> tick captured once in a HIP
graph and replayed."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import head_cases as HC
from tests import head_model as M

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes of canary on either side of scratch
INF = float("inf")


def _torch():
    import torch
    return torch


class Job:
    """One frame's device buffers: the head's storage as the case lays it out, scratch and the five outputs inside canaries."""

    def __init__(self, device, c, poison_scratch=0xA5, with_index=True):
        torch = _torch()
        self.c, n = c, c.n
        self.head = torch.from_numpy(c.raw.reshape(-1).view(np.uint8).copy()).to(device)
        self.sb = cvgs.head_decode_scratch_bytes(n)
        assert self.sb == 1024 + 8 * n
        self.scratch = torch.full((self.sb + 2 * GUARD,), poison_scratch, dtype=torch.uint8, device=device)
        self.bo = torch.full((n + 2, 4), -77.0, dtype=torch.float32, device=device)
        self.so = torch.full((n + 2,), -77.0, dtype=torch.float32, device=device)
        self.ko = torch.full((n + 2,), 12345, dtype=torch.int32, device=device)
        self.io = torch.full((n + 2,), 12345, dtype=torch.int32, device=device)
        self.co = torch.full((3,), 999, dtype=torch.int32, device=device)
        self.desc = c.desc(head=self.head, scratch=self.scratch.data_ptr() + GUARD, boxes_out=self.bo[1:], scores_out=self.so[1:], classes_out=self.ko[1:],
                           count_out=self.co[1:], index_out=self.io[1:] if with_index else None)

    def result(self):
        n = self.c.n
        return (self.bo[1:n + 1].cpu().numpy(), self.so[1:n + 1].cpu().numpy(), self.ko[1:n + 1].cpu().numpy(), self.io[1:n + 1].cpu().numpy(), int(self.co[1]))

    def canaries_intact(self, poison_scratch=0xA5):
        s = self.scratch
        return bool((s[:GUARD] == poison_scratch).all() and (s[GUARD + self.sb:] == poison_scratch).all() and (self.bo[0] == -77).all() and (self.bo[-1] == -77).all()
                    and self.so[0] == -77 and self.so[-1] == -77 and self.ko[0] == 12345 and self.ko[-1] == 12345 and self.io[0] == 12345 and self.io[-1] == 12345
                    and self.co[0] == 999 and self.co[2] == 999)


def _run(device, cases):
    """ONE cvgs_head_decode call over `cases`; every frame against the host entry, every canary intact."""
    torch = _torch()
    assert len(cases) <= 16
    jobs = [Job(device, c) for c in cases]
    cvgs.head_decode(torch.cuda.current_stream(), [j.desc for j in jobs])
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        got, ref = j.result(), j.c.host()
        c = j.c
        assert HC.same(got, ref), "frame %d of %d (%s, elem %d, N %d, C %d, obj %d): count %d, host %d\n device %s\n host   %s" % (
            k, len(jobs), c.layout, c.elem, c.n, c.num_classes, c.obj_attr, got[4], ref[4], got[3][:40], ref[3][:40])
        assert j.canaries_intact(), "frame %d: a canary around scratch or an output changed" % k
    return jobs


def test_every_element_type_form_and_objectness_in_one_call(device, lib):
    """Three element types x row form ([N, A]) and column form ([A, N]) x objectness on and off: 12 frames of one call."""
    assert hasattr(lib, "cvgs_head_decode")
    cases = [HC.make(700 + k, 300 + k, 80 if k % 2 else 3, elem, layout, obj, hot=0.2)
             for k, (elem, layout, obj) in enumerate((e, l, o) for e in (M.F32, M.F16, M.BF16) for l in ("NA", "AN") for o in (False, True))]
    jobs = _run(device, cases)
    assert all(j.result()[4] > 10 for j in jobs)
    torch = _torch()
    j = Job(device, cases[0], with_index=False)  # the optional output
    cvgs.head_decode(torch.cuda.current_stream(), [j.desc])
    torch.cuda.synchronize()
    got, ref = j.result(), cases[0].host()
    assert HC.same(got[:3] + (ref[3], got[4]), ref) and (j.io == 12345).all() and j.canaries_intact()


def test_candidate_counts_around_the_wave_the_tile_and_the_prefix(device, lib):
    """N in {1, 63, 64, 65, 255, 256, 257, 8400} with C = 3, both forms in one call; N = 65535 with C = 2: 256 tiles, the most the prefix sees."""
    ns = (1, 63, 64, 65, 255, 256, 257, 8400)
    _run(device, [HC.make(800 + k, n, 3, M.F32, layout, hot=0.3, dirty=n >= 64) for k, n in enumerate(ns) for layout in ("NA", "AN")])
    jobs = _run(device, [HC.make(820, 65535, 2, M.BF16, "NA", obj=True, hot=0.1), HC.make(821, 65535, 2, M.F16, "AN", hot=0.1)])
    assert all(3000 < j.result()[4] < 20000 for j in jobs)


def _placed(seed, n, num_classes, elem, layout):
    """Every second candidate is a member whose winning class sits at the first, the last or the 64th index (cycling)."""
    v = HC.values(seed, n, num_classes, hot=0.0, dirty=False)
    where = (0, num_classes - 1, min(63, num_classes - 1))
    for i in range(0, n, 2):
        v[i, 4 + where[(i // 2) % 3]] = 0.5 + (i % 32) / 64.0
    return HC.Case(v, elem, layout, num_classes, 0.25, False), where


def test_class_counts_around_the_wave(device, lib):
    """C in {1, 2, 63, 64, 65, 80, 257} with N = 300, both forms (14 frames of one call); the winner at the first, last and 64th index."""
    made = [_placed(840 + k, 300, nc, (M.F32, M.BF16, M.F16)[k % 3], layout) for k, nc in enumerate((1, 2, 63, 64, 65, 80, 257)) for layout in ("NA", "AN")]
    jobs = _run(device, [c for c, _ in made])
    for j, (c, where) in zip(jobs, made):
        bo, so, ko, io, k = j.result()
        assert k == 150 and io[:k].tolist() == list(range(0, 300, 2)) and ko[:k].tolist() == [where[m % 3] for m in range(150)]


def _members_at(seed, n, rows, elem, layout):
    v = HC.values(seed, n, 3, hot=0.0, dirty=False)
    v[np.array(list(rows), dtype=np.int64), 4 + 1] = 0.875
    return HC.Case(v, elem, layout, 3, 0.25, False)


def test_member_placement(device, lib):
    """N = 1000 (three full tiles and a partial one), both forms: no member, all, only the first tile, only the last (partial) tile,
    exactly 256, exactly one per tile."""
    n = 1000
    places = {"none": [], "all": range(n), "first tile": range(3, 200, 2), "last tile": range(770, 1000, 3), "exactly 256": range(100, 100 + 512, 2),
              "one per tile": (255, 256, 767, 999)}
    cases = [_members_at(860 + k, n, rows, (M.F32, M.BF16)[k % 2], layout) for k, rows in enumerate(places.values()) for layout in ("NA", "AN")]
    jobs = _run(device, cases)
    for j, rows in zip(jobs, [r for r in places.values() for _ in range(2)]):
        bo, so, ko, io, k = j.result()
        assert k == len(list(rows)) and io[:k].tolist() == list(rows) and (io[k:] == -1).all()
    assert jobs[8].result()[4] == 256 and jobs[10].result()[4] == 4


def test_ties_across_the_lane_boundary(device, lib):
    """C = 130, equal class scores on both sides of a 64-lane boundary (63 | 64, 64 | 128, 0 | 129, 5 | 69 | 70, 127 | 128 | 129): the row
    form's reduction and the column form's walk both pick the lowest index."""
    pairs = [(63, 64), (64, 128), (0, 129), (5, 69, 70), (127, 128, 129), (1, 65, 129), (62, 63), (64, 65)]
    n = 8 * len(pairs)
    v = HC.values(880, n, 130, hot=0.0, dirty=False)
    for i in range(n):
        for cls in pairs[i % len(pairs)]:
            v[i, 4 + cls] = 0.75
    cases = [HC.Case(v, elem, layout, 130, 0.5, False) for elem in (M.F32, M.F16) for layout in ("NA", "AN")]
    for j in _run(device, cases):
        bo, so, ko, io, k = j.result()
        assert k == n and ko.tolist() == [pairs[i % len(pairs)][0] for i in range(n)] and (so == 0.75).all()
    # zeros of both signs: every class score is +-0.0, the lowest index wins and its sign bit is the one stored
    z = HC.values(881, 128, 130, hot=0.0, dirty=False)
    z[:, 4:] = np.where(np.arange(130)[None, :] % 2 == (np.arange(128)[:, None] % 2), 0.0, -0.0)
    for j in _run(device, [HC.Case(z, M.F32, layout, 130, 0.0, False) for layout in ("NA", "AN")]):
        bo, so, ko, io, k = j.result()
        assert k == 128 and not ko.any() and (np.signbit(so) == (np.arange(128) % 2 == 1)).all()


def test_padded_strides_in_both_forms(device, lib):
    """Padded rows (row form), padded channels and every-second-element storage (column form), all three element types."""
    _run(device, [HC.make(890 + k, 515 + k, (2, 80, 7)[k % 3], elem, layout, obj=k % 2 == 1, hot=0.2, lead=(0, 2)[k % 2])
                  for k, (elem, layout) in enumerate((e, l) for e in (M.F32, M.F16, M.BF16) for l in ("NA_pad", "AN_pad", "NA_x2"))])


def test_sixteen_frames_of_different_shapes_types_and_layouts_in_one_call(device, lib):
    cases = HC.seeded_cases()
    assert len({(c.elem, c.layout, c.obj_attr >= 0, c.num_classes) for c in cases[:16]}) == 16 and len({c.n for c in cases[:16]}) >= 8
    _run(device, cases[:16])
    _run(device, cases[16:])


def test_scratch_contents_do_not_matter(device, lib):
    """The same call over scratch poisoned with 0x00 and with 0xFF (NaN bits, negative counts), then over its own leftovers: same outputs."""
    torch = _torch()
    for c in (HC.make(895, 700, 80, M.BF16, "AN", hot=0.2), HC.make(896, 700, 5, M.F32, "NA", obj=True, hot=0.2)):
        ref = c.host()
        for poison in (0x00, 0xFF):
            j = Job(device, c, poison)
            cvgs.head_decode(torch.cuda.current_stream(), [j.desc])
            cvgs.head_decode(torch.cuda.current_stream(), [j.desc])  # and over its own leftovers
            torch.cuda.synchronize()
            assert HC.same(j.result(), ref) and j.canaries_intact(poison)


def test_head_to_tick_in_one_graph(device, lib):
    """A copy writes the heads (the network), then cvgs_head_decode, cvgs_boxes_select, cvgs_plane_tables_from_boxes and a bilinear K1 tick
    over the device tables, captured ONCE on one stream.  A captured launch's descriptors are fixed at capture, so the one decode call
    holds BOTH descriptors -- a bf16 [A, N] head and an fp32 [N, A] head with outputs of the same size -- and the graph is replayed twice
    over different heads: each replay's tensors are bit-identical to the same tick run from boxes the two HOST entries produced."""
    torch = _torch()
    from tests.test_gpu_boxes import Frame, _chain, _out_tensor
    W, Hh, dsize, n, nc, max_out, thr = 320, 200, (64, 128), 900, 80, 24, 0.25
    frame = Frame(device, W, Hh, cvgs.CV_8UC3, W * 3 + 8, seed=21)
    xform = cvgs.letterbox_xform((W, Hh), (160, 160), cvgs.PRESERVE_AR)
    kinds = ((M.BF16, "AN"), (M.F32, "NA"))
    rounds = [[HC.Case(HC.values(900 + 10 * r + k, n, nc, hot=0.08, extent=160.0), elem, layout, nc, thr, False) for k, (elem, layout) in enumerate(kinds)]
              for r in range(2)]
    staged = [[torch.from_numpy(c.raw.reshape(-1).view(np.uint8).copy()).to(device) for c in rnd] for rnd in rounds]
    jobs = [Job(device, c) for c in rounds[0]]  # the buffers the graph works on; the heads are overwritten by the graph's first nodes
    sources = [torch.zeros_like(t) for t in staged[0]]

    def select_desc(j, sel):
        return cvgs.box_select_desc((W, Hh), j.bo[1:], j.so[1:], n, sel["scratch"], sel["bo"], sel["co"], thr, 0.5, 256, max_out, cvgs.CAND_CXCYWH_F32, 4, 1,
                                    j.ko[1:], 1, j.co[1:], xform, sel["so"], sel["io"])
    sels, tables, outs, tdescs, lows = [], [], [], [], []
    for j in jobs:
        sel = dict(scratch=torch.zeros((cvgs.boxes_select_scratch_bytes(n, 256),), dtype=torch.uint8, device=device),
                   bo=torch.zeros((max_out, 4), dtype=torch.float32, device=device), co=torch.zeros((1,), dtype=torch.int32, device=device),
                   so=torch.zeros((max_out,), dtype=torch.float32, device=device), io=torch.zeros((max_out,), dtype=torch.int32, device=device))
        sel["desc"] = select_desc(j, sel)
        table = torch.zeros((max_out, 48), dtype=torch.uint8, device=device)
        out = _out_tensor(device, max_out, 3, dsize)
        tdescs.append(cvgs.box_table_desc(frame.mat, sel["bo"], table, max_out, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYXY_F32, sel["co"], None))
        ops = _chain(cvgs.resize_boxes(frame.mat, table, max_out, dsize), 3, out, dsize)
        assert cvgs.kernel_name(*ops).startswith("k1_u8c3")
        lows.append(cvgs.lower(ops))
        sels.append(sel)
        tables.append(table)
        outs.append(out)
    arr = cvgs.pack_chains(lows)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        for j, src in zip(jobs, sources):
            j.head.copy_(src)
        cvgs.head_decode(s, [j.desc for j in jobs])
        cvgs.boxes_select(s, [sel["desc"] for sel in sels])
        cvgs.plane_tables_from_boxes(s, tdescs)
        capi.check(lib.cvgs_execute_many(arr, len(lows), cvgs.stream_handle(s)))
    torch.cuda.synchronize()
    assert all((out == -5.0).all() for out in outs), "capture itself must not run anything"
    results = []
    for r, rnd in enumerate(rounds):
        for src, st in zip(sources, staged[r]):
            src.copy_(st)
        g.replay()
        torch.cuda.synchronize()
        for k, c in enumerate(rnd):
            ref = c.host()
            assert HC.same(jobs[k].result(), ref) and jobs[k].canaries_intact() and 20 < ref[4] < 300
            hd = cvgs.box_select_desc((W, Hh), None, None, n, None, None, None, thr, 0.5, 256, max_out, cvgs.CAND_CXCYWH_F32, 4, 1, None, 1, None, xform)
            hb, hk, hs, hi = cvgs.boxes_select_host(hd, ref[0], ref[1], ref[2], ref[4])
            assert 3 <= hk <= max_out and int(sels[k]["co"][0]) == hk and (sels[k]["bo"].cpu().numpy().view(np.uint32) == hb.view(np.uint32)).all()
            # the same tick from host-decoded, host-selected boxes
            db = torch.from_numpy(hb).to(device)
            dc = torch.tensor([hk], dtype=torch.int32, device=device)
            htable = torch.zeros_like(tables[k])
            hout = _out_tensor(device, max_out, 3, dsize)
            s = torch.cuda.current_stream()
            cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(frame.mat, db, htable, max_out, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYXY_F32, dc, None)])
            cvgs.executeOperations(s, *_chain(cvgs.resize_boxes(frame.mat, htable, max_out, dsize), 3, hout, dsize))
            torch.cuda.synchronize()
            assert torch.equal(outs[k], hout), "replay %d, head %d" % (r, k)
            results.append(outs[k].clone())
    assert not torch.equal(results[0], results[2]) and not torch.equal(results[1], results[3])
