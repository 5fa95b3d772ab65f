"""cvgs_boxes_select on the GPU (include/cvgs_hip_ext.h: THE CONTRACT; csrc/k_select.hip): what the two kernels write equals
cvgs_boxes_select_host byte for byte -- which tests/test_box_select.py holds to an independent restatement on the CPU -- with canaries
around every output and around scratch; member counts around every boundary of the kernels (the wave, the 256-candidate tile, pre_nms_k =
1024) at max_candidates = 65535 behind a device count; 16 frames of different shapes in one call; an interleaved [n, 6] head read in place;
equal scores across wave and tile boundaries; and detector -> select -> table -> tick captured once in a HIP graph and replayed."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import select_cases as SC
from tests import select_model as M

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes / elements of canary on either side


def _torch():
    import torch
    return torch


class Job:
    """One frame's device buffers: the candidates as the case lays them out, a device count, scratch and outputs inside canaries."""

    def __init__(self, device, c, poison_scratch=0xA5):
        torch = _torch()
        self.c, p = c, c.p
        if c.head is not None:
            self.head = torch.from_numpy(c.head).to(device)
            base = self.head.data_ptr()
            ptrs = dict(boxes=base, scores=base + 16, classes=base + 20 if c.classes is not None else None)
        else:
            self.b = torch.from_numpy(np.ascontiguousarray(c.boxes)).to(device)
            self.s = torch.from_numpy(np.ascontiguousarray(c.scores)).to(device)
            self.k = torch.from_numpy(np.ascontiguousarray(c.classes)).to(device) if c.classes is not None else None
            ptrs = dict(boxes=self.b, scores=self.s, classes=self.k)
        self.count = None if c.count is None else torch.tensor([c.count], dtype=torch.int32, device=device)
        sb = cvgs.boxes_select_scratch_bytes(c.n, p.pre_k)
        assert sb == 8 + ((28 * p.pre_k + 7) & ~7)
        self.sb = sb
        self.scratch = torch.full((sb + 2 * GUARD,), poison_scratch, dtype=torch.uint8, device=device)
        self.bo = torch.full((p.max_out + 2, 4), -77.0, dtype=torch.float32, device=device)
        self.so = torch.full((p.max_out + 2,), -77.0, dtype=torch.float32, device=device)
        self.io = torch.full((p.max_out + 2,), 12345, dtype=torch.int32, device=device)
        self.co = torch.full((3,), 999, dtype=torch.int32, device=device)
        self.desc = c.desc(count=self.count, scratch=self.scratch.data_ptr() + GUARD, boxes_out=self.bo[1:], count_out=self.co[1:], scores_out=self.so[1:],
                           index_out=self.io[1:], **ptrs)

    def result(self):
        m = self.c.p.max_out
        return (self.bo[1:m + 1].cpu().numpy(), int(self.co[1]), self.so[1:m + 1].cpu().numpy(), self.io[1:m + 1].cpu().numpy())

    def canaries_intact(self, poison_scratch=0xA5):
        s = self.scratch
        return bool((s[:GUARD] == poison_scratch).all() and (s[GUARD + self.sb:] == poison_scratch).all() and (self.bo[0] == -77).all() and (self.bo[-1] == -77).all()
                    and self.so[0] == -77 and self.so[-1] == -77 and self.io[0] == 12345 and self.io[-1] == 12345 and self.co[0] == 999 and self.co[2] == 999)


def _run(device, cases, want=None):
    """ONE cvgs_boxes_select call over `cases`; every frame against the host entry, every canary intact."""
    torch = _torch()
    jobs = [Job(device, c) for c in cases]
    cvgs.boxes_select(torch.cuda.current_stream(), [j.desc for j in jobs])
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        got, ref = j.result(), (want[k] if want else j.c.host())
        assert SC.same(got, ref), "frame %d of %d: kept %d, host %d\n device %s\n host   %s" % (k, len(jobs), got[1], ref[1], got[3][:40], ref[3][:40])
        assert j.canaries_intact(), "frame %d: a canary around scratch or an output changed" % k
    return jobs


def _counted_case(m, seed, n=65535):
    """Exactly m members among live = m + 40 candidates of a 65535-candidate buffer; the candidates beyond the count would all be members."""
    live = m + 40
    c = SC.make(seed, live, W=1920, H=1080, score_thr=0.3, pre_k=1024, max_out=64, dirty=False, with_classes=seed % 2 == 0, count=live)
    rng = np.random.default_rng(seed)
    scores = (0.3 + np.round(rng.uniform(0, 0.7, live) * 64) / 64 * 0.999).astype(np.float32)
    is_member = np.array([M.prepare32(c.p, c.boxes[i], scores[i]) is not None for i in range(live)])
    surplus = rng.permutation(np.flatnonzero(is_member))[m:]
    scores[surplus] = 0.1
    assert int(is_member.sum()) - len(surplus) == m
    boxes = np.tile(np.array([100, 100, 400, 300], np.float32), (n, 1))
    boxes[:live] = c.boxes
    full_scores = np.full((n,), 0.95, np.float32)
    full_scores[:live] = scores
    classes = None
    if c.classes is not None:
        classes = np.zeros((n,), np.int32)
        classes[:live] = c.classes
    return SC.Case(c.p, boxes, full_scores, classes, live)


COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


def test_member_counts_around_every_boundary(device, lib):
    """11 frames in one call, max_candidates = 65535 each, a device count of members + 40: 1 .. 4097 members (the wave, the tile, pre_nms_k)."""
    cases = [_counted_case(m, 900 + k) for k, m in enumerate(COUNTS)]
    jobs = _run(device, cases)
    for j, m in zip(jobs, COUNTS):
        members = int(np.frombuffer(j.scratch[GUARD:GUARD + 4].cpu().numpy().tobytes(), np.int32)[0])
        assert members == m  # (the header of scratch: what the rank launch counted)
        assert 1 <= j.result()[1] <= min(m, 64)


def test_sixteen_frames_of_different_shapes_in_one_call(device, lib):
    """Both formats, dense and interleaved heads, classes on and off, three transforms, frames, counts, pre_nms_k and max_out."""
    cases = SC.seeded_cases()[:16]
    assert len({(c.p.fmt, c.head is not None, c.classes is not None) for c in cases}) >= 6 and len({c.n for c in cases}) >= 5
    _run(device, cases)
    _run(device, SC.seeded_cases()[16:])
    _run(device, [SC.make(77, 1)])  # one candidate, one frame


def test_interleaved_head_is_read_in_place(device, lib):
    """A [n, 6] tensor (box, score, class): box_stride = score_stride = class_stride = 6, three pointers into ONE allocation."""
    c = SC.make(41, 3000, interleaved=True, with_classes=True, pre_k=512, max_out=512, W=1280, H=720)
    j = _run(device, [c])[0]
    assert c.strides() == (6, 6, 6) and j.desc.scores - j.desc.boxes == 16 and j.desc.classes - j.desc.boxes == 20
    assert j.result()[1] > 20
    agnostic = SC.make(41, 3000, interleaved=True, with_classes=False, pre_k=512, max_out=512, W=1280, H=720)
    assert _run(device, [agnostic])[0].result()[1] < j.result()[1]  # classes let more boxes live


def test_equal_scores_across_wave_and_tile_boundaries(device, lib):
    """1,200 members on two score levels laid out so that every wave and every 256-candidate tile holds both: the order inside a level is
    the index order, the working list is cut at 1024 inside a level, and disjoint boxes keep everything."""
    n = 1200
    grid = np.array([[(i % 40) * 12, (i // 40) * 12, (i % 40) * 12 + 10, (i // 40) * 12 + 10] for i in range(n)], np.float32)
    scores = np.where(np.arange(n) % 3 == 0, 0.875, 0.75).astype(np.float32)
    c = SC.Case(M.params(480, 360, 0.5, 0.5, 1024, 1024), grid, scores, None, None)
    ref = c.host()
    hi, lo = [i for i in range(n) if i % 3 == 0], [i for i in range(n) if i % 3]
    assert ref[1] == 1024 and ref[3].tolist() == hi + lo[:1024 - len(hi)]
    _run(device, [c], [ref])
    # all equal, heavy overlap: the lowest index of every pile survives
    piles = np.array([[(i % 7) * 50, 0, (i % 7) * 50 + 40, 40] for i in range(700)], np.float32)
    c = SC.Case(M.params(480, 360, 0.5, 0.5, 1024, 50), piles, np.full((700,), 0.75, np.float32), None, None)
    ref = c.host()
    assert ref[1] == 7 and ref[3][:7].tolist() == list(range(7))
    _run(device, [c], [ref])


def test_scratch_contents_do_not_matter(device, lib):
    """The same call over scratch poisoned with 0x00 and with 0xFF (NaN bits, negative counts) writes the same outputs."""
    torch = _torch()
    c = SC.make(43, 500, pre_k=64, max_out=20)
    ref = c.host()
    for poison in (0x00, 0xFF):
        j = Job(device, c, poison)
        cvgs.boxes_select(torch.cuda.current_stream(), [j.desc])
        cvgs.boxes_select(torch.cuda.current_stream(), [j.desc])  # and over its own leftovers
        torch.cuda.synchronize()
        assert SC.same(j.result(), ref) and j.canaries_intact(poison)


def test_detector_to_tick_in_one_graph(device, lib):
    """A copy writes the candidates (the detector), then cvgs_boxes_select, cvgs_plane_tables_from_boxes and a bilinear K1 tick over the
    device table, captured ONCE on one stream; replayed twice over different candidates, each replay's tensor is bit-identical to the same
    tick run from boxes the HOST entry selected."""
    torch = _torch()
    from tests.test_gpu_boxes import Frame, _chain, _out_tensor
    W, Hh, dsize, n, max_out = 320, 200, (64, 128), 900, 24
    frame = Frame(device, W, Hh, cvgs.CV_8UC3, W * 3 + 8, seed=21)
    xform = cvgs.letterbox_xform((W, Hh), (160, 160), cvgs.PRESERVE_AR)
    rounds = [SC.make(600 + r, n, fmt=M.CXCYWH, interleaved=True, with_classes=True, xform=xform, W=W, H=Hh, pre_k=256, max_out=max_out, count=(n, 500)[r])
              for r in range(2)]
    staged = [(torch.from_numpy(c.head).to(device), torch.tensor([c.count], dtype=torch.int32, device=device)) for c in rounds]
    job = Job(device, rounds[0])  # the buffers the graph works on; the candidates and the count are overwritten by the graph's first nodes
    table = torch.zeros((max_out, 48), dtype=torch.uint8, device=device)
    out = _out_tensor(device, max_out, 3, dsize)
    tdesc = cvgs.box_table_desc(frame.mat, job.bo[1:], table, max_out, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYXY_F32, job.co[1:], None)
    ops = _chain(cvgs.resize_boxes(frame.mat, table, max_out, dsize), 3, out, dsize)
    assert cvgs.kernel_name(*ops).startswith("k1_u8c3")
    low = [cvgs.lower(ops)]
    arr = cvgs.pack_chains(low)
    src_head, src_count = torch.zeros_like(staged[0][0]), torch.zeros_like(staged[0][1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        job.head.copy_(src_head)
        job.count.copy_(src_count)
        cvgs.boxes_select(s, [job.desc])
        cvgs.plane_tables_from_boxes(s, [tdesc])
        capi.check(lib.cvgs_execute_many(arr, 1, cvgs.stream_handle(s)))
    torch.cuda.synchronize()
    assert (out == -5.0).all(), "capture itself must not run anything"
    results = []
    for r, c in enumerate(rounds):
        src_head.copy_(staged[r][0])
        src_count.copy_(staged[r][1])
        g.replay()
        torch.cuda.synchronize()
        ref = c.host()
        assert SC.same(job.result(), ref) and job.canaries_intact() and 3 <= ref[1] <= max_out
        # the same tick from host-selected boxes
        hb = torch.from_numpy(ref[0]).to(device)
        hc = torch.tensor([ref[1]], dtype=torch.int32, device=device)
        htable = torch.zeros_like(table)
        hout = _out_tensor(device, max_out, 3, dsize)
        s = torch.cuda.current_stream()
        cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(frame.mat, hb, htable, max_out, dsize, cvgs.IGNORE_AR, cvgs.BOX_XYXY_F32, hc, None)])
        cvgs.executeOperations(s, *_chain(cvgs.resize_boxes(frame.mat, htable, max_out, dsize), 3, hout, dsize))
        torch.cuda.synchronize()
        assert torch.equal(out, hout), "replay %d" % r
        results.append(out.clone())
    assert not torch.equal(results[0], results[1])
