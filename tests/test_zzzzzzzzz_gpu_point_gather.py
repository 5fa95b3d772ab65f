"""cvgs_points_gather on the GPU (include/cvgs_hip_ext.h: THE CONTRACT; csrc/k_gather.hip): what the kernel writes equals
cvgs_points_gather_host byte for byte -- which tests/test_point_gather.py holds to an independent numpy model on the CPU -- with canaries
on both sides of every output and every element compared, rows at and beyond the live count included: the seeded grid; item counts around
the wave and the workgroup; 16-bit heads that start 2 bytes into their allocation; the optional outputs present and absent; 16 different
frames in one call; hostile indices inside the live range; every 16-bit pattern; and decode -> select -> gather -> warp tables -> warp
chains captured once in a HIP graph and replayed, in Python and through the C++ facade."""
import copy
import os
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from oracle import oracle_binding
from tests import helpers as H
from tests import point_gather_cases as GC
from tests import point_gather_model as M
from tests.test_point_gather import ARCFACE5, _face_head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _torch():
    import torch
    return torch


def _without_conf(c):
    d = copy.copy(c)
    d.conf_offset = -1
    return d


class Job:
    """One frame's device buffers: the head's storage as the case lays it out (a 16-bit head 2 bytes into its allocation on request), the
    index lists, and the three outputs with one guard row on either side."""

    def __init__(self, device, c, with_source=True, head_offset=0):
        torch = _torch()
        self.c, m, k = c, c.max_out, c.n_points
        assert head_offset == 0 or (head_offset == 2 and c.elem != M.F32)
        store = np.zeros(c.raw.nbytes + 8, np.uint8)
        store[head_offset:head_offset + c.raw.nbytes] = c.raw.reshape(-1).view(np.uint8)
        self.head = torch.from_numpy(store).to(device)
        self.kept = torch.from_numpy(c.kept_index).to(device)
        self.cand = None if c.cand_index is None else torch.from_numpy(c.cand_index).to(device)
        self.count = None if c.kept_count is None else torch.tensor([c.kept_count], dtype=torch.int32, device=device)
        self.po = torch.full((m + 2, k, 2), -77.0, dtype=torch.float32, device=device)
        self.co = torch.full((m + 2, k), -77.0, dtype=torch.float32, device=device) if c.conf_offset != -1 else None
        self.so = torch.full((m + 2,), 12345, dtype=torch.int32, device=device) if with_source else None
        self.desc = c.desc(head=self.head.data_ptr() + head_offset, kept_index=self.kept, kept_count=self.count, cand_index=self.cand, points_out=self.po[1:],
                           conf_out=None if self.co is None else self.co[1:], source_out=None if self.so is None else self.so[1:])

    def result(self):
        m = self.c.max_out
        return (self.po[1:m + 1].cpu().numpy(), None if self.co is None else self.co[1:m + 1].cpu().numpy(), None if self.so is None else self.so[1:m + 1].cpu().numpy())

    def canaries_intact(self):
        ok = bool((self.po[0] == -77).all() and (self.po[-1] == -77).all())
        if self.co is not None:
            ok = ok and bool((self.co[0] == -77).all() and (self.co[-1] == -77).all())
        if self.so is not None:
            ok = ok and bool(self.so[0] == 12345 and self.so[-1] == 12345)
        return ok


def _check(jobs, what=""):
    for k, j in enumerate(jobs):
        got, ref = j.result(), j.c.host()
        c = j.c
        if got[2] is None:
            got = (got[0], got[1], ref[2])
        assert GC.same(got, ref), "%sframe %d of %d (%s, elem %d, %d x %d items, count %s, cand %s)\n device %s\n host   %s" % (
            what, k, len(jobs), c.layout, c.elem, c.max_out, c.n_points, c.kept_count, c.cand_index is not None, got[2][:24], ref[2][:24])
        assert j.canaries_intact(), "%sframe %d: a canary around an output changed" % (what, k)


def _run(device, cases, **kw):
    """ONE cvgs_points_gather call over `cases`; every frame against the host entry, every canary intact."""
    torch = _torch()
    assert len(cases) <= 16
    jobs = [Job(device, c, **kw) for c in cases]
    cvgs.points_gather(torch.cuda.current_stream(), [j.desc for j in jobs])
    torch.cuda.synchronize()
    _check(jobs)
    return jobs


# (max_out, n_points): max_out * n_points in {1, 63, 64, 65, 255, 256, 257, 513} -- around the wave, the workgroup and its second tile
SHAPES = ((1, 1), (63, 1), (21, 3), (1, 64), (4, 16), (13, 5), (15, 17), (51, 5), (16, 16), (4, 64), (257, 1), (513, 1), (27, 19))


def _shape_cases(seed0=4000):
    out = []
    for k, (m, p) in enumerate(SHAPES):
        step, conf = GC.STEPS[k % 4]
        out.append(GC.make(seed0 + k, (97, 300, 64)[k % 3], p, (M.F32, M.F16, M.BF16)[k % 3], GC.LAYOUTS[k % 4], step, conf, m,
                           ("kept", None, m + 7)[k % 3], k % 2 == 0, lead=(0, 2)[k % 2]))
    return out


def test_the_seeded_grid(device, lib):
    """The 96 cases of the CPU grid, 16 frames per call."""
    assert hasattr(lib, "cvgs_points_gather")
    cases = GC.seeded_cases()
    assert len(cases) == 96 and all(c.n <= 300 for c in cases)
    for at in range(0, 96, 16):
        _run(device, cases[at:at + 16])


def test_item_counts_around_the_wave_and_the_workgroup(device, lib):
    cases = _shape_cases()
    assert {c.items for c in cases} == {1, 63, 64, 65, 255, 256, 257, 513} and all(c.n <= 300 for c in cases)
    _run(device, cases)
    for c in cases:  # and each alone: the grid is then exactly the frame's own
        _run(device, [c])


def test_sixteen_bit_heads_two_bytes_into_their_allocation(device, lib):
    cases = [c for c in _shape_cases(4100) + GC.seeded_cases()[32:48] if c.elem != M.F32][:16]
    assert len(cases) == 16 and {c.elem for c in cases} == {M.F16, M.BF16}
    jobs = _run(device, cases, head_offset=2)
    assert all(j.desc.head % 4 == 2 for j in jobs)


def test_optional_outputs_present_and_absent(device, lib):
    """source_out absent; conf_out absent (the same head described without a confidence); both absent."""
    with_conf = [c for c in _shape_cases(4200) if c.conf_offset != -1]
    assert len(with_conf) >= 6
    for c in with_conf:
        for case in (c, _without_conf(c)):
            for src in (True, False):
                (j,) = _run(device, [case], with_source=src)
                assert (j.co is None) == (case.conf_offset == -1) and (j.so is None) == (not src)


def test_sixteen_frames_of_different_shapes_types_and_layouts_in_one_call(device, lib):
    """One item beside 513 work-items (the workgroup-uniform early exit); each frame equals its own single-frame call and the host entry."""
    torch = _torch()
    picks = [c for c in _shape_cases(4300)]
    cases = [picks[0], picks[11]] + picks[1:11] + picks[12:] + GC.seeded_cases()[5:8]
    assert len(cases) == 16 and cases[0].items == 1 and cases[1].items == 513
    assert len({c.elem for c in cases}) == 3 and len({c.layout for c in cases}) == 4 and len({c.n_points for c in cases}) >= 6 and len({c.max_out for c in cases}) >= 8
    jobs = _run(device, cases)
    for c, j in zip(cases, jobs):
        (single,) = _run(device, [c])
        a, b = j.result(), single.result()
        assert GC.same(a, b)
    assert torch.cuda.is_available()


def test_hostile_indices_inside_the_live_range(device, lib):
    """Every live row of kept_index -- then every cand_index slot live rows point at -- holds -1, max_candidates, INT32_MAX or INT32_MIN:
    all rows invalid, canaries intact, equal to the host entry.  Such indices are never dereferenced by contract."""
    cases = []
    for k, with_cand in enumerate((False, True, True)):
        c = GC.make(4400 + k, 200, 5, (M.F32, M.BF16, M.F16)[k], ("NA", "AN", "AN_pad")[k], 3, 2, 64, None, with_cand, hostile=False)
        bad = np.array([-1, c.n, GC.INT32_MAX, GC.INT32_MIN], np.int64)
        if k < 2:
            c.kept_index[:] = bad[np.arange(64) % 4].astype(np.int32)
        else:
            live = c.kept_index[c.kept_index >= 0]
            c.cand_index[live] = bad[np.arange(len(live)) % 4].astype(np.int32)
        cases.append(c)
    jobs = _run(device, cases)
    for j in jobs:
        po, co, so = j.result()
        assert (so == -1).all() and (po.view(np.uint32) == 0x7FC00000).all() and not co.view(np.uint32).any()


def test_every_fp16_and_bf16_pattern_as_a_landmark(device, lib):
    """65,535 candidates, one landmark each, every row kept: all 65536 patterns of both 16-bit types in two frames per type."""
    bits = np.arange(65536, dtype=np.uint16)
    cases = []
    for elem in (M.F16, M.BF16):
        for chunk, xform in ((bits[:65535], GC.XFORMS[0]), (bits[1:], GC.XFORMS[2])):
            c = GC.Case(np.zeros((65535, 7), np.float32), elem, "NA", 0, 1, 2, -1, 65535, np.arange(65535), None, None, xform)
            c.raw[:, 5] = chunk.view(c.raw.dtype)
            c.raw[:, 6] = chunk[::-1].view(c.raw.dtype)
            cases.append(c)
    jobs = _run(device, cases)
    assert all((j.result()[2] == np.arange(65535)).all() for j in jobs)


# ---- one captured graph: decode -> select -> gather -> warp tables -> warp chains ------------------------------------------------------------
W, HH, DSIZE, N_CAND, MAX_OUT, DET = 96, 64, (32, 32), 300, 8, 160.0


def _chain(rd, out, planes):
    f = cvgs.make_type(cvgs.CV_32F, 3)
    return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [H.K1_ALPHA] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
            cvgs.split_tensor(f, out, DSIZE[0], DSIZE[1], planes)]


def _cpu_composition(raw, elem, cs, as_, xform_box, xform_pts, tmpl, frame_host_mat):
    """(kept, points, float32 tensor [MAX_OUT, 3, 32, 32]) through the four host entries and the oracle."""
    hd = cvgs.head_desc(None, elem, N_CAND, cs, as_, 1, 0.25, None, None, None, None, None)
    bo, so, ko, io, cnt = cvgs.head_decode_host(hd, raw)
    sd = cvgs.box_select_desc((W, HH), None, None, N_CAND, None, None, None, 0.25, 0.5, 256, MAX_OUT, cvgs.CAND_CXCYWH_F32, 4, 1, None, 1, None, xform_box)
    sb, kept, ss, si = cvgs.boxes_select_host(sd, bo, so, ko, cnt)
    gd = cvgs.point_gather_desc(None, elem, N_CAND, cs, as_, 5, 2, 5, MAX_OUT, None, None, xform=xform_pts)
    po, _, src = cvgs.points_gather_host(gd, raw, si, kept, io)
    wd = cvgs.warp_table_desc(frame_host_mat, None, None, MAX_OUT, DSIZE, tmpl)
    table, valid = cvgs.build_warp_table_host(wd, po, kept)
    m = np.frombuffer(table, np.uint8).reshape(MAX_OUT, 64)[:, 20:56].copy().view(np.float32)
    rd = cvgs.ReadIOp(capi.READ_WARP_AFFINE, cvgs.CV_8UC3, [frame_host_mat] * MAX_OUT, None, DSIZE, cvgs.IGNORE_AR, None)
    rd.warp, rd.warp_sizes = [float(v) for v in m.reshape(-1)], None
    ref = np.full((MAX_OUT, 3, DSIZE[1], DSIZE[0]), -9.0, np.float32)
    oracle_binding.execute(cvgs.lower(_chain(rd, ref.ctypes.data, MAX_OUT)))
    return kept, po, ref


def test_head_to_aligned_crops_in_one_graph(device, lib):
    """Copies write the heads (the network), then cvgs_head_decode, cvgs_boxes_select, cvgs_points_gather, cvgs_warp_tables_from_points and
    one warp chain per head over the device tables, captured ONCE on one stream.  The one call of each kind holds BOTH descriptors -- a
    bf16 [A, N] head and an fp32 [N, A] head -- and the graph is replayed twice over different heads: each replay's tensors are
    bit-identical to the CPU composition (the four host entries, then the oracle over the host-built matrices)."""
    torch = _torch()
    step = W * 3 + 8
    host = H.random_u8((HH, step), seed=77)
    ft = torch.from_numpy(host).to(device)
    mat = cvgs.GpuMat(HH, W, cvgs.CV_8UC3, ft.data_ptr(), step, owner=ft)
    host_mat = cvgs.GpuMat(HH, W, cvgs.CV_8UC3, host.ctypes.data, step, owner=host)
    tmpl = [(x * 32 / 112.0, y * 32 / 112.0) for x, y in ARCFACE5]
    sx, sy = np.float32(W / DET), np.float32(HH / DET)
    xform_box = (float(sx), float(sy), 0.0, 0.0)
    xform_pts = (float(sx), float(sy), float(np.float32(0.5) * sx - np.float32(0.5)), float(np.float32(0.5) * sy - np.float32(0.5)))  # (pixel-centre landmarks)
    kinds = ((M.BF16, "AN"), (M.F32, "NA"))
    rounds = [[GC.lay_out(_face_head(600 + 10 * r + k, N_CAND), elem, layout) for k, (elem, layout) in enumerate(kinds)] for r in range(2)]
    staged = [[torch.from_numpy(raw.reshape(-1).view(np.uint8).copy()).to(device) for raw, _, _ in rnd] for rnd in rounds]
    sources = [torch.zeros_like(t) for t in staged[0]]
    heads = [torch.zeros_like(t) for t in staged[0]]

    def z(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=device)
    hds, sds, gds, wds, lows, outs, pts, cnts = [], [], [], [], [], [], [], []
    keep = []
    for k, (elem, layout) in enumerate(kinds):
        _, cs, as_ = rounds[0][k]
        dec = dict(scratch=z((cvgs.head_decode_scratch_bytes(N_CAND),), torch.uint8), bo=z((N_CAND, 4), torch.float32), so=z((N_CAND,), torch.float32),
                   ko=z((N_CAND,), torch.int32), io=z((N_CAND,), torch.int32), co=z((1,), torch.int32))
        sel = dict(scratch=z((cvgs.boxes_select_scratch_bytes(N_CAND, 256),), torch.uint8), bo=z((MAX_OUT, 4), torch.float32), co=z((1,), torch.int32),
                   so=z((MAX_OUT,), torch.float32), io=z((MAX_OUT,), torch.int32))
        po, table = z((MAX_OUT, 5, 2), torch.float32), z((MAX_OUT, 64), torch.uint8)
        out = torch.full((MAX_OUT, 3, DSIZE[1], DSIZE[0]), -5.0, dtype=torch.float32, device=device)
        hds.append(cvgs.head_desc(heads[k], elem, N_CAND, cs, as_, 1, 0.25, dec["scratch"], dec["bo"], dec["so"], dec["ko"], dec["co"], dec["io"]))
        sds.append(cvgs.box_select_desc((W, HH), dec["bo"], dec["so"], N_CAND, sel["scratch"], sel["bo"], sel["co"], 0.25, 0.5, 256, MAX_OUT, cvgs.CAND_CXCYWH_F32, 4, 1,
                                        dec["ko"], 1, dec["co"], xform_box, sel["so"], sel["io"]))
        gds.append(cvgs.point_gather_desc(heads[k], elem, N_CAND, cs, as_, 5, 2, 5, MAX_OUT, sel["io"], po, sel["co"], dec["io"], xform_pts))
        wds.append(cvgs.warp_table_desc(mat, po, table, MAX_OUT, DSIZE, tmpl, count=sel["co"]))
        lows.append(_chain(cvgs.warp_table(cvgs.WARP_AFFINE, mat, table, MAX_OUT, DSIZE), out.data_ptr(), MAX_OUT))
        outs.append(out)
        pts.append(po)
        cnts.append(sel["co"])
        keep += [dec, sel, table]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        for hd_t, src in zip(heads, sources):
            hd_t.copy_(src)
        cvgs.head_decode(s, hds)
        cvgs.boxes_select(s, sds)
        cvgs.points_gather(s, gds)
        cvgs.warp_tables_from_points(s, wds)
        for ops in lows:
            cvgs.executeOperations(s, *ops)
    torch.cuda.synchronize()
    assert all((out == -5.0).all() for out in outs), "capture itself must not run anything"
    results = []
    for r, rnd in enumerate(rounds):
        for src, st in zip(sources, staged[r]):
            src.copy_(st)
        g.replay()
        torch.cuda.synchronize()
        for k, (raw, cs, as_) in enumerate(rnd):
            kept, po, ref = _cpu_composition(raw, kinds[k][0], cs, as_, xform_box, xform_pts, tmpl, host_mat)
            assert 3 <= kept <= MAX_OUT and int(cnts[k][0]) == kept
            assert (pts[k].cpu().numpy().view(np.uint32) == po.view(np.uint32)).all(), "replay %d, head %d: points" % (r, k)
            got = outs[k].cpu().numpy()
            assert (got.view(np.uint32) == ref.view(np.uint32)).all(), "replay %d, head %d: %d values differ from the CPU composition" % (
                r, k, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
            assert len({got[i].tobytes() for i in range(kept)}) == kept  # the kept planes hold different crops
            results.append(got)
    assert not (results[0] == results[2]).all() and not (results[1] == results[3]).all()


def test_facade_program_passes():
    """tests/cpp/test_point_gather.cpp: the same chain through cvGS::DeviceHeadDecode, DeviceBoxSelect, DevicePointGather and DeviceWarps."""
    exe = os.path.join(CPP, "bin", "test_point_gather")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", CPP, "bin/test_point_gather"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_point_gather passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
