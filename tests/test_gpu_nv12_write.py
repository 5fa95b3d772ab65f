"""The CVGS_WRITE_NV12 kernels (csrc/k_nv12_write.hip) on the GPU, BIT-EXACT against the fp32 restatement of the contract
(tests/nv12_write_model.py): the float R, G, B picture in front of the write stage is the CPU oracle's (the same read and program, written as
packed CV_32FC3), the restatement turns it into the surface, and every stored byte is compared -- with a guard band of a sentinel on both
sides of every surface, the sentinel in the row padding (step = width + 24) and between the planes where uv_offset leaves a gap.

Smallest shapes that can still go wrong: a 96 x 64 NV12 source plus one 8UC3, one 16UC3 and one 32FC3 frame; targets 2 x 2 (a single block),
34 x 14 (a width tail of 2 behind the fast kernel's 4-wide lane), 260 x 4 (crosses its 256-column wave tile); up- and down-scaling; crops at
even origins; 1, 5 and 70 planes (inline 8, inline 64, a staged table); a device table; a default-value plane.

This module holds the cases (all_cases) and their runner; it defines NO test item of its own: the ONE item, with a subtest per case, is
tests/test_zz_gpu_nv12_write.py -- collected behind every existing item (tests/test_gpu_area.py says why)."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import nv12_write_model as M

GUARD = 256
SENTINEL = 0xA5
PAD = 24
SW, SH = 96, 64  # the NV12 source surface
F3 = cvgs.CV_32FC3
CROPS = [(0, 0, 96, 64), (2, 4, 40, 30), (50, 20, 46, 44), (10, 2, 20, 12), (94, 62, 2, 2), (0, 32, 96, 32), (30, 0, 18, 64)]  # even x, y, w, h


def _torch():
    import torch
    return torch


class Surface:
    """One target surface in a device buffer of its own: guard | luma rows | gap | chroma rows | guard, all SENTINEL before the launch."""

    def __init__(self, device, w, h, gap=0, step=None, lead=0):
        """step: the row pitch (default width + PAD; any value >= width, odd ones included); lead: further bytes in front of the surface,
        which shift its base address (the allocation itself is aligned)."""
        torch = _torch()
        self.w, self.h, self.step = w, h, w + PAD if step is None else step
        self.uv_off = h * self.step + gap
        self.total = self.uv_off + (h // 2) * self.step
        self.lead = GUARD + lead
        self.t = torch.full((self.lead + self.total + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.mat = cvgs.GpuMat(h, w, cvgs.CV_8UC1, self.t.data_ptr() + self.lead, self.step, owner=self.t)
        if gap:
            self.mat.uv_offset = self.uv_off

    def check(self, luma, chroma, what):
        got = self.t.cpu().numpy()
        assert (got[:self.lead] == SENTINEL).all() and (got[self.lead + self.total:] == SENTINEL).all(), "%s: the guard band changed" % what
        want = M.surface_image(luma, chroma, self.step, self.uv_off, self.total, SENTINEL)
        pay = got[self.lead:self.lead + self.total]
        bad = np.flatnonzero(pay != want)
        assert bad.size == 0, "%s: %d bytes differ, first at byte %d (row %d, column %d: got %d, want %d)" % (
            what, bad.size, bad[0], bad[0] // self.step, bad[0] % self.step, pay[bad[0]], want[bad[0]])


_frames = {}


def frame(device, name):
    """(host array, host GpuMat, device GpuMat) of a source; made once per device.  device None: the host half alone (device GpuMat None)."""
    key = (name, str(device))
    if key not in _frames:
        rng = np.random.RandomState(21)
        if name == "NV12":
            host, cv_type, rows = M.random_surface(SW, SH, 3), cvgs.CV_8UC1, SH
        elif name == "8UC3":
            host, cv_type, rows = rng.randint(0, 256, (61, 97 * 3)).astype(np.uint8), cvgs.CV_8UC3, 61
        elif name == "16UC3":
            host, cv_type, rows = rng.randint(0, 65536, (61, 97 * 3)).astype(np.uint16), cvgs.make_type(capi.DEPTH_16U, 3), 61
        else:  # 32FC3: a picture of the target's own size with values on both sides of 0..255
            host, cv_type, rows = (rng.rand(14, 34 * 3) * 300.0 - 20.0).astype(np.float32), F3, 14
        cols = SW if name == "NV12" else host.shape[1] // 3
        dm = None
        if device is not None:
            t = _torch().from_numpy(host.view(np.uint8).reshape(host.shape[0], -1)).to(device)
            dm = cvgs.GpuMat(rows, cols, cv_type, t.data_ptr(), host.strides[0], owner=t)
        _frames[key] = (host, cvgs.GpuMat(rows, cols, cv_type, host.ctypes.data, host.strides[0], owner=host), dm)
    return _frames[key]


def oracle_rgb(oracle, read, mid, dsize, batch):
    """[batch, h, w, 3] float32: what reaches the write stage, from the CPU oracle (the chain written as packed CV_32FC3)."""
    w, h = dsize
    ref = np.zeros((batch, h * w * 3), np.float32)
    oracle.execute(cvgs.lower([read] + list(mid) + [cvgs.write(F3, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (w, h))]))
    return ref.reshape(batch, h, w, 3)


def run(device, oracle, what, make_read, mid, dsize, batch, out=(M.FULL, M.BT709, M.NV12), gap=0, kernel=None, both=True, rgb=None, make_outs=None):
    """The chain as dispatched and (both) with CHAIN_FORCE_GENERIC: each against the restatement.  make_read(mats_are_on_device) -> ReadIOp.
    make_outs() -> (target GpuMats, one per plane; check(want, label)): targets other than one Surface per plane, made anew for every run."""
    torch = _torch()
    rng, prim, layout = out
    if rgb is None:
        rgb = oracle_rgb(oracle, make_read(False), mid, dsize, batch)
    want = [M.write_f32(rgb[z], rng, prim, layout) for z in range(batch)]
    for flags in ((0, capi.CHAIN_FORCE_GENERIC) if both else (0,)):
        if make_outs is None:
            outs = [Surface(device, dsize[0], dsize[1], gap) for _ in range(batch)]
            mats, check_all = [o.mat for o in outs], None
        else:
            mats, check_all = make_outs()
        ops = [make_read(True)] + list(mid) + [cvgs.write_nv12(mats, rng, prim, layout)]
        name = cvgs.kernel_name(*ops, flags=flags)
        assert name == ("nv12w_interp" if flags else (kernel or name)) and name.startswith("nv12w_"), name
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
        torch.cuda.synchronize()
        if check_all is not None:
            check_all(want, "%s, flags %d (%s)" % (what, flags, name))
            continue
        for z, o in enumerate(outs):
            o.check(want[z][0], want[z][1], "%s, plane %d, flags %d (%s)" % (what, z, flags, name))
    return want


def nv12_read(views, dsize, rng=M.LIMITED, prim=M.BT601, layout=capi.YUV_NV12, used=None, bg=None):
    rd = cvgs.read_nv12(views, dsize, rng, prim, alpha=False, layout=layout)
    if used is not None:
        rd.used_planes = used
    if bg is not None:
        rd.background = cvgs._scalar(bg)
    return rd


def case_transcode(device, lib, oracle, dsize, crops, layout_in, out, gap=0):
    """NV12 / NV21 crops -> resize -> surface with an empty program: the fast kernel, and the same chain forced generic."""
    _, hm, dm = frame(device, "NV12")
    mk = lambda dev: nv12_read([(dm if dev else hm).nv12_roi(*c) for c in crops], dsize, layout=layout_in)
    run(device, oracle, "transcode %s -> %dx%d" % (crops[:2], dsize[0], dsize[1]), mk, [], dsize, len(crops), out, gap, kernel="nv12w_nv12_resize")


def case_default_value_plane(device, lib, oracle):
    """used_planes < batch: the last plane is the background value run through the chain, written like any other -- both kernels."""
    _, hm, dm = frame(device, "NV12")
    bg = [200.0, 30.0, 90.0, 0.0]
    mk = lambda dev: nv12_read([(dm if dev else hm).nv12_roi(*c) for c in CROPS[:3]], (34, 14), used=2, bg=bg)
    want = run(device, oracle, "default-value plane", mk, [], (34, 14), 3, (M.LIMITED, M.BT709, M.NV12), kernel="nv12w_nv12_resize")
    l, c = M.write_f32(np.broadcast_to(np.array(bg[:3], np.float32), (14, 34, 3)), M.LIMITED, M.BT709)
    assert (want[2][0] == l).all() and (want[2][1] == c).all()
    mid = [cvgs.multiply(F3, [0.5, 1.0, 2.0])]
    run(device, oracle, "default-value plane behind a program", mk, mid, (34, 14), 3, (M.FULL, M.BT601, M.NV21), kernel="nv12w_interp", both=False)


def case_pixel_frames(device, lib, oracle):
    """The other reads, through the interpreted kernel: 8UC3 and 16UC3 crops resized, a 32FC3 picture and an 8UC3 one read per pixel, a
    full-resolution NV12 read, an I420 resize; the swap + mul + add program."""
    _, hm, dm = frame(device, "8UC3")
    crops = [(0, 0, 97, 61), (11, 13, 38, 19), (56, 38, 41, 23), (3, 5, 10, 6), (60, 1, 17, 50)]
    prog = [cvgs.cvtColor(cvgs.COLOR_BGR2RGB, F3), cvgs.multiply(F3, [1.1, 0.9, 1.0]), cvgs.add(F3, [-12.5, 3.0, 20.0])]
    mk = lambda dev: cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [(dm if dev else hm).roi(*c) for c in crops], (34, 14))
    run(device, oracle, "8UC3 crops, swap + mul + add", mk, prog, (34, 14), 5, (M.LIMITED, M.BT2020, M.NV21), kernel="nv12w_interp", both=False)
    mk = lambda dev: cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [(dm if dev else hm).roi(*crops[3])], (260, 4))
    run(device, oracle, "8UC3 up-scaled to 260 x 4", mk, [], (260, 4), 1, kernel="nv12w_interp", both=False)
    mk = lambda dev: cvgs.ReadIOp(capi.READ_PIXEL, cvgs.CV_8UC3, [(dm if dev else hm).roi(5, 7, 34, 14)], 1)
    run(device, oracle, "8UC3 per-pixel read", mk, [cvgs.convertTo(cvgs.CV_8UC3, F3)], (34, 14), 1, (M.FULL, M.BT601, M.NV12), kernel="nv12w_interp", both=False)
    _, hm16, dm16 = frame(device, "16UC3")
    t16 = cvgs.make_type(capi.DEPTH_16U, 3)
    mk = lambda dev: cvgs.resize(t16, cvgs.INTER_LINEAR, [(dm16 if dev else hm16).roi(*c) for c in crops[:2]], (34, 14))
    run(device, oracle, "16UC3 crops", mk, [cvgs.multiply(F3, [1.0 / 250.0] * 3)], (34, 14), 2, (M.LIMITED, M.BT601, M.NV12), kernel="nv12w_interp", both=False)
    _, hmf, dmf = frame(device, "32FC3")
    mk = lambda dev: cvgs.ReadIOp(capi.READ_PIXEL, F3, [dmf if dev else hmf], 1)
    run(device, oracle, "32FC3 per-pixel read (saturates on both sides)", mk, [], (34, 14), 1, (M.FULL, M.BT709, M.NV21), gap=40, kernel="nv12w_interp", both=False)
    _, hmy, dmy = frame(device, "NV12")
    mk = lambda dev: cvgs.read_nv12(dmy if dev else hmy, (34, 14), M.FULL, M.BT709, alpha=True, layout=capi.YUV_I420)
    run(device, oracle, "I420 surface, alpha dropped", mk, [cvgs.cvtColor(cvgs.COLOR_RGBA2RGB, cvgs.CV_32FC4, F3)], (34, 14), 1, kernel="nv12w_interp", both=False)


def case_identity_transcoding(device, lib, oracle, rng, prim):
    """A surface read at its own size and written with the same range and primaries comes back byte for byte: through the full-resolution
    NV12 read (interpreted kernel) and through the resize at factor 1 (fast kernel), NV12 and NV21."""
    host, hm, dm = frame(device, "NV12")
    for layout in (capi.YUV_NV12, capi.YUV_NV21):
        mk = lambda dev: cvgs.read_nv12(dm if dev else hm, None, rng, prim, alpha=False, layout=layout)
        want = run(device, oracle, "identity, full-resolution read", mk, [], (SW, SH), 1, (rng, prim, layout), kernel="nv12w_interp", both=False)
        assert (want[0][0] == host[:SH]).all() and (want[0][1] == host[SH:]).all(), "the restatement itself does not return the surface"
        mk = lambda dev: nv12_read([dm if dev else hm], (SW, SH), rng, prim, layout)
        want = run(device, oracle, "identity, resize at factor 1", mk, [], (SW, SH), 1, (rng, prim, layout), kernel="nv12w_nv12_resize")
        assert (want[0][0] == host[:SH]).all() and (want[0][1] == host[SH:]).all()


def case_batches(device, lib, oracle, batch):
    """1 and 5 planes travel in the kernel arguments (8 / 64 slots); 70 is beyond them: source and target descriptors go through a staged table."""
    _, hm, dm = frame(device, "NV12")
    crops = [CROPS[i % len(CROPS)] for i in range(batch)]
    mk = lambda dev: nv12_read([(dm if dev else hm).nv12_roi(*c) for c in crops], (34, 14))
    run(device, oracle, "batch %d" % batch, mk, [], (34, 14), batch, (M.LIMITED, M.BT709, M.NV12), kernel="nv12w_nv12_resize")


def case_device_table_from_boxes(device, lib, oracle):
    """A table written by cvgs_plane_tables_from_boxes over the NV12 surface: both kernels read it; the empty box comes out as background."""
    torch = _torch()
    _, hm, dm = frame(device, "NV12")
    rects = [(0, 0, 96, 64), (2, 4, 40, 30), (6, 8, 0, 10), (50, 20, 46, 44)]  # XYWH, even; the third is empty: invalid
    dsize, bg, yuv = (34, 14), [10.0, 200.0, 30.0, 0.0], (M.LIMITED, M.BT601, 0)
    boxes = torch.tensor(rects, dtype=torch.int32, device=device)
    table = torch.zeros((len(rects), 48), dtype=torch.uint8, device=device)
    rects_out = torch.zeros((len(rects), 4), dtype=torch.int32, device=device)
    s = torch.cuda.current_stream()
    cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(dm, boxes, table, len(rects), dsize, cvgs.IGNORE_AR, cvgs.BOX_XYWH_I32, None, rects_out,
                                                         capi.READ_NV12_RESIZE_LINEAR)])
    torch.cuda.synchronize()
    got = rects_out.cpu().numpy()
    for i in (0, 1, 3):
        assert tuple(got[i]) == rects[i], (i, got[i])  # the views the oracle reads are the builder's
    valid = [rects[i] for i in (0, 1, 3)]
    rgb3 = oracle_rgb(oracle, nv12_read([hm.nv12_roi(*c) for c in valid], dsize), [], dsize, 3)
    rgb = np.stack([rgb3[0], rgb3[1], np.broadcast_to(np.array(bg[:3], np.float32), (14, 34, 3)), rgb3[2]])
    mk = lambda dev: cvgs.resize_boxes(dm, table, len(rects), dsize, bg, yuv=yuv)
    run(device, oracle, "device table", mk, [], dsize, len(rects), (M.FULL, M.BT709, M.NV12), kernel="nv12w_nv12_resize", rgb=rgb)


def case_execute_many(device, lib, oracle):
    """Three chains in ONE cvgs_execute_many call run one by one: each surface bit-exact, nothing outside it changes."""
    torch = _torch()
    _, hm, dm = frame(device, "NV12")
    sets, dsize, out = [CROPS[:2], CROPS[2:5], CROPS[5:7]], (34, 14), (M.LIMITED, M.BT709, M.NV21)
    outs = [[Surface(device, 34, 14) for _ in crops] for crops in sets]
    chains = [[nv12_read([dm.nv12_roi(*c) for c in crops], dsize), cvgs.write_nv12([o.mat for o in os_], *out)] for crops, os_ in zip(sets, outs)]
    held = cvgs.executeMany(torch.cuda.current_stream(), chains)
    torch.cuda.synchronize()
    for i, (crops, os_) in enumerate(zip(sets, outs)):
        rgb = oracle_rgb(oracle, nv12_read([hm.nv12_roi(*c) for c in crops], dsize), [], dsize, len(crops))
        for z, o in enumerate(os_):
            o.check(*M.write_f32(rgb[z], *out), "execute_many chain %d plane %d" % (i, z))
    del held


def all_cases():
    """[(label, callable(device, lib, oracle))]: every case of this module, in the order they run."""
    out = []
    whole, some = [CROPS[0]], CROPS[:5]
    for dsize, crops, label in (((2, 2), whole + [CROPS[4]], "a single block"), ((34, 14), some, "down-scaling, width tail of 2"),
                                ((260, 4), whole + [CROPS[3]], "across the 256-column tile"), ((192, 128), whole, "up-scaling by 2"),
                                ((48, 32), whole, "down-scaling by 2")):
        out.append(("transcode %dx%d (%s)" % (dsize + (label,)), lambda d, l, o, s=dsize, c=crops: case_transcode(d, l, o, s, c, capi.YUV_NV12, (M.LIMITED, M.BT709, M.NV12))))
    out.append(("NV21 in, NV21 out, full range", lambda d, l, o: case_transcode(d, l, o, (34, 14), some, capi.YUV_NV21, (M.FULL, M.BT601, M.NV21))))
    out.append(("NV12 in, NV21 out, BT.2020", lambda d, l, o: case_transcode(d, l, o, (34, 14), some, capi.YUV_NV12, (M.FULL, M.BT2020, M.NV21))))
    out.append(("uv_offset that is not height * step", lambda d, l, o: case_transcode(d, l, o, (34, 14), some, capi.YUV_NV12, (M.LIMITED, M.BT601, M.NV12), gap=40)))
    out.append(("default-value plane", case_default_value_plane))
    out.append(("pixel frames and the program", case_pixel_frames))
    for rng, prim in M.PAIRS:
        out.append(("identity transcoding range %d primaries %d" % (rng, prim), lambda d, l, o, r=rng, p=prim: case_identity_transcoding(d, l, o, r, p)))
    for batch in (1, 5, 70):
        out.append(("batch %d" % batch, lambda d, l, o, b=batch: case_batches(d, l, o, b)))
    out += [("device table from boxes", case_device_table_from_boxes), ("execute_many, three chains", case_execute_many)]
    return out


def run_all(device, lib, oracle, subtests):
    """Every case as a subtest of ONE item.  Only a mismatch (AssertionError) lets the item go on to its next case: whatever else ends a case --
    an error the library returns at launch, a HIP error at the synchronisation -- ends the item, nothing more is started on a card that may have faulted."""
    cases = all_cases()
    assert len(cases) == 21
    stopped = []
    for label, body in cases:
        with subtests.test(case=label):
            assert not stopped, "not started: an earlier case ended with %s" % stopped[0]
            try:
                body(device, lib, oracle)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise
