"""The INTER_AREA kernels (csrc/k_area.hip) on the GPU, BIT-EXACT against the fp32 restatement of the contract (tests/area_model.py):
every case compares the stored bytes (uint32 / uint16 / uint8 views), with a guard band of a sentinel value around every output buffer.

One 97 x 61 source per depth (seeded random plus a ramp), targets 16 x 8 and 33 x 7 (33 is no multiple of the wave, 7 is odd): the smallest
sizes at which every path exists -- shrinking and non-shrinking axes mixed, integer and non-integer factors, one-pixel views, the clamps at
the right and bottom edge, more than one column tile is not needed by any path (one lane = one pixel, no tile-dependent code).

This module holds the 41 cases (case_*, all_cases) and their runner; it defines NO test item of its own.  The GPU suite's list of tests is
kept from growing (tests/test_gpu_warp_edges.py, tests/test_gpu_colour_model.py fold an older item into theirs); this feature leaves every
existing test file as it is and so cannot fold one: its ONE item, with a subtest per case, is tests/test_zz_gpu_area.py -- collected
behind every existing item, so that it takes no existing item's place in that list.  The 41 cases take 2.8 s on an MI355X."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as M

GUARD = 256
SENTINEL = 0xA5
MUL, SUB, DIV, ADD = [0.3] * 4, [40.0, 50.0, 60.0, 70.0], [57.0, 58.0, 59.0, 61.0], [0.125, -3.0, 2.5, 1.0]
SOURCES = {"8UC1": (capi.DEPTH_8U, 1), "8UC3": (capi.DEPTH_8U, 3), "8UC4": (capi.DEPTH_8U, 4), "16UC3": (capi.DEPTH_16U, 3),
           "16SC4": (capi.DEPTH_16S, 4), "32FC1": (capi.DEPTH_32F, 1)}
OUT_DEPTH = {"f32": capi.DEPTH_32F, "f16": capi.DEPTH_16F, "bf16": capi.DEPTH_16BF, "u8": capi.DEPTH_8U}
OUT_BYTES = {"f32": 4, "f16": 2, "bf16": 2, "u8": 1}


def _torch():
    import torch
    return torch


def out_type(out, cn):
    if out == "bf16":
        return cvgs.make_type(capi.DEPTH_16F, cn) | capi.TYPE_FLAG_BF16
    return cvgs.make_type(OUT_DEPTH[out], cn)


def chain(read, cn, out_mat, dsize, prog="none", out="f32", write="split"):
    """read -> program -> [cast] -> write over `out_mat` (only its data pointer, rows and step matter)."""
    f_type = cvgs.make_type(capi.DEPTH_32F, cn)
    ops = [read]
    if prog == "swap_mul_sub_div":
        ops.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f_type))
    if prog != "none":
        ops += [cvgs.multiply(f_type, MUL[:cn]), cvgs.subtract(f_type, SUB[:cn]), cvgs.divide(f_type, DIV[:cn])]
    if prog == "interp":  # one more stage than the compile-time programs
        ops.append(cvgs.add(f_type, ADD[:cn]))
    t = out_type(out, cn)
    if out != "f32":
        ops.append(cvgs.convertTo(f_type, t))
    if write == "split":
        ops.append(cvgs.split(t, out_mat, dsize))
    elif write == "packed":
        ops.append(cvgs.write(t, out_mat, dsize))
    else:
        ops.append(cvgs.write(t, out_mat))
    return ops


class Out:
    """A device buffer with a guard band of SENTINEL bytes on both sides; `mat(...)` views its payload."""

    def __init__(self, device, nbytes):
        torch = _torch()
        self.nbytes = nbytes
        self.t = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.ptr = self.t.data_ptr() + GUARD

    def tensor(self, batch, elems, out):
        """[batch, elems] of the scalar type of `out`: what split / the packed write take."""
        scalar = {"f32": cvgs.CV_32FC1, "f16": cvgs.CV_16FC1, "bf16": cvgs.CV_16BFC1, "u8": cvgs.CV_8UC1}[out]
        return cvgs.GpuMat(batch, elems, scalar, self.ptr, elems * OUT_BYTES[out], owner=self.t)

    def check(self, want_bytes, what):
        got = self.t.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.nbytes:] == SENTINEL).all(), "%s: the guard band changed" % what
        want = np.frombuffer(want_bytes, np.uint8)
        assert want.size == self.nbytes, (want.size, self.nbytes)
        pay = got[GUARD:GUARD + self.nbytes]
        bad = np.flatnonzero(pay != want)
        assert bad.size == 0, "%s: %d bytes differ, first at byte %d (got %d, want %d)" % (what, bad.size, bad[0], pay[bad[0]], want[bad[0]])


_frames = {}


def frames(device, name):
    """(host array, host GpuMat, device GpuMat) of a source type; made once."""
    if name not in _frames:
        depth, cn = SOURCES[name]
        host = M.make_source(depth, cn)
        t = _torch().from_numpy(host.view(np.uint8).reshape(M.SRC_H, -1)).to(device)
        cv_type = cvgs.make_type(depth, cn)
        _frames[name] = (host, cvgs.GpuMat.from_array(host, cv_type),
                         cvgs.GpuMat(M.SRC_H, M.SRC_W, cv_type, t.data_ptr(), host.strides[0], owner=t))
    return _frames[name]


def expected(host, host_mat, crops, dsize, cn, src_type, prog, out, write, ar=cvgs.IGNORE_AR, bg=None, used=None, params=None):
    """The bytes the chain must store, from the fp32 restatement.  The geometry comes from the plane table of the same read over host views."""
    batch = len(crops)
    used = batch if used is None else used
    dummy = cvgs.GpuMat(batch, cn * dsize[0] * dsize[1], cvgs.CV_8UC1, 16, 1)
    rd = cvgs.resize(src_type, cvgs.INTER_AREA, [host_mat.roi(*c) for c in crops], dsize, used, bg, ar)
    low = cvgs.lower(chain(rd, cn, dummy, dsize, prog, out, "split"))
    P = params if params is not None else M.plane_params(rd)
    srcs = [host[c[1]:c[1] + c[3], c[0]:c[0] + c[2]] for c in crops]
    vals, depth = M.area_chain(M.area_plane_f32, srcs, P, dsize, used, batch, list(low.desc.read.background), M.chain_ops(low.desc), np.float32)
    assert depth == OUT_DEPTH[out]
    if write == "split":
        vals = vals.transpose(0, 3, 1, 2)  # NCHW
    return M.store_bits(vals, depth).tobytes()


def run_case(device, name, crops, dsize, prog="none", out="f32", write="split", ar=cvgs.IGNORE_AR, bg=None, used=None, kernel=None,
             both=True):
    """Run the chain (as dispatched, and with CHAIN_FORCE_GENERIC), compare both with the restatement."""
    torch = _torch()
    depth, cn = SOURCES[name]
    host, host_mat, dev_mat = frames(device, name)
    src_type = cvgs.make_type(depth, cn)
    batch = len(crops)
    want = expected(host, host_mat, crops, dsize, cn, src_type, prog, out, write, ar, bg, used)
    elems = cn * dsize[0] * dsize[1]
    for flags in ((0, capi.CHAIN_FORCE_GENERIC) if both else (0,)):
        o = Out(device, batch * elems * OUT_BYTES[out])
        rd = cvgs.resize(src_type, cvgs.INTER_AREA, [dev_mat.roi(*c) for c in crops], dsize, used, bg, ar)
        ops = chain(rd, cn, o.tensor(batch, elems, out), dsize, prog, out, write)
        got_name = cvgs.kernel_name(*ops, flags=flags)
        assert got_name.startswith("area_"), got_name
        if flags:
            assert got_name == "area_interp", got_name
        elif kernel is not None:
            assert got_name == kernel, got_name
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
        torch.cuda.synchronize()
        o.check(want, "%s %s %s %s %s flags %d (%s)" % (name, dsize, prog, out, write, flags, got_name))


def case_every_crop_of_every_source(device, lib, name, dsize):
    """All crops of the case list in one batch: whole frame, 1 x 1, 1 x 40, 40 x 1, identity, up-scaling, mixed axes, 2.37x, exact 2x / 3x,
    the right and bottom edge -- 8UC1 / 16UC3 / 16SC4 / 32FC1 through the interpreted kernel, 8UC3 / 8UC4 through the fast one and again forced generic."""
    cn = SOURCES[name][1]
    fast = {"8UC3": "area_u8c3_interp", "8UC4": "area_u8c4_interp"}.get(name, "area_interp")
    run_case(device, name, M.CROPS, dsize, write="split" if cn > 1 else "packed", kernel=fast if cn > 1 else "area_interp")


def case_fast_kernels_equal_the_interpreted_one_and_the_model(device, lib, name, prog, out):
    """The fast kernel's three programs x three planar tensor types: same bits as the restatement, and as CHAIN_FORCE_GENERIC."""
    kernel = "area_u8c%d_%s%s" % (SOURCES[name][1], prog, {"f32": "", "f16": "_f16", "bf16": "_bf16"}[out])
    run_case(device, name, M.CROPS, (33, 7), prog, out, kernel=kernel)


def case_aspect_ratio_modes_background_and_unused_planes(device, lib, ar):
    """Letterboxed windows with a non-zero background that runs through the program, and used_planes < batch."""
    crops = M.CROPS[:9]
    for dsize in M.TARGETS:
        run_case(device, "8UC3", crops, dsize, "swap_mul_sub_div", "f32", ar=ar, bg=[11.0, 22.5, 33.0, 0.0], used=7)
    run_case(device, "16SC4", crops, (16, 8), "mul_sub_div", "f32", ar=ar, bg=[-5.0, 6.0, 7.5, 8.0], used=7)


def case_batch_sizes(device, lib, batch):
    """1 and 5 planes travel in the kernel arguments; 70 is beyond the 64 inline planes and takes the table path."""
    crops = [M.CROPS[i % len(M.CROPS)] for i in range(batch)]
    run_case(device, "8UC3", crops, (16, 8), "swap_mul_sub_div", "f32", kernel="area_u8c3_swap_mul_sub_div")
    run_case(device, "16UC3", crops, (33, 7), "mul_sub_div", "f32", both=False)


def case_96_columns_into_one(device, lib):
    run_case(device, "8UC3", [(0, 0, 96, 61), (1, 0, 96, 40)], M.NARROW_TARGET, "mul_sub_div", "f32")
    run_case(device, "32FC1", [(0, 0, 96, 61)], M.NARROW_TARGET, write="packed")


def case_packed_pixels_and_the_saturating_u8_image(device, lib):
    """WRITE_PIXEL_3D fp32, and a u8 image (PIXEL_2D with a padded step) through the saturating cast: the interpreted kernel's generic writes."""
    torch = _torch()
    run_case(device, "8UC3", M.CROPS, (33, 7), "mul_sub_div", "f32", write="packed", kernel="area_interp")
    run_case(device, "8UC4", M.CROPS[:5], (16, 8), "none", "u8", write="packed", kernel="area_interp")
    host, host_mat, dev_mat = frames(device, "8UC3")
    crop, dsize, step = (11, 13, 38, 19), (16, 8), 16 * 3 + 5
    want = np.frombuffer(expected(host, host_mat, [crop], dsize, 3, cvgs.CV_8UC3, "interp", "u8", "packed"), np.uint8).reshape(8, 48)
    padded = np.full((8, step), SENTINEL, np.uint8)
    padded[:, :48] = want
    o = Out(device, 8 * step)
    img = cvgs.GpuMat(8, 16, cvgs.CV_8UC3, o.ptr, step, owner=o.t)
    ops = chain(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, dev_mat.roi(*crop), dsize), 3, img, dsize, "interp", "u8", "image")
    assert cvgs.kernel_name(*ops) == "area_interp"
    cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    o.check(padded.tobytes(), "u8 image with a padded step (the padding must stay)")


def case_device_table_from_boxes_with_an_invalid_box(device, lib):
    """A table written by cvgs_plane_tables_from_boxes with read_kind = RESIZE_LINEAR, handed to an AREA chain: same bits as the
    restatement over the boxes' views; the invalid box comes out as background (run through the program)."""
    torch = _torch()
    host, host_mat, dev_mat = frames(device, "8UC3")
    rects = [(0, 0, 97, 61), (11, 13, 38, 19), (5, 7, 0, 10), (56, 38, 41, 23)]  # XYWH; the third is empty: invalid
    dsize, bg = (16, 8), [9.0, 8.0, 7.0, 0.0]
    boxes = torch.tensor(rects, dtype=torch.int32, device=device)
    table = torch.zeros((len(rects), 48), dtype=torch.uint8, device=device)
    rects_out = torch.zeros((len(rects), 4), dtype=torch.int32, device=device)
    s = torch.cuda.current_stream()
    cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(dev_mat, boxes, table, len(rects), dsize, cvgs.IGNORE_AR, cvgs.BOX_XYWH_I32, None, rects_out,
                                                         capi.READ_RESIZE_LINEAR)])
    torch.cuda.synchronize()
    got_rects = rects_out.cpu().numpy()
    for i in (0, 1, 3):
        assert tuple(got_rects[i]) == rects[i], (i, got_rects[i])  # the views the model reads are the builder's
    valid = [rects[i] for i in (0, 1, 3)]
    P = M.plane_params(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [host_mat.roi(*c) for c in valid], dsize))
    params = [P[0], P[1], dict(P[0], x1=0, y1=0, x2=-1, y2=-1), P[2]]  # the invalid entry: the empty window
    crops = [rects[0], rects[1], rects[0], rects[3]]
    for prog, flags in (("swap_mul_sub_div", 0), ("swap_mul_sub_div", capi.CHAIN_FORCE_GENERIC)):
        want = expected(host, host_mat, crops, dsize, 3, cvgs.CV_8UC3, prog, "f32", "split", bg=bg, params=params)
        o = Out(device, len(rects) * 3 * 16 * 8 * 4)
        rd = cvgs.resize_boxes(dev_mat, table, len(rects), dsize, bg, interp=cvgs.INTER_AREA)
        assert rd.kind == capi.READ_RESIZE_AREA
        ops = chain(rd, 3, o.tensor(len(rects), 3 * 16 * 8, "f32"), dsize, prog)
        assert cvgs.kernel_name(*ops, flags=flags) == ("area_interp" if flags else "area_u8c3_swap_mul_sub_div")
        cvgs.executeOperations(s, *ops, flags=flags)
        torch.cuda.synchronize()
        o.check(want, "device table, flags %d" % flags)
        plane = np.frombuffer(want, np.float32).reshape(4, 3, 8, 16)[2]
        bgp = (np.float32(np.array(bg[:3], np.float32)[::-1]) * np.float32(0.3) - np.array(SUB[:3], np.float32)) / np.array(DIV[:3], np.float32)
        assert (plane == bgp[:, None, None]).all(), "the invalid box is all background"


def case_execute_many_runs_three_area_chains_one_by_one(device, lib):
    """Three AREA chains in ONE cvgs_execute_many call: each bit-exact, nothing outside its own tensor changes (the tensors sit side by side
    in one allocation, a guard band between them)."""
    torch = _torch()
    host, host_mat, dev_mat = frames(device, "8UC3")
    sets = [M.CROPS[:4], M.CROPS[4:9], M.CROPS[9:13]]
    dsize, elems = (33, 7), 3 * 33 * 7
    outs = [Out(device, len(c) * elems * 4) for c in sets]
    chains = [chain(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [dev_mat.roi(*c) for c in crops], dsize), 3, o.tensor(len(crops), elems, "f32"), dsize,
                    "swap_mul_sub_div") for crops, o in zip(sets, outs)]
    held = cvgs.executeMany(torch.cuda.current_stream(), chains)
    torch.cuda.synchronize()
    for i, (crops, o) in enumerate(zip(sets, outs)):
        o.check(expected(host, host_mat, crops, dsize, 3, cvgs.CV_8UC3, "swap_mul_sub_div", "f32", "split"), "execute_many chain %d" % i)
    del held


def all_cases():
    """[(label, callable(device, lib))]: every case of this module, in the order they run."""
    ars = (("preserve", cvgs.PRESERVE_AR), ("ignore", cvgs.IGNORE_AR), ("rn_even", cvgs.PRESERVE_AR_RN_EVEN), ("left", cvgs.PRESERVE_AR_LEFT))
    out = []
    for name in SOURCES:
        for dsize in M.TARGETS:
            out.append(("crops %s %dx%d" % ((name,) + dsize), lambda d, l, n=name, s=dsize: case_every_crop_of_every_source(d, l, n, s)))
    for name in ("8UC3", "8UC4"):
        for prog in ("swap_mul_sub_div", "mul_sub_div", "interp"):
            for o in ("f32", "f16", "bf16"):
                out.append(("fast %s %s %s" % (name, prog, o),
                            lambda d, l, n=name, p=prog, t=o: case_fast_kernels_equal_the_interpreted_one_and_the_model(d, l, n, p, t)))
    for label, ar in ars:
        out.append(("aspect ratio %s" % label, lambda d, l, a=ar: case_aspect_ratio_modes_background_and_unused_planes(d, l, a)))
    for batch in (1, 5, 70):
        out.append(("batch %d" % batch, lambda d, l, b=batch: case_batch_sizes(d, l, b)))
    out += [("96 columns into one", case_96_columns_into_one), ("packed pixels and the u8 image", case_packed_pixels_and_the_saturating_u8_image),
            ("device table with an invalid box", case_device_table_from_boxes_with_an_invalid_box),
            ("execute_many, three chains", case_execute_many_runs_three_area_chains_one_by_one)]
    return out


def run_all(device, lib, subtests):
    """Every case as a subtest of ONE item.  Only a mismatch (AssertionError) lets the item go on to its next case: whatever else ends a case --
    an error the library returns at launch, a HIP error at the synchronisation -- ends the item, nothing more is started on a card that may have faulted."""
    cases = all_cases()
    assert len(cases) == 41
    stopped = []
    for label, body in cases:
        with subtests.test(case=label):
            assert not stopped, "not started: an earlier case ended with %s" % stopped[0]
            try:
                body(device, lib)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise
