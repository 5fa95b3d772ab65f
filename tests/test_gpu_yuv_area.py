"""The INTER_AREA kernels of 4:2:0 decoder surfaces (csrc/k_yuv_area.hip) on the GPU, BIT-EXACT against the fp32 restatement of the contract
(tests/yuv_area_model.py): every case compares the stored bytes, with the guard band of tests/test_gpu_area.py around every output buffer.

One 98 x 62 surface per layout (NV12, NV21, P010 with random low 6 bits; seeded random plus a ramp), targets 16 x 8, 33 x 7 and 1 x 8: the
smallest sizes at which every path exists -- shrinking and non-shrinking axes mixed, integer and non-integer factors, 2 x 2 views, odd
widths and heights (the half-weight chroma sample), the clamps at the right and bottom edge.  One lane = one pixel and no tile-dependent
code, so more than one column tile is not needed by any path.

This module holds the cases (case_*, all_cases) and their runner; it defines NO test item of its own (tests/test_gpu_area.py says why):
the ONE item, with a subtest per case, is tests/test_zz_gpu_yuv_area.py."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import area_model as A
from tests import yuv_area_model as M
from tests.test_gpu_area import OUT_BYTES, OUT_DEPTH, Out, SENTINEL, chain

YUV = {"NV12": (capi.YUV_FULL, capi.BT709), "NV21": (capi.YUV_LIMITED, capi.BT601), "P010": (capi.YUV_LIMITED, capi.BT2020)}
N_CASES = 32


def _torch():
    import torch
    return torch


_surfaces = {}


def surfaces(device, name):
    """(host array, host luma GpuMat, device luma GpuMat) of a layout; made once."""
    if name not in _surfaces:
        layout = M.LAYOUTS[name]
        host = M.make_surface(layout)
        t = _torch().from_numpy(host.view(np.uint8).reshape(host.shape[0], -1)).to(device)
        dev = M.luma_mat(host, layout, data=t.data_ptr())
        dev.owner = t
        _surfaces[name] = (host, M.luma_mat(host, layout), dev)
    return _surfaces[name]


def read(mat, name, crops, dsize, alpha, ar=cvgs.IGNORE_AR, bg=None, used=None, interp=cvgs.INTER_AREA):
    rd = cvgs.read_nv12([mat.nv12_area_roi(*c) for c in crops], dsize, YUV[name][0], YUV[name][1], bool(alpha), M.LAYOUTS[name], interp=interp)
    rd.ar = ar
    if bg is not None:
        rd.background = [float(v) for v in bg]
    if used is not None:
        rd.used_planes = used
    return rd


def expected(device, name, crops, dsize, alpha, prog, out, write, ar=cvgs.IGNORE_AR, bg=None, used=None, params=None):
    """The bytes the chain must store, from the fp32 restatement.  The geometry comes from the plane table of the same read over host views."""
    host, host_mat, _ = surfaces(device, name)
    batch, cn = len(crops), 4 if alpha else 3
    used = batch if used is None else used
    dummy = cvgs.GpuMat(batch, cn * dsize[0] * dsize[1], cvgs.CV_8UC1, 16, 1)
    rd = read(host_mat, name, crops, dsize, alpha, ar, bg, used)
    low = cvgs.lower(chain(rd, cn, dummy, dsize, prog, out, "split"))
    P = params if params is not None else A.plane_params(rd)
    vals, depth = M.yuv_area_chain(M.yuv_area_plane_f32, host, M.LAYOUTS[name], crops, P, dsize, used, list(low.desc.read.background),
                                   YUV[name] + (alpha,), A.chain_ops(low.desc), np.float32)
    assert depth == OUT_DEPTH[out]
    if write == "split":
        vals = vals.transpose(0, 3, 1, 2)  # NCHW
    return A.store_bits(vals, depth).tobytes()


def run_case(device, name, crops, dsize, alpha=0, prog="none", out="f32", write="split", ar=cvgs.IGNORE_AR, bg=None, used=None, kernel=None,
             both=True):
    """Run the chain (as dispatched, and with CHAIN_FORCE_GENERIC), compare both with the restatement."""
    torch = _torch()
    _, _, dev_mat = surfaces(device, name)
    batch, cn = len(crops), 4 if alpha else 3
    want = expected(device, name, crops, dsize, alpha, prog, out, write, ar, bg, used)
    elems = cn * dsize[0] * dsize[1]
    for flags in ((0, capi.CHAIN_FORCE_GENERIC) if both else (0,)):
        o = Out(device, batch * elems * OUT_BYTES[out])
        ops = chain(read(dev_mat, name, crops, dsize, alpha, ar, bg, used), cn, o.tensor(batch, elems, out), dsize, prog, out, write)
        got_name = cvgs.kernel_name(*ops, flags=flags)
        assert got_name.startswith("yuv_area_"), got_name
        if flags:
            assert got_name == "yuv_area_interp", got_name
        elif kernel is not None:
            assert got_name == kernel, got_name
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
        torch.cuda.synchronize()
        o.check(want, "%s %s alpha %d %s %s %s flags %d (%s)" % (name, dsize, alpha, prog, out, write, flags, got_name))


def case_every_crop_of_every_layout(device, lib, name, dsize):
    """All crops of the case list in one batch: NV12 / NV21 through the fast kernel and again forced generic, P010 through the interpreted one."""
    run_case(device, name, M.CROPS, dsize, kernel="yuv_area_interp" if name == "P010" else "yuv_area_c3_interp")


def case_fast_kernels_equal_the_interpreted_one_and_the_model(device, lib, name, alpha, prog, out):
    kernel = "yuv_area_c%d_%s%s" % (4 if alpha else 3, prog, {"f32": "", "f16": "_f16", "bf16": "_bf16"}[out])
    run_case(device, name, M.CROPS, (33, 7), alpha, prog, out, kernel=kernel)


def case_aspect_ratio_modes_background_and_unused_planes(device, lib, ar):
    """Letterboxed windows with a non-zero background that runs through the program, and used_planes < batch."""
    crops = M.CROPS[:10]
    for dsize in M.TARGETS:
        run_case(device, "NV12", crops, dsize, 0, "swap_mul_sub_div", "f32", ar=ar, bg=[11.0, 22.5, 33.0, 0.0], used=8)
    run_case(device, "P010", crops, (16, 8), 1, "mul_sub_div", "f32", ar=ar, bg=[-5.0, 6.0, 7.5, 8.0], used=8)


def case_batch_sizes(device, lib, batch):
    """1 and 5 planes travel in the kernel arguments; 70 is beyond the 64 inline planes and takes the table path.  The last plane is unused."""
    crops = [M.CROPS[i % len(M.CROPS)] for i in range(batch)]
    run_case(device, "NV21", crops, (16, 8), 1, "swap_mul_sub_div", "f32", bg=[1.0, 2.0, 3.0, 4.0], used=batch - 1, kernel="yuv_area_c4_swap_mul_sub_div")
    run_case(device, "P010", crops, (33, 7), 0, "mul_sub_div", "f32", bg=[1.0, 2.0, 3.0, 4.0], used=batch - 1, both=False)


def case_a_surface_into_one_column(device, lib):
    run_case(device, "NV12", [(0, 0, 98, 62), (2, 0, 96, 40), (2, 4, 1, 8)], M.NARROW_TARGET, 0, "mul_sub_div", "f32")
    run_case(device, "P010", [(0, 0, 98, 62)], M.NARROW_TARGET, 1, write="packed")


def case_packed_pixels_and_the_saturating_u8_image(device, lib):
    """WRITE_PIXEL_3D fp32, and a u8 image (PIXEL_2D with a padded step) through the saturating cast: the interpreted kernel's generic writes."""
    torch = _torch()
    run_case(device, "NV21", M.CROPS, (33, 7), 0, "mul_sub_div", "f32", write="packed", kernel="yuv_area_interp")
    run_case(device, "NV12", M.CROPS[:5], (16, 8), 1, "none", "u8", write="packed", kernel="yuv_area_interp")
    _, _, dev_mat = surfaces(device, "NV12")
    crop, dsize, step = (10, 12, 38, 19), (16, 8), 16 * 3 + 5
    want = np.frombuffer(expected(device, "NV12", [crop], dsize, 0, "interp", "u8", "packed"), np.uint8).reshape(8, 48)
    padded = np.full((8, step), SENTINEL, np.uint8)
    padded[:, :48] = want
    o = Out(device, 8 * step)
    img = cvgs.GpuMat(8, 16, cvgs.CV_8UC3, o.ptr, step, owner=o.t)
    ops = chain(read(dev_mat, "NV12", [crop], dsize, 0), 3, img, dsize, "interp", "u8", "image")
    assert cvgs.kernel_name(*ops) == "yuv_area_interp"
    cvgs.executeOperations(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    o.check(padded.tobytes(), "u8 image with a padded step (the padding must stay)")


def case_device_table_built_on_the_host_for_the_bilinear_kind(device, lib):
    """cvgs_plane_table_build of the chain spelled NV12_RESIZE_LINEAR, copied to the device and handed to the AREA chain."""
    torch = _torch()
    _, _, dev_mat = surfaces(device, "NV21")
    crops, dsize = M.EVEN_CROPS, (33, 7)
    raw = cvgs.build_plane_table(read(dev_mat, "NV21", crops, dsize, 0, interp=cvgs.INTER_LINEAR))
    table = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(device)
    want = expected(device, "NV21", crops, dsize, 0, "swap_mul_sub_div", "f16", "split")
    for flags in (0, capi.CHAIN_FORCE_GENERIC):
        o = Out(device, len(crops) * 3 * 33 * 7 * 2)
        rd = read(dev_mat, "NV21", crops, dsize, 0)
        rd.table = table.data_ptr()
        ops = chain(rd, 3, o.tensor(len(crops), 3 * 33 * 7, "f16"), dsize, "swap_mul_sub_div", "f16")
        low = cvgs.lower(ops)
        assert low.desc.read.flags & capi.READ_FLAG_TABLE_ON_DEVICE and low.desc.read.table_src_lo == cvgs.table_hull(read(dev_mat, "NV21", crops, dsize, 0))[0]
        assert cvgs.kernel_name(*ops, flags=flags) == ("yuv_area_interp" if flags else "yuv_area_c3_swap_mul_sub_div_f16")
        cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
        torch.cuda.synchronize()
        o.check(want, "host-built device table, flags %d" % flags)


def case_device_table_from_boxes_with_an_invalid_box(device, lib):
    """A table written by cvgs_plane_tables_from_boxes with read_kind = NV12_RESIZE_LINEAR, handed to an AREA chain: same bits as the
    restatement over the boxes' views; the invalid box comes out as background (run through the program)."""
    torch = _torch()
    _, host_mat, dev_mat = surfaces(device, "NV12")
    rects = [(0, 0, 98, 62), (10, 12, 38, 18), (4, 6, 0, 10), (56, 38, 42, 24)]  # XYWH, even; the third is empty: invalid
    dsize, bg = (16, 8), [9.0, 8.0, 7.0, 0.0]
    boxes = torch.tensor(rects, dtype=torch.int32, device=device)
    table = torch.zeros((len(rects), 48), dtype=torch.uint8, device=device)
    rects_out = torch.zeros((len(rects), 4), dtype=torch.int32, device=device)
    s = torch.cuda.current_stream()
    cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(dev_mat, boxes, table, len(rects), dsize, cvgs.IGNORE_AR, cvgs.BOX_XYWH_I32, None, rects_out,
                                                         capi.READ_NV12_RESIZE_LINEAR, capi.YUV_NV12)])
    torch.cuda.synchronize()
    got_rects = rects_out.cpu().numpy()
    for i in (0, 1, 3):
        assert tuple(got_rects[i]) == rects[i], (i, got_rects[i])  # the views the model reads are the builder's
    valid = [rects[i] for i in (0, 1, 3)]
    P = A.plane_params(read(host_mat, "NV12", valid, dsize, 0))
    params = [P[0], P[1], dict(P[0], x1=0, y1=0, x2=-1, y2=-1), P[2]]  # the invalid entry: the empty window
    crops = [rects[0], rects[1], rects[0], rects[3]]
    want = expected(device, "NV12", crops, dsize, 0, "swap_mul_sub_div", "f32", "split", bg=bg, params=params)
    for flags in (0, capi.CHAIN_FORCE_GENERIC):
        o = Out(device, len(rects) * 3 * 16 * 8 * 4)
        rd = cvgs.resize_boxes(dev_mat, table, len(rects), dsize, bg, yuv=YUV["NV12"] + (0,), layout=capi.YUV_NV12, interp=cvgs.INTER_AREA)
        assert rd.kind == capi.READ_NV12_RESIZE_AREA
        ops = chain(rd, 3, o.tensor(len(rects), 3 * 16 * 8, "f32"), dsize, "swap_mul_sub_div")
        assert cvgs.kernel_name(*ops, flags=flags) == ("yuv_area_interp" if flags else "yuv_area_c3_swap_mul_sub_div")
        cvgs.executeOperations(s, *ops, flags=flags)
        torch.cuda.synchronize()
        o.check(want, "device table from boxes, flags %d" % flags)
    plane = np.frombuffer(want, np.float32).reshape(4, 3, 8, 16)[2]
    from tests.test_gpu_area import DIV, SUB
    bgp = (np.float32(np.array(bg[:3], np.float32)[::-1]) * np.float32(0.3) - np.array(SUB[:3], np.float32)) / np.array(DIV[:3], np.float32)
    assert (plane == bgp[:, None, None]).all(), "the invalid box is all background"


def case_execute_many_runs_three_chains_one_by_one(device, lib):
    """Three AREA chains in ONE cvgs_execute_many call: each bit-exact, nothing outside its own tensor changes."""
    torch = _torch()
    _, _, dev_mat = surfaces(device, "NV12")
    sets = [M.CROPS[:4], M.CROPS[4:9], M.CROPS[9:14]]
    dsize, elems = (33, 7), 3 * 33 * 7
    outs = [Out(device, len(c) * elems * 4) for c in sets]
    chains = [chain(read(dev_mat, "NV12", crops, dsize, 0), 3, o.tensor(len(crops), elems, "f32"), dsize, "swap_mul_sub_div") for crops, o in zip(sets, outs)]
    held = cvgs.executeMany(torch.cuda.current_stream(), chains)
    torch.cuda.synchronize()
    for i, (crops, o) in enumerate(zip(sets, outs)):
        o.check(expected(device, "NV12", crops, dsize, 0, "swap_mul_sub_div", "f32", "split"), "execute_many chain %d" % i)
    del held


def all_cases():
    """[(label, callable(device, lib))]: every case of this module, in the order they run."""
    ars = (("preserve", cvgs.PRESERVE_AR), ("ignore", cvgs.IGNORE_AR), ("rn_even", cvgs.PRESERVE_AR_RN_EVEN), ("left", cvgs.PRESERVE_AR_LEFT))
    out = []
    for name in M.LAYOUTS:
        for dsize in M.TARGETS:
            out.append(("crops %s %dx%d" % ((name,) + dsize), lambda d, l, n=name, s=dsize: case_every_crop_of_every_layout(d, l, n, s)))
    fast = [("NV12", 0, p, o) for p in ("swap_mul_sub_div", "mul_sub_div", "interp") for o in ("f32", "f16", "bf16")]
    fast += [("NV21", 1, p, "f32") for p in ("swap_mul_sub_div", "mul_sub_div", "interp")] + [("NV21", 1, "swap_mul_sub_div", o) for o in ("f16", "bf16")]
    for name, alpha, prog, o in fast:
        out.append(("fast %s alpha %d %s %s" % (name, alpha, prog, o),
                    lambda d, l, n=name, a=alpha, p=prog, t=o: case_fast_kernels_equal_the_interpreted_one_and_the_model(d, l, n, a, p, t)))
    for label, ar in ars:
        out.append(("aspect ratio %s" % label, lambda d, l, a=ar: case_aspect_ratio_modes_background_and_unused_planes(d, l, a)))
    for batch in (1, 5, 70):
        out.append(("batch %d" % batch, lambda d, l, b=batch: case_batch_sizes(d, l, b)))
    out += [("a surface into one column", case_a_surface_into_one_column), ("packed pixels and the u8 image", case_packed_pixels_and_the_saturating_u8_image),
            ("device table built on the host", case_device_table_built_on_the_host_for_the_bilinear_kind),
            ("device table from boxes with an invalid box", case_device_table_from_boxes_with_an_invalid_box),
            ("execute_many, three chains", case_execute_many_runs_three_chains_one_by_one)]
    return out


def run_all(device, lib, subtests):
    """Every case as a subtest of ONE item.  Only a mismatch (AssertionError) lets the item go on to its next case: whatever else ends a case --
    an error the library returns at launch, a HIP error at the synchronisation -- ends the item, nothing more is started on a card that may have faulted."""
    cases = all_cases()
    assert len(cases) == N_CASES
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
