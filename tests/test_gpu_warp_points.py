"""cvgs_warp_tables_from_points on the GPU: the device-built warp table against cvgs_warp_table_build_host byte for byte, chains over it
against host-described warp chains (and the oracle) bit for bit, landmarks -> table -> chain inside one linear HIP graph, and bounds.

The frame is 97 x 61 with a padded step; the targets are (16, 8) and (70, 9) -- the second makes the fast kernel run two column tiles, a
partial one, and a partial 4-row tile.  Every read these tests cause lies inside the frame by construction: the warp kernels test
0 <= sx < w && 0 <= sy < h before any tap, and w / h / step / data of every table entry are the host-validated frame's."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from oracle import oracle_binding
from tests import helpers as H
from tests import warp_point_cases as P
from tests.test_bf16_types import rne_bf16
from tests.test_warp_points import N, _chain

pytestmark = pytest.mark.gpu

W, HH, STEP = 97, 61, 304
TARGETS = ((16, 8), (70, 9))
COUNTS = (None, 0, 1, "max-1", "max", "max+5", -3)
ENTRY = np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")])


def _torch():
    import torch
    return torch


class Frame:
    def __init__(self, device, cv_type=cvgs.CV_8UC3, step=STEP, seed=1):
        torch = _torch()
        self.host = H.random_u8((HH, step), seed=seed)
        self.t = torch.from_numpy(self.host).to(device)
        self.cv_type, self.step = cv_type, step
        self.mat = cvgs.GpuMat(HH, W, cv_type, self.t.data_ptr(), step, owner=self.t)
        self.host_mat = cvgs.GpuMat(HH, W, cv_type, self.host.ctypes.data, step, owner=self.host)


def _resolve(count, n):
    return {None: None, "max-1": n - 1, "max": n, "max+5": n + 5}.get(count, count)


def _sets():
    """[(name, fit, template, items)]: the CPU grid cut down (about 2,000 items in all) plus every pinned invalid case."""
    out = []
    for name, tmpl, pts in P.similarity_grid(1000, 150):
        out.append((name, P.SIMILARITY, tmpl, np.concatenate([pts, P.pinned_invalid(len(tmpl), tmpl)[0]])))
    out.append(("affine3", P.AFFINE3, P.TMPL_BOX, np.concatenate([P.random_affine_items(300, 11), P.pinned_invalid(3, P.TMPL_BOX + np.float32(5.0))[0],
                                                                 np.array([[[0, 0], [3e38, 0], [0, 3e38]]], np.float32)])))
    return out


def _device_build(device, frame, pts, tmpl, fit, dsize, count, guard=True):
    """(table bytes [n, 64], valid [n]) from ONE cvgs_warp_tables_from_points call; one guard entry on either side of both buffers."""
    torch = _torch()
    n = len(pts)
    pt = torch.from_numpy(np.ascontiguousarray(pts)).to(device)
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
    tbuf = torch.full((n + 2, 64), 0xA5, dtype=torch.uint8, device=device)
    vbuf = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    d = cvgs.warp_table_desc(frame.mat, pt, tbuf[1:], n, dsize, tmpl, fit, count=ct, valid=vbuf[1:])
    cvgs.warp_tables_from_points(torch.cuda.current_stream(), [d])
    torch.cuda.synchronize()
    assert (tbuf[0] == 0xA5).all() and (tbuf[-1] == 0xA5).all() and vbuf[0] == 0x5A5A5A5A and vbuf[-1] == 0x5A5A5A5A, "a guard entry changed"
    return tbuf[1:-1].cpu().numpy(), vbuf[1:-1].cpu().numpy()


def _host_build(frame, pts, tmpl, fit, dsize, count):
    d = cvgs.warp_table_desc(frame.mat, 4096, 8192, len(pts), dsize, tmpl, fit)
    raw, valid = cvgs.build_warp_table_host(d, pts, count)
    return np.frombuffer(raw, np.uint8).reshape(len(pts), 64), np.array(valid, np.int32)


def test_table_bytes(device, lib):
    """About 2,000 items over both fits (K = 2, 3, 5, 16, a mirrored set, every pinned invalid case), seven counts: the device-built table
    equals the host-built one byte for byte, valid_out too, and the guard entries around both buffers are unchanged."""
    frame = Frame(device)
    sets = _sets()
    assert 1900 <= sum(len(s[3]) for s in sets) <= 2400
    checked = 0
    for k, (name, fit, tmpl, pts) in enumerate(sets):
        dsize = TARGETS[k % 2]
        for count in COUNTS:
            cnt = _resolve(count, len(pts))
            want, want_v = _host_build(frame, pts, tmpl, fit, dsize, cnt)
            got, got_v = _device_build(device, frame, pts, tmpl, fit, dsize, cnt)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, "%s count %s: %d entries differ, first %d: points %s\n got  %s\n want %s" % (
                name, count, bad.size, bad[0], pts[bad[0]].tolist(), got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())
            assert (got_v == want_v).all() and (got_v.astype(bool) == P.model_valid(fit, pts, cnt)).all(), (name, count)
            checked += 1
    assert checked == len(sets) * len(COUNTS)


@pytest.mark.parametrize("n_frames", [2, 16], ids=["two_frames", "sixteen_frames"])
def test_several_frames_in_one_call_equal_single_calls(device, lib, n_frames):
    torch = _torch()
    sets = _sets()
    jobs = []
    for k in range(n_frames):
        name, fit, tmpl, pts = sets[k % len(sets)]
        pts = pts[:: (1 if k == 0 else 5 + k)]
        jobs.append((Frame(device, seed=50 + k), pts, tmpl, fit, TARGETS[k % 2], (None, len(pts) // 2, len(pts) + 3)[k % 3]))
    single = [_device_build(device, *j) for j in jobs]
    descs, outs, keep = [], [], []
    for f, pts, tmpl, fit, ds, cnt in jobs:
        pt = torch.from_numpy(np.ascontiguousarray(pts)).to(device)
        ct = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=device)
        table = torch.full((len(pts), 64), 0xCD, dtype=torch.uint8, device=device)
        valid = torch.full((len(pts),), -77, dtype=torch.int32, device=device)
        descs.append(cvgs.warp_table_desc(f.mat, pt, table, len(pts), ds, tmpl, fit, count=ct, valid=valid))
        outs.append((table, valid))
        keep += [pt, ct]
    cvgs.warp_tables_from_points(torch.cuda.current_stream(), descs)
    torch.cuda.synchronize()
    for k, ((table, valid), (want_t, want_v)) in enumerate(zip(outs, single)):
        assert (table.cpu().numpy() == want_t).all() and (valid.cpu().numpy() == want_v).all(), "frame %d of %d" % (k, n_frames)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _e2e_items(dsize, rng_seed=3):
    """(template [5, 2], points float32 [24, 5, 2], count): the template of the target under 24 similarity transforms -- rotations by 0, 90,
    180 degrees and in between, up- and down-scaling, centres inside, across each edge and far outside the frame --, a NaN item, a
    coincident item, and two items beyond the count."""
    tmpl = (P.TMPL5.astype(np.float64) * np.array([dsize[0] / 112.0, dsize[1] / 112.0])).astype(np.float32)
    c = np.array([(dsize[0] - 1) / 2.0, (dsize[1] - 1) / 2.0])
    specs = [(0, 1.0, 30, 20), (90, 1.0, 40, 30), (180, 1.0, 50, 30), (270, 2.0, 48, 30), (30, 0.5, 20, 40), (45, 3.0, 48, 30), (0, 0.25, 10, 10),
             (17, 1.5, 0, 0), (200, 1.2, 96, 60), (90, 2.5, 96, 5), (0, 4.0, 48, -10), (135, 1.0, -3, 30), (0, 1.0, 300, 300), (60, 0.7, -200, 20),
             (10, 1.0, 48, 75), (0, 6.0, 48, 30), (180, 0.4, 90, 55), (90, 0.5, 5, 55), (300, 1.1, 60, 12), (0, 1.0, 88, 30), (15, 2.0, 48, 30),
             (75, 0.9, 30, 30), (0, 1.0, 40, 20), (33, 1.3, 70, 40)]
    pts = np.zeros((len(specs), 5, 2), np.float64)
    for i, (deg, s, cx, cy) in enumerate(specs):
        a = np.deg2rad(deg)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        pts[i] = s * (tmpl.astype(np.float64) - c) @ R.T + np.array([cx, cy])
    pts = pts.astype(np.float32)
    pts[6, 2, 1] = np.nan
    pts[21] = np.float32(31.5)
    return tmpl, pts, len(specs) - 2


def _classify(tab, valid, dsize):
    """Per item: 'invalid', 'outside' (no destination pixel lands in the frame), 'partly', 'inside'."""
    ys, xs = np.mgrid[0:dsize[1], 0:dsize[0]]
    out = []
    for e, v in zip(tab, valid):
        m = e["m"].astype(np.float64)
        sx, sy = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
        ins = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < HH)
        out.append("invalid" if not v else "outside" if not ins.any() else "inside" if ins.all() else "partly")
    return out


def _nbytes(cn, dsize, kind):
    return N * cn * dsize[0] * dsize[1] * (2 if kind in ("f16", "bf16") else 4)


def _e2e(device, lib, dsize, cv_type=cvgs.CV_8UC3, cn=3, kind="f32", flags=0, warp_type=cvgs.WARP_AFFINE, used=None, default=None):
    """One chain over the device-built table == the host-described chain over the table's own floats == the oracle; the kernel's name."""
    torch = _torch()
    esz = cvgs.elem_size(cv_type)
    frame = Frame(device, cv_type, (W * esz + 15) // 8 * 8, seed=7)
    tmpl, pts, count = _e2e_items(dsize)
    assert len(pts) == N
    s = torch.cuda.current_stream()
    pt = torch.from_numpy(pts).to(device)
    ct = torch.tensor([count], dtype=torch.int32, device=device)
    table = torch.zeros((N, 64), dtype=torch.uint8, device=device)
    valid = torch.zeros((N,), dtype=torch.int32, device=device)
    cvgs.warp_tables_from_points(s, [cvgs.warp_table_desc(frame.mat, pt, table, N, dsize, tmpl, count=ct, valid=valid)])
    nb = _nbytes(cn, dsize, kind)
    out_dev = torch.full((nb,), 0x5B, dtype=torch.uint8, device=device)
    ops = _chain(cvgs.warp_table(warp_type, frame.mat, table, N, dsize, used, default), cn, out_dev.data_ptr(), dsize, kind)
    name = cvgs.kernel_name(*ops, flags=flags)
    cvgs.executeOperations(s, *ops, flags=flags)
    torch.cuda.synchronize()
    tab = np.frombuffer(table.cpu().numpy().tobytes(), ENTRY)
    cls = _classify(tab, valid.cpu().numpy(), dsize)
    assert cls.count("invalid") == 4 and cls.count("outside") >= 2 and cls.count("partly") >= 4 and cls.count("inside") >= 2, cls
    assert len([c for c in cls if c != "inside"]) >= 8  # a third of the items invalid, partly or wholly outside
    # the host-described twin: the nine floats of each table entry
    rk = capi.READ_WARP_AFFINE if warp_type == cvgs.WARP_AFFINE else capi.READ_WARP_PERSPECTIVE
    flat = [float(v) for v in tab["m"].reshape(-1)]

    def twin(mat):
        rd = cvgs.ReadIOp(rk, cv_type, [mat] * N, used, dsize, cvgs.IGNORE_AR, default)
        rd.warp, rd.warp_sizes = flat, None
        return rd

    out_host = torch.full((nb,), 0x5C, dtype=torch.uint8, device=device)
    host_ops = _chain(twin(frame.mat), cn, out_host.data_ptr(), dsize, kind)
    assert cvgs.kernel_name(*host_ops, flags=flags) == name
    cvgs.executeOperations(s, *host_ops, flags=flags)
    torch.cuda.synchronize()
    got, want = out_dev.cpu().numpy(), out_host.cpu().numpy()
    assert (got == want).all(), "%s: %d bytes differ from the host-described chain" % (name, int((got != want).sum()))
    if kind == "bf16":  # the oracle computes the fp32 chain; CV_16BF is its result rounded to nearest even (tests/test_gpu_bf16.py)
        ref32 = np.zeros((nb // 2,), np.float32)
        oracle_binding.execute(cvgs.lower(_chain(twin(frame.host_mat), cn, ref32.ctypes.data, dsize, "f32"), flags))
        ref = rne_bf16(ref32).view(np.uint8)
    else:
        ref = np.full((nb,), 0x5D, np.uint8)
        oracle_binding.execute(cvgs.lower(_chain(twin(frame.host_mat), cn, ref.ctypes.data, dsize, kind), flags))
    assert (got == ref).all(), "%s: %d bytes differ from the oracle" % (name, int((got != ref).sum()))
    per = nb // N
    planes = got.reshape(N, per)
    zero_plane = planes[[i for i, c in enumerate(cls) if c in ("invalid", "outside")][0]]
    for i, c in enumerate(cls):  # invalid and wholly outside planes: 0 through the program, all alike; the others differ from it
        if used is not None and i >= used:
            continue
        assert (planes[i] == zero_plane).all() == (c in ("invalid", "outside")), (i, c)
    return name


@pytest.mark.parametrize("dsize", TARGETS, ids=["16x8", "70x9"])
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_end_to_end_u8c3(device, lib, dsize, kind):
    want = {"f32": "warp_affine_u8c3_swap_mul_sub_div", "f16": "warp_affine_u8c3_swap_mul_sub_div_f16", "bf16": "warp_affine_u8c3_swap_mul_sub_div_bf16"}
    assert _e2e(device, lib, dsize, kind=kind) == want[kind]


@pytest.mark.parametrize("dsize", TARGETS, ids=["16x8", "70x9"])
@pytest.mark.parametrize("case", ["8UC4", "packed", "generic", "16UC3", "f64", "perspective", "used_planes"])
def test_end_to_end_variants(device, lib, case, dsize):
    if case == "8UC4":
        assert _e2e(device, lib, dsize, cvgs.CV_8UC4, 4) == "warp_affine_u8c4_swap_mul_sub_div"
    elif case == "packed":
        assert _e2e(device, lib, dsize, kind="packed") == "warp_affine_u8c3_packed_f32"
    elif case == "generic":
        assert _e2e(device, lib, dsize, flags=capi.CHAIN_FORCE_GENERIC) == "warp_affine_interp"
    elif case == "16UC3":
        assert _e2e(device, lib, dsize, cvgs.CV_16UC3, 3) == "warp_affine_interp"
    elif case == "f64":
        assert _e2e(device, lib, dsize, kind="f64") == "warp64_table"
    elif case == "perspective":
        assert _e2e(device, lib, dsize, warp_type=cvgs.WARP_PERSPECTIVE) == "warp_perspective_u8c3_swap_mul_sub_div"
    else:
        assert _e2e(device, lib, dsize, used=17, default=[10.0, 20.0, 30.0]) == "warp_affine_u8c3_swap_mul_sub_div"


# ---- no host in the loop --------------------------------------------------------------------------------------------------------------
def _host_described(device, frame, pts, tmpl, count, dsize):
    """The eager host-described result for landmarks known on the host: matrices from cvgs_warp_table_build_host."""
    torch = _torch()
    tabb, _ = _host_build(frame, pts, tmpl, P.SIMILARITY, dsize, count)
    rd = cvgs.ReadIOp(capi.READ_WARP_AFFINE, frame.cv_type, [frame.mat] * N, None, dsize, cvgs.IGNORE_AR, None)
    rd.warp, rd.warp_sizes = [float(v) for v in np.frombuffer(tabb.tobytes(), ENTRY)["m"].reshape(-1)], None
    out = torch.full((N, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device)
    cvgs.executeOperations(torch.cuda.current_stream(), *_chain(rd, 3, out.data_ptr(), dsize))
    torch.cuda.synchronize()
    return out


def test_no_host_in_the_loop(device, lib):
    """Points and count written by device copies -> cvgs_warp_tables_from_points -> the chain, captured on ONE stream as one linear graph
    and replayed twice with different device-side points and counts: each replay equals the eager host-described result."""
    torch = _torch()
    dsize = (70, 9)
    frame = Frame(device, seed=41)
    tmpl, pts_a, _ = _e2e_items(dsize)
    pts_b = np.ascontiguousarray(pts_a[::-1]) + np.float32(1.25)
    rounds = [(pts_a, N - 7), (pts_b, N + 2)]
    src_pts = torch.zeros((N, 5, 2), dtype=torch.float32, device=device)
    src_cnt = torch.zeros((1,), dtype=torch.int32, device=device)
    staged = [(torch.from_numpy(p).to(device), torch.tensor([c], dtype=torch.int32, device=device)) for p, c in rounds]
    pt = torch.zeros((N, 5, 2), dtype=torch.float32, device=device)
    ct = torch.zeros((1,), dtype=torch.int32, device=device)
    table = torch.zeros((N, 64), dtype=torch.uint8, device=device)
    out = torch.full((N, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device)
    desc = cvgs.warp_table_desc(frame.mat, pt, table, N, dsize, tmpl, count=ct)
    ops = _chain(cvgs.warp_table(cvgs.WARP_AFFINE, frame.mat, table, N, dsize), 3, out.data_ptr(), dsize)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        pt.copy_(src_pts)
        ct.copy_(src_cnt)
        cvgs.warp_tables_from_points(s, [desc])
        cvgs.executeOperations(s, *ops)
    torch.cuda.synchronize()
    assert (out == -5.0).all() and (table == 0).all(), "capture itself must not run anything"
    results = []
    for r, (p, c) in enumerate(rounds):
        src_pts.copy_(staged[r][0])  # device copies only
        src_cnt.copy_(staged[r][1])
        g.replay()
        torch.cuda.synchronize()
        want = _host_described(device, frame, p, tmpl, c, dsize)
        assert torch.equal(out, want), "replay %d" % r
        results.append(want)
    assert not torch.equal(results[0], results[1])


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def test_edge_warps_stay_inside_the_frame(device, lib):
    """The frame sits inside a larger allocation whose margin holds 255; the frame's own pixels are <= 127 and the chain is monotone, so one
    margin tap with any weight would show.  The points push the warps across every edge and corner: no output exceeds the value of a 127
    pixel or falls below that of 0, and the margin is unchanged."""
    torch = _torch()
    top, left = 8, 24
    step = left + W * 3 + 29
    big = torch.full((HH + 2 * top, step), 255, dtype=torch.uint8, device=device)
    big[top:top + HH, left:left + W * 3] = torch.from_numpy(H.random_u8((HH, W * 3), seed=77) & 0x7f).to(device)
    before = big.clone()
    mat = cvgs.GpuMat(HH, W, cvgs.CV_8UC3, big.data_ptr() + top * step + left, step, owner=big)
    s = torch.cuda.current_stream()
    for dsize in TARGETS:
        tmpl = (P.TMPL5.astype(np.float64) * np.array([dsize[0] / 112.0, dsize[1] / 112.0])).astype(np.float32)
        c = np.array([(dsize[0] - 1) / 2.0, (dsize[1] - 1) / 2.0])
        items = []
        for cx, cy in ((0, 0), (48, 0), (96, 0), (0, 30), (96, 30), (0, 60), (48, 60), (96, 60), (-0.5, -0.5), (96.5, 60.5), (48, 30), (96.99, 30)):
            for deg, sc in ((0, 1.0), (37, 2.0)):
                a = np.deg2rad(deg)
                R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
                items.append(sc * (tmpl.astype(np.float64) - c) @ R.T + np.array([cx, cy]))
        pts = np.array(items, np.float32)
        assert len(pts) == N
        pt = torch.from_numpy(pts).to(device)
        tbuf = torch.full((N + 2, 64), 0xA5, dtype=torch.uint8, device=device)
        cvgs.warp_tables_from_points(s, [cvgs.warp_table_desc(mat, pt, tbuf[1:], N, dsize, tmpl)])
        out = torch.full((N, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device)
        cvgs.executeOperations(s, *_chain(cvgs.warp_table(cvgs.WARP_AFFINE, mat, tbuf[1:], N, dsize), 3, out.data_ptr(), dsize))
        torch.cuda.synchronize()
        assert (tbuf[0] == 0xA5).all() and (tbuf[-1] == 0xA5).all()
        tab = np.frombuffer(tbuf[1:-1].cpu().numpy().tobytes(), ENTRY)
        assert (tab["data"] == mat.data).all() and (tab["w"] == W).all() and (tab["h"] == HH).all() and (tab["step"] == step).all()
        cls = _classify(tab, np.ones(N, bool), dsize)
        assert cls.count("partly") >= 16, cls  # the warps do cross the edges
        hi = max((127.0 * H.K1_ALPHA - sub) / div for sub, div in zip(H.K1_SUB[3], H.K1_DIV[3])) * (1 + 1e-5) + 1e-5
        lo = min((0.0 - sub) / div for sub, div in zip(H.K1_SUB[3], H.K1_DIV[3])) - 1e-5
        assert float(out.max()) <= hi and float(out.min()) >= lo, (float(out.min()), float(out.max()), lo, hi)
    assert torch.equal(big, before), "the margin around the frame changed"


# ---- cvgs_execute_many, CircularTensor ------------------------------------------------------------------------------------------------
def test_execute_many_runs_such_chains_and_circular_update_refuses(device, lib):
    torch = _torch()
    dsize = (16, 8)
    tmpl, pts, count = _e2e_items(dsize)
    s = torch.cuda.current_stream()
    cams = []
    for k in range(2):
        frame = Frame(device, seed=90 + k)
        pt = torch.from_numpy(np.ascontiguousarray(pts[::-1]) if k else pts).to(device)
        table = torch.zeros((N, 64), dtype=torch.uint8, device=device)
        outs = [torch.full((N, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device) for _ in range(2)]
        cams.append(dict(frame=frame, pt=pt, table=table, outs=outs, desc=cvgs.warp_table_desc(frame.mat, pt, table, N, dsize, tmpl)))
    cvgs.warp_tables_from_points(s, [cam["desc"] for cam in cams])
    low = [cvgs.lower(_chain(cvgs.warp_table(cvgs.WARP_AFFINE, cam["frame"].mat, cam["table"], N, dsize), 3, cam["outs"][0].data_ptr(), dsize)) for cam in cams]
    capi.check(lib.cvgs_execute_many(cvgs.pack_chains(low), 2, cvgs.stream_handle(s)))
    for cam in cams:
        cvgs.executeOperations(s, *_chain(cvgs.warp_table(cvgs.WARP_AFFINE, cam["frame"].mat, cam["table"], N, dsize), 3, cam["outs"][1].data_ptr(), dsize))
    torch.cuda.synchronize()
    for k, cam in enumerate(cams):
        assert torch.equal(cam["outs"][0], cam["outs"][1]) and not (cam["outs"][0] == -5.0).any(), "chain %d" % k
    assert not torch.equal(cams[0]["outs"][0], cams[1]["outs"][0])
    # CircularTensor::update refuses a warp over a device table before anything is enqueued
    ct = cvgs.CircularTensor(cvgs.CV_8UC3, cvgs.CV_32FC1, 3, 4, cvgs.NewestFirst, width=dsize[0], height=dsize[1])
    try:
        rd = cvgs.warp_table(cvgs.WARP_AFFINE, cams[0]["frame"].mat, cams[0]["table"], 1, dsize)
        with pytest.raises(capi.CvgsError) as e:
            ct.update(s, rd, ct.write_split(cvgs.CV_32FC3))
        assert e.value.code == capi.ERR_UNSUPPORTED and "device table" in str(e.value)
        assert ct.updates() == 0
    finally:
        ct.release()
