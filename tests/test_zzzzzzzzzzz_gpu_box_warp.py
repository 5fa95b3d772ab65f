"""cvgs_warp_tables_from_boxes on the GPU: the device-built table, boxes_out and valid_out against cvgs_warp_table_from_boxes_host byte for
byte (guard entries around every buffer), pixels through chains over the table against host-described warp chains with the same matrices
and against the plain pixel crop, three such chains fused into one warp tick, the whole path inside one linear HIP graph, and boxes_out fed
to cvgs_plane_tables_from_boxes.

The frames are tiny (13 x 9, and 97 x 61 for the byte comparisons, where the frame is never read).  Every read these tests cause lies inside
the frame: the warp kernels test 0 <= sx < w && 0 <= sy < h before any tap, and data / w / h / step of every table entry are the
host-validated frame's -- which the byte comparison with the host entry pins for every entry written here.

Collected behind every other module of the suite, so that it takes no existing item's place in its order."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import box_cases as B
from tests import box_warp_cases as K
from tests import helpers as H
from tests import test_zzzz_gpu_area_tick as T

pytestmark = pytest.mark.gpu

ENTRY = np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")])
CFG = (K.EXPAND, (192, 256), (1.25, 1.25), (3.5, 3.5))
FW, FH = 13, 9


def _torch():
    import torch
    return torch


class Frame:
    def __init__(self, device, w=K.W, h=K.H, step=K.STEP, seed=1):
        torch = _torch()
        self.host = H.random_u8((h, step), seed=seed)
        self.t = torch.from_numpy(self.host).to(device)
        self.w, self.h, self.step = w, h, step
        self.mat = cvgs.GpuMat(h, w, cvgs.CV_8UC3, self.t.data_ptr(), step, owner=self.t)
        self.pixels = self.host[:, :w * 3].reshape(h, w, 3)


def _mix(n):
    """n boxes drawn evenly from every family of the case set (valid, outside, ties, degenerate, non-finite, huge)."""
    boxes = K.all_boxes()
    return np.ascontiguousarray(boxes[np.linspace(0, len(boxes) - 1, n).astype(int)] if n > 1 else boxes[:1])


def _host_build(frame, boxes, count, shape, dsize, scale, pad):
    d = cvgs.box_warp_desc(frame.mat, 4096, 8192, len(boxes), dsize, shape, scale, pad)
    raw, bo, vo = cvgs.warp_table_from_boxes_host(d, boxes, count)
    return np.frombuffer(raw, np.uint8).reshape(len(boxes), 64), bo.view(np.uint32), vo


class Buffers:
    """table / boxes_out / valid_out of n items with one guard entry on either side of each."""

    def __init__(self, device, n):
        torch = _torch()
        self.n = n
        self.t = torch.full((n + 2, 64), 0xA5, dtype=torch.uint8, device=device)
        self.b = torch.full((n + 2, 4), -123.25, dtype=torch.float32, device=device)
        self.v = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=device)

    def desc(self, frame, boxes_t, count_t, shape, dsize, scale, pad):
        return cvgs.box_warp_desc(frame.mat, boxes_t, self.t[1:], self.n, dsize, shape, scale, pad, count=count_t, boxes_out=self.b[1:], valid=self.v[1:])

    def fetch(self):
        """After a synchronise: the guards are intact; (table bytes [n, 64], boxes_out bits [n, 4], valid [n])."""
        t, b, v = self.t.cpu().numpy(), self.b.cpu().numpy(), self.v.cpu().numpy()
        assert (t[0] == 0xA5).all() and (t[-1] == 0xA5).all(), "a guard entry of the table changed"
        assert (b[0] == -123.25).all() and (b[-1] == -123.25).all(), "a guard entry of boxes_out changed"
        assert v[0] == 0x5A5A5A5A and v[-1] == 0x5A5A5A5A, "a guard entry of valid_out changed"
        return t[1:-1], b[1:-1].view(np.uint32), v[1:-1]


def _device_build(device, frame, boxes, count, shape, dsize, scale, pad):
    torch = _torch()
    bt = torch.from_numpy(np.ascontiguousarray(boxes)).to(device)
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
    buf = Buffers(device, len(boxes))
    cvgs.warp_tables_from_boxes(torch.cuda.current_stream(), [buf.desc(frame, bt, ct, shape, dsize, scale, pad)])
    torch.cuda.synchronize()
    return buf.fetch()


def _same(got, want, boxes, what):
    for name, g, w in zip(("table", "boxes_out", "valid_out"), got, want):
        g2, w2 = g.reshape(len(boxes), -1), w.reshape(len(boxes), -1)
        bad = np.flatnonzero((g2 != w2).any(axis=1))
        assert bad.size == 0, "%s, %s: %d items differ, first %d: box %s\n got  %s\n want %s" % (
            what, name, bad.size, bad[0], boxes[bad[0]].tolist(), g2[bad[0]].tobytes().hex(), w2[bad[0]].tobytes().hex())


# ---- device bytes against host bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_device_bytes_equal_host_bytes(device, lib, n):
    """max_items below, at and above the workgroup size and in three workgroups, every count case: table, boxes_out and valid_out equal the
    host entry's bytes and the guard entries stay intact."""
    frame = Frame(device)
    boxes = _mix(n)
    for label, count in K.counts(n):
        _same(_device_build(device, frame, boxes, count, *CFG), _host_build(frame, boxes, count, *CFG), boxes, "n %d, count %s" % (n, label))


def test_device_bytes_equal_host_bytes_on_every_configuration(device, lib):
    """The whole case set (about 440 boxes) under both shapes, the four targets, both scales and both pads."""
    frame = Frame(device)
    boxes = K.all_boxes()
    for shape, dsize, scale, pad in K.configs():
        _same(_device_build(device, frame, boxes, None, shape, dsize, scale, pad), _host_build(frame, boxes, None, shape, dsize, scale, pad), boxes,
              "shape %d, target %s, scale %s, pad %s" % (shape, dsize, scale, pad))


def test_sixteen_frames_of_differing_sizes_in_one_call(device, lib):
    """One call, 16 frames, max_items from 1 to 130: the launch is as wide as the largest frame, so the lanes beyond a smaller frame's own
    items must return before they touch anything -- every frame's bytes equal the host's, every guard is intact."""
    torch = _torch()
    sizes = [130, 1, 63, 64, 65, 2, 100, 7, 128, 129, 33, 1, 64, 5, 90, 66]
    cfgs = K.configs()
    jobs, descs, keep = [], [], []
    for k, n in enumerate(sizes):
        frame = Frame(device, seed=20 + k)
        boxes = _mix(n) if k % 2 == 0 else _mix(n)[::-1].copy()
        count = (None, n // 2, n + 3, 0)[k % 4]
        shape, dsize, scale, pad = cfgs[(5 * k) % len(cfgs)]
        bt = torch.from_numpy(boxes).to(device)
        ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
        buf = Buffers(device, n)
        descs.append(buf.desc(frame, bt, ct, shape, dsize, scale, pad))
        jobs.append((buf, frame, boxes, count, shape, dsize, scale, pad))
        keep += [bt, ct]
    cvgs.warp_tables_from_boxes(torch.cuda.current_stream(), descs)
    torch.cuda.synchronize()
    for k, (buf, frame, boxes, count, shape, dsize, scale, pad) in enumerate(jobs):
        _same(buf.fetch(), _host_build(frame, boxes, count, shape, dsize, scale, pad), boxes, "frame %d (%d items)" % (k, len(boxes)))


def test_optional_outputs_may_be_absent(device, lib):
    torch = _torch()
    frame = Frame(device)
    boxes = _mix(65)
    bt = torch.from_numpy(boxes).to(device)
    table = torch.full((67, 64), 0xA5, dtype=torch.uint8, device=device)
    cvgs.warp_tables_from_boxes(torch.cuda.current_stream(), [cvgs.box_warp_desc(frame.mat, bt, table[1:], 65, CFG[1], CFG[0], CFG[2], CFG[3])])
    torch.cuda.synchronize()
    t = table.cpu().numpy()
    assert (t[0] == 0xA5).all() and (t[-1] == 0xA5).all() and (t[1:-1] == _host_build(frame, boxes, None, *CFG)[0]).all()


# ---- pixels -----------------------------------------------------------------------------------------------------------------------------
PIXEL_BOXES = np.array([(2, 1, 10, 7), (-3, -2, 5, 4), (8.5, 4.25, 16, 12), (-2, -2, 15, 11), (5.5, 3.5, 6.5, 4.5), (10, 0, 13.5, 9), (20, 3, 30, 6), (np.nan, 1, 4, 4),
                        (4, 4, 4, 8)], np.float32)


def _program_chain(rd, out_ptr, dsize, n):
    f = cvgs.CV_32FC3
    return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [H.K1_ALPHA] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
            cvgs.split_tensor(f, out_ptr, dsize[0], dsize[1], n)]


def _host_described(frame, table_rows, dsize):
    n = len(table_rows)
    rd = cvgs.ReadIOp(capi.READ_WARP_AFFINE, cvgs.CV_8UC3, [frame.mat] * n, None, dsize, cvgs.IGNORE_AR, None)
    rd.warp, rd.warp_sizes = [float(v) for v in np.frombuffer(table_rows.tobytes(), ENTRY)["m"].reshape(-1)], None
    return rd


@pytest.mark.parametrize("flags,name", [(0, "warp_affine_u8c3_swap_mul_sub_div"), (capi.CHAIN_FORCE_GENERIC, "warp_affine_interp")], ids=["fast", "interpreted"])
@pytest.mark.parametrize("dsize", [(8, 6), (5, 7)], ids=["8x6", "5x7"])
def test_pixels_equal_the_host_described_warp(device, lib, dsize, flags, name):
    """A 13 x 9 frame, boxes inside, partly outside, wholly outside and invalid: the chain over the device-built table equals the
    host-described warp chain over the same nine floats per plane, bit for bit; planes that see nothing of the frame are all alike."""
    torch = _torch()
    frame = Frame(device, FW, FH, FW * 3 + 5, seed=3)
    n = len(PIXEL_BOXES)
    s = torch.cuda.current_stream()
    bt = torch.from_numpy(PIXEL_BOXES).to(device)
    table = torch.zeros((n, 64), dtype=torch.uint8, device=device)
    valid = torch.zeros((n,), dtype=torch.int32, device=device)
    cvgs.warp_tables_from_boxes(s, [cvgs.box_warp_desc(frame.mat, bt, table, n, dsize, cvgs.BOX_SHAPE_EXPAND, (1.25, 1.25), (0.0, 0.0), valid=valid)])
    out = torch.full((n, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device)
    ops = _program_chain(cvgs.warp_table(cvgs.WARP_AFFINE, frame.mat, table, n, dsize), out.data_ptr(), dsize, n)
    assert cvgs.kernel_name(*ops, flags=flags) == name
    cvgs.executeOperations(s, *ops, flags=flags)
    torch.cuda.synchronize()
    rows = table.cpu().numpy()
    assert (rows == _host_build(frame, PIXEL_BOXES, None, cvgs.BOX_SHAPE_EXPAND, dsize, (1.25, 1.25), (0.0, 0.0))[0]).all()
    assert valid.cpu().tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0]
    want = torch.full((n, 3, dsize[1], dsize[0]), -6.0, dtype=torch.float32, device=device)
    host_ops = _program_chain(_host_described(frame, rows, dsize), want.data_ptr(), dsize, n)
    assert cvgs.kernel_name(*host_ops, flags=flags) == name
    cvgs.executeOperations(s, *host_ops, flags=flags)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "%d values differ from the host-described chain" % int((out != want).sum())
    planes = out.cpu().numpy().reshape(n, -1)
    for i in range(n):  # box 6 lies wholly outside the frame, 7 and 8 are invalid: 0 through the program, all alike; the others see pixels
        assert (planes[i] == planes[7]).all() == (i >= 6), i


@pytest.mark.parametrize("box", [(2, 1, 10, 7), (-3, -2, 5, 4), (8, 4, 16, 12), (-2, -2, 15, 11), (13, 2, 20, 6)],
                         ids=["inside", "top-left", "bottom-right", "larger", "outside-right"])
def test_integer_box_is_the_pixel_crop_with_a_zero_border(device, lib, box):
    """Integer edges, scale 1, pad 0, STRETCH, target = the box's size: the warp is the plain pixel crop, 0 outside the frame."""
    torch = _torch()
    frame = Frame(device, FW, FH, FW * 3 + 5, seed=3)
    xa, ya, xb, yb = box
    w, h = xb - xa, yb - ya
    s = torch.cuda.current_stream()
    bt = torch.tensor([box], dtype=torch.float32, device=device)
    table = torch.zeros((1, 64), dtype=torch.uint8, device=device)
    cvgs.warp_tables_from_boxes(s, [cvgs.box_warp_desc(frame.mat, bt, table, 1, (w, h), cvgs.BOX_SHAPE_STRETCH, (1.0, 1.0), (0.0, 0.0))])
    out = torch.full((1, 3, h, w), -5.0, dtype=torch.float32, device=device)
    cvgs.executeOperations(s, cvgs.warp_table(cvgs.WARP_AFFINE, frame.mat, table, 1, (w, h)), cvgs.split_tensor(cvgs.CV_32FC3, out.data_ptr(), w, h, 1))
    torch.cuda.synchronize()
    want = np.zeros((h, w, 3), np.float32)
    for v in range(h):
        for u in range(w):
            if 0 <= ya + v < FH and 0 <= xa + u < FW:
                want[v, u] = frame.pixels[ya + v, xa + u]
    assert (out.cpu().numpy()[0] == want.transpose(2, 0, 1)).all()


# ---- fusion -----------------------------------------------------------------------------------------------------------------------------
def _three_cameras(device, dsize, n):
    """Three frames, their boxes and tables (ONE cvgs_warp_tables_from_boxes call), and per camera two output tensors."""
    torch = _torch()
    cams = []
    for k in range(3):
        frame = Frame(device, FW, FH, FW * 3 + 5, seed=60 + k)
        boxes = np.ascontiguousarray(np.roll(PIXEL_BOXES, k, axis=0)[:n] + np.float32(0.25 * k))
        bt = torch.from_numpy(boxes).to(device)
        table = torch.zeros((n, 64), dtype=torch.uint8, device=device)
        outs = [torch.full((n, 3, dsize[1], dsize[0]), -5.0, dtype=torch.float32, device=device) for _ in range(2)]
        cams.append(dict(frame=frame, boxes=boxes, bt=bt, table=table, outs=outs,
                         desc=cvgs.box_warp_desc(frame.mat, bt, table, n, dsize, cvgs.BOX_SHAPE_EXPAND, (1.25, 1.25), (0.0, 0.0))))
    return cams


def _lower(cam, which, dsize, n):
    return cvgs.lower(_program_chain(cvgs.warp_table(cvgs.WARP_AFFINE, cam["frame"].mat, cam["table"], n, dsize), cam["outs"][which].data_ptr(), dsize, n))


def test_three_chains_over_tables_of_one_call_fuse_into_one_warp_tick(device, lib):
    torch = _torch()
    dsize, n = (8, 6), 8
    cams = _three_cameras(device, dsize, n)
    cvgs.warp_tables_from_boxes(torch.cuda.current_stream(), [c["desc"] for c in cams])
    torch.cuda.synchronize()
    low = [_lower(c, 0, dsize, n) for c in cams]
    nodes, note = T._nodes(lib, low, device)
    assert nodes == 1 and note.startswith("tick:"), (nodes, note)
    note = T._execute_many(lib, low)
    assert note.startswith("tick:"), note
    T._execute_each(lib, [_lower(c, 1, dsize, n) for c in cams])
    torch.cuda.synchronize()
    for k, c in enumerate(cams):
        assert torch.equal(c["outs"][0].view(torch.int32), c["outs"][1].view(torch.int32)) and not (c["outs"][0] == -5.0).any(), "chain %d" % k
    assert not torch.equal(cams[0]["outs"][0], cams[1]["outs"][0])


# ---- no host in the loop ----------------------------------------------------------------------------------------------------------------
def test_boxes_to_tick_as_one_linear_graph(device, lib):
    """Device copies writing boxes and count -> cvgs_warp_tables_from_boxes -> the warp tick, captured on ONE stream and replayed twice
    with different device-side boxes and counts: each replay equals the eager host-described result."""
    torch = _torch()
    dsize, n = (5, 7), 8
    cams = _three_cameras(device, dsize, n)
    rounds = [[(c["boxes"], n - 2 - k) for k, c in enumerate(cams)], [(np.ascontiguousarray(c["boxes"][::-1]) + np.float32(1.5), n + 4) for c in cams]]
    src_b = [torch.zeros((n, 4), dtype=torch.float32, device=device) for _ in cams]
    src_c = [torch.zeros((1,), dtype=torch.int32, device=device) for _ in cams]
    cnt = [torch.zeros((1,), dtype=torch.int32, device=device) for _ in cams]
    staged = [[(torch.from_numpy(b).to(device), torch.tensor([c], dtype=torch.int32, device=device)) for b, c in r] for r in rounds]
    descs = [cvgs.box_warp_desc(c["frame"].mat, c["bt"], c["table"], n, dsize, cvgs.BOX_SHAPE_EXPAND, (1.25, 1.25), (0.0, 0.0), count=cnt[k]) for k, c in enumerate(cams)]
    low = [_lower(c, 0, dsize, n) for c in cams]
    tick = cvgs.pack_chains(low)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        for k, c in enumerate(cams):
            c["bt"].copy_(src_b[k])
            cnt[k].copy_(src_c[k])
        cvgs.warp_tables_from_boxes(s, descs)
        capi.check(lib.cvgs_execute_many(tick, len(low), cvgs.stream_handle(s)))
    torch.cuda.synchronize()
    assert all((c["outs"][0] == -5.0).all() and (c["table"] == 0).all() for c in cams), "capture itself must not run anything"
    results = []
    for r, items in enumerate(rounds):
        for k in range(len(cams)):  # device copies only
            src_b[k].copy_(staged[r][k][0])
            src_c[k].copy_(staged[r][k][1])
        g.replay()
        torch.cuda.synchronize()
        for k, (c, (boxes, count)) in enumerate(zip(cams, items)):
            rows = _host_build(c["frame"], boxes, count, cvgs.BOX_SHAPE_EXPAND, dsize, (1.25, 1.25), (0.0, 0.0))[0]
            want = torch.full((n, 3, dsize[1], dsize[0]), -6.0, dtype=torch.float32, device=device)
            cvgs.executeOperations(torch.cuda.current_stream(), *_program_chain(_host_described(c["frame"], rows, dsize), want.data_ptr(), dsize, n))
            torch.cuda.synchronize()
            assert torch.equal(c["outs"][0].view(torch.int32), want.view(torch.int32)), "replay %d, chain %d" % (r, k)
        results.append(cams[0]["outs"][0].clone())
    assert not torch.equal(results[0], results[1])


# ---- boxes_out as the boxes of the crop builder -------------------------------------------------------------------------------------------
def test_boxes_out_feeds_the_crop_builder(device, lib):
    """boxes_out of one call as the XYXY_F32 boxes of cvgs_plane_tables_from_boxes on the same stream: rects_out equals the box rule's
    model (tests/box_cases.py) of the host entry's boxes_out -- a view with the margin for a valid item that meets the frame, the invalid
    view for (0, 0, 0, 0)."""
    torch = _torch()
    frame = Frame(device)
    boxes = K.all_boxes()
    n = len(boxes)
    s = torch.cuda.current_stream()
    bt = torch.from_numpy(boxes).to(device)
    buf = Buffers(device, n)
    cvgs.warp_tables_from_boxes(s, [buf.desc(frame, bt, None, *CFG)])
    ptab = torch.zeros((n, 48), dtype=torch.uint8, device=device)
    rects = torch.full((n, 4), -9, dtype=torch.int32, device=device)
    cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(frame.mat, buf.b[1:], ptab, n, (64, 128), rects=rects)])
    torch.cuda.synchronize()
    _, bo, vo = cvgs.warp_table_from_boxes_host(cvgs.box_warp_desc(frame.mat, 4096, 8192, n, CFG[1], CFG[0], CFG[2], CFG[3]), boxes)
    want = [r if r is not None else B.INVALID_RECT for r in B.rects(bo, B.XYXY_F32, K.W, K.H)]
    got = [tuple(int(x) for x in r) for r in rects.cpu().numpy()]
    assert got == [tuple(w) for w in want]
    assert all(g == B.INVALID_RECT for g, ok in zip(got, vo) if not ok) and sum(1 for g in got if g != B.INVALID_RECT) > 150  # (many views, not a list of invalid ones)


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_program_passes():
    """tests/cpp/test_box_warps.cpp: cvGS::DeviceWarps::updateFromBoxes against the host twin's bytes and host-described warps, a ChainBatch
    tick and recorded ticks over three cameras."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cpp = os.path.join(root, "tests", "cpp")
    exe = os.path.join(cpp, "bin", "test_box_warps")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", os.path.join(root, "oracle")], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", cpp, "bin/test_box_warps"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_box_warps passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
