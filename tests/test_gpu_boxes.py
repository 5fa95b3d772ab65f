"""cvgs_plane_tables_from_boxes on the GPU: the device-built plane table against the host builder byte for byte, chains over it against
chains over host views bit for bit, the whole detector -> crops step inside one linear HIP graph, and bounds.

The box rule comes from tests/box_cases.py (an independent integer / float32 model); the expected table of a valid box is what
cvgs_plane_table_build writes for the model's view, the expected table of an invalid box is the documented entry (include/cvgs_hip_ext.h):
the frame's own data / width / height / step / chroma offset, fx = fy = 1, the empty window (0, 0, -1, -1)."""
import ctypes as C
import struct

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import box_cases as B
from tests import helpers as H

pytestmark = pytest.mark.gpu

ARS = (cvgs.IGNORE_AR, cvgs.PRESERVE_AR, cvgs.PRESERVE_AR_RN_EVEN, cvgs.PRESERVE_AR_LEFT)
TARGETS = ((64, 128), (7, 5), (300, 17))
COUNTS = (None, 0, 1, "max-1", "max", "max+5", -3)
YUV = (capi.YUV_FULL, capi.BT709, 0)


def _torch():
    import torch
    return torch


class Frame:
    """A frame inside a device allocation: `mat` is the whole-frame GpuMat, view(rect) the host-style view of a model rectangle."""

    def __init__(self, device, W, Hh, cv_type, step, nv12=False, seed=1, low=False):
        torch = _torch()
        self.W, self.H, self.cv_type, self.step, self.nv12 = W, Hh, cv_type, step, nv12
        rows = Hh * 3 // 2 if nv12 else Hh
        host = H.random_u8((rows, step), seed=seed)
        if low:
            host &= 0x7f
        self.host = host
        self.t = torch.from_numpy(host).to(device)
        self.mat = cvgs.GpuMat(Hh, W, cv_type, self.t.data_ptr(), step, owner=self.t)

    def view(self, r):
        l, t, w, h = r
        return self.mat.nv12_roi(l, t, w, h) if self.nv12 else self.mat.roi(l, t, w, h)

    def invalid_entry(self):
        uv = self.H * self.step if self.nv12 else 0
        return struct.pack("<Q3i2f5i", self.mat.data, self.W, self.H, self.step, 1.0, 1.0, 0, 0, -1, -1, uv)

    def read_kind(self):
        return capi.READ_NV12_RESIZE_LINEAR if self.nv12 else capi.READ_RESIZE_LINEAR

    def host_read(self, views, dsize, ar, background=None, used=None, layout=capi.YUV_NV12):
        rd = cvgs.ReadIOp(self.read_kind(), self.cv_type, views, len(views) if used is None else used, dsize, ar, background, YUV if self.nv12 else None)
        rd.yuv_layout = layout if self.nv12 else 0
        return rd


def _expected_tables(frame, model_rects, dsize, ar):
    """uint8 [n, 48]: cvgs_plane_table_build on the model's views for the valid boxes, the documented entry for the others."""
    valid = [i for i, r in enumerate(model_rects) if r]
    out = np.tile(np.frombuffer(frame.invalid_entry(), np.uint8), (len(model_rects), 1))
    if valid:
        raw = cvgs.build_plane_table(frame.host_read([frame.view(model_rects[i]) for i in valid], dsize, ar))
        out[valid] = np.frombuffer(raw, np.uint8).reshape(len(valid), 48)
    return out


def _resolve(count, n):
    return {None: None, "max-1": n - 1, "max": n, "max+5": n + 5}.get(count, count)


def _device_build(device, frame, boxes, fmt, dsize, ar, count=None, layout=capi.YUV_NV12, stream=None):
    """(table bytes [n, 48], rects [n, 4]) written by ONE cvgs_plane_tables_from_boxes call for one frame."""
    torch = _torch()
    n = len(boxes)
    bt = torch.from_numpy(np.ascontiguousarray(boxes)).to(device)
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
    table = torch.full((n, 48), 0xCD, dtype=torch.uint8, device=device)
    rects = torch.full((n, 4), -77, dtype=torch.int32, device=device)
    d = cvgs.box_table_desc(frame.mat, bt, table, n, dsize, ar, fmt, ct, rects, frame.read_kind(), layout)
    cvgs.plane_tables_from_boxes(stream if stream is not None else torch.cuda.current_stream(), [d])
    torch.cuda.synchronize()
    return table.cpu().numpy(), rects.cpu().numpy()


def _rects_array(model_rects):
    return np.array([r if r else B.INVALID_RECT for r in model_rects], np.int32).reshape(-1, 4)


FRAMES = {  # name -> (W, H, type, step, nv12)
    "8UC3": (B.W0, B.H0, cvgs.CV_8UC3, 800, False),
    "16UC4": (B.W0, B.H0, cvgs.CV_16UC4, B.W0 * 8 + 24, False),
    "32FC1": (B.W0, B.H0, cvgs.CV_32FC1, B.W0 * 4 + 12, False),
    "NV12": (B.WY, B.HY, cvgs.CV_8UC1, 136, True),
}


def _boxes_for(name, fmt):
    W, Hh = FRAMES[name][0], FRAMES[name][1]
    arr = B.covering_boxes(fmt, W, Hh)
    if FRAMES[name][4]:
        arr = np.concatenate([arr, B.boxes_array([b for b, _ in (B.PINNED_420_XYXY if fmt == B.XYXY_F32 else B.PINNED_420_XYWH)], fmt)])
    return arr


@pytest.mark.parametrize("fmt", [B.XYXY_F32, B.XYWH_I32], ids=["xyxy_f32", "xywh_i32"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_table_bytes(device, lib, name, fmt):
    """About 2,000 boxes (every width and height of the frame, clipped / invalid / pinned edge cases), three targets, four aspect-ratio
    modes, seven counts: the device-built table equals the host-built one byte for byte, rects_out equals the model."""
    W, Hh, cv_type, step, nv12 = FRAMES[name]
    frame = Frame(device, W, Hh, cv_type, step, nv12)
    boxes = _boxes_for(name, fmt)
    n = len(boxes)
    all_rects = B.rects(boxes, fmt, W, Hh, None, nv12)
    assert sum(1 for r in all_rects if r) > 800 and sum(1 for r in all_rects if not r) > 100
    inv = np.frombuffer(frame.invalid_entry(), np.uint8)
    checked = 0
    for dsize in TARGETS:
        for ar in ARS:
            want_all = _expected_tables(frame, all_rects, dsize, ar)
            for count in COUNTS:
                cnt = _resolve(count, n)
                model = B.apply_count(all_rects, cnt)
                live = np.array([r is not None for r in model])
                want = np.where(live[:, None], want_all, inv[None, :])
                got, got_rects = _device_build(device, frame, boxes, fmt, dsize, ar, cnt)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, "%s fmt %d dsize %s ar %d count %s: %d entries differ, first %d: box %s model %s\n got  %s\n want %s" % (
                    name, fmt, dsize, ar, count, bad.size, bad[0], boxes[bad[0]], model[bad[0]], got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())
                assert (got_rects == _rects_array(model)).all(), (name, fmt, dsize, ar, count)
                checked += 1
    assert checked == len(TARGETS) * len(ARS) * len(COUNTS)


def test_pinned_cases_on_the_device(device, lib):
    """The hand-pinned rectangles themselves (not only the model that agrees with them) against rects_out."""
    for fmt, cases, name in ((B.XYXY_F32, B.PINNED_XYXY, "8UC3"), (B.XYWH_I32, B.PINNED_XYWH, "8UC3"), (B.XYXY_F32, B.PINNED_420_XYXY, "NV12"),
                             (B.XYWH_I32, B.PINNED_420_XYWH, "NV12")):
        W, Hh, cv_type, step, nv12 = FRAMES[name]
        frame = Frame(device, W, Hh, cv_type, step, nv12)
        _tab, got = _device_build(device, frame, B.boxes_array([b for b, _ in cases], fmt), fmt, (64, 128), cvgs.IGNORE_AR)
        assert got.tolist() == [list(r if r else B.INVALID_RECT) for _, r in cases]


@pytest.mark.parametrize("n_frames", [2, 17], ids=["two_frames", "seventeen_frames"])
def test_several_frames_in_one_call_equal_single_calls(device, lib, n_frames):
    """n descriptors in ONE launch (grid y = frame; 17 frames take the larger argument block) write the bytes of n single calls; the frames
    differ in type, size, box format, target, aspect-ratio mode, number of boxes and count."""
    torch = _torch()
    names = list(FRAMES)
    jobs = []
    for k in range(n_frames):
        name = names[k % len(names)]
        fmt = (B.XYXY_F32, B.XYWH_I32)[(k // 2) % 2]
        W, Hh, cv_type, step, nv12 = FRAMES[name]
        frame = Frame(device, W, Hh, cv_type, step, nv12, seed=50 + k)
        boxes = _boxes_for(name, fmt)[:: (1 if k == 0 else 9 + k)]  # ~2,000 boxes for the first frame, 70-200 for the others
        count = (None, len(boxes) // 2, len(boxes) + 3)[k % 3]
        jobs.append((frame, boxes, fmt, TARGETS[k % 3], ARS[k % 4], count))
    single = [_device_build(device, f, b, fmt, ds, ar, cnt) for f, b, fmt, ds, ar, cnt in jobs]
    descs, outs, keep = [], [], []
    for f, b, fmt, ds, ar, cnt in jobs:
        bt = torch.from_numpy(np.ascontiguousarray(b)).to(device)
        ct = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device=device)
        table = torch.full((len(b), 48), 0xCD, dtype=torch.uint8, device=device)
        rects = torch.full((len(b), 4), -77, dtype=torch.int32, device=device)
        descs.append(cvgs.box_table_desc(f.mat, bt, table, len(b), ds, ar, fmt, ct, rects, f.read_kind()))
        outs.append((table, rects))
        keep += [bt, ct]
    cvgs.plane_tables_from_boxes(torch.cuda.current_stream(), descs)
    torch.cuda.synchronize()
    for k, ((table, rects), (want_t, want_r)) in enumerate(zip(outs, single)):
        assert (table.cpu().numpy() == want_t).all() and (rects.cpu().numpy() == want_r).all(), "frame %d of %d" % (k, n_frames)
        assert not (want_t == 0xCD).all(axis=1).any()  # every entry was written


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _chain(rd, cn, out_t, dsize, out="f32"):
    f_type = cvgs.make_type(cvgs.CV_32F, cn)
    ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f_type), cvgs.multiply(f_type, [H.K1_ALPHA] * cn),
           cvgs.subtract(f_type, H.K1_SUB[cn]), cvgs.divide(f_type, H.K1_DIV[cn])]
    o_type = f_type
    if out != "f32":
        o_type = cvgs.make_type(cvgs.CV_16F, cn) | (capi.TYPE_FLAG_BF16 if out == "bf16" else 0)
        ops.append(cvgs.convertTo(f_type, o_type))
    ops.append(cvgs.split_tensor(o_type, out_t.data_ptr(), dsize[0], dsize[1], out_t.shape[0], keep=out_t))
    return ops


def _out_tensor(device, n, cn, dsize, out="f32"):
    torch = _torch()
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[out]
    return torch.full((n, cn, dsize[1], dsize[0]), -5.0, dtype=dt, device=device)


E2E_BOXES_XYWH = [(5, 5, 40, 30), (0, 0, 97, 61), (90, 50, 30, 30), (-10, -10, 30, 30), (50, 20, 0, 10), (96, 60, 1, 1), (97, 10, 5, 5), (10, 10, 3, 2),
                  (20, 61, 5, 5), (30, 30, 20, 25), (-50, 5, 20, 20), (60, 0, 37, 61), (1, 1, 1, 1), (40, 40, -3, 5), (12, 7, 64, 50), (70, 5, 20, 40),
                  (0, 30, 97, 1), (33, 0, 1, 61), (200, 200, 5, 5), (80, 40, 100, 100), (3, 3, 90, 55), (45, 22, 8, 16), (10, 50, 5, -1), (25, 25, 50, 30)]


def _e2e(device, lib, cv_type, cn, dsize, out="f32", flags=0, ar=cvgs.IGNORE_AR, background=None, nv12=False, layout=capi.YUV_NV12, fmt=B.XYWH_I32):
    """One chain over the device-built table against host-described chains over the model's rectangles; returns the kernel's name."""
    torch = _torch()
    W, Hh = (B.WY, B.HY) if nv12 else (97, 61)
    esz = cvgs.elem_size(cv_type)
    frame = Frame(device, W, Hh, cv_type, (W * esz + 15) // 8 * 8, nv12, seed=7)
    boxes = B.boxes_array(E2E_BOXES_XYWH, B.XYWH_I32)
    if fmt == B.XYXY_F32:
        boxes = np.array([(x + 0.25, y + 0.5, x + w - 0.25, y + h - 0.5) for x, y, w, h in E2E_BOXES_XYWH], np.float32)
    n = len(boxes)
    model = B.rects(boxes, fmt, W, Hh, None, nv12)
    n_inv = sum(1 for r in model if not r)
    n_clipped = sum(1 for r, b in zip(model, E2E_BOXES_XYWH) if r and r != tuple(b))  # (fractional edges grow outwards: clipped or not, they differ)
    assert n == 24 and n_inv >= 4 and n_inv + n_clipped >= 8  # a third of the boxes invalid or clipped
    s = torch.cuda.current_stream()
    bt = torch.from_numpy(boxes).to(device)
    table = torch.zeros((n, 48), dtype=torch.uint8, device=device)
    cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(frame.mat, bt, table, n, dsize, ar, fmt, None, None, frame.read_kind(), layout)])
    out_dev = _out_tensor(device, n, cn, dsize, out)
    rd = cvgs.resize_boxes(frame.mat, table, n, dsize, background, ar, YUV if nv12 else None, layout)
    ops = _chain(rd, cn, out_dev, dsize, out)
    name = cvgs.kernel_name(*ops, flags=flags)
    cvgs.executeOperations(s, *ops, flags=flags)
    # host-described: the valid views in one chain, and ONE default plane (used_planes = 0) for every invalid box
    valid = [i for i, r in enumerate(model) if r]
    out_valid = _out_tensor(device, len(valid), cn, dsize, out)
    cvgs.executeOperations(s, *_chain(frame.host_read([frame.view(model[i]) for i in valid], dsize, ar, background, layout=layout), cn, out_valid, dsize, out), flags=flags)
    out_bg = _out_tensor(device, 1, cn, dsize, out)
    cvgs.executeOperations(s, *_chain(frame.host_read([frame.mat], dsize, ar, background, used=0, layout=layout), cn, out_bg, dsize, out), flags=flags)
    torch.cuda.synchronize()
    assert not torch.isnan(out_dev.float()).any()
    for j, i in enumerate(valid):
        assert torch.equal(out_dev[i], out_valid[j]), "plane %d (box %s, rect %s) differs from the host-described crop [%s]" % (i, boxes[i], model[i], name)
    for i in range(n):
        if not model[i]:
            assert torch.equal(out_dev[i], out_bg[0]), "invalid plane %d (box %s) is not the default plane [%s]" % (i, boxes[i], name)
    assert not torch.equal(out_valid[0], out_bg[0])
    return name


@pytest.mark.parametrize("dsize", [(16, 8), (64, 128)], ids=["16x8", "64x128"])
@pytest.mark.parametrize("fmt", [B.XYWH_I32, B.XYXY_F32], ids=["xywh_i32", "xyxy_f32"])
def test_end_to_end_u8c3(device, lib, dsize, fmt):
    assert _e2e(device, lib, cvgs.CV_8UC3, 3, dsize, fmt=fmt) == "k1_u8c3_swap_mul_sub_div"


@pytest.mark.parametrize("dsize", [(16, 8), (64, 128)], ids=["16x8", "64x128"])
@pytest.mark.parametrize("case", ["8UC4", "16UC3", "f16", "bf16", "generic", "preserve_ar_bg"])
def test_end_to_end_variants(device, lib, case, dsize):
    if case == "8UC4":
        name = _e2e(device, lib, cvgs.CV_8UC4, 4, dsize)
        assert name.startswith("k1_u8c4"), name
    elif case == "16UC3":
        name = _e2e(device, lib, cvgs.CV_16UC3, 3, dsize)
        assert name.startswith("k1_"), name
    elif case in ("f16", "bf16"):
        name = _e2e(device, lib, cvgs.CV_8UC3, 3, dsize, out=case)
        assert name.startswith("k1_u8c3") and case in name and ("bf16" in name) == (case == "bf16"), name
    elif case == "generic":
        assert _e2e(device, lib, cvgs.CV_8UC3, 3, dsize, flags=capi.CHAIN_FORCE_GENERIC) == "generic_table"
    else:
        name = _e2e(device, lib, cvgs.CV_8UC3, 3, dsize, ar=cvgs.PRESERVE_AR, background=[10.0, 20.0, 30.0])
        assert name.startswith("k1_u8c3"), name


@pytest.mark.parametrize("dsize", [(16, 8), (64, 128)], ids=["16x8", "64x128"])
@pytest.mark.parametrize("layout", [capi.YUV_NV12, capi.YUV_NV21], ids=["nv12", "nv21"])
def test_end_to_end_nv12(device, lib, layout, dsize):
    """Crops of a 130 x 66 decoder surface from device-side boxes.  Device tables of 4:2:0 surfaces run the interpreted kernel today (the
    K4 launcher checks its planes on the host); a K4 kernel that learns to read them may take over."""
    name = _e2e(device, lib, cvgs.CV_8UC1, 3, dsize, nv12=True, layout=layout)
    print("4:2:0 device table, layout %d: %s" % (layout, name))
    assert name == "generic_table" or name.startswith("k4_"), name


def _tick(device, n_chains, dsize, n_boxes, seeds):
    """n_chains cameras: frames, box buffers, counts, tables, outputs, and the descs / chains that use them."""
    torch = _torch()
    cams = []
    for k in range(n_chains):
        frame = Frame(device, 97, 61, cvgs.CV_8UC3, 304, seed=seeds + k)
        bt = torch.zeros((n_boxes, 4), dtype=torch.int32, device=device)
        ct = torch.zeros((1,), dtype=torch.int32, device=device)
        table = torch.zeros((n_boxes, 48), dtype=torch.uint8, device=device)
        out = _out_tensor(device, n_boxes, 3, dsize)
        desc = cvgs.box_table_desc(frame.mat, bt, table, n_boxes, dsize, cvgs.IGNORE_AR, B.XYWH_I32, ct, None)
        ops = _chain(cvgs.resize_boxes(frame.mat, table, n_boxes, dsize), 3, out, dsize)
        cams.append(dict(frame=frame, boxes=bt, count=ct, table=table, out=out, desc=desc, ops=ops))
    return cams


def _host_planes(device, frame, boxes, count, dsize):
    """The eager host-described result for one camera: [n, 3, h, w], invalid boxes = the default plane."""
    torch = _torch()
    model = B.rects(boxes, B.XYWH_I32, frame.W, frame.H, count)
    valid = [i for i, r in enumerate(model) if r]
    want = _out_tensor(device, len(boxes), 3, dsize)
    s = torch.cuda.current_stream()
    bg = _out_tensor(device, 1, 3, dsize)
    cvgs.executeOperations(s, *_chain(frame.host_read([frame.mat], dsize, cvgs.IGNORE_AR, used=0), 3, bg, dsize))
    want[:] = bg[0]
    if valid:
        got = _out_tensor(device, len(valid), 3, dsize)
        cvgs.executeOperations(s, *_chain(frame.host_read([frame.view(model[i]) for i in valid], dsize, cvgs.IGNORE_AR), 3, got, dsize))
        want[torch.tensor(valid, device=device)] = got
    torch.cuda.synchronize()
    return want


def _random_boxes(rng, n):
    b = np.stack([rng.integers(-20, 100, n), rng.integers(-20, 70, n), rng.integers(-2, 80, n), rng.integers(-2, 60, n)], axis=1)
    return b.astype(np.int32)


def test_three_chain_tick_is_one_fused_k1_launch(device, lib):
    """cvgs_execute_many over three device-built tables whose chains state their frame's byte range: still ONE kernel node (the fused K1
    launch), and plane by plane the eager host-described result."""
    torch = _torch()
    from tests.test_gpu_many import _captured_kernel_nodes
    dsize, n = (64, 128), 24
    cams = _tick(device, 3, dsize, n, seeds=300)
    rng = np.random.default_rng(5)
    boxes = [_random_boxes(rng, n) for _ in cams]
    counts = [n, n - 5, n + 5]
    for cam, b, c in zip(cams, boxes, counts):
        cam["boxes"].copy_(torch.from_numpy(b).to(device))
        cam["count"].fill_(c)
    s = torch.cuda.current_stream()
    cvgs.plane_tables_from_boxes(s, [cam["desc"] for cam in cams])
    low = [cvgs.lower(cam["ops"]) for cam in cams]
    for cam, lc in zip(cams, low):
        r = lc.desc.read
        assert (r.table_src_lo, r.table_src_hi) == (cam["frame"].mat.data, cam["frame"].mat.data + 60 * 304 + 97 * 3)
        assert (r.batch, r.used_planes) == (n, n)
    assert cvgs.kernel_name(*cams[0]["ops"]) == "k1_u8c3_swap_mul_sub_div"
    arr = cvgs.pack_chains(low)
    assert _captured_kernel_nodes(lib, arr, 3, device) == 1, "the tick over device-built tables is not ONE fused launch"
    capi.check(lib.cvgs_execute_many(arr, 3, cvgs.stream_handle(s)))
    torch.cuda.synchronize()
    for k, (cam, b, c) in enumerate(zip(cams, boxes, counts)):
        assert torch.equal(cam["out"], _host_planes(device, cam["frame"], b, c, dsize)), "camera %d" % k


def test_no_host_in_the_loop(device, lib):
    """boxes written by a device op -> cvgs_plane_tables_from_boxes -> the tick, captured on ONE stream as one linear graph; the source
    tensors are then overwritten with device copies only and the graph replayed: each replay equals the eager host-described result."""
    torch = _torch()
    dsize, n = (16, 8), 24
    cams = _tick(device, 2, dsize, n, seeds=400)
    rng = np.random.default_rng(9)
    rounds = [([_random_boxes(rng, n) for _ in cams], [n - 7, 3]), ([_random_boxes(rng, n) for _ in cams], [n + 2, n - 1])]
    # the "detector output": one source tensor per camera for the boxes and one for the count, overwritten between the replays
    src_boxes = [torch.zeros((n, 4), dtype=torch.int32, device=device) for _ in cams]
    src_count = [torch.zeros((1,), dtype=torch.int32, device=device) for _ in cams]
    staged = [([torch.from_numpy(b).to(device) for b in bs], [torch.tensor([c], dtype=torch.int32, device=device) for c in cs]) for bs, cs in rounds]
    low = [cvgs.lower(cam["ops"]) for cam in cams]
    arr = cvgs.pack_chains(low)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream()
        for cam, sb, sc in zip(cams, src_boxes, src_count):
            cam["boxes"].copy_(sb)
            cam["count"].copy_(sc)
        cvgs.plane_tables_from_boxes(s, [cam["desc"] for cam in cams])
        capi.check(lib.cvgs_execute_many(arr, len(cams), cvgs.stream_handle(s)))
    torch.cuda.synchronize()
    for cam in cams:
        assert (cam["out"] == -5.0).all(), "capture itself must not run anything"
    for r, (bs, cs) in enumerate(rounds):
        for k in range(len(cams)):  # device copies only
            src_boxes[k].copy_(staged[r][0][k])
            src_count[k].copy_(staged[r][1][k])
        g.replay()
        torch.cuda.synchronize()
        for k, cam in enumerate(cams):
            assert torch.equal(cam["out"], _host_planes(device, cam["frame"], bs[k], cs[k], dsize)), "replay %d, camera %d" % (r, k)
    assert not torch.equal(_host_planes(device, cams[0]["frame"], rounds[0][0][0], rounds[0][1][0], dsize),
                           _host_planes(device, cams[0]["frame"], rounds[1][0][0], rounds[1][1][0], dsize))


def test_edge_boxes_stay_inside_the_frame(device, lib):
    """The frame sits inside a larger allocation whose margin -- rows above and below, bytes left and right of every row -- holds a sentinel
    (255; the frame's own pixels are <= 127, and the chain is monotone, so one sentinel tap with any weight would show).  The pinned edge
    boxes of both formats: the margin and the guards around the table and rectangle buffers stay as they were, every emitted view lies
    inside the frame, and no output value exceeds what a 127 pixel gives."""
    torch = _torch()
    W, Hh, top, left = 97, 61, 8, 24
    step = left + W * 3 + 29
    big = torch.full((Hh + 2 * top, step), 255, dtype=torch.uint8, device=device)
    pix = torch.from_numpy(H.random_u8((Hh, W * 3), seed=77) & 0x7f).to(device)
    big[top:top + Hh, left:left + W * 3] = pix
    before = big.clone()
    base = big.data_ptr() + top * step + left
    mat = cvgs.GpuMat(Hh, W, cvgs.CV_8UC3, base, step, owner=big)
    dsize = (16, 8)
    s = torch.cuda.current_stream()
    for fmt, cases in ((B.XYXY_F32, B.PINNED_XYXY), (B.XYWH_I32, B.PINNED_XYWH)):
        boxes = B.boxes_array([b for b, _ in cases], fmt)
        n = len(boxes)
        bt = torch.from_numpy(boxes).to(device)
        tbuf = torch.full((n + 2, 48), 0xA5, dtype=torch.uint8, device=device)   # one guard entry on either side
        rbuf = torch.full((n + 2, 4), 0x5A5A5A5A, dtype=torch.int32, device=device)
        for count in (None, n + 5):
            ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=device)
            cvgs.plane_tables_from_boxes(s, [cvgs.box_table_desc(mat, bt, tbuf[1:], n, dsize, cvgs.PRESERVE_AR, fmt, ct, rbuf[1:])])
        out = _out_tensor(device, n, 3, dsize)
        cvgs.executeOperations(s, *_chain(cvgs.resize_boxes(mat, tbuf[1:], n, dsize, [0.0, 0.0, 0.0], cvgs.PRESERVE_AR), 3, out, dsize))
        torch.cuda.synchronize()
        assert (tbuf[0] == 0xA5).all() and (tbuf[-1] == 0xA5).all() and (rbuf[0] == 0x5A5A5A5A).all() and (rbuf[-1] == 0x5A5A5A5A).all()
        model = B.rects(boxes, fmt, W, Hh)
        assert (rbuf[1:-1].cpu().numpy() == _rects_array(model)).all()
        tab = np.frombuffer(tbuf[1:-1].cpu().numpy().tobytes(), np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("rest", "V28")]))
        for e in tab:  # every view, valid or not, lies inside the frame
            off = int(e["data"]) - base
            y, x = divmod(off, step)
            assert off >= 0 and x % 3 == 0 and e["step"] == step and e["w"] >= 1 and e["h"] >= 1 and x // 3 + e["w"] <= W and y + e["h"] <= Hh, e
        # (px * alpha - sub) / div is increasing in px and the bilinear weights sum to 1 within a few ulp: nothing may exceed the value of a 127 pixel
        hi = max((127.0 * H.K1_ALPHA - sub) / div for sub, div in zip(H.K1_SUB[3], H.K1_DIV[3])) * (1 + 1e-5) + 1e-5
        lo = min((0.0 - sub) / div for sub, div in zip(H.K1_SUB[3], H.K1_DIV[3])) - 1e-5
        assert float(out.max()) <= hi and float(out.min()) >= lo, (float(out.min()), float(out.max()), lo, hi)
    assert torch.equal(big, before), "the margin around the frame changed"
