#!/usr/bin/env python3
"""cvgs_warp_tables_from_boxes timed, in ONE GPU process, legs alternated ABAB.  Workload: a tick of 16 1080p frames, each with an
8,400-candidate fp32 row-major head (cx, cy, w, h, score in the letterboxed 640 x 640 input) of which about 300 candidates are over the
threshold and 50 are kept; every kept box grows by 1.25, its shorter side to 192:256, and is sampled to [3, 256, 192] fp32 even where it
leaves the frame.  Under graph replay with HIP events around the replays:
  box_warps       (1) K cvgs_warp_tables_from_boxes calls (16 frames each): the call alone
  torch_corners   (2) the path it replaces on the same boxes: the same shaping spelled in framework element-wise ops on the device,
                  producing three corners per box, then cvgs_warp_tables_from_points with the AFFINE3 fit
  pipeline        (3) head -> cvgs_head_decode -> cvgs_boxes_select -> cvgs_warp_tables_from_boxes -> the warp tick, one graph
(1) and (2) must describe the same warps: their matrices agree to 1e-3 of the box's size (the framework path computes in fp32), asserted
before anything is timed.  No threshold is set: the figures and their run-to-run spread are the result.
usage: bench_box_warp.py [--out profiles/box_warp_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_area_tick import _capture, _time_graph  # noqa: E402  (the protocol's two helpers)
from tools.bench_point_gather import _head  # noqa: E402  (the detector head of the landmark bench: boxes, one score)
from tools.bench_warp_tick import DIV, MUL, SUB  # noqa: E402

DST = (192, 256)
SCALE, PAD = (1.25, 1.25), (0.0, 0.0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_warp_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, MEMBERS, PRE_K, MAX_OUT, DET, K, THR, A = 16, 8400, 300, 1024, 50, 640, 4, 0.25, 20
    fw, fh = W.FRAME_1080P
    xform = cvgs.letterbox_xform((fw, fh), (DET, DET), cvgs.PRESERVE_AR)
    rng = np.random.default_rng(W.SEED)
    head = torch.from_numpy(np.stack([_head(np, rng, N, MEMBERS, DET) for _ in range(M)])).to(dev)  # [M, N, 20] fp32
    frames = [W.random_u8_torch((fh, fw, 3), W.SEED + f, dev) for f in range(M)]
    mats = [cvgs.GpuMat.from_tensor(fr, cvgs.CV_8UC3) for fr in frames]

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def z(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def padded(nbytes):
        return (nbytes + 255) // 256 * 256

    scratch = z((M, padded(cvgs.head_decode_scratch_bytes(N))), torch.uint8)
    d_boxes, d_scores, d_classes, d_index, d_count = z((M, N, 4), torch.float32), z((M, N), torch.float32), z((M, N), torch.int32), z((M, N), torch.int32), z((M, 64), torch.int32)
    s_scratch = z((M, padded(cvgs.boxes_select_scratch_bytes(N, PRE_K))), torch.uint8)
    s_boxes, s_count = z((M, MAX_OUT, 4), torch.float32), z((M, 64), torch.int32)
    tables, tables_t = z((M, MAX_OUT, 64), torch.uint8), z((M, MAX_OUT, 64), torch.uint8)
    corners = z((M, MAX_OUT, 3, 2), torch.float32)
    out = z((M, MAX_OUT, 3 * DST[0] * DST[1]), torch.float32)
    hdescs = (capi.HeadDesc * M)(*[cvgs.head_desc(head[f], cvgs.HEAD_F32, N, A, 1, 1, THR, scratch[f], d_boxes[f], d_scores[f], d_classes[f], d_count[f], d_index[f]) for f in range(M)])
    sdescs = (capi.BoxSelectDesc * M)(*[cvgs.box_select_desc((fw, fh), d_boxes[f], d_scores[f], N, s_scratch[f], s_boxes[f], s_count[f], THR, 0.45, PRE_K, MAX_OUT,
                                                             cvgs.CAND_CXCYWH_F32, 4, 1, d_classes[f], 1, d_count[f], xform) for f in range(M)])
    bdescs = (capi.BoxWarpDesc * M)(*[cvgs.box_warp_desc(mats[f], s_boxes[f], tables[f], MAX_OUT, DST, cvgs.BOX_SHAPE_EXPAND, SCALE, PAD, count=s_count[f]) for f in range(M)])
    # the destination's corners in pixel-centre coordinates: the edge coordinates 0, dst_w, dst_h, less half a pixel
    tmpl3 = [(-0.5, -0.5), (DST[0] - 0.5, -0.5), (-0.5, DST[1] - 0.5)]
    wdescs = (capi.WarpTableDesc * M)(*[cvgs.warp_table_desc(mats[f], corners[f], tables_t[f], MAX_OUT, DST, tmpl3, cvgs.WARP_FIT_AFFINE3, count=s_count[f]) for f in range(M)])
    f32 = cvgs.CV_32FC3
    chains = [cvgs.lower([cvgs.warp_table(cvgs.WARP_AFFINE, mats[f], tables[f], MAX_OUT, DST), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f32), cvgs.multiply(f32, MUL),
                          cvgs.subtract(f32, SUB), cvgs.divide(f32, DIV), cvgs.split_tensor(f32, out[f].data_ptr(), DST[0], DST[1], MAX_OUT, keep=out)]) for f in range(M)]
    tick = cvgs.pack_chains(chains)

    def box_fn():
        for _ in range(K):
            capi.check(lib.cvgs_warp_tables_from_boxes(bdescs, M, stream()))

    def torch_once():
        xa, ya, xb, yb = s_boxes[..., 0], s_boxes[..., 1], s_boxes[..., 2], s_boxes[..., 3]
        w1 = (xb - xa) * SCALE[0] + PAD[0]
        h1 = (yb - ya) * SCALE[1] + PAD[1]
        t1, t2 = w1 * DST[1], h1 * DST[0]
        h2 = torch.where(t1 > t2, t1 / DST[0], h1)
        w2 = torch.where(t2 > t1, t2 / DST[1], w1)
        x0, y0 = (xa + xb) * 0.5 - w2 * 0.5 - 0.5, (ya + yb) * 0.5 - h2 * 0.5 - 0.5
        corners.copy_(torch.stack([torch.stack([x0, y0], -1), torch.stack([x0 + w2, y0], -1), torch.stack([x0, y0 + h2], -1)], -2))
        capi.check(lib.cvgs_warp_tables_from_points(wdescs, M, stream()))

    def torch_fn():
        for _ in range(K):
            torch_once()

    def pipeline_fn():
        for _ in range(K):
            capi.check(lib.cvgs_head_decode(hdescs, M, stream()))
            capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))
            capi.check(lib.cvgs_warp_tables_from_boxes(bdescs, M, stream()))
            capi.check(lib.cvgs_execute_many(tick, M, stream()))

    # the pipeline once; then (1) and (2) describe the same warps
    pipeline_fn()
    torch.cuda.synchronize()
    note = lib.cvgs_last_error().decode()
    assert note.startswith("tick:"), "the warp tick did not fuse: %s" % note
    kept = [int(x) for x in s_count[:, 0].cpu()]
    torch_once()
    torch.cuda.synchronize()
    entry = np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")])
    ma = np.frombuffer(tables.cpu().numpy().tobytes(), entry)["m"].reshape(M, MAX_OUT, 9).astype(np.float64)
    mb = np.frombuffer(tables_t.cpu().numpy().tobytes(), entry)["m"].reshape(M, MAX_OUT, 9).astype(np.float64)
    worst = 0.0
    for f in range(M):
        size = np.maximum(np.abs(ma[f, :kept[f], [0, 4]]).max(axis=0) * max(DST), 1.0)[:, None]  # the shaped box's larger side, in pixels
        worst = max(worst, float((np.abs(ma[f, :kept[f]] - mb[f, :kept[f]]) * np.array([DST[0], 1, 1, 1, DST[1], 1, 1, 1, 1]) / size).max()))
        assert (ma[f, kept[f]:] == mb[f, kept[f]:]).all()
    assert worst < 1e-3, "the framework path's warps differ from cvgs_warp_tables_from_boxes': %g of the box's size" % worst
    graphs = {"box_warps": _capture(box_fn), "torch_corners": _capture(torch_fn), "pipeline": _capture(pipeline_fn)}
    per = {k: [] for k in graphs}
    for _ in range(a.rounds):  # ABAB: every round times every leg once
        for k, g in graphs.items():
            per[k].append(_time_graph(g, a.reps) / K)
    res = {"workload": "16 1080p frames x 8400-candidate fp32 heads (box, score), ~300 over the score threshold 0.25, pre_nms_k 1024, max_out 50; every kept box x 1.25, "
                       "shorter side grown to 192:256, sampled unclamped; warp tick: 16 x 50 crops -> [50,3,256,192] fp32; us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "kept_per_frame": kept, "tick_note": note,
           "framework_path_worst_difference_of_box_size": worst}
    for k, ts in per.items():
        res[k] = {"us": round(float(np.median(ts)), 3), "min_us": round(float(np.min(ts)), 3), "max_us": round(float(np.max(ts)), 3),
                  "legs_us": [round(float(x), 3) for x in ts]}
    res["torch_corners_over_box_warps"] = round(res["torch_corners"]["us"] / res["box_warps"]["us"], 3)
    print(json.dumps({k: (v["us"] if isinstance(v, dict) else v) for k, v in res.items() if k not in ("kept_per_frame", "workload")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
