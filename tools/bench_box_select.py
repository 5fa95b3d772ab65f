#!/usr/bin/env python3
"""cvgs_boxes_select timed, in ONE GPU process, legs alternated ABAB.  Workload: a tick of 16 frames (1920 x 1080 u8c3), each with a
[8400, 6] detector head (cx, cy, w, h, score, class in the letterboxed 640 x 640 input) of which about 300 candidates pass the score
threshold; pre_nms_k 1024, max_out 50; the selected boxes feed cvgs_plane_tables_from_boxes and the bilinear K1 tick -> [50,3,128,64] fp32.
  select_graph     K cvgs_boxes_select calls (16 frames each) captured in a HIP graph, HIP events around the replays: the call alone
  device_graph     select + table build + tick as ONE graph, events around the replays
  device_wall      one tick of the same as a graph, replay + synchronise, wall clock (what a host that needs the tensor waits for)
  host_wall        the path replaced, wall clock: D2H copy of the 16 heads (pinned), synchronise, cvgs_boxes_select_host per frame, H2D copy
                   of the boxes and counts, table build + tick, synchronise
No threshold is set: the figures and their run-to-run spread are the result.
usage: bench_box_select.py [--out profiles/box_select_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_area_tick import _capture, _time_graph  # noqa: E402  (the protocol's two helpers)


def _head(np, rng, n, members, det):
    """[n, 6] float32: clustered CXCYWH boxes in detector pixels, `members` scores in [0.3, 1), the rest below 0.2, a class in 0..2."""
    k = 40
    centres, sizes = rng.uniform(0.1 * det, 0.9 * det, (k, 2)), rng.uniform(det / 30, det / 5, (k, 2))
    which = rng.integers(0, k, n)
    head = np.zeros((n, 6), np.float32)
    head[:, 0:2] = centres[which] + rng.normal(0, det / 100, (n, 2))
    head[:, 2:4] = sizes[which] * rng.uniform(0.8, 1.25, (n, 2))
    head[:, 4] = rng.uniform(0.0, 0.2, n)
    head[rng.permutation(n)[:members], 4] = rng.uniform(0.3, 1.0, members)
    head.view(np.int32)[:, 5] = rng.integers(0, 3, n)
    return head


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_select_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, MEMBERS, PRE_K, MAX_OUT, DET, K = 16, 8400, 300, 1024, 50, 640, 8
    fw, fh = W.FRAME_1080P
    xform = cvgs.letterbox_xform((fw, fh), (DET, DET), cvgs.PRESERVE_AR)
    rng = np.random.default_rng(W.SEED)
    plane = 3 * W.DST[0] * W.DST[1]
    heads_h = [_head(np, rng, N, MEMBERS, DET) for _ in range(M)]
    heads = [torch.from_numpy(h).to(dev) for h in heads_h]
    frames = [W.random_u8_torch((fh, fw, 3), W.SEED + f, dev) for f in range(M)]
    out = torch.zeros((M, MAX_OUT, plane), dtype=torch.float32, device=dev)
    sb = cvgs.boxes_select_scratch_bytes(N, PRE_K)
    scratch = torch.zeros((M, (sb + 255) // 256 * 256), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((M, MAX_OUT, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros((M, 64), dtype=torch.int32, device=dev)  # one count per 256 bytes
    tables = torch.zeros((M, MAX_OUT, 48), dtype=torch.uint8, device=dev)

    def sel_desc(f, ptr=None):
        base = heads[f].data_ptr() if ptr is None else ptr
        return cvgs.box_select_desc((fw, fh), base, base + 16, N, scratch[f], boxes[f], counts[f], 0.25, 0.45, PRE_K, MAX_OUT, cvgs.CAND_CXCYWH_F32, 6, 6, base + 20, 6,
                                    None, xform)

    sdescs = (capi.BoxSelectDesc * M)(*[sel_desc(f) for f in range(M)])
    tdescs, lowered = [], []
    for f in range(M):
        src = cvgs.GpuMat.from_tensor(frames[f], cvgs.CV_8UC3)
        tdescs.append(cvgs.box_table_desc(src, boxes[f], tables[f], MAX_OUT, W.DST, cvgs.IGNORE_AR, cvgs.BOX_XYXY_F32, counts[f], None))
        ops = W.k1_chain(src, W.random_crops(MAX_OUT, fw, fh, seed=W.SEED + f), cvgs.GpuMat.from_tensor(out[f], cvgs.CV_32FC1))
        ops[0] = cvgs.resize_boxes(src, tables[f], MAX_OUT, W.DST)
        lowered.append(cvgs.lower(ops))
    tarr = (capi.BoxTableDesc * M)(*tdescs)
    chains = cvgs.pack_chains(lowered)
    kernel = cvgs.kernel_name(*ops)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def select_fn():
        for _ in range(K):
            capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))

    def tail(s):
        capi.check(lib.cvgs_plane_tables_from_boxes(tarr, M, s))
        capi.check(lib.cvgs_execute_many(chains, M, s))

    def device_fn():
        for _ in range(K):
            capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))
            tail(stream())

    # the path replaced: pinned staging, the host entry on HOST copies of the heads
    heads_pin = [torch.zeros((N, 6), dtype=torch.float32).pin_memory() for _ in range(M)]
    boxes_pin = torch.zeros((M, MAX_OUT, 4), dtype=torch.float32).pin_memory()
    counts_pin = torch.zeros((M, 64), dtype=torch.int32).pin_memory()
    hdescs = [sel_desc(f, heads_pin[f].data_ptr()) for f in range(M)]

    def host_tick():
        for f in range(M):
            heads_pin[f].copy_(heads[f], non_blocking=True)
        torch.cuda.synchronize()
        for f in range(M):
            capi.check(lib.cvgs_boxes_select_host(C.byref(hdescs[f]), boxes_pin[f].data_ptr(), counts_pin[f].data_ptr(), None, None))
        boxes.copy_(boxes_pin, non_blocking=True)
        counts.copy_(counts_pin, non_blocking=True)
        tail(stream())
        torch.cuda.synchronize()

    # the two paths select the same boxes
    host_tick()
    want_b, want_c, want_o = boxes.clone(), counts[:, 0].clone(), out.clone()
    boxes.zero_(), counts.zero_(), out.zero_()
    capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))
    tail(stream())
    torch.cuda.synchronize()
    assert torch.equal(boxes.view(torch.int32), want_b.view(torch.int32)) and torch.equal(counts[:, 0], want_c) and torch.equal(out, want_o)
    kept = [int(v) for v in want_c.cpu()]

    def device_one():
        capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))
        tail(stream())

    g_select, g_device, g_one = _capture(select_fn), _capture(device_fn), _capture(device_one)

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) * 1e6 / reps

    def device_wall():
        g_one.replay()
        torch.cuda.synchronize()

    per = {"select_graph": [], "device_graph": [], "device_wall": [], "host_wall": []}
    for _ in range(a.rounds):  # ABAB: every round times every leg once
        per["select_graph"].append(_time_graph(g_select, a.reps) / K)
        per["device_graph"].append(_time_graph(g_device, a.reps) / K)
        per["device_wall"].append(wall(device_wall, a.reps))
        per["host_wall"].append(wall(host_tick, a.reps))
    res = {"workload": "16 frames x [8400, 6] CXCYWH heads, ~300 over the score threshold per frame, pre_nms_k 1024, max_out 50, 1080p u8c3 frames -> "
                       "[50,3,128,64] fp32; us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "tick_kernel": kernel, "kept_per_frame": kept,
           "note": "device_wall replays a one-tick graph and synchronises once per tick; host_wall synchronises twice per tick: the host path cannot do otherwise"}
    for k, v in per.items():
        res[k] = {"us": round(float(np.median(v)), 3), "min_us": round(float(np.min(v)), 3), "max_us": round(float(np.max(v)), 3),
                  "legs_us": [round(float(x), 3) for x in v]}
    res["host_over_device_wall"] = round(res["host_wall"]["us"] / res["device_wall"]["us"], 3)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
