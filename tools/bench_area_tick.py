#!/usr/bin/env python3
"""The headline tick spelled INTER_AREA, in ONE GPU process, legs alternated ABAB: 16 frames x 50 variable crops of a 4K u8c3 frame ->
[50,3,128,64] fp32 per frame, device plane tables, K ticks captured into a HIP graph and replayed on a rotation of 64 resident 4K frames
(inputs rotated as bench.py does), HIP events around the replays.
  A  area_each    16 cvgs_execute calls per tick -- what cvgs_execute_many did for AREA chains before the AREA tick kernel
  B  area_tick    ONE cvgs_execute_many per tick (k_area_fast_many, grid z = frame)
  linear_tick     the bilinear tick on the same frames and crops, for scale
The condition on B: not slower than A by more than A's own run-to-run spread (max - min of A's legs).  No ratio is promised: the AREA kernel
reads every byte of every crop, so launch boundaries are a smaller share than in the bilinear tick.
usage: bench_area_tick.py [--out profiles/area_tick_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_graph(g, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per replay


def _capture(fn):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    torch.cuda.synchronize()
    return g


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_tick_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, FRAMES, K = 16, 50, 64, 8
    plane = 3 * W.DST[0] * W.DST[1]
    fw, fh = W.FRAME_4K
    frames = [W.random_u8_torch((fh, fw, 3), W.SEED + f, dev) for f in range(FRAMES)]
    crops = [W.random_crops(N, fw, fh, seed=W.SEED + 500000 + f) for f in range(FRAMES)]
    keep, names, chains_of, groups = [], {}, {}, {}
    for kind, interp in (("area", cvgs.INTER_AREA), ("linear", cvgs.INTER_LINEAR)):
        out = torch.zeros((FRAMES, N, plane), dtype=torch.float32, device=dev)
        keep.append(out)
        chains_of[kind], groups[kind] = [], []
        for f in range(FRAMES):
            src = cvgs.GpuMat.from_tensor(frames[f], cvgs.CV_8UC3)
            ops = W.k1_chain(src, crops[f], cvgs.GpuMat.from_tensor(out[f], cvgs.CV_32FC1))
            ops[0] = cvgs.resize(cvgs.CV_8UC3, interp, [src.roi(*c) for c in crops[f]], W.DST)
            tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).to(dev)
            keep.append(tab)
            ops[0].table = tab.data_ptr()
            chains_of[kind].append(cvgs.lower(ops))
        names[kind] = cvgs.kernel_name(*ops)
        for g in range(FRAMES // M):
            groups[kind].append(cvgs.pack_chains(chains_of[kind][g * M:(g + 1) * M]))
    notes = {}

    def tick_fn(kind):
        def fn():
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(K):
                capi.check(lib.cvgs_execute_many(groups[kind][i % len(groups[kind])], M, s))
            notes[kind] = lib.cvgs_last_error().decode()
        return fn

    def each_fn():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in range(K):
            g = i % (FRAMES // M)
            for lc in chains_of["area"][g * M:(g + 1) * M]:
                capi.check(lib.cvgs_execute(C.byref(lc.desc), s))

    legs = {"area_each": _capture(each_fn), "area_tick": _capture(tick_fn("area")), "linear_tick": _capture(tick_fn("linear"))}
    assert notes["area"].startswith("tick:"), "the AREA tick did not fuse: %s" % notes["area"]
    per = {k: [] for k in legs}
    for _ in range(a.rounds):  # ABAB: every round times every leg once
        for k, g in legs.items():
            per[k].append(_time_graph(g, a.reps) / K)
    res = {"workload": "16 frames x 50 variable crops of a 4K u8c3 frame -> [50,3,128,64] fp32, device plane tables; us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "kernels": names, "notes": notes}
    for k, v in per.items():
        res[k] = {"us": round(float(np.median(v)), 3), "min_us": round(float(np.min(v)), 3), "max_us": round(float(np.max(v)), 3),
                  "us_per_frame": round(float(np.median(v)) / M, 4), "legs_us": [round(float(x), 3) for x in v]}
    A, B = res["area_each"], res["area_tick"]
    res["a_spread_us"] = round(A["max_us"] - A["min_us"], 3)
    res["b_minus_a_us"] = round(B["us"] - A["us"], 3)
    res["a_over_b"] = round(A["us"] / B["us"], 4)
    res["b_not_slower_than_a_by_more_than_its_spread"] = bool(B["us"] - A["us"] <= A["max_us"] - A["min_us"])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0 if res["b_not_slower_than_a_by_more_than_its_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
