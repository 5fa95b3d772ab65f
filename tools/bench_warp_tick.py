#!/usr/bin/env python3
"""The landmark side's tick, in ONE GPU process, legs alternated ABAB: 16 frames x 50 five-landmark similarity items of a 4K u8c3 frame ->
[50,3,112,112] fp32 per frame (swap-mul-sub-div), the device warp tables of the 16 frames from ONE cvgs_warp_tables_from_points call, K ticks
captured into a HIP graph and replayed on a rotation of 64 resident 4K frames, HIP events around the replays.
  A  warp_tick    ONE cvgs_execute_many per tick (k_warp_fast_many, grid z = frame)
  B  warp_each    16 cvgs_execute calls per tick -- what cvgs_execute_many did for warp chains before the warp tick kernel
The condition on A: faster than B by more than the larger of the two legs' run-to-run spreads (max - min over the rounds).  No ratio is
promised.
usage: bench_warp_tick.py [--out profiles/warp_tick_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_area_tick import _capture, _time_graph  # noqa: E402

TMPL5 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]  # the five-landmark face template, 112 x 112
DST = (112, 112)
MUL, SUB, DIV = [1.0 / 255.0] * 3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _landmarks(np, n, fw, fh, seed):
    """n items: the template rotated by up to +-30 degrees, scaled 0.8 .. 3 and moved anywhere in the frame (some partly outside)"""
    r = np.random.default_rng(seed)
    t = np.array(TMPL5, np.float64)
    pts = np.zeros((n, 5, 2), np.float32)
    for i in range(n):
        a, s = r.uniform(-np.pi / 6, np.pi / 6), r.uniform(0.8, 3.0)
        R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        pts[i] = (t - t.mean(axis=0)) @ R.T + np.array([r.uniform(0, fw), r.uniform(0, fh)])
    return pts


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_tick_bench.json"))
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
    plane = 3 * DST[0] * DST[1]
    fw, fh = W.FRAME_4K
    frames = [W.random_u8_torch((fh, fw, 3), W.SEED + f, dev) for f in range(FRAMES)]
    mats = [cvgs.GpuMat.from_tensor(fr, cvgs.CV_8UC3) for fr in frames]
    pts = [torch.from_numpy(_landmarks(np, N, fw, fh, W.SEED + 700000 + f)).to(dev) for f in range(FRAMES)]
    tables = [torch.zeros((N, 64), dtype=torch.uint8, device=dev) for _ in range(FRAMES)]
    s0 = torch.cuda.current_stream()
    for g in range(FRAMES // M):  # the tables of a tick's 16 frames: ONE builder launch
        cvgs.warp_tables_from_points(s0, [cvgs.warp_table_desc(mats[f], pts[f], tables[f], N, DST, TMPL5) for f in range(g * M, (g + 1) * M)])
    torch.cuda.synchronize()
    out = torch.zeros((FRAMES, N, plane), dtype=torch.float32, device=dev)
    f32 = cvgs.CV_32FC3
    chains, ops = [], None
    for f in range(FRAMES):
        ops = [cvgs.warp_table(cvgs.WARP_AFFINE, mats[f], tables[f], N, DST), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f32), cvgs.multiply(f32, MUL),
               cvgs.subtract(f32, SUB), cvgs.divide(f32, DIV), cvgs.split_tensor(cvgs.CV_32FC3, out[f].data_ptr(), DST[0], DST[1], N, keep=out)]
        chains.append(cvgs.lower(ops))
    kernel = cvgs.kernel_name(*ops)
    groups = [cvgs.pack_chains(chains[g * M:(g + 1) * M]) for g in range(FRAMES // M)]
    notes = {}

    def tick_fn():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in range(K):
            capi.check(lib.cvgs_execute_many(groups[i % len(groups)], M, s))
        notes["warp_tick"] = lib.cvgs_last_error().decode()

    def each_fn():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in range(K):
            g = i % (FRAMES // M)
            for lc in chains[g * M:(g + 1) * M]:
                capi.check(lib.cvgs_execute(C.byref(lc.desc), s))

    # both legs write the same tensors: their bytes must agree before anything is timed
    each_fn()
    torch.cuda.synchronize()
    want = out.clone()
    out.zero_()
    tick_fn()
    torch.cuda.synchronize()
    assert notes["warp_tick"].startswith("tick:"), "the warp tick did not fuse: %s" % notes["warp_tick"]
    assert torch.equal(out, want), "the tick's bytes differ from the chains sent one by one"
    legs = {"warp_tick": _capture(tick_fn), "warp_each": _capture(each_fn)}
    per = {k: [] for k in legs}
    for _ in range(a.rounds):  # ABAB: every round times every leg once
        for k, g in legs.items():
            per[k].append(_time_graph(g, a.reps) / K)
    res = {"workload": "16 frames x 50 five-landmark similarity items of a 4K u8c3 frame -> [50,3,112,112] fp32, device warp tables from one "
                       "cvgs_warp_tables_from_points call per 16 frames; us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "kernel": kernel, "notes": notes}
    for k, v in per.items():
        res[k] = {"us": round(float(np.median(v)), 3), "min_us": round(float(np.min(v)), 3), "max_us": round(float(np.max(v)), 3),
                  "spread_us": round(float(np.max(v) - np.min(v)), 3), "us_per_frame": round(float(np.median(v)) / M, 4),
                  "legs_us": [round(float(x), 3) for x in v]}
    A, B = res["warp_tick"], res["warp_each"]
    res["larger_spread_us"] = max(A["spread_us"], B["spread_us"])
    res["b_minus_a_us"] = round(B["us"] - A["us"], 3)
    res["a_over_b"] = round(A["us"] / B["us"], 4)
    res["a_faster_than_b_by_more_than_the_larger_spread"] = bool(B["us"] - A["us"] > res["larger_spread_us"])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
    return 0 if res["a_faster_than_b_by_more_than_the_larger_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
