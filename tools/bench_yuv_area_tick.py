#!/usr/bin/env python3
"""The decode-side tick spelled INTER_AREA, in ONE GPU process, legs alternated ABAB: 16 NV12 surfaces x 50 variable crops of a 4K surface
(BT.709 limited) -> BGR -> [50,3,128,64] fp32 per surface, device plane tables, K ticks captured into a HIP graph and replayed on a rotation
of 64 resident 4K surfaces (inputs rotated as bench.py does), HIP events around the replays.
  A  yuv_area_each   16 cvgs_execute calls per tick -- what cvgs_execute_many did for these chains before their tick kernel
  B  yuv_area_tick   ONE cvgs_execute_many per tick (k_yuv_area_fast_many, grid z = surface)
  linear_tick        the bilinear K4 tick on the same surfaces and crops, for scale (host descriptors in the kernel arguments: K4 takes no
                     device tables in a tick)
No ratio is promised and nothing is asserted about B against A: the figures go into the JSON as measured (a_over_b, A's run-to-run spread).
The one condition is that B really is one fused launch per tick (its note starts with "tick:").
usage: bench_yuv_area_tick.py [--out profiles/yuv_area_tick_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_area_tick import _capture, _time_graph  # noqa: E402
from bench_yuv_area import _even_crops  # noqa: E402


def _commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or "unknown"
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_area_tick_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--commit", default=None, help="the commit the figures belong to (default: git rev-parse of the tree)")
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, SURFACES, K = 16, 50, 64, 8
    dw, dh = W.DST
    plane = 3 * dw * dh
    sw, sh = W.FRAME_4K
    f3 = cvgs.CV_32FC3
    surf = [W.random_u8_torch((sh * 3 // 2, sw), W.SEED + f, dev) for f in range(SURFACES)]
    crops = [_even_crops(N, sw, sh, W.SEED + 700000 + f) for f in range(SURFACES)]
    keep, names, chains_of, groups = [], {}, {}, {}
    for kind, interp, tables in (("area", cvgs.INTER_AREA, True), ("linear", cvgs.INTER_LINEAR, False)):
        out = torch.zeros((SURFACES, N, plane), dtype=torch.float32, device=dev)
        keep.append(out)
        chains_of[kind], groups[kind] = [], []
        for f in range(SURFACES):
            m = cvgs.GpuMat(sh, sw, cvgs.CV_8UC1, surf[f].data_ptr(), sw, owner=surf[f])
            rd = cvgs.read_nv12([m.nv12_roi(*c) for c in crops[f]], W.DST, capi.YUV_LIMITED, capi.BT709, False, interp=interp)
            if tables:
                tab = torch.frombuffer(bytearray(cvgs.build_plane_table(rd)), dtype=torch.uint8).to(dev)
                keep.append(tab)
                rd.table = tab.data_ptr()
            ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f3), cvgs.multiply(f3, [W.K1_ALPHA] * 3), cvgs.subtract(f3, W.K1_SUB[3]), cvgs.divide(f3, W.K1_DIV[3]),
                   cvgs.split(f3, cvgs.GpuMat(N, plane, cvgs.CV_32FC1, out[f].data_ptr(), plane * 4, owner=out), W.DST)]
            chains_of[kind].append(cvgs.lower(ops))
        names[kind] = cvgs.kernel_name(*ops)
        for g in range(SURFACES // M):
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
            g = i % (SURFACES // M)
            for lc in chains_of["area"][g * M:(g + 1) * M]:
                capi.check(lib.cvgs_execute(C.byref(lc.desc), s))

    legs = {"yuv_area_each": _capture(each_fn), "yuv_area_tick": _capture(tick_fn("area")), "linear_tick": _capture(tick_fn("linear"))}
    assert notes["area"].startswith("tick:"), "the AREA tick of decoder surfaces did not fuse: %s" % notes["area"]
    per = {k: [] for k in legs}
    for _ in range(a.rounds):  # ABAB: every round times every leg once
        for k, g in legs.items():
            per[k].append(_time_graph(g, a.reps) / K)
    res = {"workload": "16 NV12 surfaces x 50 variable crops of a 4K surface (BT.709 limited) -> BGR -> [50,3,128,64] fp32, device plane tables "
                       "(linear_tick: host descriptors); us per TICK (16 surfaces)",
           "commit": a.commit or _commit(), "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "kernels": names, "notes": notes}
    for k, v in per.items():
        res[k] = {"us": round(float(np.median(v)), 3), "min_us": round(float(np.min(v)), 3), "max_us": round(float(np.max(v)), 3),
                  "us_per_surface": round(float(np.median(v)) / M, 4), "legs_us": [round(float(x), 3) for x in v]}
    A, B = res["yuv_area_each"], res["yuv_area_tick"]
    res["a_spread_us"] = round(A["max_us"] - A["min_us"], 3)
    res["b_spread_us"] = round(B["max_us"] - B["min_us"], 3)
    res["b_minus_a_us"] = round(B["us"] - A["us"], 3)
    res["b_over_a"] = round(B["us"] / A["us"], 4)
    res["a_over_b"] = round(A["us"] / B["us"], 4)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
