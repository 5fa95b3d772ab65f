#!/usr/bin/env python3
"""bf16 (CV_16BF) hand-off tensors against fp32 and fp16, in ONE GPU process, variants alternated ABAB:
  tick       16 frames x 50 crops -> [50,3,128,64] per frame through cvgs_execute_many (device plane tables), K ticks captured into a HIP
             graph and replayed on a rotation of 64 resident 4K frames: fp32 / fp16 / bf16 stores, and the fp32 tick followed by torch's
             fp32 -> bf16 copy of its output -- what a bf16 consumer pays without CV_16BF
  nv12       cfg #3: a 6K NV12 surface -> 1280x720 planar tensor, one launch per frame, fp16 vs bf16
  circular   a CircularTensor update (depth 16, 1080p u8 frame -> normalised 3-plane tensor), fp16 vs bf16
usage: bench_bf16.py [--out profiles/bf16_bench.json] [--rounds 6] [--only tick,nv12,circular]"""
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


def _alternate(variants, rounds, reps):
    """variants: {name: (graph, steps per replay)} -> per variant the median / min / max us per step over `rounds` ABAB rounds"""
    import numpy as np
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (g, steps) in variants.items():
            res[k].append(_time_graph(g, reps) / steps)
    return {k: {"us": round(float(np.median(v)), 3), "min_us": round(float(np.min(v)), 3), "max_us": round(float(np.max(v)), 3)} for k, v in res.items()}


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


def ticks(dev, rounds):
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    M, N, FRAMES, K = 16, 50, 64, 8
    plane = 3 * W.DST[0] * W.DST[1]
    fw, fh = W.FRAME_4K
    frames = [W.random_u8_torch((fh, fw, 3), W.SEED + f, dev) for f in range(FRAMES)]
    crops = [W.random_crops(N, fw, fh, seed=W.SEED + 500000 + f) for f in range(FRAMES)]
    keep, names, outs, groups = [], {}, {}, {}
    types = {"f32": (torch.float32, cvgs.CV_32FC3, cvgs.CV_32FC1), "f16": (torch.float16, cvgs.CV_16FC3, cvgs.CV_16FC1),
             "bf16": (torch.bfloat16, cvgs.CV_16BFC3, cvgs.CV_16BFC1)}
    for kind, (dt, t3, t1) in types.items():
        out = torch.zeros((FRAMES, N, plane), dtype=dt, device=dev)  # one buffer per variant: the separate cast is ONE kernel per tick
        outs[kind] = out
        groups[kind] = []
        for g in range(FRAMES // M):
            chains = []
            for f in range(g * M, (g + 1) * M):
                o = cvgs.GpuMat.from_tensor(out[f], t1)
                ops = W.k1_chain(cvgs.GpuMat.from_tensor(frames[f], cvgs.CV_8UC3), crops[f], o)
                if kind != "f32":
                    ops = ops[:-1] + [cvgs.convertTo(cvgs.CV_32FC3, t3), cvgs.split(t3, o, W.DST)]
                tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).to(dev)
                keep.append(tab)
                ops[0].table = tab.data_ptr()
                chains.append(cvgs.lower(ops))
            names[kind] = cvgs.kernel_name(*ops)
            keep.append(chains)
            groups[kind].append(cvgs.pack_chains(chains))
    cast_dst = torch.empty((M, N, plane), dtype=torch.bfloat16, device=dev)

    def tick_fn(kind, cast=False):
        def fn():
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(K):
                g = i % len(groups[kind])
                capi.check(lib.cvgs_execute_many(groups[kind][g], M, s))
                if cast:
                    cast_dst.copy_(outs[kind][g * M:(g + 1) * M])  # fp32 -> bf16, round to nearest even
        return fn

    variants = {"f32": (_capture(tick_fn("f32")), K), "f16": (_capture(tick_fn("f16")), K), "bf16": (_capture(tick_fn("bf16")), K),
                "f32_then_cast": (_capture(tick_fn("f32", True)), K)}
    r = _alternate(variants, rounds, 20)
    r["kernels"] = names
    r["bf16_over_f16"] = round(r["bf16"]["us"] / r["f16"]["us"], 4)
    r["f32_over_bf16"] = round(r["f32"]["us"] / r["bf16"]["us"], 4)
    r["f32_then_cast_over_bf16"] = round(r["f32_then_cast"]["us"] / r["bf16"]["us"], 4)
    return r


def nv12(dev, rounds):
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    lib = capi.load_library()
    w, h, dst, F = 6144, 3456, (1280, 720), 4
    surf = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device=dev) for _ in range(F)]
    f = cvgs.CV_32FC3
    variants, names, keep = {}, {}, []
    for kind, t3, t1, dt in (("f16", cvgs.CV_16FC3, cvgs.CV_16FC1, torch.float16), ("bf16", cvgs.CV_16BFC3, cvgs.CV_16BFC1, torch.bfloat16)):
        out = torch.zeros((F, 3 * dst[0] * dst[1]), dtype=dt, device=dev)
        lowered = []
        for i in range(F):
            m = cvgs.GpuMat(h, w, cvgs.CV_8UC1, surf[i].data_ptr(), w, owner=surf[i])
            ops = [cvgs.read_nv12([m], dst, capi.YUV_LIMITED, capi.BT709, False), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
                   cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225]),
                   cvgs.convertTo(f, t3), cvgs.split(t3, cvgs.GpuMat.from_tensor(out[i:i + 1], t1), dst)]
            lowered.append(cvgs.lower(ops))
        names[kind] = cvgs.kernel_name(*ops)
        keep += [out, lowered]

        def fn(lowered=lowered):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(16):
                capi.check(lib.cvgs_execute(C.byref(lowered[i % F].desc), s))

        variants[kind] = (_capture(fn), 16)
    r = _alternate(variants, rounds, 20)
    r["kernels"] = names
    r["bf16_over_f16"] = round(r["bf16"]["us"] / r["f16"]["us"], 4)
    return r


def circular(dev, rounds):
    import torch
    from cvgpuspeedup_amd import cvgs
    W_, H_, B = 1920, 1080, 16
    frame = torch.randint(0, 256, (H_, W_, 3), dtype=torch.uint8, device=dev)
    f = cvgs.CV_32FC3
    variants, cts = {}, []
    for kind, e1, e3 in (("f16", cvgs.CV_16FC1, cvgs.CV_16FC3), ("bf16", cvgs.CV_16BFC1, cvgs.CV_16BFC3)):
        ct = cvgs.CircularTensor(cvgs.CV_8UC3, e1, 3, B, cvgs.NewestFirst, cvgs.Standard, W_, H_, capturable=True)
        cts.append(ct)
        pw = [cvgs.convertTo(cvgs.CV_8UC3, f), cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]),
              cvgs.divide(f, [0.229, 0.224, 0.225]), cvgs.convertTo(f, e3)]

        def fn(ct=ct, pw=pw, e3=e3):
            for _ in range(8):
                ct.update(torch.cuda.current_stream(), cvgs.GpuMat.from_tensor(frame, cvgs.CV_8UC3), *pw, ct.write_split(e3))

        variants[kind] = (_capture(fn), 8)
    r = _alternate(variants, rounds, 10)
    r["bf16_over_f16"] = round(r["bf16"]["us"] / r["f16"]["us"], 4)
    for ct in cts:
        ct.release()
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_bench.json"))
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--only", default="tick,nv12,circular")
    a = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds}
    for part, fn in (("tick", ticks), ("nv12", nv12), ("circular", circular)):
        if part in a.only.split(","):
            res[part] = fn(dev, a.rounds)
            print(part, json.dumps(res[part]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
