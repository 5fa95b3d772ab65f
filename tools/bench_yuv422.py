#!/usr/bin/env python3
"""Packed 4:2:2 (YUYV) reads against their NV12 twins, in ONE GPU process, variants alternated ABAB, graph-replayed:
  tick   16 surfaces x 50 crops of 4K -> [50,3,128,64] per surface through cvgs_execute_many (host descriptors inside the kernel
         arguments), K ticks captured into a HIP graph on a rotation of resident surfaces: YUYV vs NV12 (the same crops, even
         x / y / width / height so that both layouts can express them), fp32 and bf16 tensors
         and "before": a YUYV -> BGR conversion with plain torch ops into BGR frames + the existing K1 tick on them (the pass the
         feature removes)
  frame  cfg #3: a whole 6K surface -> 1280 x 720 planar fp32 tensor, one launch per surface: YUYV vs NV12
The yardstick is the NV12 twin measured in the same run.  A 4:2:2 surface holds 2 B per pixel against 1.5: R = (touched 128-byte-line
bytes of the YUYV crops + tensor bytes) / (the same for NV12), from workloads' sector census, is what the YUYV tick may cost more.
The rotations are sized by workloads.rotation_units from the bytes a launch touches on the read side.
usage: bench_yuv422.py [--out profiles/yuv422_bench.json] [--rounds 6] [--only tick,frame]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bf16 import _alternate, _capture  # noqa: E402


def yuyv_touched(crops, surf_w, surf_h, dst, sector):
    """workloads' sector census for crops of ONE packed 4:2:2 surface: a pixel's luma and the chroma of its pair sit in one 4-byte pixel
    pair, so the census of 2-byte pixels in rows of 2 * surf_w bytes counts them (the same function K1's frames are counted with)."""
    from cvgpuspeedup_amd import workloads as W
    return W.k1_sector_read_bytes(crops, surf_w, surf_h, dst, px_bytes=2, sector=sector, step=2 * surf_w)


def ticks(dev, rounds, before=True):
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    M, N, K = 16, 50, 8
    dst = W.DST
    plane = 3 * dst[0] * dst[1]
    fw, fh = W.FRAME_4K
    f = cvgs.CV_32FC3
    c8u2 = cvgs.make_type(cvgs.DEPTH_8U, 2)
    mk_crops = lambda fr: [(x & ~1, y & ~1, max(4, w & ~1), max(4, h & ~1)) for x, y, w, h in W.random_crops(N, fw, fh, seed=W.SEED + 500000 + fr)]
    # rotation: sized from the bytes a launch TOUCHES on the read side (64-byte sectors), by the variant that touches least
    sample = [mk_crops(fr) for fr in range(8)]
    touched = {"yuyv": sum(yuyv_touched(c, fw, fh, dst, 64) for c in sample) / len(sample),
               "nv12": sum(W.nv12_crops_sector_read_bytes(c, fw, fh, dst, 1, 64) for c in sample) / len(sample)}
    FRAMES = -(-W.rotation_units(min(touched.values())) // M) * M
    crops = [mk_crops(fr) for fr in range(FRAMES)]
    surf = {"yuyv": [torch.randint(0, 256, (fh, fw, 2), dtype=torch.uint8, device=dev) for _ in range(FRAMES)],
            "nv12": [torch.randint(0, 256, (fh * 3 // 2, fw), dtype=torch.uint8, device=dev) for _ in range(FRAMES)]}
    keep, names, groups = [], {}, {}
    norm = lambda: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225])]
    for lay in ("yuyv", "nv12"):
        for kind, dt, t3, t1 in (("f32", torch.float32, cvgs.CV_32FC3, cvgs.CV_32FC1), ("bf16", torch.bfloat16, cvgs.CV_16BFC3, cvgs.CV_16BFC1)):
            out = torch.zeros((FRAMES, N, plane), dtype=dt, device=dev)
            key = lay + "_" + kind
            groups[key] = []
            for g in range(FRAMES // M):
                chains = []
                for fr in range(g * M, (g + 1) * M):
                    s = surf[lay][fr]
                    if lay == "yuyv":
                        m = cvgs.GpuMat(fh, fw, c8u2, s.data_ptr(), 2 * fw, owner=s)
                        rd = cvgs.read_yuv422([m.yuv422_roi(*c) for c in crops[fr]], dst, capi.YUV_LIMITED, capi.BT709, False)
                    else:
                        m = cvgs.GpuMat(fh, fw, cvgs.CV_8UC1, s.data_ptr(), fw, owner=s)
                        rd = cvgs.read_nv12([m.nv12_roi(*c) for c in crops[fr]], dst, capi.YUV_LIMITED, capi.BT709, False)
                    ops = [rd] + norm()
                    if kind == "bf16":
                        ops.append(cvgs.convertTo(f, t3))
                    ops.append(cvgs.split(t3, cvgs.GpuMat.from_tensor(out[fr], t1), dst))
                    chains.append(cvgs.lower(ops))
                names[key] = cvgs.kernel_name(*ops)
                keep += [chains, out]
                groups[key].append(cvgs.pack_chains(chains))

    def tick_fn(key):
        def fn():
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(K):
                capi.check(lib.cvgs_execute_many(groups[key][i % len(groups[key])], M, s))
        return fn

    variants = {k: (_capture(tick_fn(k)), K) for k in groups}
    if before:
        # what a 4:2:2 caller pays without the feature: a YUYV -> BGR conversion pass (plain torch ops, limited-range BT.709) into BGR
        # frames, then the existing K1 tick on those frames
        bgr = torch.zeros((M, fh, fw, 3), dtype=torch.uint8, device=dev)
        out_b = torch.zeros((M, N, plane), dtype=torch.float32, device=dev)
        stacked = [torch.stack(surf["yuyv"][g * M:(g + 1) * M]) for g in range(FRAMES // M)]
        k1_groups = []
        for g in range(FRAMES // M):
            chains = []
            for i in range(M):
                ops = W.k1_chain(cvgs.GpuMat.from_tensor(bgr[i], cvgs.CV_8UC3), crops[g * M + i], cvgs.GpuMat.from_tensor(out_b[i], cvgs.CV_32FC1))
                chains.append(cvgs.lower(ops))
            names["before_k1"] = cvgs.kernel_name(*ops)
            keep.append(chains)
            k1_groups.append(cvgs.pack_chains(chains))

        def convert(s):
            y = (s[..., 0].float() - 16.0) * 1.164383
            cb = s[:, :, 0::2, 1].float().repeat_interleave(2, dim=2) - 128.0
            cr = s[:, :, 1::2, 1].float().repeat_interleave(2, dim=2) - 128.0
            bgr[..., 0] = (y + 2.112402 * cb).clamp_(0, 255)
            bgr[..., 1] = (y - 0.213249 * cb - 0.532909 * cr).clamp_(0, 255)
            bgr[..., 2] = (y + 1.792741 * cr).clamp_(0, 255)

        def before_fn():
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(2):
                g = i % len(k1_groups)
                convert(stacked[g])
                capi.check(lib.cvgs_execute_many(k1_groups[g], M, s))

        variants["before_torch_convert_then_k1"] = (_capture(before_fn), 2)
    r = _alternate(variants, rounds, 20)
    r["kernels"] = names
    r["rotation"] = {"surfaces": FRAMES, "yuyv": W.residency(FRAMES, touched["yuyv"], N * plane * 4), "nv12": W.residency(FRAMES, touched["nv12"], N * plane * 4)}
    for kind, esz in (("f32", 4), ("bf16", 2)):
        tensor = M * N * plane * esz
        ty = sum(yuyv_touched(crops[fr], fw, fh, dst, 128) for fr in range(M)) + tensor
        tn = sum(W.nv12_crops_sector_read_bytes(crops[fr], fw, fh, dst, 1, 128) for fr in range(M)) + tensor
        r["R_" + kind] = round(ty / tn, 4)  # touched 128-byte-line bytes + tensor bytes, YUYV over NV12
        r["yuyv_over_nv12_" + kind] = round(r["yuyv_" + kind]["us"] / r["nv12_" + kind]["us"], 4)
        r["within_R_plus_5pct_" + kind] = bool(r["yuyv_" + kind]["us"] <= r["R_" + kind] * r["nv12_" + kind]["us"] * 1.05)
    return r


def frame(dev, rounds):
    """cfg #3.  NV12 whole frames take K4's two-pixels-per-lane form (k4_nv12_x2); the 4:2:2 family has no such form yet, so the ratio here
    compares kernels of different shapes as well as 2 B against 1.5 B per pixel."""
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    w, h, dst = 6144, 3456, (1280, 720)
    f = cvgs.CV_32FC3
    touched = {"yuyv": yuyv_touched([(0, 0, w, h)], w, h, dst, 64), "nv12": W.nv12_sector_read_bytes(w, h, dst[0], dst[1])}
    F = W.rotation_units(min(touched.values()))
    variants, names, keep = {}, {}, []
    for lay in ("yuyv", "nv12"):
        out = torch.zeros((F, 3 * dst[0] * dst[1]), dtype=torch.float32, device=dev)
        lowered = []
        for i in range(F):
            if lay == "yuyv":
                s = torch.randint(0, 256, (h, w, 2), dtype=torch.uint8, device=dev)
                rd = cvgs.read_yuv422([cvgs.GpuMat(h, w, cvgs.make_type(cvgs.DEPTH_8U, 2), s.data_ptr(), 2 * w, owner=s)], dst, capi.YUV_LIMITED, capi.BT709, False)
            else:
                s = torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device=dev)
                rd = cvgs.read_nv12([cvgs.GpuMat(h, w, cvgs.CV_8UC1, s.data_ptr(), w, owner=s)], dst, capi.YUV_LIMITED, capi.BT709, False)
            ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]),
                   cvgs.divide(f, [0.229, 0.224, 0.225]), cvgs.split(f, cvgs.GpuMat.from_tensor(out[i:i + 1], cvgs.CV_32FC1), dst)]
            lowered.append(cvgs.lower(ops))
            keep.append(s)
        names[lay] = cvgs.kernel_name(*ops)
        keep += [out, lowered]

        def fn(lowered=lowered):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(F):
                capi.check(lib.cvgs_execute(C.byref(lowered[i].desc), s))

        variants[lay] = (_capture(fn), F)
    r = _alternate(variants, rounds, 8)
    r["kernels"] = names
    r["rotation"] = {"surfaces": F, "yuyv": W.residency(F, touched["yuyv"], 3 * dst[0] * dst[1] * 4), "nv12": W.residency(F, touched["nv12"], 3 * dst[0] * dst[1] * 4)}
    r["yuyv_over_nv12"] = round(r["yuyv"]["us"] / r["nv12"]["us"], 4)
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv422_bench.json"))
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--only", default="tick,frame")
    a = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds}
    for part, fn in (("tick", ticks), ("frame", frame)):
        if part in a.only.split(","):
            res[part] = fn(dev, a.rounds)
            print(part, json.dumps(res[part]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
