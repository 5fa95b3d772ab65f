#!/usr/bin/env python3
"""Planar 4:4:4 (I444) reads against their NV12 twins and against the pass the feature removes, in ONE GPU process, variants alternated
ABAB, graph-replayed:
  tick   16 surfaces x 50 crops of 4K -> [50,3,128,64] per surface through cvgs_execute_many (host descriptors inside the kernel
         arguments), K ticks captured into a HIP graph on a rotation of resident surfaces:
           (a) the I444 tick, fp32 and bf16 tensors;
           (b) its NV12 twin on a 4:2:0 version of the same pictures (the same crops, even x / y / width / height so that both
               layouts can express them);
           (c) "before": an I444 -> packed BGR u8 conversion with plain torch ops + the existing K1 tick on those frames.
Expectation from the byte counts: (a) reads 3 B per source pixel where (b) reads 1.5 B and issues six tap loads where K4 issues four,
so (a) sits above (b); R = (touched 128-byte-line bytes of the I444 crops + tensor bytes) / (the same for NV12), from workloads' sector
census.  The requirement is that (a) is faster than (c).  The rotations are sized by workloads.rotation_units from the bytes a launch
touches on the read side.
usage: bench_yuv444.py [--out profiles/yuv444_bench.json] [--rounds 6]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bf16 import _alternate, _capture  # noqa: E402


def i444_touched(crops, surf_w, surf_h, dst, sector):
    """workloads' sector census for crops of ONE planar 4:4:4 surface: three planes of 1-byte samples, each tapped like a 1-byte frame."""
    from cvgpuspeedup_amd import workloads as W
    return 3 * W.k1_sector_read_bytes(crops, surf_w, surf_h, dst, px_bytes=1, sector=sector, step=surf_w)


def nv12_of(t):
    """The NV12 surface ((H * 3 / 2, W) u8) of a [3, H, W] picture: luma as it is, chroma sample (2y, 2x) of every 2 x 2 block."""
    import torch
    _, h, w = t.shape
    nv = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=t.device)
    nv[:h] = t[0]
    nv[h:, 0::2] = t[1, 0::2, 0::2]
    nv[h:, 1::2] = t[2, 0::2, 0::2]
    return nv


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
    mk_crops = lambda fr: [(x & ~1, y & ~1, max(4, w & ~1), max(4, h & ~1)) for x, y, w, h in W.random_crops(N, fw, fh, seed=W.SEED + 500000 + fr)]
    # rotation: sized from the bytes a launch TOUCHES on the read side (64-byte sectors), by the variant that touches least
    sample = [mk_crops(fr) for fr in range(8)]
    touched = {"i444": sum(i444_touched(c, fw, fh, dst, 64) for c in sample) / len(sample),
               "nv12": sum(W.nv12_crops_sector_read_bytes(c, fw, fh, dst, 1, 64) for c in sample) / len(sample)}
    FRAMES = -(-W.rotation_units(min(touched.values())) // M) * M
    crops = [mk_crops(fr) for fr in range(FRAMES)]
    surf = {"i444": [torch.randint(0, 256, (3, fh, fw), dtype=torch.uint8, device=dev) for _ in range(FRAMES)]}
    surf["nv12"] = [nv12_of(s) for s in surf["i444"]]  # the same pictures, chroma subsampled 2 x 2
    keep, names, groups = [], {}, {}
    norm = lambda: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225])]
    for lay in ("i444", "nv12"):
        for kind, dt, t3, t1 in (("f32", torch.float32, cvgs.CV_32FC3, cvgs.CV_32FC1), ("bf16", torch.bfloat16, cvgs.CV_16BFC3, cvgs.CV_16BFC1)):
            out = torch.zeros((FRAMES, N, plane), dtype=dt, device=dev)
            key = lay + "_" + kind
            groups[key] = []
            for g in range(FRAMES // M):
                chains = []
                for fr in range(g * M, (g + 1) * M):
                    s = surf[lay][fr]
                    if lay == "i444":
                        m = cvgs.GpuMat.from_yuv444_tensor(s)
                        rd = cvgs.read_yuv444([m.yuv444_roi(*c) for c in crops[fr]], dst, capi.YUV_LIMITED, capi.BT709, False)
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
        # what a 4:4:4 caller pays without the feature: an I444 -> BGR conversion pass (plain torch ops, limited-range BT.709) into packed
        # BGR u8 frames, then the existing K1 tick on those frames
        bgr = torch.zeros((M, fh, fw, 3), dtype=torch.uint8, device=dev)
        out_b = torch.zeros((M, N, plane), dtype=torch.float32, device=dev)
        stacked = [torch.stack(surf["i444"][g * M:(g + 1) * M]) for g in range(FRAMES // M)]
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
            y = (s[:, 0].float() - 16.0) * 1.164383
            cb = s[:, 1].float() - 128.0
            cr = s[:, 2].float() - 128.0
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
    r["rotation"] = {"surfaces": FRAMES, "i444": W.residency(FRAMES, touched["i444"], N * plane * 4), "nv12": W.residency(FRAMES, touched["nv12"], N * plane * 4)}
    for kind, esz in (("f32", 4), ("bf16", 2)):
        tensor = M * N * plane * esz
        ty = sum(i444_touched(crops[fr], fw, fh, dst, 128) for fr in range(M)) + tensor
        tn = sum(W.nv12_crops_sector_read_bytes(crops[fr], fw, fh, dst, 1, 128) for fr in range(M)) + tensor
        r["R_" + kind] = round(ty / tn, 4)  # touched 128-byte-line bytes + tensor bytes, I444 over NV12
        r["i444_over_nv12_" + kind] = round(r["i444_" + kind]["us"] / r["nv12_" + kind]["us"], 4)
    if before:
        r["i444_over_before_f32"] = round(r["i444_f32"]["us"] / r["before_torch_convert_then_k1"]["us"], 4)
        r["i444_faster_than_before"] = bool(r["i444_f32"]["us"] < r["before_torch_convert_then_k1"]["us"])
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv444_bench.json"))
    p.add_argument("--rounds", type=int, default=6)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv444.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "tick": ticks(dev, a.rounds)}
    print("tick", json.dumps(res["tick"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
