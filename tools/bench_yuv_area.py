#!/usr/bin/env python3
"""INTER_AREA of NV12 decoder surfaces in ONE launch (CVGS_READ_NV12_RESIZE_AREA), in ONE GPU process, variants alternated ABAB on a rotating
set of resident surfaces that is larger than the Infinity Cache, the launches of one pass over the set captured into a HIP graph per variant.
Two shapes:
  cfg3    a 6K NV12 surface (6144 x 3456) -> BGR -> 1280 x 720 -> normalize -> planar fp32 (BASELINE cfg #3)
  crops   50 crops (w 32..512, h 64..1024, even) of a 4K NV12 surface -> BGR -> 64 x 128 -> normalize -> planar fp32 (the decode-side tick shape)
Three variants each:
  area      read_nv12(..., interp=INTER_AREA) -> program -> split: the new chain (yuv_area_c3_swap_mul_sub_div)
  linear    the same chain through the bilinear kind (K4): 2 x 2 taps per output pixel, most of the surface never read
  two_pass  what the new chain replaces: the whole surface NV12 -> packed CV_8UC3 (per-pixel read), then CVGS_READ_RESIZE_AREA over the
            packed picture -- two launches, the packed picture written and read in between
The time of `area` is read against its own algorithmic bytes (every byte of every view once + the tensor) over the copy ceiling measured
in the same process, not against `linear`, which reads a fraction of the surface.
usage: bench_yuv_area.py [--out profiles/yuv_area_bench.json] [--rounds 6]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bf16 import _alternate, _capture  # noqa: E402


def _even_crops(n, w, h, seed):
    from cvgpuspeedup_amd import workloads as W
    out = []
    for (x, y, cw, ch) in W.random_crops(n, w, h, seed=seed):
        out.append((x & ~1, y & ~1, max(cw & ~1, 2), max(ch & ~1, 2)))
    return out


def shape(lib, dev, name, size, dsize, n_surfaces, crops_of, rounds):
    """One shape: {variant: us per surface}, kernel names and the new chain's algorithmic bytes."""
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    sw, sh = size
    dw, dh = dsize
    f3 = cvgs.CV_32FC3
    surf = [torch.randint(0, 256, (sh * 3 // 2, sw), dtype=torch.uint8, device=dev) for _ in range(n_surfaces)]
    n_rgb = max(2, (W.LLC_BYTES * 5 // 4) // (sw * sh * 3) + 1)  # the packed pictures of the two-pass route rotate past the cache too
    rgb = [torch.zeros((sh, sw * 3), dtype=torch.uint8, device=dev) for _ in range(n_rgb)]
    keep, names, variants = [surf, rgb], {}, {}

    def tail(rd, out, batch):
        return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f3), cvgs.multiply(f3, [W.K1_ALPHA] * 3), cvgs.subtract(f3, W.K1_SUB[3]),
                cvgs.divide(f3, W.K1_DIV[3]), cvgs.split(f3, cvgs.GpuMat(batch, 3 * dw * dh, cvgs.CV_32FC1, out.data_ptr(), 3 * dw * dh * 4, owner=out), (dw, dh))]

    algo = 0
    for kind in ("area", "linear", "two_pass"):
        lowered = []
        for i in range(n_surfaces):
            crops = crops_of(i)
            batch = len(crops)
            out = torch.zeros((batch, 3 * dw * dh), dtype=torch.float32, device=dev)
            keep.append(out)
            m = cvgs.GpuMat(sh, sw, cvgs.CV_8UC1, surf[i].data_ptr(), sw, owner=surf[i])
            if kind == "two_pass":
                pic = rgb[i % n_rgb]
                img = cvgs.GpuMat(sh, sw, cvgs.CV_8UC3, pic.data_ptr(), sw * 3, owner=pic)
                first = [cvgs.read_nv12(m, None, capi.YUV_LIMITED, capi.BT709, False), cvgs.convertTo(f3, cvgs.CV_8UC3), cvgs.write(cvgs.CV_8UC3, img)]
                second = tail(cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_AREA, [img.roi(*c) for c in crops], (dw, dh)), out, batch)
                lowered.append((cvgs.lower(first), cvgs.lower(second)))
                names[kind] = [cvgs.kernel_name(*first), cvgs.kernel_name(*second)]
            else:
                interp = cvgs.INTER_AREA if kind == "area" else cvgs.INTER_LINEAR
                ops = tail(cvgs.read_nv12([m.nv12_roi(*c) for c in crops], (dw, dh), capi.YUV_LIMITED, capi.BT709, False, interp=interp), out, batch)
                lowered.append((cvgs.lower(ops),))
                names[kind] = cvgs.kernel_name(*ops)
                if kind == "area":
                    algo += sum(c[2] * c[3] * 3 // 2 for c in crops) + batch * 3 * dw * dh * 4
        keep.append(lowered)

        def fn(lowered=lowered):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for chains in lowered:
                for low in chains:
                    capi.check(lib.cvgs_execute(C.byref(low.desc), s))

        variants[kind] = (_capture(fn), n_surfaces)
    r = _alternate(variants, rounds, 10)
    return {"workload": name, "surfaces": n_surfaces, "kernels": names, "us": r, "algorithmic_bytes_per_surface": algo // n_surfaces,
            "area_over_two_pass": round(r["area"]["us"] / r["two_pass"]["us"], 4), "area_over_linear": round(r["area"]["us"] / r["linear"]["us"], 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_area_bench.json"))
    p.add_argument("--rounds", type=int, default=6)
    a = p.parse_args()
    import torch
    from bench import copy_ceiling
    from cvgpuspeedup_amd import capi
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    ceiling = copy_ceiling(dev)  # GB/s, read + write bytes
    res = {"copy_ceiling_GBps": ceiling, "rounds": a.rounds, "shapes": {}}
    whole6k = [(0, 0) + W.FRAME_6K]
    res["shapes"]["cfg3"] = shape(lib, dev, "6K NV12 (BT.709 limited) -> BGR -> 1280 x 720 -> normalize -> planar fp32, one surface per launch",
                                  W.FRAME_6K, (1280, 720), 10, lambda i: whole6k, a.rounds)
    res["shapes"]["crops"] = shape(lib, dev, "50 crops of a 4K NV12 surface (BT.709 limited) -> BGR -> 64 x 128 -> normalize -> planar fp32, one surface per launch",
                                   W.FRAME_4K, W.DST, 24, lambda i: _even_crops(50, W.FRAME_4K[0], W.FRAME_4K[1], W.SEED + 700000 + i), a.rounds)
    for s in res["shapes"].values():
        if ceiling:
            s["copy_ceiling_us"] = round(s["algorithmic_bytes_per_surface"] / (ceiling * 1e3), 3)
            s["area_fraction_of_copy_ceiling"] = round(s["copy_ceiling_us"] / s["us"]["area"]["us"], 4)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
