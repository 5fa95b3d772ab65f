#!/usr/bin/env python3
"""A 4K NV12 surface -> a 1080p NV12 surface in ONE launch (CVGS_WRITE_NV12), in ONE GPU process, variants alternated ABAB on a rotating set
of resident surfaces, 16 launches captured into a HIP graph per variant:
  nv12_fast      resize(read_nv12) -> write_nv12: the fast kernel (nv12w_nv12_resize)
  nv12_interp    the same chain with CVGS_CHAIN_FORCE_GENERIC: the interpreted kernel (nv12w_interp)
  packed_u8c3    the chain this one replaces the first half of: the same read written as a packed CV_8UC3 image
                 (resize(read_nv12) -> cvtColor<RGB2BGR> -> convertTo<CV_32FC3, CV_8UC3> -> write), twice the store bytes
BT.601 limited in, BT.709 limited out.  The roofline figure is the new chain's algorithmic bytes (the 4K surface read once + the 1080p
surface written once) over 8 TB/s.
usage: bench_nv12_write.py [--out profiles/nv12_write_bench.json] [--rounds 6]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bf16 import _alternate, _capture  # noqa: E402

HBM_BYTES_PER_US = 8.0e6  # 8 TB/s


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "nv12_write_bench.json"))
    p.add_argument("--rounds", type=int, default=6)
    a = p.parse_args()
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    (sw, sh), (dw, dh), F, K = (3840, 2160), (1920, 1080), 8, 16
    surf = [torch.randint(0, 256, (sh * 3 // 2, sw), dtype=torch.uint8, device=dev) for _ in range(F)]
    f3 = cvgs.CV_32FC3
    variants, names, keep = {}, {}, []
    for kind in ("nv12_fast", "nv12_interp", "packed_u8c3"):
        lowered = []
        for i in range(F):
            m = cvgs.GpuMat(sh, sw, cvgs.CV_8UC1, surf[i].data_ptr(), sw, owner=surf[i])
            rd = cvgs.read_nv12([m], (dw, dh), capi.YUV_LIMITED, capi.BT601, False)
            if kind == "packed_u8c3":
                out = torch.zeros((dh, dw * 3), dtype=torch.uint8, device=dev)
                ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f3), cvgs.convertTo(f3, cvgs.CV_8UC3), cvgs.write(cvgs.CV_8UC3, cvgs.GpuMat(dh, dw, cvgs.CV_8UC3, out.data_ptr(), dw * 3, owner=out))]
                flags = 0
            else:
                out = torch.zeros((dh * 3 // 2, dw), dtype=torch.uint8, device=dev)
                ops = [rd, cvgs.write_nv12(cvgs.GpuMat(dh, dw, cvgs.CV_8UC1, out.data_ptr(), dw, owner=out), capi.YUV_LIMITED, capi.BT709)]
                flags = capi.CHAIN_FORCE_GENERIC if kind == "nv12_interp" else 0
            keep.append(out)
            lowered.append(cvgs.lower(ops, flags))
        names[kind] = cvgs.kernel_name(*ops, flags=flags)
        keep.append(lowered)

        def fn(lowered=lowered):
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(K):
                capi.check(lib.cvgs_execute(C.byref(lowered[i % F].desc), s))

        variants[kind] = (_capture(fn), K)
    r = _alternate(variants, a.rounds, 20)
    algo = sw * sh * 3 // 2 + dw * dh * 3 // 2
    res = {"workload": "4K NV12 (BT.601 limited) -> 1080p NV12 (BT.709 limited), one launch per surface, %d resident surfaces, %d launches per graph" % (F, K),
           "rounds": a.rounds, "kernels": names, "us": r,
           "algorithmic_bytes": algo, "roofline_us_at_8TBs": round(algo / HBM_BYTES_PER_US, 3),
           "roofline_fraction_nv12_fast": round(algo / HBM_BYTES_PER_US / r["nv12_fast"]["us"], 4),
           "nv12_fast_over_packed_u8c3": round(r["nv12_fast"]["us"] / r["packed_u8c3"]["us"], 4),
           "nv12_interp_over_nv12_fast": round(r["nv12_interp"]["us"] / r["nv12_fast"]["us"], 4)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
