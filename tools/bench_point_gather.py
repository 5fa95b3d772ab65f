#!/usr/bin/env python3
"""cvgs_points_gather timed, in ONE GPU process, legs alternated ABAB.  Workload: a tick of 16 1080p frames, each with an 8,400-candidate
face head (cx, cy, w, h, score, 5 landmarks in the letterboxed 640 x 640 input) of which about 300 candidates are over the threshold
and 50 are kept; two variants: a bf16 channel-major [4 + 1 + 15, 8400] head (x, y, confidence per landmark) and an fp32 row-major
[8400, 4 + 1 + 10] head.  Per variant, under graph replay with HIP events around the replays:
  gather          (1) K cvgs_points_gather calls (16 frames each): the call alone
  torch_gather    (2b) the same gather spelled in framework indexing ops on the device (index through both lists, slice, cast, multiply,
                  add, mask the rows beyond the count)
  pipeline        (3) head -> cvgs_head_decode -> cvgs_boxes_select -> cvgs_points_gather -> cvgs_warp_tables_from_points -> the warp tick
                  (16 x 50 faces to [50, 3, 112, 112] fp32), one graph
and in wall clock (perf_counter around enqueue + synchronise, decode and select already done):
  device_path     gather -> warp tables -> warp tick, nothing leaves the device
  host_path       (2a) D2H of the two index lists, the count and the head (the host cannot gather without it), synchronise, a numpy
                  gather, H2D of the points, then warp tables -> warp tick
(1) and (2b) must write the same points; that is asserted before anything is timed.  No threshold is set: the figures and their
run-to-run spread are the result.
usage: bench_point_gather.py [--out profiles/point_gather_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_area_tick import _capture, _time_graph  # noqa: E402  (the protocol's two helpers)
from tools.bench_warp_tick import DIV, DST, MUL, SUB, TMPL5  # noqa: E402


def _head(np, rng, n, members, det):
    """float32 [n, 4 + 1 + 5 * 3]: clustered CXCYWH boxes in detector pixels, one score (`members` of them in [0.3, 1), the rest below
    0.2) and five landmarks (x, y, confidence): the face template placed in the box."""
    k = 60
    centres, sizes = rng.uniform(0.1 * det, 0.9 * det, (k, 2)), rng.uniform(det / 30, det / 6, (k, 2))
    which = rng.integers(0, k, n)
    head = np.zeros((n, 20), np.float32)
    head[:, 0:2] = centres[which] + rng.normal(0, det / 100, (n, 2))
    head[:, 2:4] = sizes[which] * rng.uniform(0.8, 1.25, (n, 2))
    head[:, 4] = rng.uniform(0.0, 0.2, n)
    head[rng.permutation(n)[:members], 4] = rng.uniform(0.3, 1.0, members)
    t = np.asarray(TMPL5, np.float32) / 112.0 - 0.5
    lm = head[:, None, 0:2] + t[None] * head[:, None, 2:4] + rng.normal(0, 0.5, (n, 5, 2))
    head[:, 5:] = np.concatenate([lm, rng.uniform(0.5, 1.0, (n, 5, 1))], axis=2).reshape(n, 15)
    return head


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_gather_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, MEMBERS, PRE_K, MAX_OUT, DET, K, THR, P = 16, 8400, 300, 1024, 50, 640, 4, 0.25, 5
    fw, fh = W.FRAME_1080P
    xform = cvgs.letterbox_xform((fw, fh), (DET, DET), cvgs.PRESERVE_AR)
    rng = np.random.default_rng(W.SEED)
    base = np.stack([_head(np, rng, N, MEMBERS, DET) for _ in range(M)])  # [M, N, 20] fp32
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
    s_boxes, s_count, s_index = z((M, MAX_OUT, 4), torch.float32), z((M, 64), torch.int32), z((M, MAX_OUT), torch.int32)
    points, points_t = z((M, MAX_OUT, P, 2), torch.float32), z((M, MAX_OUT, P, 2), torch.float32)
    tables = z((M, MAX_OUT, 64), torch.uint8)
    out = z((M, MAX_OUT, 3 * DST[0] * DST[1]), torch.float32)
    sdescs = (capi.BoxSelectDesc * M)(*[cvgs.box_select_desc((fw, fh), d_boxes[f], d_scores[f], N, s_scratch[f], s_boxes[f], s_count[f], THR, 0.45, PRE_K, MAX_OUT,
                                                             cvgs.CAND_CXCYWH_F32, 4, 1, d_classes[f], 1, d_count[f], xform, None, s_index[f]) for f in range(M)])
    wdescs = (capi.WarpTableDesc * M)(*[cvgs.warp_table_desc(mats[f], points[f], tables[f], MAX_OUT, DST, TMPL5, count=s_count[f]) for f in range(M)])
    f32 = cvgs.CV_32FC3
    chains = [cvgs.lower([cvgs.warp_table(cvgs.WARP_AFFINE, mats[f], tables[f], MAX_OUT, DST), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f32), cvgs.multiply(f32, MUL),
                          cvgs.subtract(f32, SUB), cvgs.divide(f32, DIV), cvgs.split_tensor(f32, out[f].data_ptr(), DST[0], DST[1], MAX_OUT, keep=out)]) for f in range(M)]
    tick = cvgs.pack_chains(chains)
    sxy = torch.tensor([xform[0], xform[1]], dtype=torch.float32, device=dev)
    oxy = torch.tensor([xform[2], xform[3]], dtype=torch.float32, device=dev)
    rows = torch.arange(MAX_OUT, device=dev)[None, :]
    fidx = torch.arange(M, device=dev)[:, None]
    nan = torch.tensor(float("nan"), dtype=torch.float32, device=dev)
    res = {"workload": "16 1080p frames x 8400-candidate face heads (box, score, 5 landmarks), ~300 over the score threshold 0.25, pre_nms_k 1024, max_out 50; "
                       "warp tick: 16 x 50 five-landmark similarity crops -> [50,3,112,112] fp32; us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "variants": {}}
    for name, dtype, elem, channel_major in (("bf16_channel_major_xyc", torch.bfloat16, cvgs.HEAD_BF16, True), ("fp32_row_major_xy", torch.float32, cvgs.HEAD_F32, False)):
        step, A = (3, 20) if channel_major else (2, 15)
        vals = base if channel_major else np.concatenate([base[:, :, :5], base[:, :, 5:].reshape(M, N, 5, 3)[:, :, :, :2].reshape(M, N, 10)], axis=2)
        t = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
        head = (t.transpose(1, 2) if channel_major else t).to(dtype).contiguous()  # [M, A, N] or [M, N, A]
        cs, as_ = (1, N) if channel_major else (A, 1)
        hdescs = (capi.HeadDesc * M)(*[cvgs.head_desc(head[f], elem, N, cs, as_, 1, THR, scratch[f], d_boxes[f], d_scores[f], d_classes[f], d_count[f], d_index[f])
                                       for f in range(M)])
        gdescs = (capi.PointGatherDesc * M)(*[cvgs.point_gather_desc(head[f], elem, N, cs, as_, 5, step, P, MAX_OUT, s_index[f], points[f], s_count[f], d_index[f], xform)
                                              for f in range(M)])

        def gather_fn():
            for _ in range(K):
                capi.check(lib.cvgs_points_gather(gdescs, M, stream()))

        def torch_once():
            c = torch.gather(d_index, 1, s_index.clamp(min=0).long()).clamp(min=0).long()  # [M, MAX_OUT] raw candidates
            cand = (head.transpose(1, 2) if channel_major else head)[fidx, c]               # [M, MAX_OUT, A]
            xy = cand[:, :, 5:5 + P * step].reshape(M, MAX_OUT, P, step)[..., :2].float()
            xy = xy * sxy
            xy = xy + oxy
            points_t.copy_(torch.where((rows < s_count[:, :1])[:, :, None, None], xy, nan))

        def torch_fn():
            for _ in range(K):
                torch_once()

        def pipeline_fn():
            for _ in range(K):
                capi.check(lib.cvgs_head_decode(hdescs, M, stream()))
                capi.check(lib.cvgs_boxes_select(sdescs, M, stream()))
                capi.check(lib.cvgs_points_gather(gdescs, M, stream()))
                capi.check(lib.cvgs_warp_tables_from_points(wdescs, M, stream()))
                capi.check(lib.cvgs_execute_many(tick, M, stream()))

        def tail():
            capi.check(lib.cvgs_warp_tables_from_points(wdescs, M, stream()))
            capi.check(lib.cvgs_execute_many(tick, M, stream()))

        def device_path():
            capi.check(lib.cvgs_points_gather(gdescs, M, stream()))
            tail()
            torch.cuda.synchronize()

        def host_path():
            si, sc, di, hh = s_index.cpu(), s_count[:, 0].cpu(), d_index.cpu(), head.cpu()  # (each .cpu() synchronises)
            si, sc, di = si.numpy(), sc.numpy(), di.numpy()
            hv = (hh.float() if dtype == torch.bfloat16 else hh).numpy()
            pts = np.full((M, MAX_OUT, P, 2), np.nan, np.float32)
            for f in range(M):
                k = int(sc[f])
                c = di[f][si[f][:k]]
                cand = hv[f][:, c].T if channel_major else hv[f][c]
                xy = cand[:, 5:5 + P * step].reshape(k, P, step)[..., :2]
                pts[f, :k] = xy * np.float32([xform[0], xform[1]]) + np.float32([xform[2], xform[3]])
            points.copy_(torch.from_numpy(pts))
            tail()
            torch.cuda.synchronize()

        # the pipeline once; then (1) and (2b) write the same points
        pipeline_fn()
        torch.cuda.synchronize()
        note = lib.cvgs_last_error().decode()
        assert note.startswith("tick:"), "the warp tick did not fuse: %s" % note
        kept = [int(x) for x in s_count[:, 0].cpu()]
        want_out = out.clone()
        torch_once()
        torch.cuda.synchronize()
        same = torch.equal(points.view(torch.int32)[~torch.isnan(points)], points_t.view(torch.int32)[~torch.isnan(points_t)]) and torch.equal(torch.isnan(points), torch.isnan(points_t))
        assert same, "%s: the framework gather's points differ from cvgs_points_gather's" % name
        host_path()
        assert torch.equal(out, want_out), "%s: the host path's tensors differ from the device path's" % name
        graphs = {"gather": _capture(gather_fn), "torch_gather": _capture(torch_fn), "pipeline": _capture(pipeline_fn)}
        per = {k: [] for k in list(graphs) + ["device_path_wall", "host_path_wall"]}
        for _ in range(a.rounds):  # ABAB: every round times every leg once
            for k, g in graphs.items():
                per[k].append(_time_graph(g, a.reps) / K)
            for k, fn in (("device_path_wall", device_path), ("host_path_wall", host_path)):
                fn()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                per[k].append((time.perf_counter() - t0) * 1e6 / a.reps)
        v = {"head_bytes": int(head.numel() * head.element_size()), "members_per_frame": [int(x) for x in d_count[:, 0].cpu()], "kept_per_frame": kept}
        for k, ts in per.items():
            v[k] = {"us": round(float(np.median(ts)), 3), "min_us": round(float(np.min(ts)), 3), "max_us": round(float(np.max(ts)), 3),
                    "legs_us": [round(float(x), 3) for x in ts]}
        v["torch_gather_over_gather"] = round(v["torch_gather"]["us"] / v["gather"]["us"], 3)
        v["host_path_over_device_path_wall"] = round(v["host_path_wall"]["us"] / v["device_path_wall"]["us"], 3)
        res["variants"][name] = v
        print(json.dumps({name: {k: (x["us"] if isinstance(x, dict) else x) for k, x in v.items() if k not in ("members_per_frame", "kept_per_frame")}}), flush=True)
        del graphs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
