#!/usr/bin/env python3
"""cvgs_head_decode timed, in ONE GPU process, under graph replay, legs alternated ABAB.  Workload: a tick of 16 frames, each with a
(4 + 80) x 8,400 detector head (cx, cy, w, h, 80 class probabilities in the letterboxed 640 x 640 input) of which about 300 candidates
have a class score over the threshold; four variants: bf16 / fp32 x channel-major [84, 8400] / row-major [8400, 84].  Per variant:
  decode          (a) K cvgs_head_decode calls (16 frames each) captured in a HIP graph, HIP events around the replays: the call alone
  decode_select   (b) decode + cvgs_boxes_select over the decoder's outputs and device count (pre_nms_k 1024, max_out 50)
  torch_select    (c) the path replaced: the framework ops that produce dense fp32 boxes, scores and classes (cast, max with indices,
                  transpose / make contiguous, class to int32), then cvgs_boxes_select over all 8,400 candidates
  copy            (d) a plain device copy of the 16 heads' bytes, in the same run: the copy ceiling for (a)
(b) and (c) must select the same boxes; that is asserted before anything is timed.  No threshold is set: the figures and their
run-to-run spread are the result.
usage: bench_head_decode.py [--out profiles/head_decode_bench.json] [--rounds 8] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_area_tick import _capture, _time_graph  # noqa: E402  (the protocol's two helpers)


def _head(np, rng, n, nc, members, det):
    """float32 [n, 4 + nc]: clustered CXCYWH boxes in detector pixels; class scores in [0, 0.2), `members` candidates with one in [0.3, 1)."""
    k = 40
    centres, sizes = rng.uniform(0.1 * det, 0.9 * det, (k, 2)), rng.uniform(det / 30, det / 5, (k, 2))
    which = rng.integers(0, k, n)
    head = np.zeros((n, 4 + nc), np.float32)
    head[:, 0:2] = centres[which] + rng.normal(0, det / 100, (n, 2))
    head[:, 2:4] = sizes[which] * rng.uniform(0.8, 1.25, (n, 2))
    head[:, 4:] = rng.uniform(0.0, 0.2, (n, nc))
    rows = rng.permutation(n)[:members]
    head[rows, 4 + rng.integers(0, nc, members)] = rng.uniform(0.3, 1.0, members)
    return head


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_decode_bench.json"))
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    import numpy as np
    import torch
    from cvgpuspeedup_amd import capi, cvgs
    from cvgpuspeedup_amd import workloads as W
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    M, N, NC, MEMBERS, PRE_K, MAX_OUT, DET, K, THR = 16, 8400, 80, 300, 1024, 50, 640, 4, 0.25
    A = 4 + NC
    fw, fh = W.FRAME_1080P
    xform = cvgs.letterbox_xform((fw, fh), (DET, DET), cvgs.PRESERVE_AR)
    rng = np.random.default_rng(W.SEED)
    base = torch.from_numpy(np.stack([_head(np, rng, N, NC, MEMBERS, DET) for _ in range(M)])).to(dev)  # [M, N, A] fp32

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def padded(nbytes):
        return (nbytes + 255) // 256 * 256

    # the decoder's buffers and the two selectors' outputs (one count per 256 bytes)
    sb = cvgs.head_decode_scratch_bytes(N)
    scratch = torch.zeros((M, padded(sb)), dtype=torch.uint8, device=dev)
    d_boxes = torch.zeros((M, N, 4), dtype=torch.float32, device=dev)
    d_scores = torch.zeros((M, N), dtype=torch.float32, device=dev)
    d_classes = torch.zeros((M, N), dtype=torch.int32, device=dev)
    d_index = torch.zeros((M, N), dtype=torch.int32, device=dev)
    d_count = torch.zeros((M, 64), dtype=torch.int32, device=dev)
    ssb = cvgs.boxes_select_scratch_bytes(N, PRE_K)
    s_scratch = torch.zeros((M, padded(ssb)), dtype=torch.uint8, device=dev)
    s_boxes = torch.zeros((M, MAX_OUT, 4), dtype=torch.float32, device=dev)
    s_count = torch.zeros((M, 64), dtype=torch.int32, device=dev)

    def select_descs(boxes, scores, classes, counts):
        return (capi.BoxSelectDesc * M)(*[cvgs.box_select_desc((fw, fh), boxes[f], scores[f], N, s_scratch[f], s_boxes[f], s_count[f], THR, 0.45, PRE_K, MAX_OUT,
                                                               cvgs.CAND_CXCYWH_F32, 4, 1, classes[f], 1, None if counts is None else counts[f], xform)
                                          for f in range(M)])

    sel_compact = select_descs(d_boxes, d_scores, d_classes, d_count)
    res = {"workload": "16 frames x (4 + 80) x 8400 CXCYWH heads, ~300 candidates over the score threshold 0.25 per frame; select: pre_nms_k 1024, max_out 50; "
                       "us per TICK (16 frames)",
           "rounds": a.rounds, "reps_per_round": a.reps, "ticks_per_replay": K, "variants": {}}
    for name, dtype, elem, channel_major in (("bf16_channel_major", torch.bfloat16, cvgs.HEAD_BF16, True), ("fp32_channel_major", torch.float32, cvgs.HEAD_F32, True),
                                             ("bf16_row_major", torch.bfloat16, cvgs.HEAD_BF16, False), ("fp32_row_major", torch.float32, cvgs.HEAD_F32, False)):
        head = (base.transpose(1, 2) if channel_major else base).to(dtype).contiguous()  # [M, A, N] or [M, N, A]
        spare = torch.zeros_like(head)
        cs, as_ = (1, N) if channel_major else (A, 1)
        hdescs = (capi.HeadDesc * M)(*[cvgs.head_desc(head[f], elem, N, cs, as_, NC, THR, scratch[f], d_boxes[f], d_scores[f], d_classes[f], d_count[f], d_index[f])
                                       for f in range(M)])
        keep = []  # the framework path's tensors of the last call (the captured ones live in the graph's pool)

        def decode_fn():
            for _ in range(K):
                capi.check(lib.cvgs_head_decode(hdescs, M, stream()))

        def decode_select_fn():
            for _ in range(K):
                capi.check(lib.cvgs_head_decode(hdescs, M, stream()))
                capi.check(lib.cvgs_boxes_select(sel_compact, M, stream()))

        def torch_dense():
            h = head.float()
            if channel_major:
                scores, cls = h[:, 4:, :].max(dim=1)
                boxes = h[:, :4, :].transpose(1, 2).contiguous()
            else:
                scores, cls = h[:, :, 4:].max(dim=2)
                boxes = h[:, :, :4].contiguous()
            return boxes, scores.contiguous(), cls.to(torch.int32)

        def torch_select_fn():
            for _ in range(K):
                t = torch_dense()
                keep.append(t)
                capi.check(lib.cvgs_boxes_select(select_descs(t[0], t[1], t[2], None), M, stream()))

        def copy_fn():
            for _ in range(K):
                spare.copy_(head)

        # (b) and (c) select the same boxes
        torch_select_fn()
        torch.cuda.synchronize()
        want_b, want_c = s_boxes.clone(), s_count[:, 0].clone()
        s_boxes.zero_(), s_count.zero_()
        decode_select_fn()
        torch.cuda.synchronize()
        assert torch.equal(s_boxes.view(torch.int32), want_b.view(torch.int32)) and torch.equal(s_count[:, 0], want_c), name
        del keep[:]
        graphs = {"decode": _capture(decode_fn), "decode_select": _capture(decode_select_fn), "torch_select": _capture(torch_select_fn), "copy": _capture(copy_fn)}
        per = {k: [] for k in graphs}
        for _ in range(a.rounds):  # ABAB: every round times every leg once
            for k, g in graphs.items():
                per[k].append(_time_graph(g, a.reps) / K)
        v = {"head_bytes": int(head.numel() * head.element_size()), "members_per_frame": [int(x) for x in d_count[:, 0].cpu()],
             "kept_per_frame": [int(x) for x in want_c.cpu()]}
        for k, t in per.items():
            v[k] = {"us": round(float(np.median(t)), 3), "min_us": round(float(np.min(t)), 3), "max_us": round(float(np.max(t)), 3),
                    "legs_us": [round(float(x), 3) for x in t]}
        v["decode_over_copy"] = round(v["decode"]["us"] / v["copy"]["us"], 3)
        v["torch_select_over_decode_select"] = round(v["torch_select"]["us"] / v["decode_select"]["us"], 3)
        v["select_after_decode_us"] = round(v["decode_select"]["us"] - v["decode"]["us"], 3)
        res["variants"][name] = v
        print(json.dumps({name: {k: (x["us"] if isinstance(x, dict) else x) for k, x in v.items() if k not in ("members_per_frame", "kept_per_frame")}}), flush=True)
        del graphs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
