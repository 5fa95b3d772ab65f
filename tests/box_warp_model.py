"""A model of cvgs_warp_tables_from_boxes' contract (include/cvgs_hip_ext.h, steps 1-8) that does not call the library and shares no code
with csrc/cvgs_geometry.h: whole-array numpy, np.float64 for every operation in the order the header writes them (one IEEE operation per
numpy operation, so one rounding each; numpy never fuses), np.float32 for the final narrowing.

`variant` selects a deliberately WRONG model for the sensitivity tests: "shrink" (EXPAND shrinks the longer side instead of growing the
shorter one), "no_centre_term" (drops + (m0 * 0.5 - 0.5)), "clamp_out" (clamps boxes_out into the frame).
"""
import struct

import numpy as np

STRETCH, EXPAND = 0, 1
INVALID_M = np.array([0, 0, -1, 0, 0, -1, 0, 0, 1], np.float32)


def live_items(count, max_items):
    return max_items if count is None else min(max(int(count), 0), max_items)


def shape_boxes(boxes, count, dsize, shape, scale, pad, variant=None, frame_size=None):
    """(m float32 [n, 9], boxes_out float32 [n, 4], valid int32 [n]) for float32 boxes [n, 4]."""
    b32 = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    n = len(b32)
    dw, dh = np.float64(dsize[0]), np.float64(dsize[1])
    sx, sy = np.float64(np.float32(scale[0])), np.float64(np.float32(scale[1]))
    px, py = np.float64(np.float32(pad[0])), np.float64(np.float32(pad[1]))
    with np.errstate(all="ignore"):
        b = b32.astype(np.float64)
        xa, ya, xb, yb = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        ok = (np.arange(n) < live_items(count, n)) & np.isfinite(b).all(axis=1)  # step 1
        w, h = xb - xa, yb - ya                                                   # step 2
        ok &= (w > 0) & (h > 0)
        cx, cy = (xa + xb) * 0.5, (ya + yb) * 0.5
        w1 = w * sx                                                                # step 3
        w1 = w1 + px
        h1 = h * sy
        h1 = h1 + py
        if shape == EXPAND:                                                        # step 4
            t1, t2 = w1 * dh, h1 * dw
            if variant == "shrink":
                w1, h1 = np.where(t1 > t2, t2 / dh, w1), np.where(t2 > t1, t1 / dw, h1)
            else:
                h1, w1 = np.where(t1 > t2, t1 / dw, h1), np.where(t2 > t1, t2 / dh, w1)
        m0, m4 = w1 / dw, h1 / dh                                                  # step 5
        x0, y0 = cx - w1 * 0.5, cy - h1 * 0.5
        if variant == "no_centre_term":
            m2, m5 = x0, y0
        else:
            m2, m5 = x0 + (m0 * 0.5 - 0.5), y0 + (m4 * 0.5 - 0.5)
        four = np.stack([m0, m2, m4, m5], axis=1).astype(np.float32)             # step 6
        ok &= np.isfinite(four).all(axis=1)
        rect = np.stack([x0, y0, cx + w1 * 0.5, cy + h1 * 0.5], axis=1)          # step 7
        if variant == "clamp_out":
            rect[:, 0::2] = np.clip(rect[:, 0::2], 0, frame_size[0])
            rect[:, 1::2] = np.clip(rect[:, 1::2], 0, frame_size[1])
        rect = rect.astype(np.float32)
    m = np.tile(INVALID_M, (n, 1))
    m[ok, 0], m[ok, 2], m[ok, 4], m[ok, 5] = four[ok, 0], four[ok, 1], four[ok, 2], four[ok, 3]
    rect[~ok] = 0
    return m, rect, ok.astype(np.int32)


def table_bytes(data, width, height, step, m, dsize):
    """The 64-byte entries: {data, width, height, step}, float m[9], {dst_width, dst_height}."""
    return b"".join(struct.pack("<Qiii", data, width, height, step) + np.ascontiguousarray(row, "<f4").tobytes() + struct.pack("<ii", dsize[0], dsize[1])
                    for row in m)


def model_bytes(frame, boxes, count, dsize, shape, scale, pad, variant=None):
    """(table bytes, boxes_out bytes, valid_out bytes); frame = (data, width, height, step)."""
    m, rect, valid = shape_boxes(boxes, count, dsize, shape, scale, pad, variant, (frame[1], frame[2]))
    return table_bytes(frame[0], frame[1], frame[2], frame[3], m, dsize), rect.astype("<f4").tobytes(), valid.astype("<i4").tobytes()
