"""Two numpy models of the INTER_AREA read (CVGS_READ_RESIZE_AREA), written from the arithmetic contract in include/cvgs_hip.h.  Neither
calls the library for a pixel: the library only supplies the plane GEOMETRY (fx, fy and the aspect-ratio window, cvgs.build_plane_table --
held to the oracle by tests/test_abi.py) and the chain's own operands (read back from the lowered descriptor).

  * area_plane_f32: the fp32 restatement -- np.float32 arithmetic in the written order (every operation rounded once), vectorised over the
    pixels of a plane with the tap loops in Python.  The kernels are held to it BIT FOR BIT (tests/test_gpu_area.py).
  * area_plane_f64: the float64 model -- the same coverage integral as two dense weight matrices (rows x source rows, columns x source
    columns) applied by matrix product, normalised by their row sums, from the same float32 fx, fy.  It says what the fp32 order costs.

Both share one chain tail (apply_program) for the pointwise stages and the casts, and one case list (the GPU test's)."""
import struct

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests.test_bf16_types import rne_bf16

F32 = np.float32

# ---- the case list of tests/test_gpu_area.py: one 97 x 61 source, targets 16 x 8 and 33 x 7 (33: no multiple of the wave, 7: odd) ----------
SRC_W, SRC_H = 97, 61
TARGETS = ((16, 8), (33, 7))
CROPS = (  # (x, y, w, h)
    (0, 0, 97, 61),     # the whole frame
    (5, 5, 1, 1),
    (7, 3, 1, 40),
    (3, 9, 40, 1),
    (10, 10, 16, 8),    # identity for 16 x 8
    (20, 30, 33, 7),    # identity for 33 x 7
    (30, 20, 7, 5),     # both axes non-shrinking (for both targets)
    (2, 40, 90, 6),     # x shrinks, y does not
    (11, 13, 38, 19),   # 2.37x (16 x 8)
    (8, 4, 32, 16),     # exactly 2x (16 x 8)
    (1, 2, 48, 24),     # exactly 3x (16 x 8)
    (9, 1, 66, 14),     # exactly 2x (33 x 7)
    (56, 38, 41, 23),   # touches the right and the bottom edge: the clamp of b to w and of i1
    (0, 0, 96, 61),     # 96 columns (-> 1 column with the target (1, 8))
)
NARROW_TARGET = (1, 8)


def make_source(depth, cn, seed=0xA2EA):
    """The 61 x 97 source of a depth: seeded random values plus a ramp (so that a shifted footprint shows)."""
    rng = np.random.default_rng(seed + 16 * depth + cn)
    ramp = (np.arange(SRC_W)[None, :, None] * 3 + np.arange(SRC_H)[:, None, None] * 5 + np.arange(cn)[None, None, :] * 7)
    if depth == capi.DEPTH_8U:
        a = (rng.integers(0, 200, (SRC_H, SRC_W, cn)) + ramp % 56).astype(np.uint8)
    elif depth == capi.DEPTH_16U:
        a = (rng.integers(0, 60000, (SRC_H, SRC_W, cn)) + ramp * 9).astype(np.uint16)
    elif depth == capi.DEPTH_16S:
        a = (rng.integers(-30000, 30000, (SRC_H, SRC_W, cn)) + ramp * 4).astype(np.int16)
    elif depth == capi.DEPTH_32F:
        a = (rng.standard_normal((SRC_H, SRC_W, cn)) * 100.0 + ramp * 0.25).astype(np.float32)
    else:
        raise ValueError("no source for depth %d" % depth)
    return np.ascontiguousarray(a)


def plane_params(read_iop):
    """[dict(w, h, step, fx, fy, x1, y1, x2, y2)] of a read stage over HOST views: the plane table the library builds for it."""
    raw = cvgs.build_plane_table(read_iop)
    out = []
    for z in range(read_iop.batch):
        _data, w, h, step, fx, fy, x1, y1, x2, y2, _uv = struct.unpack_from("<QiiiffiiiiI", raw, 48 * z)
        out.append(dict(w=w, h=h, step=step, fx=F32(fx), fy=F32(fy), x1=x1, y1=y1, x2=x2, y2=y2))
    return out


# ---- the fp32 restatement --------------------------------------------------------------------------------------------------------------
def axis_taps_f32(n_out, f, n):
    """One axis, output coordinates t = 0 .. n_out-1 inside the window: (idx[t, j], wt[t, j], live[t, j], W[t]) -- tap j of pixel t reads
    source index idx with weight wt when live; W is the weights' fp32 sum in ascending order (1.0 by definition when not shrinking)."""
    f = F32(f)
    t = np.arange(n_out, dtype=np.int64)
    tf = t.astype(F32)
    if not f > F32(1.0):
        s = tf * f
        i0 = np.floor(s).astype(np.int64)
        idx = np.stack([i0, np.minimum(i0 + 1, n - 1)], axis=1)
        wt = np.stack([(i0 + 1).astype(F32) - s, s - i0.astype(F32)], axis=1).astype(F32)
        return idx, wt, np.ones((n_out, 2), bool), np.ones(n_out, F32)
    a = tf * f
    b = np.minimum((t + 1).astype(F32) * f, F32(n)).astype(F32)
    i0 = np.minimum(np.floor(a).astype(np.int64), n - 1)
    i1 = np.maximum(np.minimum(np.ceil(b).astype(np.int64), n), i0 + 1)
    cnt = i1 - i0
    J = int(cnt.max())
    idx = np.zeros((n_out, J), np.int64)
    wt = np.zeros((n_out, J), F32)
    live = np.zeros((n_out, J), bool)
    W = np.zeros(n_out, F32)
    single = b <= a
    for j in range(J):
        i = i0 + j
        w = (np.minimum((i + 1).astype(F32), b) - np.maximum(i.astype(F32), a)).astype(F32)
        w = np.where(single, F32(1.0), w).astype(F32)
        lv = j < cnt
        idx[:, j] = np.where(lv, i, i0)
        wt[:, j] = w
        live[:, j] = lv
        W = np.where(lv, (W + w).astype(F32), W).astype(F32)
    return idx, wt, live, W


def area_plane_f32(src, P, dst_w, dst_h, bg):
    """One plane: src (h, w, cn) of any served depth -> (dst_h, dst_w, cn) float32; outside the window the background."""
    cn = src.shape[2]
    assert src.shape[0] == P["h"] and src.shape[1] == P["w"]
    out = np.empty((dst_h, dst_w, cn), F32)
    out[:] = np.asarray(bg[:cn], F32)
    x1, y1, x2, y2 = P["x1"], P["y1"], P["x2"], P["y2"]
    if x2 < x1 or y2 < y1:
        return out
    v = src.astype(F32)  # exact for 8U / 16U / 16S; 32F as it is
    ix, wx, lx, Wx = axis_taps_f32(x2 - x1 + 1, P["fx"], P["w"])
    iy, wy, ly, Wy = axis_taps_f32(y2 - y1 + 1, P["fy"], P["h"])
    ny, nx = iy.shape[0], ix.shape[0]
    acc = np.zeros((ny, nx, cn), F32)
    for jj in range(iy.shape[1]):
        rows = v[iy[:, jj]]  # (ny, w, cn)
        row = np.zeros((ny, nx, cn), F32)
        for ii in range(ix.shape[1]):
            term = (rows[:, ix[:, ii], :] * wx[None, :, ii, None]).astype(F32)
            row = np.where(lx[None, :, ii, None], (row + term).astype(F32), row)
        acc = np.where(ly[:, jj, None, None], (acc + (row * wy[:, jj, None, None]).astype(F32)).astype(F32), acc)
    inv = (F32(1.0) / (Wx[None, :] * Wy[:, None]).astype(F32)).astype(F32)
    out[y1:y2 + 1, x1:x2 + 1, :] = (acc * inv[:, :, None]).astype(F32)
    return out


# ---- the float64 model -----------------------------------------------------------------------------------------------------------------
def axis_matrix_f64(n_out, f, n):
    """(n_out, n) float64: row t holds the share of every source pixel in output pixel t, normalised to sum 1."""
    f = float(F32(f))
    M = np.zeros((n_out, n), np.float64)
    i = np.arange(n, dtype=np.float64)
    for t in range(n_out):
        if not f > 1.0:
            s = t * f
            i0 = int(np.floor(s))
            M[t, i0] += (i0 + 1) - s
            M[t, min(i0 + 1, n - 1)] += s - i0
            continue
        a, b = t * f, min((t + 1) * f, float(n))
        if b <= a:
            M[t, min(int(np.floor(a)), n - 1)] = 1.0
            continue
        cover = np.clip(np.minimum(i + 1, b) - np.maximum(i, a), 0.0, None)
        M[t] = cover / cover.sum()
    return M


def area_plane_f64(src, P, dst_w, dst_h, bg):
    cn = src.shape[2]
    out = np.empty((dst_h, dst_w, cn), np.float64)
    out[:] = np.asarray(bg[:cn], F32).astype(np.float64)
    x1, y1, x2, y2 = P["x1"], P["y1"], P["x2"], P["y2"]
    if x2 < x1 or y2 < y1:
        return out
    Mx = axis_matrix_f64(x2 - x1 + 1, P["fx"], P["w"])
    My = axis_matrix_f64(y2 - y1 + 1, P["fy"], P["h"])
    out[y1:y2 + 1, x1:x2 + 1, :] = np.einsum("yj,jic,xi->yxc", My, src.astype(np.float64), Mx)
    return out


# ---- the chain tail both models share ----------------------------------------------------------------------------------------------------
def chain_ops(desc):
    """[(opcode, aux, operand[4] float32)] of a lowered chain descriptor (NOPs dropped)."""
    return [(desc.ops[k].opcode, desc.ops[k].aux, np.array(list(desc.ops[k].operand), F32)) for k in range(desc.n_ops)
            if desc.ops[k].opcode != capi.OP_NOP]


def apply_program(x, ops):
    """The pointwise stages on (..., cn) values of dtype float32 (each stage rounded once) or float64 (the model: arithmetic only, casts to
    a float type keep the value).  Returns (values, depth): depth 8U values are exact integers, 16F / 16BF values the floats they round to."""
    dt = x.dtype
    depth = capi.DEPTH_32F
    for opcode, aux, operand in ops:
        cn = x.shape[-1]
        o = operand[:cn].astype(dt)
        if opcode == capi.OP_MUL:
            x = (x * o).astype(dt)
        elif opcode == capi.OP_ADD:
            x = (x + o).astype(dt)
        elif opcode == capi.OP_SUB:
            x = (x - o).astype(dt)
        elif opcode == capi.OP_DIV:
            x = (x / o).astype(dt)
        elif opcode == capi.OP_REORDER:
            x = np.stack([x[..., (aux >> (2 * c)) & 3] for c in range(cn)], axis=-1)
        elif opcode == capi.OP_CAST:
            if aux == capi.DEPTH_8U:      # cv::saturate_cast: round to nearest even, clamp, NaN -> 0
                r = np.rint(x) + dt.type(0.0)
                x = np.clip(np.where(np.isnan(x), dt.type(0.0), r), 0.0, 255.0).astype(dt)
            elif aux == capi.DEPTH_16F and dt == F32:
                x = x.astype(np.float16).astype(F32)
            elif aux == capi.DEPTH_16BF and dt == F32:
                x = (rne_bf16(x).astype(np.uint32) << 16).view(F32).reshape(x.shape)
            elif aux not in (capi.DEPTH_32F, capi.DEPTH_16F, capi.DEPTH_16BF):
                raise NotImplementedError("cast to depth %d" % aux)
            depth = aux
        else:
            raise NotImplementedError("opcode %d" % opcode)
    return x, depth


def area_chain(plane_fn, srcs, params, dsize, used, batch, bg, ops, dtype):
    """(batch, dst_h, dst_w, cn_out): every plane through plane_fn (area_plane_f32 / _f64), planes >= used take the default value, then
    the program on everything."""
    dst_w, dst_h = dsize
    cn = len([s for s in srcs if s is not None][0][0, 0]) if any(s is not None for s in srcs) else 3
    planes = []
    for z in range(batch):
        if z < used:
            planes.append(plane_fn(srcs[z], params[z], dst_w, dst_h, bg).astype(dtype))
        else:
            p = np.empty((dst_h, dst_w, cn), dtype)
            p[:] = np.asarray(bg[:cn], F32).astype(dtype)
            planes.append(p)
    return apply_program(np.stack(planes), ops)


def store_bits(values, depth):
    """The bytes a write stage stores for the tail's values: float32 / float16 / bf16 bits / uint8."""
    if depth == capi.DEPTH_32F:
        return np.ascontiguousarray(values, F32)
    if depth == capi.DEPTH_16F:
        return np.ascontiguousarray(values.astype(np.float16))
    if depth == capi.DEPTH_16BF:
        return np.ascontiguousarray(rne_bf16(values)).reshape(values.shape)
    if depth == capi.DEPTH_8U:
        return np.ascontiguousarray(values.astype(np.uint8))
    raise NotImplementedError(depth)
