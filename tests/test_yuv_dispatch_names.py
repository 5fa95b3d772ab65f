"""The kernel every YUV resize chain of a grid is dispatched to (cvgs_kernel_name: the real dispatch as a dry run, no GPU), compared
with tests/golden/yuv_dispatch_names.json.

The fixture is a RECORDING, not a specification: it holds what the commit before the 4:2:0 layouts moved onto the shared launcher
(k_yuv_family.hpp) answered for every case of the grid below, cases a family does not take included (they are recorded under whatever
name that commit reported, e.g. the interpreted kernel's).  It says that the move changed no dispatch decision; it does not say
that every decision is the best one.  Produced on that commit with `python -m tests.test_yuv_dispatch_names --record`, which writes
the names of exactly this grid; record again only when a dispatch rule is changed on purpose, and review the diff of the file."""
import json
import os
import sys

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import yuv422_cases as Y422
from tests import yuv444_cases as Y444

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yuv_dispatch_names.json")
LAYOUTS = {"nv12": capi.YUV_NV12, "nv21": capi.YUV_NV21, "p010": capi.YUV_P010, "i420": capi.YUV_I420, "yv12": capi.YUV_YV12,
           "yuyv": capi.YUV_YUYV, "uyvy": capi.YUV_UYVY, "i444": capi.YUV_I444}
TARGETS = ["planar_f32", "planar_f16", "planar_bf16", "packed_f32", "u8c3", "u8c4"]
K4_X2_ROWS = 4096  # kK4X2MinWaveRows (cvgs_device.h): output rows x 64-column tiles x surfaces
_OUT = np.zeros(4 * 64 * K4_X2_ROWS, np.float32)  # every case's target: a dry run writes nothing


def _surface(layout, w, h):
    """The luma view (4:2:2: the packed surface) of a w x h picture in `layout`."""
    if layout in Y422.LAYOUTS:
        return Y422.wrap_array(Y422.random_surface(w + (w & 1), h, 1, layout)).yuv422_roi(0, 0, w, h)  # (an odd width: a view of whole pairs)
    if layout == capi.YUV_I444:
        return Y444.wrap_array(Y444.Surf(w, h, 1))
    if layout == capi.YUV_P010:
        s = np.zeros((h + h // 2, w), np.uint16)
        return cvgs.GpuMat(h, w, cvgs.CV_16UC1, s.ctypes.data, s.strides[0], owner=s)
    s = np.zeros((h + h // 2, w), np.uint8)
    return cvgs.GpuMat(h, w, cvgs.CV_8UC1, s.ctypes.data, s.strides[0], owner=s)


def _program(prog, cn):
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    swap = cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f)
    norm = [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.subtract(f, [0.485, 0.456, 0.406, 0.5][:cn]), cvgs.divide(f, [0.229, 0.224, 0.225, 0.25][:cn])]
    return {"none": [], "swap": [swap], "swap_mul_sub_div": [swap] + norm, "mul_sub_div": norm,
            "arith": [swap, cvgs.multiply(f, [0.3] * cn), cvgs.add(f, [0.5] * cn)],  # a canonical-arithmetic chain
            # three linear stages in front of the division: the interpreter's
            "interp": [cvgs.add(f, [1.0] * cn), cvgs.multiply(f, [0.5] * cn), cvgs.subtract(f, [0.25] * cn), cvgs.divide(f, [3.0, 7.0, 9.0, 2.0][:cn])]}[prog]


def _ops(layout, target, prog, src=(64, 36), dst=(20, 10), batch=1, used=None, ar=None):
    cn = 4 if target == "u8c4" else 3
    w, h = dst
    m = _surface(layout, *src)
    rd = cvgs.read_nv12([m] * batch if batch > 1 else m, dst, capi.YUV_LIMITED, capi.BT709, cn == 4, layout=layout)
    if used is not None:
        rd.used_planes = used
    if ar is not None:
        rd.ar = ar
    f, u = cvgs.make_type(cvgs.DEPTH_32F, cn), cvgs.make_type(cvgs.DEPTH_8U, cn)
    out = lambda t, rows, cols: cvgs.GpuMat(rows, cols, t, _OUT.ctypes.data, cols * cvgs.elem_size(t), owner=_OUT)
    if prog == "cast_then_reorder":  # the reference's spelling of a BGR(A) u8 image: SaturateCast, then the reorder on bytes
        assert target in ("u8c3", "u8c4")
        stages = [cvgs.convertTo(f, u), cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, u)]
    else:
        stages = _program(prog, cn) + ([cvgs.convertTo(f, u)] if target.startswith("u8") else [])
    if target.startswith("planar"):
        h16 = {"planar_f32": None, "planar_f16": cvgs.CV_16FC3, "planar_bf16": cvgs.CV_16BFC3}[target]
        if h16 is None:
            return [rd] + stages + [cvgs.split(f, out(cvgs.CV_32FC1, batch, 3 * w * h), dst)]
        c1 = cvgs.CV_16FC1 if target == "planar_f16" else cvgs.CV_16BFC1
        return [rd] + stages + [cvgs.convertTo(f, h16), cvgs.split(h16, out(c1, batch, 3 * w * h), dst)]
    t = f if target == "packed_f32" else u
    return [rd] + stages + [cvgs.write(t, out(t, batch, w * h), dst) if batch > 1 else cvgs.write(t, out(t, h, w))]


def grid():
    """{case id: (ops, chain flags)}"""
    g = {}
    for ln, lay in LAYOUTS.items():
        # every target x every program, one stretched plane
        for t in TARGETS:
            for p in ["none", "swap", "swap_mul_sub_div", "mul_sub_div", "arith", "interp"] + (["cast_then_reorder"] if t.startswith("u8") else []):
                g["%s/%s/%s" % (ln, t, p)] = (_ops(lay, t, p), 0)
        # the argument-block sizes: 8 | 64 | 320 planes in the arguments, beyond: a table
        for n in (1, 8, 9, 64, 65, 320, 321):
            for t, p in (("planar_f32", "swap_mul_sub_div"), ("planar_f16", "arith"), ("packed_f32", "none"), ("u8c3", "none")):
                g["%s/%s/%s/batch%d" % (ln, t, p, n)] = (_ops(lay, t, p, batch=n), 0)
        # rows narrower than K4's chroma window (4:2:0 surfaces have even sizes: 2; the others: 3), alone and next to a wide plane's size
        nw = 2 if lay in (capi.YUV_NV12, capi.YUV_NV21, capi.YUV_P010, capi.YUV_I420, capi.YUV_YV12) else 3
        for t in ("planar_f32", "u8c3"):
            g["%s/%s/none/width%d" % (ln, t, nw)] = (_ops(lay, t, "none", src=(nw, 4)), 0)
            g["%s/%s/none/width4" % (ln, t)] = (_ops(lay, t, "none", src=(4, 4)), 0)
        # frame size: at and below the wave rows from which K4 prefers its two-pixel kernel, with and without thread fusion
        for p in ("swap_mul_sub_div", "mul_sub_div"):
            for rows in (K4_X2_ROWS, K4_X2_ROWS - 1):
                for fl in (0, capi.CHAIN_NO_THREAD_FUSION):
                    g["%s/planar_f32/%s/rows%d/flags%d" % (ln, p, rows, fl)] = (_ops(lay, "planar_f32", p, src=(64, 36), dst=(64, rows)), fl)
            g["%s/planar_f16/%s/rows%d" % (ln, p, K4_X2_ROWS)] = (_ops(lay, "planar_f16", p, dst=(64, K4_X2_ROWS)), 0)
        g["%s/planar_f32/swap_mul_sub_div/1280x720" % ln] = (_ops(lay, "planar_f32", "swap_mul_sub_div", src=(640, 360), dst=(1280, 720)), 0)
        # the windowed kernels: default-value planes, an aspect-ratio window
        for t in ("planar_f32", "planar_f16", "packed_f32", "u8c3"):
            g["%s/%s/swap/used2of3" % (ln, t)] = (_ops(lay, t, "swap", batch=3, used=2), 0)
            g["%s/%s/swap/preserve_ar" % (ln, t)] = (_ops(lay, t, "swap", dst=(20, 20), ar=cvgs.PRESERVE_AR), 0)
    return g


def names():
    os.environ.pop("CVGS_K4_X2", None)  # (the tuning hook of the frame-size kernel would change the answers)
    out = {}
    for cid, (ops, flags) in grid().items():
        try:
            out[cid] = cvgs.kernel_name(*ops, flags=flags)
        except Exception as e:  # a chain the engine refuses: recorded as such
            out[cid] = "refused: %s" % e
    return out


@pytest.fixture(scope="module")
def answers():
    return names()


def test_grid_is_the_recorded_one(answers):
    assert sorted(answers) == sorted(json.load(open(FIXTURE)))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_dispatch_names_equal_the_recording(answers, layout):
    """Every case of one layout: the name reported now is the name recorded before the move (see the module's docstring: the fixture
    records what the engine answered, it does not prescribe it)."""
    want = {k: v for k, v in json.load(open(FIXTURE)).items() if k.startswith(layout + "/")}
    assert len(want) > 60
    got = {k: answers[k] for k in want}
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_the_recording_holds_every_family():
    rec = json.load(open(FIXTURE))
    for prefix in ("k4_nv12_resize_", "k4_nv12_x2_", "k_yuv422_resize_", "k_yuv444_resize_"):
        assert sum(v.startswith(prefix) for v in rec.values()) >= 4, prefix
    k4 = {v for v in rec.values() if v.startswith("k4_nv12_resize_")}
    assert len(k4) >= 15  # the fifteen names of the family's table, bf16 twins aside


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(FIXTURE, "w") as fh:
        json.dump(names(), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", FIXTURE)
