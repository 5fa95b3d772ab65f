"""The case table that runs BOTH forms of K4's two-pixel kernel (csrc/k_nv12_x2.hip) on small, odd and batched targets, shared by
tests/test_k4_x2_cases.py (no GPU: names, the launcher's rule, the table's own non-vacuity, the oracle inside the float64 model's bound)
and tests/test_zz_gpu_k4_x2_rows.py (the one GPU item: guard bands, bit-exactness, the other kernels, the model).  No test item here.

launch_nv12_x2 takes one of two forms: one row per wave (plain global stores; an odd target's last lane stores ONE pixel) or the pipelined
form, kN2Rows = 2 rows per wave with the next row's tap words in flight and every store through one buffer descriptor over the whole
tensor (a row past the target gets an offset the hardware drops).  The pipelined form needs an even dst_w, a tensor below 4 GiB - 64 KiB and
batch * dst_h * ceil(dst_w / 128) >= 4096: rows_per_wave() below restates that rule, and under the CVGS_K4_X2 hook cvgs_kernel_name says
which form was taken ("@r1" / "@r2").  tests/test_gpu_k4_x2.py forces the kernel on small shapes, all of which the rule gives the one-row
form; the cases here sit at and around the threshold, so that the pipelined form meets: a last wave whose second row lies past the target
(odd dst_h: the dropped store, the min(y, dst_h - 1) clamp of load_row), surfaces z = 1..7 (a.plane[z], per-plane uv_off, z * img_stride
in the 32-bit byte offset), CNHW strides (ch_stride > img_stride in total_bytes and the descriptor's extent), the program without the
swap, NV21, limited range, a ragged last 128-column tile with one live lane, sources as narrow as the chroma window (P.w - 4 == 0),
0 / 255 checkerboards, mixed scales per plane, and the smallest admissible crop in the bottom-right corner of a surface that ends where
its allocation ends.

Left out: the descriptor's 4 GiB - 64 KiB limit -- no tensor of a size a test may have reaches it.

A case: (name, surface, crops, layout, range, primaries, swap, write kind, dst = (w, h), hook on / off, expected name incl. suffix).  Crops are
(x, y, w, h) views of ONE surface, all even, w >= 4; the batches hold different views (the whole surface and the bottom-right corner among
them), so that uv_off differs per plane.  Surfaces are seeded; oracle pictures and model results are computed once per process and shared."""
import collections

import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import helpers as H

X2_MIN_WAVE_ROWS = 4096  # kK4X2MinWaveRows (cvgs_device.h): batch * dst_h * ceil(dst_w / 64) from which launch_nv12 prefers the two-pixel kernel
PIPE_MIN_ROWS = 4096     # launch_nv12_x2: batch * dst_h * ceil(dst_w / 128) from which it walks kN2Rows rows per wave
N2_ROWS = 2              # kN2Rows
SPLIT, T_SPLIT = capi.WRITE_TENSOR_SPLIT, capi.WRITE_TENSOR_T_SPLIT
MUL, SUB, DIV = [1 / 255.0] * 3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]  # tests/test_gpu_k4_x2.py's program

Case = collections.namedtuple("Case", "name surface crops layout range_ prim swap write dst hook want")


# ---- the launcher's rule, restated ------------------------------------------------------------------------------------------------------------
def takes_x2(batch, dst, hook):
    """K4FamilyBase::frame_kernel: the hook takes every eligible chain, else the size rule"""
    return hook or batch * dst[1] * ((dst[0] + 63) // 64) >= X2_MIN_WAVE_ROWS


def rows_per_wave(batch, dst, write):
    """launch_nv12_x2's `pipe`: the strides are those of a dense [N, 3, h, w] (split) or [3, N, h, w] (splitT) fp32 tensor"""
    w, h = dst
    img_stride, ch_stride = (3 * w * h, w * h) if write == SPLIT else (w * h, batch * w * h)
    total_bytes = ((batch - 1) * img_stride + 2 * ch_stride + h * w) * 4
    assert total_bytes == batch * 3 * w * h * 4  # (dense tensors: the descriptor spans exactly the tensor)
    pipe = w % 2 == 0 and 0 < total_bytes < (1 << 32) - 65536 and batch * h * ((w + 127) // 128) >= PIPE_MIN_ROWS
    return N2_ROWS if pipe else 1


def expected_name(case):
    """the name the rule gives a case: the program's, and under the hook the form"""
    assert takes_x2(len(case.crops), case.dst, case.hook), case.name
    base = "k4_nv12_x2_swap_mul_sub_div" if case.swap else "k4_nv12_x2_mul_sub_div"
    return base + ("@r%d" % rows_per_wave(len(case.crops), case.dst, case.write) if case.hook else "")


# ---- surfaces: name -> (w, h, builder of the (h * 3 / 2, w) array) ------------------------------------------------------------------------
def _checker():
    """tests/test_gpu_k4_x2.py's extreme samples: 0 / 255 checkerboards in luma and in both chroma channels"""
    w, h = 256, 128
    s = np.zeros((h + h // 2, w), np.uint8)
    s[:h:2, ::2] = 255
    s[1:h:2, 1::2] = 255
    s[h:, ::4] = 255
    s[h + 1::2, 1::4] = 255
    return s


SURFACES = {"rand322": (322, 198, lambda: H.random_u8((198 + 99, 322), 8322)),
            "rand64": (64, 36, lambda: H.random_u8((36 + 18, 64), 8064)),
            "tiny": (4, 2, lambda: H.random_u8((3, 4), 8004)),
            "checker": (256, 128, _checker),
            "tall": (640, 1240, lambda: H.random_u8((1240 + 620, 640), 8640))}
_surfaces = {}


def surface(name):
    """(w, h, array): made once, never written"""
    if name not in _surfaces:
        w, h, make = SURFACES[name]
        s = np.ascontiguousarray(make())
        assert s.shape == (h + h // 2, w) and s.dtype == np.uint8
        s.setflags(write=False)
        _surfaces[name] = (w, h, s)
    return _surfaces[name]


# eight different views of the 322 x 198 surface: the whole surface, the smallest admissible crop in the bottom-right corner, a crop that ends at
# the right and bottom edge, one chroma-window-wide column, a band of 6 rows ...
CROPS8 = [(0, 0, 322, 198), (318, 196, 4, 2), (2, 4, 64, 36), (100, 50, 222, 148), (10, 20, 300, 170), (160, 0, 4, 198), (0, 98, 322, 6), (46, 66, 130, 128)]
CROPS3 = [(0, 0, 322, 198), (318, 196, 4, 2), (36, 2, 258, 152)]
CHECKER8 = [(0, 0, 256, 128), (252, 126, 4, 2), (2, 2, 252, 124), (0, 0, 4, 128), (128, 64, 128, 64), (6, 10, 26, 52), (0, 62, 256, 4), (100, 0, 130, 128)]
# 640 x 1240 -> (130, 257): 4.8x down in both axes (cfg #3's scale), ~2x up in both, and everything between, per plane
MIXED8 = [(0, 0, 624, 1234), (10, 20, 64, 128), (0, 0, 640, 1240), (636, 1238, 4, 2), (2, 2, 130, 256), (320, 600, 320, 640), (100, 0, 26, 1240), (0, 620, 640, 6)]

NV12, NV21, FULL, LIMITED = capi.YUV_NV12, capi.YUV_NV21, capi.YUV_FULL, capi.YUV_LIMITED
B601, B709, B2020 = capi.BT601, capi.BT709, capi.BT2020
_SWAP, _PLAIN = "k4_nv12_x2_swap_mul_sub_div", "k4_nv12_x2_mul_sub_div"

CASES = collections.OrderedDict()


def add(name, surf, crops, layout, range_, prim, swap, write, dst, hook, want):
    assert name not in CASES, name
    w, h, _ = SURFACES[surf]
    for x, y, cw, ch in crops:
        assert not (x | y | cw | ch) & 1 and cw >= 4 and ch >= 2 and 0 <= x and 0 <= y and x + cw <= w and y + ch <= h, (name, (x, y, cw, ch))
    CASES[name] = Case(name, surf, list(crops), layout, range_, prim, swap, write, dst, hook, want)


# exactly at the threshold: 8 * 256 * 2 = 4096; the second column tile has ONE live lane (columns 128, 129)
add("at_4096_130x256_x8", "rand322", CROPS8, NV12, FULL, B709, True, SPLIT, (130, 256), True, _SWAP + "@r2")
# one row short of it: 4080; an odd height in the one-row form
add("below_4080_130x255_x8", "rand322", CROPS8, NV12, FULL, B709, True, SPLIT, (130, 255), True, _SWAP + "@r1")
# odd height: the last wave's second row is past the target; z = 1..7
add("odd_height_130x257_x8", "rand322", CROPS8, NV12, FULL, B709, True, SPLIT, (130, 257), True, _SWAP + "@r2")
# batch 1, odd height, nine column tiles, the last with one live lane: 457 * 9 = 4113
add("one_surface_1026x457", "rand322", CROPS8[:1], NV12, FULL, B709, True, SPLIT, (1026, 457), True, _SWAP + "@r2")
# an odd width is never pipelined, whatever the size
add("odd_width_1025x457", "rand322", CROPS8[:1], NV12, FULL, B709, True, SPLIT, (1025, 457), True, _SWAP + "@r1")
# CNHW strides (ch_stride = 3 planes > img_stride) and NCHW: 3 * 456 * 3 = 4104
add("cnhw_258x456_x3", "rand322", CROPS3, NV12, FULL, B709, True, T_SPLIT, (258, 456), True, _SWAP + "@r2")
add("nchw_258x456_x3", "rand322", CROPS3, NV12, FULL, B709, True, SPLIT, (258, 456), True, _SWAP + "@r2")
add("cnhw_odd_height_130x257_x8", "rand322", CROPS8, NV21, LIMITED, B709, False, T_SPLIT, (130, 257), True, _PLAIN + "@r2")
# no hook: the product's own rules reach the form (2048 * 4 = 8192 wave rows -> x2; 2048 * 2 = 4096 -> pipelined); the name stays plain
add("hook_off_256x2048", "rand64", [(0, 0, 64, 36)], NV12, FULL, B709, True, SPLIT, (256, 2048), False, _SWAP)
# the other conversion paths: NV21 (sel_u / sel_v with vu), limited range (n2_tap<false>), the program without the swap
add("nv21_limited_601_noswap_130x257_x8", "rand322", CROPS8, NV21, LIMITED, B601, False, SPLIT, (130, 257), True, _PLAIN + "@r2")
add("nv12_limited_2020_swap_130x257_x8", "rand322", CROPS8, NV12, LIMITED, B2020, True, SPLIT, (130, 257), True, _SWAP + "@r2")
# a 4 x 2 surface eight times: every lane's luma and chroma window is clamped back, P.w - 4 == 0
add("tiny_4x2_130x257_x8", "tiny", [(0, 0, 4, 2)] * 8, NV12, FULL, B709, True, SPLIT, (130, 257), True, _SWAP + "@r2")
# 0 / 255 checkerboards: the range's ends through the conversion and the division by the uniform divisor: 1025 * 4 = 4100
add("checker_512x1025", "checker", CHECKER8[:1], NV12, FULL, B601, True, SPLIT, (512, 1025), True, _SWAP + "@r2")
add("checker_130x257_x8", "checker", CHECKER8, NV12, FULL, B601, True, SPLIT, (130, 257), True, _SWAP + "@r2")
add("checker_nv21_limited_noswap_130x257_x8", "checker", CHECKER8, NV21, LIMITED, B709, False, SPLIT, (130, 257), True, _PLAIN + "@r2")
# 4.8x down and 2x up in one batch: fx, fy per plane, y2r clamped at P.h - 1 on the up-scaled planes, chroma rows shared by both taps
add("mixed_scales_130x257_x8", "tall", MIXED8, NV12, FULL, B709, True, SPLIT, (130, 257), True, _SWAP + "@r2")
# the bottom-right corner crop as the LAST plane (z = 7): its chroma row ends with the allocation; 8 * 259 * 2 = 4144
add("corner_last_130x259_x8", "rand322", CROPS8[2:] + CROPS8[:2], NV12, LIMITED, B709, True, SPLIT, (130, 259), True, _SWAP + "@r2")


# ---- chains ---------------------------------------------------------------------------------------------------------------------------------------
def tensor_bytes(case):
    return len(case.crops) * 3 * case.dst[0] * case.dst[1] * 4


def ops(case, surf_ptr, out_ptr, keep=None):
    """the chain over a surface at `surf_ptr` (host or device) into a dense fp32 tensor at `out_ptr`"""
    w, h, _ = surface(case.surface)
    luma = cvgs.GpuMat(h, w, cvgs.CV_8UC1, surf_ptr, w, owner=keep)
    f = cvgs.CV_32FC3
    chain = [cvgs.read_nv12([luma.nv12_roi(*c) for c in case.crops], case.dst, case.range_, case.prim, False, layout=case.layout)]
    if case.swap:
        chain.append(cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f))
    chain += [cvgs.multiply(f, MUL), cvgs.subtract(f, SUB), cvgs.divide(f, DIV)]
    make = cvgs.split_tensor if case.write == SPLIT else cvgs.splitT
    return chain + [make(f, out_ptr, case.dst[0], case.dst[1], len(case.crops), keep=keep)]


def host_ops(case, out=None):
    """(chain over host memory, its output array): what the CPU oracle executes and what a dry run names"""
    _, _, s = surface(case.surface)
    out = np.zeros(tensor_bytes(case) // 4, np.float32) if out is None else out
    return ops(case, s.ctypes.data, out.ctypes.data, keep=(s, out)), out


_oracle, _model = {}, {}


def oracle_output(oracle, case):
    """the CPU oracle's picture of a case (flat fp32, the write's memory order): computed once, read-only"""
    if case.name not in _oracle:
        chain, out = host_ops(case)
        oracle.execute(cvgs.lower(chain))
        out.setflags(write=False)
        _oracle[case.name] = out
    return _oracle[case.name]


def model_result(case):
    """(iops, Result) of the float64 model: a 4:2:0 resize read, the arithmetic stages, a planar fp32 tensor -- every case of this table"""
    if case.name not in _model:
        _, h, s = surface(case.surface)
        chain, _ = host_ops(case)
        _model[case.name] = (chain, F.evaluate(chain, [F.View(s, x, y, cw, ch, luma_h=h) for x, y, cw, ch in case.crops]))
    return _model[case.name]


def check_against_model(case, got):
    """(ok, ratio) per element of a flat fp32 output against the model's value and derived bound"""
    chain, res = model_result(case)
    return res.check(res.logical(np.asarray(got, np.float32).astype(np.float64), chain[-1].kind))
