"""The case grid that holds K1's 2- and 4-rows-per-wave kernels to the float64 model (tests/f64_model.py) at SMALL targets, shared by
tests/test_k1_rows_cases.py (CPU oracle, the grid's own non-vacuity), tests/k1_rows_worker.py (one child per CVGS_K1_RPW setting) and
tests/test_gpu_k1_rows.py (the parent: names, model bound, identity across settings).

launch_k1 picks 2 or 4 rows per wave only from 16 Ki wave-rows on; under the CVGS_K1_RPW hook every launch takes the row count asked for,
so the row loop of k1_resize_split meets what large launches almost never give it: a row group that straddles the target's last row
(y = min(row0 + j, dst_h - 1) against the store's y < dst_h), an aspect-ratio window edge inside a row group (in_y[j]), background planes
over RPW rows, ragged column tiles under the wave-uniform u8c3 tile store (x0 + 63 < dst_w), sources of one pixel / one row / one column
/ narrower than a tap window.

Targets: every height of HEIGHTS at width 65, every width of WIDTHS at heights 5 and 8 -- with kK1Waves waves per workgroup
(CVGS_K1_WPB) and 4 rows per wave a workgroup owns kK1Waves * 4 rows, and HEIGHTS holds one fewer, exactly that and one more.

A case names the rows per wave the table of k1_rows_instantiated (k_k1_impl.hpp) gives it under each setting; the GPU test compares that
with the "@rN" suffix of cvgs_kernel_name.  Cases are held to the float64 model, except the separate pitched planes (WRITE_SPLIT_2D has
no place in the model's output layouts): those are held to the CPU oracle bit for bit.  The CircularTensor sequence is compared across
settings only."""
import collections
import os
import re
import struct

from cvgpuspeedup_amd import capi, cvgs
from tests import circular_cases as CC
from tests import f64_model as F
from tests import model_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (1, 2, 4)


def k1_waves():
    """kK1Waves: -DCVGS_K1_WPB=<n> of the build (the Makefile's flags), else the header's default"""
    csrc = os.path.join(ROOT, "cvgpuspeedup_amd", "csrc")
    m = re.search(r"-DCVGS_K1_WPB=(\d+)", open(os.path.join(csrc, "Makefile")).read())
    if m is None:
        m = re.search(r"#define CVGS_K1_WPB (\d+)", open(os.path.join(csrc, "k_k1_impl.hpp")).read())
    return int(m.group(1))


HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 17)
WIDTHS = (1, 63, 64, 65, 130)
SIZES = [(65, h) for h in HEIGHTS] + [(w, h) for h in (5, 8) for w in WIDTHS if w != 65]  # (width, height)

# requested rows per wave -> instantiated rows, by launcher (the table of k1_rows_instantiated)
ROWS_U8 = {1: 1, 2: 2, 4: 4}       # launch_rpw: u8 C3 / C4 into a planar tensor, compile-time programs
ROWS_WIDE = {1: 1, 2: 4, 4: 4}     # launch_rpw: 16-bit / fp32 C3 / C4 into a planar tensor
ROWS_OTHER = {1: 1, 2: 1, 4: 4}    # launch_other (packed pixels, separate planes), launch_few_planar
ROWS_INTERP = {1: 1, 2: 1, 4: 1}   # interpreted programs into a planar tensor

U8, U16, S16, F32, F16, BF16 = cvgs.CV_8U, cvgs.CV_16U, cvgs.CV_16S, cvgs.CV_32F, cvgs.CV_16F, capi.DEPTH_16BF
FRAME, CROPS = MC.FRAME, MC.CROPS
LAST_BYTE = [(60, 30, 37, 31), (96, 60, 1, 1), (0, 60, 97, 1)]  # crops that end at the frame's last byte
CROPS65 = [(i % 60, (i * 7) % 30, 5 + (i * 3) % 33, 4 + (i * 5) % 27) for i in range(65)]  # one more than the 4 KB argument block holds

# kind: chain (build(B) -> iops, views) | tick (build = [build, ...]: one cvgs_execute_many call) | circular (build = a circular_cases.Case)
Case = collections.namedtuple("Case", "name family kind build rows kernel model oracle_exact")
CASES = collections.OrderedDict()


def add(name, family, build, rows, kernel, kind="chain", model=True, oracle_exact=False):
    assert name not in CASES, name
    CASES[name] = Case(name, family, kind, build, rows, kernel, model, oracle_exact)


def _sz(dst):
    return "%dx%d" % dst


def plane_params(rd):
    """the lowered PlaneParams of a read stage (cvgs_plane_table_build; cvgs_device.h): dicts with w, h, x1, y1, x2, y2"""
    raw = cvgs.build_plane_table(rd)
    out = []
    for z in range(len(raw) // 48):
        _, w, h, _, _, _, x1, y1, x2, y2, _ = struct.unpack_from("<QiiiffiiiiI", raw, 48 * z)
        out.append({"w": w, "h": h, "x1": x1, "y1": y1, "x2": x2, "y2": y2})
    return out


def edges_inside_a_row_group(planes, dst_h, rows=4):
    """planes whose window starts AND ends strictly inside a group of `rows` target rows (the group holds rows of both kinds)"""
    return [p for p in planes if 0 < p["y1"] and p["y2"] < dst_h - 1 and p["y1"] % rows != 0 and (p["y2"] + 1) % rows != 0]


def window_case(depth, cn, crops, dst, ar, **kw):
    """resize_case under an aspect-ratio mode.  Only SOME planes of a case carry the property the case is there for: the builder asserts
    from the lowered PlaneParams that at least two of the used planes (one if only one is used; used = 0: none, the case is all
    background) have both window edges strictly inside a 4-row group.  The other crops of a list add other windows -- the tall crop an x
    window over every row, the one-pixel source a square one -- and are held to nothing but the model.  Every fitted extent is away from
    a .5 tie (the model's rule and the product's agree there).  Window cases keep their planes in the kernel arguments: the assertion
    reads the host descriptors."""
    assert not kw.get("table"), "a window case with a device table would skip the PlaneParams assertion"
    inner = MC.resize_case(depth, cn, FRAME, crops, dst, ar=ar, **kw)

    def build(B):
        iops, views = inner(B)
        rd = iops[0]
        pp = plane_params(rd)[:rd.used_planes]  # (planes at or beyond usedPlanes carry the background: no window)
        assert len(edges_inside_a_row_group(pp, dst[1])) >= min(2, rd.used_planes), pp
        for (x, y, w, h), p in zip(crops, pp):
            x1, y1, x2, y2, margin = F.exact_window(w, h, dst[0], dst[1], ar)
            assert margin >= 0.2 and (x1, y1, x2, y2) == (p["x1"], p["y1"], p["x2"], p["y2"]), ((w, h), p, margin)
        return iops, views
    build.window = (crops, dst, ar)
    return build


# ---- u8 C3 / C4 into planar tensors, compile-time programs: rows 1 / 2 / 4 ------------------------------------------------------------------
_A = "u8 planar"
for _dst in SIZES:  # the headline program at every target of the grid
    add("u8c3_norm_f32_" + _sz(_dst), _A, MC.resize_case(U8, 3, FRAME, CROPS, _dst, tail="normalise", seed=101), ROWS_U8, "k1_u8c3_swap_mul_sub_div")
add("u8c4_msd_f16_splitT_65x5", _A, MC.resize_case(U8, 4, FRAME, CROPS, (65, 5), tail="mul_sub_div", out16=F16, write="splitT", seed=102), ROWS_U8, "k1_u8c4_mul_sub_div_f16")
add("u8c4_msd_f16_splitT_64x8", _A, MC.resize_case(U8, 4, FRAME, CROPS, (64, 8), tail="mul_sub_div", out16=F16, write="splitT", seed=103), ROWS_U8, "k1_u8c4_mul_sub_div_f16")
add("u8c3_arith_bf16_65x9", _A, MC.resize_case(U8, 3, FRAME, CROPS, (65, 9), tail="arith", out16=BF16, seed=104), ROWS_U8, "k1_u8c3_arith_bf16")
add("u8c3_arith_bf16_130x5", _A, MC.resize_case(U8, 3, FRAME, CROPS, (130, 5), tail="arith", out16=BF16, seed=105), ROWS_U8, "k1_u8c3_arith_bf16")
add("u8c4_none_f32_65x7", _A, MC.resize_case(U8, 4, FRAME, CROPS, (65, 7), seed=106), ROWS_U8, "k1_u8c4_arith")
add("u8c4_none_f32_splitT_63x8", _A, MC.resize_case(U8, 4, FRAME, CROPS, (63, 8), write="splitT", seed=107), ROWS_U8, "k1_u8c4_arith")
add("u8c3_none_f16_65x3", _A, MC.resize_case(U8, 3, FRAME, CROPS, (65, 3), out16=F16, seed=108), ROWS_U8, "k1_u8c3_arith_f16")
add("u8c4_norm_bf16_65x17", _A, MC.resize_case(U8, 4, FRAME, CROPS, (65, 17), tail="normalise", out16=BF16, seed=109), ROWS_U8, "k1_u8c4_swap_mul_sub_div_bf16")
# 65 planes: the 16 KB argument block
add("u8c3_norm_f32_65planes_65x5", _A, MC.resize_case(U8, 3, FRAME, CROPS65, (65, 5), tail="normalise", seed=110), ROWS_U8, "k1_u8c3_swap_mul_sub_div")
add("u8c4_arith_f16_65planes_65x9", _A, MC.resize_case(U8, 4, FRAME, CROPS65, (65, 9), tail="arith", out16=F16, seed=111), ROWS_U8, "k1_u8c4_arith_f16")
# a resident device plane table (cvgs_plane_table_build)
add("u8c3_norm_f32_table_65x5", _A, MC.resize_case(U8, 3, FRAME, CROPS, (65, 5), tail="normalise", table=True, seed=112), ROWS_U8, "k1_u8c3_swap_mul_sub_div")
add("u8c4_msd_bf16_splitT_table_130x8", _A, MC.resize_case(U8, 4, FRAME, CROPS, (130, 8), tail="mul_sub_div", out16=BF16, write="splitT", table=True, seed=113),
    ROWS_U8, "k1_u8c4_mul_sub_div_bf16")
# sources: one pixel, one row, one column, a row narrower than one tap window (2 pixels of u8c3 = 6 bytes < 8), crops ending at the last byte
_SOURCES = {"1x1": ((1, 1), [(0, 0, 1, 1)]), "w_x1": ((1, 40), [(0, 0, 40, 1), (7, 0, 2, 1), (39, 0, 1, 1)]), "1xh": ((33, 1), [(0, 0, 1, 33), (0, 31, 1, 2)]),
            "2wide": ((29, 2), [(0, 0, 2, 29), (0, 3, 2, 2), (1, 28, 1, 1)]), "lastbyte": (FRAME, LAST_BYTE)}
for _nm, (_hw, _cr) in _SOURCES.items():
    add("u8c3_norm_f32_src_%s_65x5" % _nm, _A, MC.resize_case(U8, 3, _hw, _cr, (65, 5), tail="normalise", seed=120), ROWS_U8, "k1_u8c3_swap_mul_sub_div")
    add("u8c4_none_f32_src_%s_65x9" % _nm, _A, MC.resize_case(U8, 4, _hw, _cr, (65, 9), seed=121), ROWS_U8, "k1_u8c4_arith")
# an interpreted program: one row per wave whatever is asked for
add("u8c3_interp_f32_65x5", "interpreted", MC.resize_case(U8, 3, FRAME, CROPS[:6], (65, 5), tail="interp", seed=122), ROWS_INTERP, "k1_u8c3_interp")

# ---- 16-bit / fp32 C3 / C4 and 1- / 2-channel sources into planar tensors: rows 1 / 4 -----------------------------------------------------------
_B = "wide and few planar"
add("u16c3_norm_65x5", _B, MC.resize_case(U16, 3, FRAME, CROPS, (65, 5), tail="normalise", seed=130), ROWS_WIDE, "k1_u16c3_swap_mul_sub_div")
add("u16c3_norm_65x9", _B, MC.resize_case(U16, 3, FRAME, CROPS, (65, 9), tail="normalise", seed=131), ROWS_WIDE, "k1_u16c3_swap_mul_sub_div")
add("s16c4_msd_splitT_65x7", _B, MC.resize_case(S16, 4, FRAME, CROPS, (65, 7), tail="mul_sub_div", write="splitT", seed=132), ROWS_WIDE, "k1_s16c4_mul_sub_div")
add("s16c4_msd_130x8", _B, MC.resize_case(S16, 4, FRAME, CROPS, (130, 8), tail="mul_sub_div", seed=133), ROWS_WIDE, "k1_s16c4_mul_sub_div")
add("f32c3_arith_65x5", _B, MC.resize_case(F32, 3, FRAME, CROPS, (65, 5), tail="arith", seed=134), ROWS_WIDE, "k1_f32c3_arith")
add("f32c3_none_63x8", _B, MC.resize_case(F32, 3, FRAME, CROPS, (63, 8), seed=135), ROWS_WIDE, "k1_f32c3_arith")
add("f32c3_none_src_1x1_65x9", _B, MC.resize_case(F32, 3, (1, 1), [(0, 0, 1, 1)], (65, 9), seed=136), ROWS_WIDE, "k1_f32c3_arith")
add("u8c1_msd_65x5", _B, MC.resize_case(U8, 1, FRAME, CROPS, (65, 5), tail="mul_sub_div", seed=137), ROWS_OTHER, "k1_u8c1_mul_sub_div")
add("u8c2_arith_65x9", _B, MC.resize_case(U8, 2, FRAME, CROPS, (65, 9), tail="arith", seed=138), ROWS_OTHER, "k1_u8c2_arith")
add("u8c2_arith_src_1x1_64x8", _B, MC.resize_case(U8, 2, (1, 1), [(0, 0, 1, 1)], (64, 8), tail="arith", seed=139), ROWS_OTHER, "k1_u8c2_arith")
add("u16c1_msd_65x7", _B, MC.resize_case(U16, 1, FRAME, CROPS, (65, 7), tail="mul_sub_div", seed=140), ROWS_OTHER, "k1_u16c1_mul_sub_div")
add("u16c2_msd_130x5", _B, MC.resize_case(U16, 2, FRAME, CROPS, (130, 5), tail="mul_sub_div", seed=141), ROWS_OTHER, "k1_u16c2_mul_sub_div")

# ---- packed targets: rows 1 / 4; u8c3 -> u8 stores whole 64-column tiles at 4 rows per wave (store_u8c3_tile) ---------------------------------
_C = "packed"
for _dst in SIZES:
    add("u8c3_packed_u8_" + _sz(_dst), _C, MC.resize_case(U8, 3, FRAME, CROPS, _dst, write="packed", out_int=U8, seed=150), ROWS_OTHER, "k1_u8c3_packed_u8")
for _dst in ((64, 5), (65, 8), (130, 9)):
    add("u8c3_packed_u8_arith_" + _sz(_dst), _C, MC.resize_case(U8, 3, FRAME, CROPS, _dst, tail="arith", write="packed", out_int=U8, seed=151), ROWS_OTHER,
        "k1_u8c3_packed_u8_arith")
for _nm, (_hw, _cr) in _SOURCES.items():
    add("u8c3_packed_u8_src_%s_130x8" % _nm, _C, MC.resize_case(U8, 3, _hw, _cr, (130, 8), write="packed", out_int=U8, seed=152), ROWS_OTHER, "k1_u8c3_packed_u8")
for _cn in (1, 2, 4):
    add("u8c%d_packed_u8_65x5" % _cn, _C, MC.resize_case(U8, _cn, FRAME, CROPS, (65, 5), write="packed", out_int=U8, seed=153), ROWS_OTHER, "k1_u8c%d_packed_u8" % _cn)
    add("u8c%d_packed_u8_130x8" % _cn, _C, MC.resize_case(U8, _cn, FRAME, CROPS, (130, 8), tail="arith", write="packed", out_int=U8, seed=154), ROWS_OTHER,
        "k1_u8c%d_packed_u8_arith" % _cn)
add("u8c3_packed_f32_65x5", _C, MC.resize_case(U8, 3, FRAME, CROPS, (65, 5), write="packed", seed=155), ROWS_OTHER, "k1_u8c3_packed_f32")
add("u8c3_packed_f32_arith_64x8", _C, MC.resize_case(U8, 3, FRAME, CROPS, (64, 8), tail="arith", write="packed", seed=156), ROWS_OTHER, "k1_u8c3_packed_f32_arith")
add("u8c3_packed_f16_65x9", _C, MC.resize_case(U8, 3, FRAME, CROPS, (65, 9), tail="arith", write="packed", out16=F16, seed=157), ROWS_OTHER, "k1_u8c3_packed_f16_arith")
add("u8c3_packed_f16_interp_130x5", _C, MC.resize_case(U8, 3, FRAME, CROPS, (130, 5), tail="interp", write="packed", out16=F16, seed=158), ROWS_OTHER, "k1_u8c3_packed_f16")
add("u8c3_packed_bf16_65x7", _C, MC.resize_case(U8, 3, FRAME, CROPS, (65, 7), tail="arith", write="packed", out16=BF16, seed=159), ROWS_OTHER, "k1_u8c3_packed_bf16_arith")
add("u8c3_packed_bf16_interp_63x8", _C, MC.resize_case(U8, 3, FRAME, CROPS, (63, 8), tail="interp", write="packed", out16=BF16, seed=160), ROWS_OTHER, "k1_u8c3_packed_bf16")
for _d, _cn, _dn in ((U16, 3, "u16"), (S16, 1, "s16"), (F32, 1, "f32")):
    add("%sc%d_packed_own_65x5" % (_dn, _cn), _C, MC.resize_case(_d, _cn, FRAME, CROPS, (65, 5), write="packed", out_int=None if _d == F32 else _d, seed=161), ROWS_OTHER,
        "k1_%sc%d_packed_%s" % (_dn, _cn, _dn))
    add("%sc%d_packed_own_65x9" % (_dn, _cn), _C, MC.resize_case(_d, _cn, FRAME, CROPS, (65, 9), write="packed", out_int=None if _d == F32 else _d, seed=162), ROWS_OTHER,
        "k1_%sc%d_packed_%s" % (_dn, _cn, _dn))

# ---- separate pitched planes: rows 1 / 4; no place in the model's layouts -> the CPU oracle, bit for bit ------------------------------------------
_D = "separate planes"
for _dst in ((65, 5), (65, 9), (130, 8)):
    add("u8c3_planes2d_" + _sz(_dst), _D, MC.resize_case(U8, 3, FRAME, CROPS[:5], _dst, tail="normalise", write="planes2d", seed=170), ROWS_OTHER, "k1_u8c3_planes2d_f32",
        model=False, oracle_exact=True)
for _dst in ((65, 5), (65, 7)):
    add("u16c4_planes2d_" + _sz(_dst), _D, MC.resize_case(U16, 4, FRAME, CROPS[:4], _dst, tail="mul_sub_div", write="planes2d", seed=171), ROWS_OTHER, "k1_u16c4_planes2d_f32",
        model=False, oracle_exact=True)

# ---- aspect-ratio windows with an edge inside a 4-row group; planes at or beyond usedPlanes over a non-zero background -------------------------
_E = "windows"
# (sizes found with f64_model.exact_window: both y edges inside a 4-row group, the fitted extent >= 0.2 away from a .5 tie; a tall crop gives an
# x window, the 1 x 1 source a square one)
WINDOW_CROPS = {(40, 24): [(3, 5, 34, 11), (4, 7, 34, 5), (5, 6, 27, 13), (5, 6, 20, 40), (10, 11, 1, 1)],
                (65, 9): [(3, 5, 62, 5), (4, 7, 48, 3), (5, 6, 34, 3), (5, 6, 21, 40), (10, 11, 1, 1)]}
for _ar, _nm in ((cvgs.PRESERVE_AR, "ar"), (cvgs.PRESERVE_AR_RN_EVEN, "ar_even"), (cvgs.PRESERVE_AR_LEFT, "ar_left")):
    for _dst, _cr in WINDOW_CROPS.items():
        add("u8c3_%s_planar_%s" % (_nm, _sz(_dst)), _E, window_case(U8, 3, _cr, _dst, _ar, tail="normalise", seed=180), ROWS_U8, "k1_u8c3_swap_mul_sub_div")
        add("u8c3_%s_packed_u8_%s" % (_nm, _sz(_dst)), _E, window_case(U8, 3, _cr, _dst, _ar, write="packed", out_int=U8, seed=181), ROWS_OTHER, "k1_u8c3_packed_u8")
for _used, _un in ((0, "used0"), (3, "usedNm2")):  # N = 5 crops
    add("u8c3_ar_%s_planar_65x9" % _un, _E, window_case(U8, 3, WINDOW_CROPS[(65, 9)], (65, 9), cvgs.PRESERVE_AR, used=_used, tail="normalise", seed=182), ROWS_U8,
        "k1_u8c3_swap_mul_sub_div")
    add("u8c3_ar_%s_packed_u8_65x9" % _un, _E, window_case(U8, 3, WINDOW_CROPS[(65, 9)], (65, 9), cvgs.PRESERVE_AR, used=_used, write="packed", out_int=U8, seed=183), ROWS_OTHER,
        "k1_u8c3_packed_u8")

# ---- one cvgs_execute_many tick: three u8c3 chains of batch 1, 4, 2 (z >= batch returns early inside the fused grid) ---------------------------------
_TICK_CROPS = [CROPS[1:2], CROPS[2:6], [CROPS[8], CROPS[0]]]
for _tb, _tn in ((False, "host"), (True, "tables")):
    add("tick_u8c3_%s_65x5" % _tn, "tick", [MC.resize_case(U8, 3, FRAME, _c, (65, 5), tail="normalise", table=_tb, seed=190 + _i) for _i, _c in enumerate(_TICK_CROPS)],
        ROWS_U8, "k1_u8c3_swap_mul_sub_div", kind="tick")

# ---- one CircularTensor sequence: three resize pushes into a ring of three, height 5 (the row loop's out2 stores); across settings only -----------
CIRCULAR = CC.Case("k1_rows_ring", "def", False, "of", "std", "32f", 3, 3, 65, 5, "rs")
CIRCULAR_UPDATES = 3
add("circular_u8c3_65x5", "circular", CIRCULAR, ROWS_U8, "k1_u8c3_arith", kind="circular", model=False)

FAMILIES = list(collections.OrderedDict((c.family, None) for c in CASES.values()))


# ---- running a case on the CPU oracle / against the model ----------------------------------------------------------------------------------
def chains_of(case):
    """[(tag, build)] of the chains a case holds to the model / the oracle (a tick: one per chain)"""
    if case.kind == "tick":
        return [("%s#%d" % (case.name, i), b) for i, b in enumerate(case.build)]
    return [(case.name, case.build)] if case.kind == "chain" else []


def model_side(build):
    """(iops, views) as the model sees them: the chain itself (bf16 as bit patterns, the conversion to bf16 as a stage), over host memory"""
    return build(MC.HostBackend(bf16_twin=False))


def oracle_output(oracle, build):
    """the output array the CPU oracle writes for a chain, in the output's own number format (CV_16BF: its fp32 twin, rounded on the host)"""
    from tests.test_bf16_types import rne_bf16
    B = MC.HostBackend()
    iops, _ = build(B)
    oracle.execute(cvgs.lower(iops))
    got = B.result()
    return rne_bf16(got) if B.rounded_to_bf16 else got


def check_against_model(res, iops, got):
    """(ok, ratio) of an output array (own number format, memory order of the write) against a model Result"""
    return res.check(res.logical(MC.widen_output(got, iops[-1].dst_type), iops[-1].kind))


def out_dtype(iops):
    return MC.np_dtype(iops[-1].dst_type)
