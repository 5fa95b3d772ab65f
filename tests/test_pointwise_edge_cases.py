"""The grid of tests/pointwise_edge_cases.py without a GPU (404 cases; this module takes about 5 s; no kernel code changed with it): every chain is one
the product accepts, the dry run names the thread-fused kernel the case states (cvgs.kernel_name needs no device) and an interpreted one under
CHAIN_FORCE_GENERIC and under CHAIN_NO_THREAD_FUSION, the grid holds what its docstring says -- asserted against the literals below, from the built
chains and from store_path --, and the CPU oracle gives the EXACT expectation bit for bit on every case, the whole buffer compared and the padding
intact (bf16 through the fp32 twin, which must hold the unrounded value).  That proves the expectation here, before any kernel runs.

Coverage.  store_path restates which branch of pw4_write a case's waves take.  Every (source depth, store) family must hold every branch that
can exist for it: the planar, the per-plane and the direct packed stores with their ragged tails and the full-group transpose on all eight
families, the narrow dense transpose on the fp32 ones (16-bit stores leave it at compile time: those families must hold a narrow dense PLANE that
takes the direct path).  Two rows per thread is a property of the launch, not of the store, and differs between depths in the load only; its four
large cases are u8 and s16 planes, packed and planar, as many as the grid may afford.

Near-misses.  The expectation is written for five rules (pointwise_edge_cases.RULES): the product's, and four near-misses of it -- the ragged
tail's pixels taken as zero, a default plane reading its source, the swap left out, `(v - 16) * 0.5` and `v * 0.5 - 16` exchanged.  Each differs
from the product's rule on at least one case of every family, in the bytes of the family's store (bf16's one rounding included)."""
import collections
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import model_cases as MC
from tests import pointwise_edge_cases as P

# What the grid must hold, restated here as literals (NOT taken from tests/pointwise_edge_cases.py)
U8_NAMES = {"pointwise4_u8_%s%s" % (p, s) for p in ("cast_mul_sub_div", "cast", "interp") for s in ("", "_f16", "_bf16")}
DEPTH_NAMES = {"pointwise4_s8", "pointwise4_u16", "pointwise4_s16", "pointwise4_s32", "pointwise4_f32"}
FAMILIES = {"u8 f32", "u8 f16", "u8 bf16", "s8 f32", "u16 f32", "s16 f32", "s32 f32", "f32 f32"}
WIDTHS = {1, 2, 3, 4, 5, 7, 8, 60, 63, 64, 65, 68, 124, 127, 128, 129, 132, 255, 256, 257, 511, 512, 513, 515}
HEIGHTS = {1, 2, 3, 4, 5, 7, 8, 9, 17}
EVERY_STORE = {"planar x4", "planar tail", "per-plane x4", "per-plane tail", "direct x4", "direct tail", "full group"}
KERNARG_PLANES = 64  # CVGS_KERNARG_PLANES of include/cvgs_hip.h
LARGE = {(1021, 1029), (1024, 1025), (1024, 1023)}

_BUILT = {}


def built(name, twin=False):
    """(backend, iops) of a case over host memory, built once.  twin=False: the chain as the GPU runs it (bf16 types included)"""
    if (name, twin) not in _BUILT:
        B = MC.HostBackend(bf16_twin=twin)
        _BUILT[(name, twin)] = (B, P.CASES[name].build(B)[0])
    return _BUILT[(name, twin)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def test_every_chain_validates_and_names_its_kernel(lib):
    assert len(U8_NAMES) == 9
    for c in P.CASES.values():
        _, iops = built(c.name)
        assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, (c.name, lib.cvgs_last_error())
        assert cvgs.kernel_name(*iops) == c.kernel, (c.name, cvgs.kernel_name(*iops))
        assert c.kernel in (U8_NAMES if c.depth == "u8" else DEPTH_NAMES) and (c.depth == "u8" or c.kernel == "pointwise4_" + c.depth), c.name
        assert c.kernel.endswith({"f32": ("sub_div", "cast", "interp"), "f16": ("_f16",), "bf16": ("_bf16",)}[c.store]) or c.depth != "u8", c.name
        for flags in (capi.CHAIN_NO_THREAD_FUSION, capi.CHAIN_FORCE_GENERIC):
            assert cvgs.kernel_name(*iops, flags=flags).startswith("generic"), (c.name, flags, cvgs.kernel_name(*iops, flags=flags))
        rd, wr = iops[0], iops[-1]
        assert rd.batch == c.n and rd.used_planes == c.used and rd.table is None and c.table == (c.n > KERNARG_PLANES), c.name
        kinds = {"split": capi.WRITE_TENSOR_SPLIT, "splitT": capi.WRITE_TENSOR_T_SPLIT, "packed3d": capi.WRITE_PIXEL_3D, "packed2d": capi.WRITE_PIXEL_2D,
                 "split2d": capi.WRITE_SPLIT_2D}
        assert wr.kind == kinds[c.write], c.name
    assert {c.kernel for c in P.CASES.values()} == U8_NAMES | DEPTH_NAMES  # every name the dry run can give for these chains


def test_store_path_on_the_named_near_misses():
    """store_path against branch sets written out by hand: one step inside the narrow dense path's condition and one step outside it"""
    sp = lambda name: (P.store_path(P.CASES[name]).narrow, set(P.store_path(P.CASES[name]).branches))
    for d in ("u8", "s16"):
        assert sp(d + "_dense_pitch+0_64x8") == (2, {"narrow dense"}) and sp(d + "_dense_pitch+4_64x8") == (2, {"direct x4"}) and sp(d + "_dense_pitch+16_64x8") == (2, {"direct x4"})
        assert sp(d + "_dense_pitch+0_128x4") == (1, {"narrow dense"}) and sp(d + "_dense_pitch+4_128x4") == (1, {"direct x4"})
        assert sp(d + "_dense_pitch+0_124x2") == (1, {"narrow dense"}) and sp(d + "_dense_pitch+16_60x4") == (2, {"direct x4"})
        assert sp(d + "_dense_limit_w63") == (2, {"direct x4", "direct tail"}) and sp(d + "_dense_limit_w64") == (2, {"narrow dense"})
        assert sp(d + "_dense_limit_w65") == (1, {"direct x4", "direct tail"}) and sp(d + "_dense_limit_w127") == (1, {"direct x4", "direct tail"})
        assert sp(d + "_dense_limit_w128") == (1, {"narrow dense"}) and sp(d + "_dense_limit_w129") == (0, {"direct x4", "direct tail"})
        assert sp(d + "_dense_rows_64x4") == (2, {"narrow dense"}) and sp(d + "_dense_rows_64x5") == (2, {"narrow dense", "direct x4"})
        assert sp(d + "_dense_rows_128x16") == (1, {"narrow dense"}) and sp(d + "_dense_rows_128x17") == (1, {"narrow dense", "direct x4"})
        assert sp(d + "_dense_rows_8x1") == (2, {"direct x4"}) and sp(d + "_dense_rows_8x3") == (2, {"direct x4"}) and sp(d + "_dense_rows_4x7") == (2, {"narrow dense", "direct x4"})
    for s in ("f16", "bf16"):  # 16-bit stores on a narrow dense plane: the direct path
        assert sp("u8_%s_dense_plane_64x8" % s) == (2, {"direct x4"}) and sp("u8_%s_dense_plane_128x4" % s) == (1, {"direct x4"})
    assert sp("u8_rows2_1021x1029_packed3d") == (0, {"full group", "direct x4", "direct tail", "rows2"})
    assert sp("s16_rows2_1021x1029_splitT") == (0, {"planar x4", "planar tail", "rows2"}) and sp("u8_rows2_1024x1025_split") == (0, {"planar x4", "rows2"})
    assert sp("s16_below_rows2_1024x1023_packed3d") == (0, {"full group"})
    assert sp("u8_f32_anchor_packed2d_257x3") == (0, {"full group", "direct tail"}) and sp("u8_f32_anchor_packed3d_515x2") == (0, {"full group", "direct tail"})


def test_the_grid_covers_what_it_says():
    cases = list(P.CASES.values())
    assert 300 <= len(cases) <= 420 and {c.family for c in cases} == FAMILIES and set(P.FAMILIES) == FAMILIES
    # every (source depth x store x branch) that can exist, and every kernel name with each store path it can reach
    table = collections.defaultdict(set)
    for c in cases:
        table[c.kernel] |= set(P.store_path(c).branches)
    for family in FAMILIES:
        mine = [c for c in cases if c.family == family]
        f32 = family.endswith(" f32")
        held = set().union(*[P.store_path(c).branches for c in mine]) - {"rows2"}
        assert held == EVERY_STORE | ({"narrow dense"} if f32 else set()), (family, sorted(held))
        assert {P.store_path(c).narrow for c in mine} == {0, 1, 2}
        if not f32:  # a plane that WOULD be narrow dense with a 4-byte element
            assert any(c.write == "packed3d" and c.w in (64, 128) and c.h >= 4 and P.store_path(c).branches == {"direct x4"} for c in mine), family
        # shapes, on each family
        assert {c.w for c in mine} >= WIDTHS and {c.h for c in mine} >= HEIGHTS, family
        assert {c.cn for c in mine} == {1, 2, 3, 4} and {c.prog for c in mine} == {"plain", "cast", "interp"}
        assert {c.write for c in mine} == {"split", "splitT", "packed3d", "packed2d", "split2d"}, family
        assert {c.n for c in mine} == {1, 5, KERNARG_PLANES, KERNARG_PLANES + 1} and any(c.table and c.used < c.n for c in mine) and any(c.used < c.n and not c.table for c in mine)
        assert all((c.w, c.h) == (5, 3) for c in mine if c.n >= KERNARG_PLANES)
        # source memory: dense and pitched views; bases 0, 1, 3, 5 bytes into the allocation (wider samples: 0 or one element)
        eb = P.elem_bytes(mine[0].depth)
        assert {c.src_off for c in mine} == ({0, 1, 3, 5} if eb == 1 else {0, eb}) and {c.src_pad == 0 for c in mine} == {True, False}, family
        # pitched images: every offset and every padding; dense tensors on an address that is only element-aligned
        es = 4 if f32 else 2
        p2d = [c for c in mine if c.write == "packed2d"]
        assert {c.out_off for c in p2d} == ({0, 4, 8, 12} if f32 else {0, 2, 6, 10}) and {c.out_pad for c in p2d} == {0, 4, 16, 20}, family
        assert any(c.out_off == es for c in mine if c.write in ("split", "splitT")) and any(c.out_off == es for c in mine if c.write == "packed3d"), family
        assert any(c.n * c.cn > 16 for c in mine if c.write == "split2d") and any(c.n * c.cn <= 16 for c in mine if c.write == "split2d")  # kInlineDst
    for name in sorted(U8_NAMES | DEPTH_NAMES):
        f32 = not name.endswith("f16")
        want = EVERY_STORE | {"narrow dense"} if f32 else EVERY_STORE
        assert table[name] >= want, (name, sorted(want - table[name]))
    # two rows per thread: the four large cases, and nothing else is large
    large = [c for c in cases if c.w * c.h * c.n >= 4096 * 4]
    assert len(large) == 4 and {(c.w, c.h) for c in large} == LARGE and all(c.cn == 1 and c.n == 1 for c in large)
    assert {(c.depth, c.write.startswith("packed")) for c in large if P.store_path(c).rows2} == {("u8", True), ("u8", False), ("s16", False)}
    assert [c.name for c in large if not P.store_path(c).rows2] == ["s16_below_rows2_1024x1023_packed3d"]
    assert all(not P.store_path(c).rows2 for c in cases if c not in large)
    # the tick: cases of the shape cvgs_execute_many takes, on every program and on the narrow dense path
    tick = [c for c in cases if P.takes_tick(c)]
    assert {c.prog for c in tick} == {"plain", "cast", "interp"} and {c.write for c in tick} == {"split", "splitT", "packed3d"} and len(tick) >= 40
    assert any("narrow dense" in P.store_path(c).branches for c in tick) and any("full group" in P.store_path(c).branches for c in tick)
    # what the built chains say about memory
    for c in cases:
        B, iops = built(c.name)
        es = 4 if c.store == "f32" else 2
        assert len(B.placed) == (c.n * c.cn if c.write == "split2d" else 1), c.name
        for z, m in enumerate(iops[0].mats):
            assert (m.cols, m.rows, m.step) == (c.w, c.h, c.w * c.cn * P.elem_bytes(c.depth) + c.src_pad) and m.data % 256 == c.src_off, c.name
            assert (P.source(c, z) != 0).all()
        if c.write == "packed2d":
            assert iops[-1].step == c.w * c.cn * es + c.out_pad == B.placed[0].pitch and iops[-1].data % 256 == c.out_off, c.name
        elif c.write == "split2d":
            pl = iops[-1].planes2d
            assert [(p.step, p.data % 16) for p in pl] == [(q.pitch, q.origin % 16) for q in B.placed], c.name
            assert len({q.pitch for q in B.placed}) > 1 and len({q.origin % 16 for q in B.placed}) > 1, c.name
        else:
            assert iops[-1].data % 256 == c.out_off, c.name
        for q in B.placed:
            assert q.fill.size >= q.origin + (q.rows - 1) * q.pitch + q.row_bytes + 64


def _oracle_run(oracle, c):
    B, iops = built(c.name, twin=True)
    B.outs[0][...] = B.placed[0].fill.reshape(1, -1)  # (a rebuilt case starts from its fill)
    oracle.execute(cvgs.lower(iops))
    got, moved = P.split_whole(B.placed, B.result(), c.write, c.n, c.cn)
    assert moved.size == 0, "%s: the oracle wrote %d padding bytes" % (c.name, moved.size)
    return B, got


@pytest.mark.parametrize("family", sorted(FAMILIES), ids=[f.replace(" ", "_") for f in sorted(FAMILIES)])
def test_oracle_gives_the_exact_expectation(oracle, family):
    failed, ran = [], 0
    for c in P.cases_of(family):
        B, got = _oracle_run(oracle, c)
        ran += 1
        want = c.expected(B)
        assert want.shape == got.shape and want.dtype == got.dtype, c.name
        assert want.dtype == (np.float32 if c.store != "f16" else np.float16), c.name  # (bf16: the fp32 twin, the unrounded value)
        bad = bits(want) != bits(got)
        if bad.any():
            at = np.unravel_index(int(np.argmax(bad)), bad.shape)
            failed.append("%s: %d of %d elements differ, first at %r: %r, expected %r" % (c.name, int(bad.sum()), bad.size, at, got[at], want[at]))
    assert ran >= 38 and not failed, "%d of %d cases:\n%s" % (len(failed), ran, "\n".join(failed))


def test_the_exact_expectation_tells_four_near_misses_apart():
    """see the module docstring"""
    can = {"tail_zero": lambda c: c.w % 4 != 0 and c.used > 0, "default_reads_source": lambda c: c.used < c.n,
           "no_swap": lambda c: c.prog == "interp" and c.cn >= 3, "exchanged": lambda c: c.prog != "cast"}
    told = collections.defaultdict(set)
    for c in P.CASES.values():
        if c.w * c.h > 4096:
            continue  # (the four large planes add nothing here)
        spec = P.expected_values(c)
        for rule in P.RULES[1:]:
            other = P.expected_values(c, rule)
            if not can[rule](c):
                assert (spec == other).all(), (c.name, rule)  # the rules differ in nothing else
                continue
            assert (spec != other).any(), (c.name, rule)
            if (bits(P.to_store_bits(spec, c.store)) != bits(P.to_store_bits(other, c.store))).any():
                told[c.family].add(rule)
    assert all(told[f] == set(P.RULES[1:]) for f in FAMILIES), {f: sorted(set(P.RULES[1:]) - told[f]) for f in FAMILIES}
