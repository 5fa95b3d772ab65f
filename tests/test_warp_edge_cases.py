"""The grid of tests/warp_edge_cases.py without a GPU: every chain is one the product accepts, the dry run names the fast warp kernel the case
expects (cvgs.kernel_name needs no device) and an interpreted one under CHAIN_FORCE_GENERIC, the grid holds what its docstring says -- asserted
against the literals below, from the built chains and the cases' own coordinates --, and the CPU oracle gives the EXACT expectation bit for bit on
every exact case it can run (it runs no device tables) and lies within the float64 model's bound on the modelled ones.  Every modelled case
excludes at most 1 % of each plane (tests/test_gpu_model.held_to_model's condition, asserted here from the model alone: a case that would hide a
failure behind the model's exclusions cannot be added).

Near-misses.  The exact expectation is written for four rules (warp_edge_cases.RULES): the product's, and three near-misses of it -- the right
tap taken as zero instead of replicated, the bottom row not clamped, `sx <= w-1` as the inside test.  A near-miss can only show where a case has the
taps it is about (sx in (w-1, w), sy in (h-1, h)): an integer translation has none.  So the assertion is: wherever a case has such taps, its
expectation DIFFERS from the near-miss's (sources hold no zero, so it must); every kernel key has a case that tells all three apart; and a case
without such taps gives the same bytes under all four rules (the rules differ in nothing else).

Largest |oracle - model| / tolerance on the modelled cases (1 = at the bound): affine 0.2671 (fp32), 0.9944 (fp16: one rounding of the format), 0.2663
(packed); perspective 0.2243, 0.9889, 0.2238.  Largest excluded share of a plane: 0.31 %."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import f64_model as F
from tests import model_cases as MC
from tests import warp_edge_cases as W

# What the grid must hold, restated here as literals (NOT taken from tests/warp_edge_cases.py)
PROGRAMS = ("swap_mul_sub_div", "mul_sub_div", "interp")
PLANAR_NAMES = {"warp_%s_u8c%d_%s%s" % (t, cn, p, s) for t in ("affine", "perspective") for cn in (3, 4) for p in PROGRAMS for s in ("", "_f16", "_bf16")}
PACKED_NAMES = {"warp_affine_u8c3_packed_f32", "warp_affine_u8c4_packed_f32", "warp_perspective_u8c3_packed_f32", "warp_perspective_u8c4_packed_f32"}
SRC_WIDTHS = {3: {1, 2, 3, 5, 13}, 4: {1, 2, 3, 13}}
SRC_HEIGHTS = {1, 2, 9}
DST_WIDTHS, DST_HEIGHTS = {1, 63, 64, 65, 130}, {1, 3, 4, 5}
PLANE_COUNTS = {1, 4, 5, 52, 53}
SRC_OFFSETS = {0, 1, 3, 5}
INLINE_WARP = 52  # kInlineWarp of cvgs_device.h

_BUILT = {}


def built(name, twin=False):
    """(backend, iops, views) of a case over host memory, built once.  twin=False: the chain as the GPU runs it (bf16 types included)"""
    if (name, twin) not in _BUILT:
        B = MC.HostBackend(bf16_twin=twin)
        iops, views = W.CASES[name].build(B)
        _BUILT[(name, twin)] = (B, iops, views)
    return _BUILT[(name, twin)]


def test_every_chain_validates_and_names_its_kernel(lib):
    assert len(PLANAR_NAMES) == 36
    for c in W.CASES.values():
        _, iops, _ = built(c.name)
        assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, (c.name, lib.cvgs_last_error())
        assert cvgs.kernel_name(*iops) == c.kernel, (c.name, cvgs.kernel_name(*iops))
        assert c.kernel in (PACKED_NAMES if c.write.startswith("packed") else PLANAR_NAMES), c.name
        assert cvgs.kernel_name(*iops, flags=capi.CHAIN_FORCE_GENERIC) == ("warp_perspective_interp" if c.persp else "warp_affine_interp"), c.name
        rd = iops[0]
        assert c.table == (rd.table is not None or rd.batch > INLINE_WARP), c.name  # where the kernel takes its plane descriptors from
        assert rd.batch == c.n and rd.used_planes == c.used


def test_the_grid_covers_what_it_says():
    cases = list(W.CASES.values())
    exact = [c for c in cases if c.cls == W.EXACT]
    assert len(cases) <= 160 and all(c.cls in (W.EXACT, W.MODELLED) for c in cases) and len(cases) - len(exact) >= 8
    # every key -- (kernel name, descriptors from a table) -- in an exact case: 72 planar keys, and the 4 packed names both ways
    keys = {W.key_of(c) for c in exact}
    want = {(n, t) for n in PLANAR_NAMES | PACKED_NAMES for t in (False, True)}
    assert keys >= want and len(want) == 72 + 8, sorted(want - keys)
    assert {c.kernel for c in cases} == PLANAR_NAMES | PACKED_NAMES
    assert {c.kernel for c in cases if c.cls == W.MODELLED} & PACKED_NAMES and {c.store for c in cases if c.cls == W.MODELLED} >= {"f32", "f16"}
    # shapes: every source width per channel count, every source height, every target width and height -- on exact cases, on each store
    for cn in (3, 4):
        mine = [c for c in exact if c.cn == cn]
        assert {p.w for c in mine for p in c.planes[:c.used]} == SRC_WIDTHS[cn]
        assert {p.h for c in mine for p in c.planes[:c.used]} == SRC_HEIGHTS
        for persp in (False, True):
            sub = [c for c in mine if c.persp == persp]
            assert {p.w for c in sub for p in c.planes[:c.used]} == SRC_WIDTHS[cn] and {p.h for c in sub for p in c.planes[:c.used]} == SRC_HEIGHTS
    few = [c for c in exact if c.n <= 5]
    assert {c.dsize[0] for c in few} == DST_WIDTHS and {c.dsize[1] for c in few} == DST_HEIGHTS
    for store in ("f32", "f16", "bf16"):
        assert {c.dsize[0] for c in few if c.store == store} == DST_WIDTHS and {c.dsize[1] for c in few if c.store == store} == DST_HEIGHTS, store
    assert all(c.dsize == (5, 3) for c in exact if c.n >= 52) and max(c.dsize[0] for c in cases) <= 130 and max(c.dsize[1] for c in cases) <= 16
    assert {c.n for c in exact} >= PLANE_COUNTS
    # the table variant's `z < used ? z : 0`: used in {0, n-2, n} on 53 planes with a background; a caller-owned device table
    assert {c.used for c in exact if c.n == 53} == {0, 51, 53}
    assert {c.used for c in exact if c.n == 52} >= {50, 52} and {c.used for c in exact if c.n == 4} >= {2, 4}
    dev = [c for c in exact if built(c.name)[1][0].table is not None]
    assert len(dev) >= 2 and all(c.table and not c.oracle and c.used < c.n for c in dev) and {c.persp for c in dev} == {False, True}
    assert all(c.oracle for c in cases if c not in dev)
    # writes: both planar orders on every 16-bit store and on fp32, dense packed pixels and one pitched packed image with padding
    for store in ("f32", "f16", "bf16"):
        assert {c.write for c in exact if c.store == store} >= {"split", "splitT"}, store
    assert {c.write for c in exact if c.store == "f32"} >= {"packed3d", "packed2d"}
    for c in exact:
        B, iops, _ = built(c.name)
        kinds = {"split": capi.WRITE_TENSOR_SPLIT, "splitT": capi.WRITE_TENSOR_T_SPLIT, "packed3d": capi.WRITE_PIXEL_3D, "packed2d": capi.WRITE_PIXEL_2D}
        assert iops[-1].kind == kinds[c.write], c.name
        if c.write == "packed2d":
            assert B.placed.pitch > B.placed.row_bytes and B.placed.rows == c.dsize[1] and iops[-1].step == B.placed.pitch
        assert B.placed.origin >= 0 and B.placed.fill.size >= B.placed.origin + (B.placed.rows - 1) * B.placed.pitch + B.placed.row_bytes + 64
    # source memory: dense and pitched views, bases 0, 1, 3, 5 bytes into an aligned allocation, on each channel count; the bytes around the
    # view are not the image's
    for cn in (3, 4):
        mine = [c for c in exact if c.cn == cn]
        assert {c.src_off for c in mine} == SRC_OFFSETS and {c.src_pad == 0 for c in mine} == {True, False}
    for c in cases:
        _, iops, views = built(c.name)
        for z in range(c.used):
            m, pl = iops[0].mats[z] if iops[0].mats else iops[0].frame, c.planes[z]
            assert (m.cols, m.rows, m.step) == (pl.w, pl.h, pl.w * c.cn + c.src_pad) and m.data % 256 == c.src_off, c.name
            assert views[z].arr.min() >= 1 and views[z].arr.shape == (pl.h, pl.w, c.cn)
    # the taps: on exact cases of each channel count and transform
    for cn in (3, 4):
        for persp in (False, True):
            facts = sum((W.tap_facts(c) for c in exact if c.cn == cn and c.persp == persp), W.collections.Counter())
            for what in ("sx==0", "sx==w-1", "sx in (w-1,w)", "sy==0", "sy==h-1", "sy in (h-1,h)", "outside", "all outside", "tiny c%d" % cn, "windowed c%d" % cn,
                         "window clamped"):
                assert facts[what] > 0, (cn, persp, what)
    # ... and per key: border taps of each kind, a tiny and a windowed row
    for key in sorted(want):
        facts = sum((W.tap_facts(c) for c in exact if W.key_of(c) == key), W.collections.Counter())
        cn = 3 if "c3" in key[0] else 4
        for what in ("sx==0", "sx==w-1", "sx in (w-1,w)", "sy in (h-1,h)", "tiny c%d" % cn, "windowed c%d" % cn):
            assert facts[what] > 0, (key, what)
    # the perspective twins: a constant third row of 2 and of 0.5, the first two rows scaled by it
    m8 = {p.m[8] for c in exact if c.persp and c.oracle for p in c.planes}
    assert m8 == {2.0, 0.5} and all(p.m[6] == 0 and p.m[7] == 0 for c in exact for p in c.planes)
    assert all(p.m[8] == 1.0 for c in exact if not c.persp for p in c.planes)
    # the modelled cases: fractional coefficients, a perspective row that is no constant
    for c in cases:
        if c.cls == W.MODELLED:
            assert all(any(v * 2 != np.rint(v * 2) for v in p.m[:6]) for p in c.planes) and (not c.persp or all(p.m[6] != 0 and p.m[7] != 0 for p in c.planes))


def _oracle_run(oracle, c):
    B, iops, views = built(c.name, twin=True)
    B.outs[0][...] = B.placed.fill.reshape(1, -1)  # (a rebuilt case starts from its fill)
    oracle.execute(cvgs.lower(iops))
    got, moved = K.split_output(B.placed, B.result())
    assert moved.size == 0, "%s: the oracle wrote %d padding bytes" % (c.name, moved.size)
    return B, iops, views, got


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def held_to_model(c, iops, views, got):
    """(ok, worst ratio, largest excluded share of a plane, text): Result.check's bound, the output in its own number format"""
    res = F.evaluate(iops, views)
    ok, ratio = res.check(res.logical(MC.widen_output(np.ascontiguousarray(got).reshape(-1), iops[-1].dst_type), iops[-1].kind))
    share = float(res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1).max())
    worst = float(np.nanmax(ratio))
    return bool(ok.all()), worst, share, "%d of %d elements outside the bound, worst ratio %.3f" % (int((~ok).sum()), ok.size, worst)


@pytest.mark.parametrize("family", W.FAMILIES, ids=[f.replace(" ", "_") for f in W.FAMILIES])
def test_oracle_gives_the_exact_expectation(oracle, family):
    failed, ran, worst = [], 0, 0.0
    for c in W.cases_of(family):
        if not c.oracle:
            continue
        B, iops, views, got = _oracle_run(oracle, c)
        ran += 1
        if c.cls == W.EXACT:
            want = c.expected(B)
            assert want.shape == got.shape and want.dtype == got.dtype, c.name
            bad = bits(want) != bits(got)
            if bad.any():
                at = np.unravel_index(int(np.argmax(bad)), bad.shape)
                failed.append("%s: %d of %d elements differ, first at %r: %r, expected %r" % (c.name, int(bad.sum()), bad.size, at, got[at], want[at]))
        else:
            ok, ratio, _, text = held_to_model(c, iops, views, got)
            worst = max(worst, ratio)
            if not ok:
                failed.append("%s: %s" % (c.name, text))
    print("RATIO oracle %-20s %-12s %.4f" % (family, "%d cases" % ran, worst))
    assert ran >= 10 and not failed, "%d of %d cases:\n%s" % (len(failed), ran, "\n".join(failed))


def test_modelled_cases_exclude_at_most_one_percent_of_a_plane():
    """from the model alone: tests/test_gpu_model.held_to_model's condition, per plane"""
    largest = 0.0
    for c in W.CASES.values():
        if c.cls != W.MODELLED:
            continue
        _, iops, views = built(c.name)
        res = F.evaluate(iops, views)
        share = res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1)
        largest = max(largest, float(share.max()))
        assert (share <= 0.01).all(), (c.name, share)
        inside = (res.v != W.apply_tail(np.zeros(c.cn), c.tail, c.cn)[0]).any(axis=-1).reshape(c.n, -1).mean(axis=1)
        assert (inside > 0.1).all() and (inside < 1.0).all(), (c.name, inside)  # the planes cross a border and are not empty
    print("EXCLUDED largest share of a plane %.4f" % largest)


def test_the_model_alone_could_not_hold_an_integer_translation():
    """the figure of the module docstring of tests/warp_edge_cases.py: [1 0 -3; 0 1 -2] on a 13 x 9 source into 20 x 16 excludes 13.75 % of the plane"""
    pl = W.Plane(13, 9, (1.0, 0.0, -3.0, 0.0, 1.0, -2.0, 0.0, 0.0, 1.0), 0)
    B = MC.HostBackend()
    iops, views = W.warp_edge_case(3, False, "plain", "f32", "split", [pl], (20, 16))(B)
    res = F.evaluate(iops, views)
    assert abs(float(res.excluded.mean()) - 0.1375) < 1e-12


def test_the_exact_expectation_tells_three_near_misses_apart():
    """see the module docstring"""
    needs = {"right_tap_zero": ("sx in (w-1,w)",), "inside_up_to_w-1": ("sx in (w-1,w)",), "bottom_row_unclamped": ("sy in (h-1,h)",)}
    told = {}
    for c in W.CASES.values():
        if c.cls != W.EXACT:
            continue
        facts = W.tap_facts(c)
        spec = W.expected_values(c)
        for rule in W.RULES[1:]:
            other = W.expected_values(c, rule)
            has = any(facts[k] > 0 for k in needs[rule])
            assert bool((spec != other).any()) == has, (c.name, rule, facts)
            if (bits(W.to_store_bits(spec, c.store)) != bits(W.to_store_bits(other, c.store))).any():  # (bf16's one rounding may hide a single tap)
                told.setdefault(W.key_of(c), set()).add(rule)
    want = {(n, t) for n in PLANAR_NAMES | PACKED_NAMES for t in (False, True)}
    assert all(told.get(k) == set(W.RULES[1:]) for k in want), sorted(k for k in want if told.get(k) != set(W.RULES[1:]))
