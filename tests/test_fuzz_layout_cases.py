"""The generator of the layout fuzzer (tests/fuzz_layout_cases.py) pinned on the CPU: every chain it spells is one the library accepts
(cvgs_validate) and dispatches (cvgs_kernel_name, the real dispatch as a dry run), its expected value is computable and non-trivial, the
default seed ranges of tests/test_gpu_fuzz_layouts.py cover the space and the kernel families, and the expected values -- composed from two
oracle runs for 4:2:2 / 4:4:4, the oracle's fp32 twin rounded on the host for bf16 -- lie within the derived bound of the independent
float64 model (tests/f64_model.py).  No GPU needed.

Kernel names the default seed ranges (seeds 0..479 with their flags, big seeds 500000..500023) reach:
  generic_inline8, generic64_inline8, warp64_inline8, warp_affine_interp, warp_perspective_interp (the interpreted kernels);
  k_yuv422_resize_arith, k_yuv422_resize_arith_bf16, k_yuv422_resize_arith_f16, k_yuv422_resize_interp;
  k_yuv444_resize_arith, k_yuv444_resize_interp;
  pointwise4_yuv422, pointwise4_yuv422_bf16, pointwise4_yuv422_f16, pointwise4_yuv444, pointwise4_yuv444_bf16, pointwise4_yuv444_f16,
  pointwise4_i420_bf16, pointwise4_p010_bf16;
  k1_u8c3_packed_bf16, k1_u8c4_mul_sub_div_bf16; k4_nv12_resize_arith_bf16, k4_nv12_resize_swap_mul_sub_div_bf16;
  warp_affine_u8c3_swap_mul_sub_div_bf16, warp_affine_u8c4_interp_bf16, warp_perspective_u8c3_interp_bf16."""
import collections
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import fuzz_layout_cases as G
from tests import model_cases as MC
from tests import yuv422_cases as Y422

DEFAULT_SEEDS = list(range(G.DEFAULT_N)) + [G.BIG_BASE + i for i in range(G.DEFAULT_BIG_N)]


def flags_of(seed):
    return 0 if seed >= G.BIG_BASE else G.FLAGS[seed % 4]


class Record:
    """What the tests below ask about one seed; the case itself (sources, expected value: megabytes at frame sizes) is dropped at once, so
    that this file leaves nothing behind in the process that runs the rest of the suite."""

    def __init__(self, lib, seed):
        c = G.case(seed, big=seed >= G.BIG_BASE)
        ops, _ = c.lowered(bf=True)
        self.what, self.family, self.read, self.layout, self.views = c.what, c.family, c.read, c.layout, list(c.views)
        self.bf16_source, self.bf16_store, self.write_kind, self.used, self.n, self.dsize = c.bf16_source, c.bf16_store, c.write_kind, c.used, c.n, c.dsize
        self.crop_mode, self.resize = c.crop_mode, c.resize
        s = c.sources[0]
        self.odd_coprime = c.read == "yuv444" and bool(s.step & 1 and s.uv & 1 and np.gcd(s.step, s.uv) == 1)
        rc = lib.cvgs_validate(C.byref(cvgs.lower(ops, flags_of(seed)).desc))
        self.refusal = lib.cvgs_last_error().decode() if rc else None
        self.kernel = cvgs.kernel_name(*ops, flags=flags_of(seed)) if rc == 0 else None
        self.ref_ok = c.ref.shape == tuple(c.shape) and c.ref.dtype == c.np_dtype and bool(c.ref.any())
        self.model = None
        if seed < G.BIG_BASE:
            r = held_to_model(c)
            if r is not None:
                ok, ratio, checked, share = r
                bad = ~ok & checked
                self.model = dict(checked=int(checked.sum()), bad=int(bad.sum()), first=tuple(int(i) for i in np.argwhere(bad)[0]) if bad.any() else None,
                                  worst=float(np.nanmax(np.where(checked, ratio, 0))) if checked.any() else 0.0,
                                  share=None if share is None else [float(v) for v in share[:max(c.used, 1)]])


@pytest.fixture(scope="module")
def records(lib):
    """one pass over the default seed ranges"""
    return {seed: Record(lib, seed) for seed in DEFAULT_SEEDS}


def test_every_chain_is_valid_and_has_a_nontrivial_expected_value(records):
    """300 seeds and 20 whole-frame ones: accepted by cvgs_validate, dispatched without a refusal, expected value not all zero"""
    for seed in list(range(300)) + [G.BIG_BASE + i for i in range(20)]:
        r = records[seed]
        assert r.refusal is None and r.kernel, (r.what, r.refusal)
        assert r.ref_ok, r.what


def test_the_default_seed_ranges_cover_the_space(records):
    """each class at least 10 times over the default ranges: a generator that collapses fails here"""
    count = collections.Counter()
    for seed in DEFAULT_SEEDS:
        c = records[seed]
        if c.read == "yuv422":
            count["layout %d" % c.layout] += 1
            count["4:2:2 odd width"] += any(v[3] & 1 for v in c.views)
            count["4:2:2 odd y"] += any(v[2] & 1 for v in c.views)
        if c.read == "yuv444":
            count["i444 odd origin"] += any((v[1] & 1) and (v[2] & 1) for v in c.views)
            count["i444 one or two columns"] += any(v[3] <= 2 for v in c.views)
            count["i444 odd coprime step"] += c.odd_coprime
        count["bf16 source"] += c.bf16_source
        count["bf16 store"] += c.bf16_store
        count["write " + c.write_kind] += 1
        count["used < n"] += c.used < c.n
        count["crop views"] += bool(c.crop_mode and c.read in ("yuv422", "yuv444"))
        count["family %d" % c.family] += 1
        if c.resize or c.read == "warp":
            count["width %d" % c.dsize[0]] += 1
            count["height %d" % c.dsize[1]] += 1
    want = ["layout %d" % l for l in Y422.LAYOUTS] + ["4:2:2 odd width", "4:2:2 odd y", "i444 odd origin", "i444 one or two columns", "i444 odd coprime step",
                                                      "bf16 source", "bf16 store", "used < n", "crop views"]
    want += ["write " + k for k in G.WRITE_KINDS] + ["family %d" % f for f in G.FAMILIES] + ["width %d" % w for w in G.EDGE_W] + ["height %d" % h for h in G.EDGE_H]
    print("COVERAGE", [(k, count[k]) for k in want])
    assert not [k for k in want if count[k] < 10], {k: count[k] for k in want if count[k] < 10}


def test_the_default_seed_ranges_reach_the_kernel_families(records):
    """cvgs_kernel_name of every default seed under its flags (the set is recorded in the module's docstring)"""
    names = collections.Counter()
    by_read = collections.defaultdict(set)
    for seed in DEFAULT_SEEDS:
        names[records[seed].kernel] += 1
        by_read[records[seed].read].add(records[seed].kernel)
    print("KERNELS", sorted(names.items()))
    reached = lambda pool, pre, suf="": any(n.startswith(pre) and n.endswith(suf) for n in pool)  # noqa: E731
    assert reached(by_read["yuv422"], "k_yuv422_resize") and reached(by_read["yuv444"], "k_yuv444_resize")
    assert reached(by_read["yuv422"], "pointwise4_yuv422") and reached(by_read["yuv444"], "pointwise4_yuv444")
    assert reached(names, "generic") and reached(by_read["yuv422"], "generic") and reached(by_read["yuv444"], "generic")  # the interpreted kernel
    assert reached(names, "k1_", "_bf16"), "no bf16-storing K1 kernel"
    assert reached(names, "k4_nv12_", "_bf16") or reached(names, "k_yuv4", "_bf16"), "no bf16-storing K4 / YUV kernel"
    assert reached(names, "k_yuv422_resize", "_bf16") or reached(names, "k_yuv444_resize", "_bf16")
    assert reached(names, "pointwise", "_bf16"), "no bf16-storing pointwise kernel"
    assert reached(names, "warp_", "_bf16"), "no bf16-storing warp kernel"


# ---- the float64 model --------------------------------------------------------------------------------------------------------------------
def model_views(c):
    out = []
    for (i, x, y, w, h) in c.views:
        s = c.sources[i]
        if c.read == "yuv422":
            out.append(F.View(s.s[:, :s.w], x, y, w, h))
        elif c.read == "yuv444":
            out.append(F.View(np.stack(s.planes), x, y, w, h))
        elif c.read == "yuv420":
            out.append(F.View(s.arr, x, y, w, h, luma_h=s.luma_rows))
        else:
            out.append(F.View(s.arr, x, y, w, h))
    return out


def held_to_model(c):
    """None: the chain is outside the model (CV_64F values, arithmetic on integer-typed values, GRAY on other depths).  Else (ok, ratio,
    checked, excluded share per plane): ok / ratio over [plane][y][x][c]; checked: the elements the model speaks about.

    The model's bound is relative (u |result| per operation): it says nothing where an operation overflows or lands among the subnormals.  A
    CV_16BF source holds such values on purpose, so the pixels whose READ-stage value (the model's own, from the source alone) is not finite,
    non-zero below 1e-30, or large enough to overflow at some stage are left out, all channels of the pixel (a reorder or GRAY mixes them);
    so are the default-value planes of a per-pixel read, which the model does not draw, and the
    part of a plane beyond its own (smaller) warp size."""
    if any(isinstance(s, G.PlainSrc) and capi.type_depth(s.cv_type) == cvgs.CV_64F for s in c.sources):
        return None
    ops, _ = c.lowered(bf=True)
    views = model_views(c)
    try:
        with np.errstate(all="ignore"):
            res = F.evaluate(ops, views)
            rd_only = F.evaluate([ops[0], ops[-1]], views)
    except NotImplementedError:
        return None
    got = MC.widen_output(c.logical(c.ref), ops[-1].dst_type)[:, :res.v.shape[1], :res.v.shape[2]]  # (differently sized warps: the largest plane)
    with np.errstate(all="ignore"):
        ok, ratio = res.check(got)
        v0 = np.abs(rd_only.v)
        wild = (~np.isfinite(v0) | ~np.isfinite(rd_only.b) | ((v0 > 0) & (v0 < 1e-30))).any(axis=-1)  # (b: a warp's bound looks at the 3 x 3 cells around)
        # the largest magnitude a pixel can reach at any stage, from the program's own constants: beyond the largest float (the largest
        # binary16 value at a cast to CV_16F) the operation overflows
        reach = np.where(np.isfinite(v0), v0, 0.0).max(axis=-1)
        for iop in ops[1:-1]:
            for opcode, aux, operand in iop.ops:
                mags = [abs(float(x)) for x in (operand or []) if float(x) != 0.0]
                if opcode == F.OP_MUL and mags:
                    reach = reach * max(max(mags), 1.0)
                elif opcode == F.OP_DIV and mags:
                    reach = reach / min(min(mags), 1.0)
                elif opcode in (F.OP_ADD, F.OP_SUB) and mags:
                    reach = reach + max(mags)
                elif opcode in (F.OP_CAST, F.OP_CAST_TRUNC) and aux == F.DEPTH_16F:
                    wild |= reach > 65000.0
                wild |= reach > 1e38
    checked = np.broadcast_to(~wild[..., None], ok.shape).copy()
    if ops[0].dsize is None:
        checked[c.used:] = False
    if c.warp_sizes:
        for z, (w, h) in enumerate(c.warp_sizes):
            checked[z, h:] = False
            checked[z, :, w:] = False
    share = res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1) if res.excluded is not None else None
    return ok, ratio, checked, share


@pytest.mark.parametrize("first", range(0, G.DEFAULT_N, 60))
def test_expected_values_lie_within_the_model_bound(records, first):
    """the fuzz expectations tied to the independent model as well as to the oracle; a warp case leaves at most 1 % of a plane out near the
    source border (the condition of tests/test_gpu_model.py)"""
    held = 0
    for seed in range(first, first + 60):
        r, m = records[seed], records[seed].model
        if m is None:
            continue
        if m["share"] is not None:
            assert max(m["share"]) <= 0.01, (r.what, m["share"])
        if not m["checked"]:
            continue
        held += 1
        assert not m["bad"], "%s: %d of %d elements outside the bound, worst ratio %.3f at %r" % (r.what, m["bad"], m["checked"], m["worst"], m["first"])
    print("MODEL seeds %d..%d: %d held to the model" % (first, first + 59, held))
    assert held >= 10


def test_the_model_subset_holds_every_family(records):
    fams = collections.Counter()
    for seed in range(G.DEFAULT_N):
        if records[seed].model is not None:
            fams[(records[seed].family, records[seed].read)] += 1
    print("MODEL SUBSET", sorted(fams.items()))
    for fam in G.FAMILIES:
        assert sum(v for (f, _), v in fams.items() if f == fam) >= 10, fams
    assert sum(v for (_, r), v in fams.items() if r == "yuv422") >= 10 and sum(v for (_, r), v in fams.items() if r == "yuv444") >= 10
