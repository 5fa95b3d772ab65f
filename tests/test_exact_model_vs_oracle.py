"""The CPU oracle held to the exact model (tests/exact_model.py) over the grid of tests/exact_cases.py: casts between all nine depths, arithmetic
on integer-typed values, CV_64F chains, channel moves, write kinds, default-value planes.  The comparison is EQUALITY.  No GPU needed.

The oracle does not know bfloat16: cases with a CV_16BF source, stage or output are evaluated by the model only here (tests/test_bf16_types.py
pins the bit-level rule the model's rounding is checked against below) and are held on the GPU.

The sensitivity test flips each defining choice of the model in turn and asserts that the oracle then DIFFERS from the model on some case of
the grid: a switch the grid could not see would mean the grid is missing an input."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import exact_cases as X
from tests import exact_model as E

_ORACLE_CACHE = {}


def built(name):
    """(build, iops, arrays, got in logical order or None for a bf16 case, output depth) of a case run on the oracle"""
    if name not in _ORACLE_CACHE:
        from oracle import oracle_binding
        _, build = X.CASES[name]
        B = X.HostBackend()
        iops, arrays = build(B)
        got = None
        if not X.has_bf16(iops):
            oracle_binding.execute(cvgs.lower(iops))
            shape = (iops[0].batch,) + np.asarray(arrays[0]).shape[:2] + (capi.type_cn(iops[-1].dst_type),)
            got = X.written(build, B.results(), shape)
        _ORACLE_CACHE[name] = (build, iops, arrays, got, E.depth_of(iops[-1].dst_type))
    return _ORACLE_CACHE[name]


def describe(name, iops, arrays, got, want, bad):
    k = np.argwhere(bad)[:6]
    src = np.stack([np.asarray(a) for a in arrays]) if len(arrays) else None
    rows = []
    for idx in k:
        z, y, x, c = (int(v) for v in idx)
        s = src[z, y, x].tolist() if src is not None and z < src.shape[0] else "default value"
        rows.append("at %r: source %r, got %r, model %r" % ((z, y, x, c), s, got[z, y, x, c].item(), want[z, y, x, c].item()))
    return "%s: %d of %d elements differ; %s" % (name, int(bad.sum()), bad.size, "; ".join(rows))


@pytest.mark.parametrize("group", X.GROUPS)
def test_oracle_equals_the_exact_model(oracle, group):
    compared = 0
    for name in X.names_of(group):
        build, iops, arrays, got, depth = built(name)
        want = E.evaluate(iops, arrays)
        assert want.dtype == E.NP_DTYPE[depth] and want.shape[0] == iops[0].batch, name
        if got is None:
            continue
        bad = E.differs(got, want, depth)
        assert not bad.any(), describe(name, iops, arrays, got, want, bad)
        compared += 1
    assert compared > 0 or group == "cast 16bf", group  # (every case of that group has a CV_16BF source)


def test_only_bf16_cases_are_model_only():
    skipped = [n for n in sorted(X.CASES) if built(n)[3] is None]
    assert skipped and all("16bf" in n for n in skipped), skipped
    assert len(skipped) < len(X.CASES) / 3


def test_every_case_is_one_the_product_accepts_and_reaches_its_kernels(lib):
    """the GPU file runs the same grid: a case the library refused, or a kernel the grid stopped reaching, would only show there"""
    seen = set()
    for name, (group, build) in sorted(X.CASES.items()):
        iops, _ = build(X.HostBackend())
        assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, (name, lib.cvgs_last_error())
        for flags in (capi.CHAIN_DEFAULT, capi.CHAIN_FORCE_GENERIC):
            k = cvgs.kernel_name(*iops, flags=flags)
            seen.add(k)
            if flags == capi.CHAIN_FORCE_GENERIC:
                assert k.startswith("generic") or k.endswith("_interp"), (name, k)
            if X.has_64f(iops):
                assert k.startswith("generic64"), (name, k)
    assert {"generic_inline8", "generic64_inline8"} <= seen, seen
    assert seen & {"generic_inline64", "generic_table"}, seen
    assert any(k.startswith("pointwise") for k in seen), seen


@pytest.mark.parametrize("name", sorted(X.REFUSED))
def test_refused_chains_are_refused_with_their_text(lib, name):
    build, text = X.REFUSED[name]
    iops, _ = build(X.HostBackend())
    assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == capi.ERR_UNSUPPORTED
    assert text in lib.cvgs_last_error().decode(), lib.cvgs_last_error()
    with pytest.raises(ValueError):
        E.evaluate(iops, [np.zeros((2, X.W, 3), E.NP_DTYPE[E.depth_of(iops[0].src_type)])])


def test_the_refused_list_covers_no_cast_pair():
    for name, (build, _) in X.REFUSED.items():
        iops, _ = build(X.HostBackend())
        assert any(o[0] in (capi.OP_MUL, capi.OP_ADD, capi.OP_SUB, capi.OP_DIV) for i in iops[1:-1] for o in i.ops), name
    pairs = {(s, d, m) for s in X.DEPTHS for d in X.DEPTHS for m in ("round", "trunc")}
    assert all("cast_%s_%s_%s_c1" % (X.NAMES[s], X.NAMES[d], m) in X.CASES for s, d, m in pairs) and len(pairs) == 162


def test_the_grid_is_what_it_says():
    """sources hold their whole edge list; rows are no multiple of 4 or 64; every write kind, a default-value plane per source class, nine planes"""
    for d in X.DEPTHS:
        a = X.source(d, 1, 0, rows=2)
        e = X.edge_list(d)
        assert a.reshape(-1)[:e.size].tobytes() == e.tobytes() and e.size < a.size / 1.5, X.NAMES[d]
    i32 = set(X.edge_list(X.D32S).tolist())
    assert {0x7F800000, 0x7F800001, 0x7FC00000, 0xFF800001 - 2 ** 32, 0xFFC00000 - 2 ** 32, 2 ** 24 + 1, 2 ** 24 + 3, -2 ** 31, 2 ** 31 - 1} <= i32
    f64 = set(X.edge_list(X.D64F).tolist())
    assert {2147483647.4, 2147483647.5, 2049.0000001, 65519.9, 65520.0, 1e300, -1e300, 2147483520.0, -2147483904.0, 0.49999997019767761} <= f64
    writes, used, batches = set(), set(), set()
    for name, (group, build) in X.CASES.items():
        assert build.w <= 131 and build.w % 4 and build.w % 64 and build.rows <= 3, name
        iops, _ = build(X.HostBackend())
        writes.add(build.write)
        batches.add(build.batch)
        if iops[0].used_planes < iops[0].batch:
            d = E.depth_of(iops[0].src_type)
            used.add("int" if E.is_int(d) else X.NAMES[d])
    assert writes == {"packed2d", "packed3d", "split", "splitT", "batch2d"} and max(batches) >= 9 and {"int", "32f", "64f"} <= used


# which cases show each switch first (any case of the grid may; these keep the pass cheap)
HINTS = {
    "half_rounds_once": ["cast_64f_16f_round"], "float_rounds_toward_zero": ["cast_32s_32f_round"], "subnormals_flushed": ["cast_32f_16f_round"],
    "zero_sign_dropped": ["cast_32f_64f_round"], "nan_to_int_is_min": ["cast_32f_8u_round"], "convert_truncates": ["cast_32f_8u_round"],
    "cast_rounds": ["cast_32f_8u_trunc"], "s32_overflow_is_min": ["cast_32f_32s_round"], "int_to_int_wraps": ["cast_16s_8u_round"],
    "alpha_beta_as_double": ["f64_8u_cvt_to_64f"], "convert_in_double": ["write_split_u8_f32", "f64_32f_cvt_to_32f"], "f64_scalar_narrowed": ["f64_64f_add_to_64f"],
    "f32_stage_in_double": ["f64_32f_mixed_to_64f", "f64_32f_mixed_to_32f"], "int_scalar_rounds": ["int_16s_c1_chain0"], "int_scalar_unclamped": ["int_8u_c3_chain1", "int_8u_c4_chain3"],
    "int_arith_in_32_bits": ["int_32s_c3_chain2"], "int_div_floors": ["int_16s_c1_chain3"], "int_div_by_zero_is_max": ["int_8u_c3_chain1"],
    "int_result_wraps": ["int_8u_c1_chain0"], "background_skips_chain": ["used_"], "background_as_double": ["used_64f", "used_32s"],
}


def test_every_switch_has_a_hint():
    assert set(HINTS) == set(E.SPEC) and not any(E.SPEC.values())


@pytest.mark.parametrize("switch", sorted(E.SPEC))
def test_flipping_a_defining_choice_is_seen_by_the_oracle(oracle, switch):
    sw = E.switches(**{switch: True})
    hinted = [n for n in sorted(X.CASES) if any(n.startswith(h) for h in HINTS[switch])]
    for name in hinted + [n for n in sorted(X.CASES) if n not in hinted]:
        build, iops, arrays, got, depth = built(name)
        if got is None:
            continue
        bad = E.differs(got, E.evaluate(iops, arrays, sw), depth)
        if bad.any():
            print("SENSITIVITY %-26s %-36s %d of %d elements" % (switch, name, int(bad.sum()), bad.size))
            return
    pytest.fail("no case of the grid shows %s: the grid is missing an input" % switch)


def _bf16_bits_rule(f32):
    """round to nearest even on the bits (tests/test_bf16_types.py pins this rule against torch)"""
    b = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f32), np.uint16(0x7FC0), r)


def test_sixteen_bit_roundings_on_every_pattern():
    """the model's binary16 rounding against numpy's float16, its bfloat16 rounding against the bit-level rule: around EVERY one of the 2^16
    patterns of each format -- the value itself, the midpoint to its successor, and one float ulp to either side of both"""
    for depth in (E.DEPTH_16F, E.DEPTH_16BF):
        pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        with np.errstate(all="ignore"):
            v = pat.view(np.float16).astype(np.float32) if depth == E.DEPTH_16F else E.widen(pat, depth)
            nxt = np.roll(v, -1)
            mid = ((v.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)  # exact: neighbours of a 16-bit format, in float
            cand = np.concatenate([v, mid, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf)),
                                   np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                                   np.array([65519.996, 65520.0, 3.3961775e38, 3.4028235e38, 2.9802322e-08, 1e-46], np.float32)])
            cand = np.concatenate([cand, -cand])
            got = E.round_to_format(cand.astype(np.float64), depth).astype(np.float32)
            if depth == E.DEPTH_16F:
                want = cand.astype(np.float16).astype(np.float32)
            else:
                want = E.widen(_bf16_bits_rule(cand), depth)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (depth, cand[~same][:8], got[~same][:8], want[~same][:8])
        assert E.narrow(got, depth).dtype == E.NP_DTYPE[depth]
    # and the float format itself against numpy's double -> float conversion
    x = X.source(X.D64F, 1, 5, rows=3).reshape(-1)
    with np.errstate(all="ignore"):
        assert not E.differs(E.round_to_format(x, E.DEPTH_32F).astype(np.float32), x.astype(np.float32), E.DEPTH_32F).any()
