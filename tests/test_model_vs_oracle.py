"""The CPU oracle held to the independent float64 model (tests/f64_model.py) over the grid of tests/model_cases.py: every output element
must lie within the model's DERIVED bound.  No GPU needed.

The sensitivity tests flip each defining choice of the model in turn and assert that the oracle then falls OUTSIDE the bound on some case
of the grid: the bound is tight enough to catch each of those mistakes.

Largest |oracle - model| / tolerance per family on this grid (1 = at the bound):  K1 8u 0.36, 16u 0.38, 16s 0.34, 32f 0.47, 16f 0.34,
16bf 0.35; YUV nv12 / nv21 / i420 / yv12 0.79, p010 0.75, yuyv / uyvy 0.80, i444 0.59; warp 0.33 (fp32 outputs; 0.50 is the integer output's half
step); chains 0.60; stores 1.00 -- a 16-bit float output's tolerance IS one rounding of its format, which a random input reaches, so
that figure says nothing about slack; the chain bound underneath it is the K1 / chains one.  No family sits below 0.01."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import model_cases as MC
from tests.test_bf16_types import rne_bf16

_ORACLE_CACHE = {}


def oracle_output(oracle, name):
    """(iops, views, got as float64 in logical order, write kind) of a case run on the oracle."""
    if name in _ORACLE_CACHE:
        return _ORACLE_CACHE[name]
    family, build, _ = MC.CASES[name]
    B = MC.HostBackend()
    iops, views = build(B)
    if getattr(build, "layout422", None) is not None:
        from tests import yuv422_cases as Y
        Y.Expect(oracle, B.sources, build.layout422).run(iops)
    elif getattr(build, "layout444", False):
        from tests import yuv444_cases as Y444
        Y444.Expect(oracle, B.surfs444).run(iops)
    else:
        oracle.execute(cvgs.lower(iops))
    got = B.result()
    if B.twin:  # the model sees the chain itself (bf16 sources as bit patterns, the conversion to bf16 as a stage), not the oracle's twin
        iops, views = build(MC.HostBackend(bf16_twin=False))
    if B.rounded_to_bf16:  # the oracle's fp32 twin, rounded on the host (tests/test_bf16_types.py pins rne_bf16 against torch)
        got = F.widen(rne_bf16(got), F.DEPTH_16BF)
    else:
        got = MC.widen_output(got, iops[-1].dst_type)
    _ORACLE_CACHE[name] = (iops, views, got, iops[-1].kind)
    return _ORACLE_CACHE[name]


def compare(oracle, name, sw=F.SPEC):
    iops, views, got, kind = oracle_output(oracle, name)
    res = F.evaluate(iops, views, sw)
    return res, res.check(res.logical(got, kind))


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_oracle_within_the_model_bound(oracle, name):
    res, (ok, ratio) = compare(oracle, name)
    print("RATIO oracle %-10s %-40s %.4f" % (MC.CASES[name][0], name, float(np.nanmax(ratio))))
    if res.excluded is not None:
        share = res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1)
        assert (share <= 0.01).all(), "excluded share of a warp plane above 1 %%: %r" % share
    assert np.isfinite(res.v[~np.isnan(res.v)]).all() and res.v.std() > 0
    assert ok.all(), "%s: %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        name, int((~ok).sum()), ok.size, float(np.nanmax(ratio)), np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


def test_every_case_is_one_the_product_accepts(lib):
    """the GPU file runs the same grid: a case the library refused would only show there"""
    for name, (family, build, kernel) in sorted(MC.CASES.items()):
        B = MC.HostBackend(bf16_twin=False)
        iops, _ = build(B)
        assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, name
        if kernel is not None:
            assert cvgs.kernel_name(*iops).startswith(kernel), (name, cvgs.kernel_name(*iops))


def test_excluded_share_needs_no_code_under_test():
    """the warp matrices keep the share of pixels within delta of the source border at or below 1 % by the model alone"""
    for name, (family, build, _) in sorted(MC.CASES.items()):
        if family != "warp":
            continue
        iops, views = build(MC.HostBackend())
        res = F.evaluate(iops, views)
        assert res.excluded is not None and res.excluded.mean() <= 0.01, name
        assert (res.v != 0).mean() > 0.3, name  # and most of the picture is drawn


# which cases can show each switch (a subset keeps the pass cheap; any one of them falling outside the bound proves the point)
SENSITIVITY = {
    "half_pixel_centres": ["k1_8uc3", "k1_32fc1"],
    "weights_from_clamped": ["k1_8uc3_up", "k1_8uc3"],
    "chroma_rounds_up": ["yuv_px_nv12_chroma_checker", "yuv_rs_yuyv_chroma_checker"],
    "chroma_from_crop_origin": ["yuv_rs_nv12_crop", "yuv_rs_yuyv_crop_odd_y"],
    "uv_swapped": ["yuv_px_nv12_r0_p0_a0", "yuv_rs_i420_r1_p1_a0"],
    "yuyv_uyvy_swapped": ["yuv_px_yuyv_r0_p0_a0", "yuv_rs_uyvy_r1_p1_a0"],
    "blend_before_convert": ["yuv_rs_nv12_chroma_checker", "yuv_rs_yuyv_r1_p1_a0"],
    "limited_as_full": ["yuv_px_nv12_r1_p0_a0", "yuv_rs_p010_r1_p2_a1"],
    "bt601_for_bt709": ["yuv_px_nv12_r0_p1_a0", "yuv_rs_uyvy_r1_p1_a0"],
    "saturate_truncates": ["chain_convert_saturates", "chain_sat_f32"],
    "ar_extent_truncated": ["k1_8uc3_ar", "k1_8uc3_ar_left"],
    "warp_border_replicate": ["warp_affine", "warp_persp_0"],
    "coefficient_digit_off": ["yuv_px_nv12_r0_p0_a0", "yuv_px_p010_r1_p2_a0", "yuv_px_nv12_r1_p1_a0"],
    "i444_chroma_subsampled": ["yuv_px_i444_chroma_checker", "yuv_rs_i444_crop_odd"],
}


def test_every_switch_has_a_sensitivity_case():
    assert set(SENSITIVITY) == set(F.SPEC) and not any(F.SPEC.values())


@pytest.mark.parametrize("switch", sorted(F.SPEC))
def test_flipping_a_defining_choice_is_caught(oracle, switch):
    caught = {}
    for name in SENSITIVITY[switch]:
        _, (ok, ratio) = compare(oracle, name, F.switches(**{switch: True}))
        caught[name] = (int((~ok).sum()), float(np.nanmax(ratio)))
    print("SENSITIVITY %-26s %r" % (switch, caught))
    assert any(n > 0 for n, _ in caught.values()), caught


def test_number_formats_against_numpy():
    """the model's binary16 rounding against numpy's, its bfloat16 rounding against the bit-level rule, on every class of value"""
    from tests.test_bf16_types import special_values
    v = special_values().astype(np.float64)
    v = v[np.isfinite(v)]
    with np.errstate(over="ignore"):
        want16 = v.astype(np.float32).astype(np.float16).astype(np.float64)
    assert np.array_equal(F.rne_float(v, F.DEPTH_16F), want16)
    assert np.array_equal(F.rne_float(v, F.DEPTH_16BF), F.widen(rne_bf16(v.astype(np.float32)), F.DEPTH_16BF))
    assert F.half_ulp(1.0, F.DEPTH_16F) == 2.0 ** -11 and F.half_ulp(1.0, F.DEPTH_16BF) == 2.0 ** -8 and F.half_ulp(3.0, F.DEPTH_32F) == 2.0 ** -23
