"""The table of tests/k4_x2_cases.py without a GPU: every case is one the product sends to k4_nv12_x2 in the form the table names (a dry
run over host views; under the CVGS_K4_X2 hook the name carries "@r1" / "@r2", without it the name is what it always was), that form is
what the Python restatement of launch_nv12_x2's rule gives, the table holds what its docstring says, and the CPU oracle's picture of
every case lies within the float64 model's derived bound (tests/f64_model.py) -- the figure the GPU item then holds the kernels to."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import k4_x2_cases as K

CASES = list(K.CASES.values())


def _name(monkeypatch, case, flags=0):
    if case.hook:
        monkeypatch.setenv("CVGS_K4_X2", "1")
    else:
        monkeypatch.delenv("CVGS_K4_X2", raising=False)
    chain, _ = K.host_ops(case)
    return cvgs.kernel_name(*chain, flags=flags)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_product_names_the_form_the_rule_gives(monkeypatch, lib, case):
    chain, _ = K.host_ops(case)
    assert lib.cvgs_validate(C.byref(cvgs.lower(chain).desc)) == 0
    got = _name(monkeypatch, case)
    assert got == case.want, got
    assert case.want == K.expected_name(case), (case.want, K.expected_name(case))
    # the other two kernels the GPU item compares with are other kernels, and carry no suffix under the hook
    assert _name(monkeypatch, case, capi.CHAIN_NO_THREAD_FUSION) == case.want.split("@")[0].replace("k4_nv12_x2", "k4_nv12_resize")
    assert "x2" not in _name(monkeypatch, case, capi.CHAIN_FORCE_GENERIC)


def test_the_suffix_appears_under_the_hook_only(monkeypatch):
    case = K.CASES["hook_off_256x2048"]  # x2 by the size rule
    monkeypatch.delenv("CVGS_K4_X2", raising=False)
    chain, _ = K.host_ops(case)
    assert cvgs.kernel_name(*chain) == "k4_nv12_x2_swap_mul_sub_div"
    monkeypatch.setenv("CVGS_K4_X2", "1")
    assert cvgs.kernel_name(*chain) == "k4_nv12_x2_swap_mul_sub_div@r2"
    monkeypatch.setenv("CVGS_K4_X2", "0")  # never x2: the one-pixel kernel, no suffix
    assert cvgs.kernel_name(*chain) == "k4_nv12_resize_swap_mul_sub_div"


def test_the_table_is_not_vacuous():
    rows = {c.name: K.rows_per_wave(len(c.crops), c.dst, c.write) for c in CASES}
    piped = [c for c in CASES if rows[c.name] == 2]
    assert all(c.want.endswith("@r2") for c in piped if c.hook) and all("@" not in c.want for c in CASES if not c.hook)
    assert len([c for c in piped if c.want.endswith("@r2")]) >= 10
    assert len([c for c in piped if c.dst[1] % 2 == 1]) >= 3            # a last wave whose second row is past the target
    assert any(len(c.crops) > 1 and c.write == K.T_SPLIT for c in piped)  # CNHW strides with z != 0
    assert any(not c.hook for c in piped)                                 # the product's own rules reach the form
    assert any(rows[c.name] == 1 and c.dst[0] % 2 == 1 for c in CASES) and any(rows[c.name] == 1 and c.dst[0] % 2 == 0 for c in CASES)
    # the conversion variants, all in the pipelined form
    assert {(c.layout, c.range_, c.swap) for c in piped} >= {(K.NV12, K.FULL, True), (K.NV21, K.LIMITED, False), (K.NV12, K.LIMITED, True)}
    assert {c.prim for c in piped} == {K.B601, K.B709, K.B2020}
    # a ragged last column tile with ONE live lane (dst_w % 128 == 2), at one and at nine tiles; a source as narrow as the chroma window
    assert {c.dst[0] for c in piped if c.dst[0] % 128 == 2} >= {130, 1026}
    assert any(all(cw == 4 for _, _, cw, _ in c.crops) for c in piped)
    # batches hold DIFFERENT views: the whole surface and its bottom-right corner among them, z up to 7
    for c in piped:
        if len(c.crops) == 8 and c.surface != "tiny":
            w, h, _ = K.surface(c.surface)
            assert len(set(c.crops)) == 8 and (w - 4, h - 2, 4, 2) in c.crops and ((0, 0, w, h) in c.crops), c.name
    assert K.CASES["corner_last_130x259_x8"].crops[-1] == (318, 196, 4, 2)
    # mixed scales in one batch: 4.8x down and 2x up
    sc = [(cw / 130.0, ch / 257.0) for _, _, cw, ch in K.CASES["mixed_scales_130x257_x8"].crops]
    assert max(s[0] for s in sc) >= 4.8 and max(s[1] for s in sc) >= 4.8 and min(s[0] for s in sc) < 0.5 and min(s[1] for s in sc) < 0.5
    # every tensor is a few MB
    assert max(K.tensor_bytes(c) for c in CASES) <= 7 << 20


def test_one_pair_either_side_of_each_threshold():
    at, below = K.CASES["at_4096_130x256_x8"], K.CASES["below_4080_130x255_x8"]
    assert len(at.crops) * at.dst[1] * 2 == 4096 and len(below.crops) * below.dst[1] * 2 == 4080
    assert at._replace(name="", dst=None, want="") == below._replace(name="", dst=None, want="")  # (nothing else differs)
    assert (at.want[-3:], below.want[-3:]) == ("@r2", "@r1")
    even, odd = K.CASES["one_surface_1026x457"], K.CASES["odd_width_1025x457"]
    assert even._replace(name="", dst=None, want="") == odd._replace(name="", dst=None, want="") and even.dst[1] == odd.dst[1]
    assert (even.dst[0] % 2, odd.dst[0] % 2) == (0, 1) and (even.want[-3:], odd.want[-3:]) == ("@r2", "@r1")
    assert odd.dst[1] * ((odd.dst[0] + 127) // 128) >= 4096  # (the size alone would pipeline it)
    # the restated rule at the threshold itself, and at the frame_kernel's
    assert K.rows_per_wave(1, (128, 4096), K.SPLIT) == 2 and K.rows_per_wave(1, (128, 4095), K.SPLIT) == 1
    assert K.takes_x2(1, (64, 4096), False) and not K.takes_x2(1, (64, 4095), False) and K.takes_x2(1, (2, 1), True)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_within_the_model_bound(oracle, case):
    got = K.oracle_output(oracle, case)
    _, res = K.model_result(case)
    ok, ratio = K.check_against_model(case, got)
    print("RATIO oracle %-40s %.4f" % (case.name, float(np.nanmax(ratio))))
    assert np.isfinite(res.v).all() and res.v.std() > 0 and got.any()
    assert ok.all(), "%s: %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        case.name, int((~ok).sum()), ok.size, float(np.nanmax(ratio)), np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))
