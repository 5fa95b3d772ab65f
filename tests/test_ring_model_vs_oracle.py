"""The CPU oracle's CircularTensor (oracle.OracleCircular) held to the independent ring model (tests/ring_model.py) over the grid of
tests/circular_cases.py: the WHOLE tensor after EVERY one of BATCH + 3 updates, every slot that shows a frame within f64_model's derived
bound of that frame, every never-written slot bit-zero.  No element is excluded.  No GPU needed.

The sensitivity tests flip each defining choice of the ring model in turn and assert that the oracle then falls OUTSIDE the model on a named
case: the model is tight enough to catch an age reversal, a wrong plane order, stale content in unwritten slots and a slot off by one."""
import numpy as np
import pytest

from cvgpuspeedup_amd import cvgs
from tests import circular_cases as CC
from tests import ring_model as R
from tests.test_bf16_types import rne_bf16

_MODEL_FRAMES = {}


def model_frame(case, i):
    """(computed once per case and update, shared by every test of this module)"""
    if (case.name, i) not in _MODEL_FRAMES:
        _MODEL_FRAMES[(case.name, i)] = CC.model_frame(case, i)
    return _MODEL_FRAMES[(case.name, i)]


def oracle_bytes(case, oc):
    """the oracle's tensor as bytes in the case's own element format (bfloat16: the fp32 twin rounded on the host, which
    tests/test_bf16_types.py pins against torch)"""
    if case.depth == "16bf":
        return np.ascontiguousarray(rne_bf16(oc.array(np.float32))).view(np.uint8)
    return oc.array(np.uint8)


def run_on_oracle(oracle, case, sw=R.SPEC, updates=None):
    """(bad elements summed over every update, worst ratio, first failure)"""
    twin = case.depth == "16bf"
    oc = oracle.OracleCircular(case.w, case.h, CC.elem_type(case, twin), CC.color_planes(case), case.batch, CC.order_of(case), CC.mode_of(case))
    ring = CC.ring(case)
    bad, worst, where = 0, 0.0, None
    for i in range(case.batch + 3 if updates is None else updates):
        a = CC.frame(case, i)
        oc.update(cvgs.lower(CC.chain(case, cvgs.GpuMat.from_array(a, cvgs.make_type(cvgs.CV_8U, case.cn)), CC.host_write(case, twin), twin)))
        ring.push(model_frame(case, i))
        n, r, w = ring.check(oracle_bytes(case, oc), sw)
        bad, worst, where = bad + n, max(worst, r), where or w
    return bad, worst, where


@pytest.mark.parametrize("name", list(CC.CASES))
def test_oracle_ring_within_the_model(oracle, name):
    case = CC.CASES[name]
    CC.assert_preconditions(case)
    bad, worst, where = run_on_oracle(oracle, case)
    print("RATIO oracle ring %-5s %-62s %.4f" % (case.depth, name, worst))
    assert bad == 0, "%s: %s" % (name, where)


def test_frames_are_distinct_and_the_grid_is_small():
    assert len(CC.CASES) <= 80
    for case in CC.CASES.values():
        frames = [CC.frame(case, i) for i in range(2 * case.batch + 7)]
        assert all(f.std() > 30 for f in frames), case.name
        assert all((frames[i] != frames[j]).mean() > 0.9 for i in range(len(frames)) for j in range(i)), case.name


def test_the_grid_reaches_what_it_is_there_for():
    """every instantiation and branch the grid was written for, by route and shape (the names say which case)"""
    C_ = list(CC.CASES.values())

    def has(**want):
        route = want.pop("route", None)
        return any(all(getattr(c, k) == v for k, v in want.items()) and (route is None or CC.route(c) == route) for c in C_)
    for h in ("def", "dev"):
        for width in (16, 4, 1):  # every copy width with main and tail loops live, outside the push kernel
            assert any(c.handle == h and CC.route(c) in ("stage", "chain+copy") and CC.copy_geometry(c)[0] == width and CC.main_and_tail_live(c)
                       for c in C_), (h, width)
        assert any(c.handle == h and CC.route(c) == "push" and CC.main_and_tail_live(c) for c in C_), h
        for cn in (1, 2, 3, 4):
            for layout in ("std", "pk"):
                assert has(handle=h, cn=cn, layout=layout, route="push"), (h, cn, layout)
        for prog in ("px_msd", "px_cast", "px_mad"):
            for depth in ("32f", "16f", "16bf"):
                assert has(handle=h, push=prog, depth=depth, route="push"), (h, prog, depth)
        for b in (1, 2, 5):
            for m in (False, True):
                assert has(handle=h, batch=b, mirrored=m, push="rs") and has(handle=h, batch=b, mirrored=m, push="px_msd"), (h, b, m)
        for o in ("nf", "of"):
            assert has(handle=h, order=o, layout="tr", push="rs") and has(handle=h, order=o, layout="tr", route="push"), (h, o)
            assert has(handle=h, order=o, mirrored=True), (h, o)
        assert has(handle=h, layout="pk", mirrored=True, push="rs") and has(handle=h, layout="pk", mirrored=True, push="px_mad"), h
        for depth in ("64f", "8u"):
            assert has(handle=h, depth=depth), (h, depth)
        for odd in (True, False):  # a resize push and 64F elements, each on an odd-sized and on an aligned plane
            assert any(c.handle == h and c.push == "rs" and (CC.plane_bytes(c) % 16 != 0) == odd for c in C_), (h, odd)
            assert any(c.handle == h and c.depth == "64f" and (CC.plane_bytes(c) % 16 != 0) == odd for c in C_), (h, odd)
    # capturable stage-then-shift: BATCH 1 and 2, the mirrored form, and for non-8UC3-resize pushes
    for b in (1, 2):
        assert has(handle="dev", batch=b, mirrored=False, route="stage") and has(handle="dev", batch=b, mirrored=True, route="stage"), b
    assert has(handle="dev", route="stage", layout="pk") and has(handle="dev", route="stage", layout="tr") and has(handle="dev", route="stage", push="px_mad")


# which cases can show each switch (any one of them falling outside the model proves the point)
SENSITIVITY = {
    "age_reversed": ["depth_copy_def_ring_of_std_32fc3_b5_40x24_rs", "push_def_c2_ring_nf_std_16fc2_b3_40x24_px_cast"],
    "transposed_as_standard": ["transposed_push_def_ring_nf_tr_32fc3_b3_40x24_px_msd", "transposed_copy_def_ring_of_tr_16fc2_b3_37x23_rs"],
    "unwritten_holds_first_frame": ["depth_push_def_ring_of_std_32fc3_b2_40x24_px_msd", "packed_def_copy1_ring_nf_pk_8uc3_b3_37x23_rs"],
    "newest_slot_off_by_one": ["depth_push_def_ring_nf_std_32fc3_b5_40x24_px_msd", "def_copy1_ring_nf_std_16bfc3_b3_37x23_px_msd"],
}


def test_every_switch_has_a_sensitivity_case():
    assert set(SENSITIVITY) == set(R.SPEC) and not any(R.SPEC.values())
    assert all(name in CC.CASES for names in SENSITIVITY.values() for name in names)


@pytest.mark.parametrize("switch", sorted(R.SPEC))
def test_flipping_a_defining_choice_is_caught(oracle, switch):
    caught = {}
    for name in SENSITIVITY[switch]:
        bad, _, where = run_on_oracle(oracle, CC.CASES[name], R.switches(**{switch: True}))
        caught[name] = (bad, where)
    print("SENSITIVITY ring %-28s %r" % (switch, caught))
    assert any(n > 0 for n, _ in caught.values()), caught


def test_expected_slots_spelled_out():
    """the model's own function against the reference's documented sequence, written out by hand for BATCH 3"""
    nf = [R.expected(k, 3, R.NEWEST_FIRST) for k in range(6)]
    assert nf == [[None, None, None], [0, None, None], [1, 0, None], [2, 1, 0], [3, 2, 1], [4, 3, 2]]
    of = [R.expected(k, 3, R.OLDEST_FIRST) for k in range(6)]
    assert of == [[None, None, None], [None, None, 0], [None, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4]]
    assert R.expected(4, 1, R.NEWEST_FIRST) == [3] == R.expected(4, 1, R.OLDEST_FIRST)
