"""The C++ facade (cvgpuspeedup_amd/include: cvGPUSpeedup.h, cvgs/fk_compat.h, cv2cuda_types.h) held to the independent float64 model
(tests/f64_model.py) on real images.  No GPU needed.

tests/cpp/*.cpp check kernels against the oracle UNDER the facade's own lowering, so a chain the facade lowers wrongly is wrong on both
sides there.  Here tests/cpp/bin/facade_model builds every chain of tests/facade_cases.py in the facade's spelling over inputs written
from Python, lowers it (fk::lowerChain), has the product validate it and runs it on the CPU oracle over host memory; the expected values
come from the Python spelling of the same chain through the model alone.  Every output element must lie within the model's DERIVED
bound, every canary band must come back untouched.  Chains the oracle does not know (packed 4:2:2, planar 4:4:4, bfloat16) are lowered and
validated here and run in tests/test_gpu_facade_model.py.

The discrimination test shows that the inputs can tell: for every case, the output falls OUTSIDE the bound of every near-miss spelling
(Scalar channels reversed, Size transposed, the neighbouring colour code, the next AspectRatio, alpha and beta exchanged, another range /
primaries / layout, the warp matrix read column-major or not inverted, usedPlanes +- 1).  For the chains the oracle does not know, the
stand-in for the output is the model's own value of the right spelling, rounded to the output format.

Largest |oracle - model| / tolerance per family on this table (1 = at the bound): resize 0.40, convertTo 1.00 (0.9959, the CV_16F output: its
tolerance IS one rounding of the format, which a random input reaches; every other case of the family at most 0.50), arithmetic 0.55, cvtColor 0.67
(the gray codes; the permutations and casts are exact, 0.00), writes 0.40, warp 0.35, YUV nv12 0.59, YUV p010 0.39, fk 0.50 (an integer output's
half step).  No case of the oracle leg was outside the bound: the facade's lowering and the Python builders agree on every overload of the table.
One-off check: the program built with -fsanitize=address,undefined ran its oracle mode clean and wrote the same bytes."""
import os
import subprocess

import numpy as np
import pytest

from tests import facade_cases as FC
from tests import model_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PROGRAM = os.path.join(CPP, "bin", "facade_model")


def build_program():
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CPP, "bin/facade_model"], check=True, stdout=subprocess.DEVNULL)


def assert_held(name, res, iops, payload, what):
    """the acceptance of tests/test_gpu_model.py::held_to_model on the program's payload bytes"""
    ok, ratio = FC.held(res, iops, payload)
    print("RATIO %s %-14s %-40s %.4f" % (what, FC.CASES[name].family, name, float(np.nanmax(ratio))))
    if res.excluded is not None:
        share = res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1)
        assert (share <= 0.01).all(), "%s: excluded share of a warp plane above 1 %%: %r" % (name, share)
    assert ok.all(), "%s (%s): %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        name, what, int((~ok).sum()), ok.size, float(np.nanmax(ratio)), np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


def stand_in(res, iops):
    """the model's own value in the output's number format, as payload bytes (what a right facade delivers, to within the bound)"""
    from tests import f64_model as F
    from tests.test_bf16_types import rne_bf16
    dst_type = iops[-1].dst_type
    v = res.v
    kind = FC.logical_kind(iops[-1].kind)
    if kind == F.WRITE_SPLIT:
        v = v.transpose(0, 3, 1, 2)
    elif kind == F.WRITE_T_SPLIT:
        v = v.transpose(3, 0, 1, 2)
    if F.depth_of(dst_type) == F.DEPTH_16BF:
        return np.ascontiguousarray(rne_bf16(v.astype(np.float32))).reshape(-1).view(np.uint8)
    dt = MC.np_dtype(dst_type)
    if np.issubdtype(dt, np.integer):
        v = np.clip(np.rint(v), np.iinfo(dt).min, np.iinfo(dt).max)
    return np.ascontiguousarray(v.astype(dt)).reshape(-1).view(np.uint8)


@pytest.fixture(scope="session")
def oracle_run(tmp_path_factory):
    """the inputs written once, the program run once in oracle mode: (directory, {name: input arrays})"""
    build_program()
    d = str(tmp_path_factory.mktemp("facade_model"))
    arrays = FC.write_inputs(d)
    r = subprocess.run([PROGRAM, d, "oracle"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return d, arrays


def test_the_two_tables_hold_the_same_names():
    build_program()
    r = subprocess.run([PROGRAM, "--list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == list(FC.CASES)


def test_every_builder_family_is_in_the_table():
    families = {c.family.split()[0] for c in FC.CASES.values()}
    assert families == {"resize", "convertTo", "arithmetic", "cvtColor", "writes", "warp", "YUV", "fk"}
    assert {c.family for c in FC.CASES.values() if c.family.startswith("YUV")} == {"YUV " + ln for ln, _ in FC.LAYOUTS}
    assert all(c.near for c in FC.CASES.values())


@pytest.mark.parametrize("name", [n for n, c in FC.CASES.items() if c.oracle])
def test_facade_on_the_oracle_within_the_model_bound(oracle_run, name):
    d, arrays = oracle_run
    res, iops = FC.model_of(name, arrays[name])
    assert np.isfinite(res.v[~np.isnan(res.v)]).all() and res.v.std() > 0
    assert_held(name, res, iops, FC.read_output(d, name), "oracle")


@pytest.mark.parametrize("name", [n for n, c in FC.CASES.items() if not c.oracle])
def test_chains_the_oracle_does_not_know_are_lowered_and_validated(oracle_run, name):
    """the program has lowered and validated them (a refused chain ends it with an error) and has written no output for them"""
    d, _ = oracle_run
    assert not os.path.exists(os.path.join(d, name + ".out"))


def test_warp_transforms_stay_under_the_excluded_cap_by_the_model_alone(oracle_run):
    _, arrays = oracle_run
    for name, case in FC.CASES.items():
        if case.family != "warp":
            continue
        res, _ = FC.model_of(name, arrays[name])
        assert res.excluded is not None and (res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1) <= 0.01).all(), name
        assert (res.v != 0).mean() > 0.3, name  # and most of the picture is drawn


@pytest.mark.parametrize("name", list(FC.CASES))
def test_every_near_miss_spelling_is_told_apart(oracle_run, name):
    d, arrays = oracle_run
    case = FC.CASES[name]
    res, iops = FC.model_of(name, arrays[name])
    payload = FC.read_output(d, name) if case.oracle else stand_in(res, iops)
    ok, _ = FC.held(res, iops, payload)
    assert ok.all(), name  # (the stand-in, too, is inside the right spelling's bound)
    for label, variant in case.near:
        res2, iops2 = FC.model_of(name, arrays[name], **variant)
        ok2, ratio2 = FC.held(res2, iops2, payload)
        print("NEAR-MISS %-40s %-34s %d of %d outside, worst ratio %.3g" % (name, label, int((~ok2).sum()), ok2.size, float(np.nanmax(ratio2))))
        assert not ok2.all(), "%s: the inputs cannot tell the facade from one with '%s'" % (name, label)
