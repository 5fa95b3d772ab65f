"""The C++ facade on the GPU held to the independent float64 model (tests/f64_model.py): tests/cpp/bin/facade_model builds every chain of
tests/facade_cases.py in the facade's own spelling, uploads the inputs, runs cvGS::executeOperations on a stream and downloads each output
between its canary bands -- one process, one time limit, no retry; a non-zero exit fails the module.  All cases are checked inside ONE test, which
goes through every case and names each failing one.  The expected values come
from the Python spelling of the same chain through the model alone, the acceptance is that of tests/test_gpu_model.py, and the cases whose
Python twin in tests/model_cases.py names a fast kernel must have reached the same kernel prefix from the facade's lowering.  The chains the CPU
oracle does not know (packed 4:2:2, planar 4:4:4, bfloat16) are run here only; for them the near-miss spellings are told apart here as well.

Largest |kernel - model| / tolerance per family, measured on an MI355X (1 = at the bound): resize 0.40, convertTo 1.00 (0.9959 CV_16F, 0.9960
CV_16BF: a 16-bit float output's tolerance IS one rounding of its format; the other cases at most 0.50), arithmetic 0.55, cvtColor 0.67, writes 0.40,
warp 0.35, YUV nv12 0.59, p010 0.39, yuy2 / uyvy 0.58, yuv444 0.56, fk 0.50 -- the oracle leg's figures of tests/test_facade_model.py to four
decimals where both legs run a case.  The whole module takes under three seconds, the program itself well under one."""
import os
import subprocess

import numpy as np
import pytest

from tests import facade_cases as FC
from tests.test_facade_model import PROGRAM, assert_held, build_program

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_run(device, tmp_path_factory):
    """(directory, {name: input arrays}, {name: kernel name}) of ONE run of the program in gpu mode"""
    if not os.path.exists(PROGRAM):
        build_program()
    d = str(tmp_path_factory.mktemp("facade_model_gpu"))
    arrays = FC.write_inputs(d)
    r = subprocess.run([PROGRAM, d, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    kernels = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("KERNEL "))
    return d, arrays, kernels


def check_case(name, d, arrays, kernels):
    case = FC.CASES[name]
    res, iops = FC.model_of(name, arrays[name])
    payload = FC.read_output(d, name)
    if case.kernel is not None:
        assert kernels[name].startswith(case.kernel), (name, kernels[name])
    assert_held(name, res, iops, payload, "gpu %s" % kernels[name])
    if not case.oracle:
        for label, variant in case.near:
            res2, iops2 = FC.model_of(name, arrays[name], **variant)
            assert not FC.held(res2, iops2, payload)[0].all(), "%s: the inputs cannot tell the facade from one with '%s'" % (name, label)


def test_facade_on_the_gpu_within_the_model_bound(gpu_run):
    """Every case of the table, in ONE test (the cases share one run of the program, and the suite's count of GPU tests stays small): each
    case is checked in full, a failing case does not hide the ones behind it, and the message names every failing case with its figures."""
    d, arrays, kernels = gpu_run
    failures = []
    for name in FC.CASES:
        try:
            check_case(name, d, arrays, kernels)
        except Exception as e:  # noqa: BLE001  (an assertion, a missing output file, an output of the wrong size)
            failures.append("%s: %s: %s" % (name, type(e).__name__, e))
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), len(FC.CASES), "\n".join(failures))


def test_every_case_named_its_kernel(gpu_run):
    assert sorted(gpu_run[2]) == sorted(FC.CASES)
