"""The gfx950 kernels held DIRECTLY to the exact model (tests/exact_model.py), without the CPU oracle in between: the grid of
tests/exact_cases.py -- casts between all nine depths (CV_16BF included, which the oracle does not know), arithmetic on integer-typed values,
CV_64F chains, channel moves, write kinds, default-value planes, nine planes and more -- with default dispatch and on the interpreted path
(capi.CHAIN_FORCE_GENERIC).  Every output sits between canary bands; the comparison is EQUALITY (integers byte for byte, floats bit for bit,
any NaN equal to any NaN, the sign of zero counts).

Each case is one tiny launch (at most 3 x 131 pixels per plane), so the file's time is a function of the case count: the cases of one source
depth run as one test.  Measured on an MI355X: 494 cases x 2 runs = 988 launches; the 19 group tests take 0.01 - 0.02 s each after the first
(0.18 s, which carries the first launch), 0.4 s together; the whole file, 28 tests, 2.3 s with the interpreter's start and the runtime's.
First run: every kernel equals the model on every element of every case, on both paths; kernels reached: generic_inline8, generic_inline64,
generic64_inline8, generic64_table, pointwise4_u8_cast, pointwise4_u8_interp, pointwise4_u8_u8_interp, pointwise4_s8, pointwise4_u16,
pointwise4_s16, pointwise4_s32, pointwise4_f32."""
import time

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import exact_cases as X
from tests import exact_model as E

pytestmark = pytest.mark.gpu

SEEN = {}   # group -> kernel names its cases ran on


def run_case(name, flags):
    import torch
    _, build = X.CASES[name]
    B = X.DeviceBackend()
    iops, arrays = build(B)
    kname = cvgs.kernel_name(*iops, flags=flags)
    cvgs.executeOperations(torch.cuda.current_stream(), *iops, flags=flags)
    torch.cuda.synchronize()
    shape = (iops[0].batch,) + np.asarray(arrays[0]).shape[:2] + (capi.type_cn(iops[-1].dst_type),)
    return iops, arrays, kname, X.written(build, B.results(), shape)


def describe(name, what, kname, arrays, got, want, bad):
    src = np.stack([np.asarray(a) for a in arrays])
    rows = []
    for idx in np.argwhere(bad)[:5]:
        z, y, x, c = (int(v) for v in idx)
        s = src[z, y, x].tolist() if z < src.shape[0] else "default value"
        rows.append("at %r: source %r, kernel %r, model %r" % ((z, y, x, c), s, got[z, y, x, c].item(), want[z, y, x, c].item()))
    return "%s (%s, kernel %s): %d of %d elements differ; %s" % (name, what, kname, int(bad.sum()), bad.size, "; ".join(rows))


@pytest.mark.parametrize("group", X.GROUPS)
def test_kernels_equal_the_exact_model(device, group):
    t0 = time.perf_counter()
    failures, names = [], SEEN.setdefault(group, set())
    cases = X.names_of(group)
    for name in cases:
        want = None
        for what, flags in (("default", capi.CHAIN_DEFAULT), ("generic", capi.CHAIN_FORCE_GENERIC)):
            iops, arrays, kname, got = run_case(name, flags)
            names.add(kname)
            if what == "generic" and not (kname.startswith("generic") or kname.endswith("_interp")):
                failures.append("%s: the forced run chose %s" % (name, kname))
            if X.has_64f(iops) and not kname.startswith("generic64"):
                failures.append("%s (%s): a chain with a CV_64F stage chose %s" % (name, what, kname))
            if want is None:
                want = E.evaluate(iops, arrays)  # (the inputs are seeded: the same for both runs)
            depth = E.depth_of(iops[-1].dst_type)
            bad = E.differs(got, want, depth)
            if bad.any():
                failures.append(describe(name, what, kname, arrays, got, want, bad))
    print("EXACT gpu %-10s %3d cases x 2 runs, %.2f s, kernels %s" % (group, len(cases), time.perf_counter() - t0, sorted(names)))
    assert not failures, "%d failures in %r:\n%s" % (len(failures), group, "\n".join(failures[:40]))


@pytest.mark.parametrize("name", sorted(X.REFUSED))
def test_refused_chains_are_refused_on_the_device(device, name):
    import torch
    build, text = X.REFUSED[name]
    B = X.DeviceBackend()
    iops, _ = build(B)
    with pytest.raises(capi.CvgsError) as err:
        cvgs.executeOperations(torch.cuda.current_stream(), *iops)
    assert err.value.code == capi.ERR_UNSUPPORTED and text in str(err.value)
    torch.cuda.synchronize()
    assert all(not r.any() for r in B.results()), "a refused chain wrote"


def test_the_grid_reached_its_kernels(device):
    """otherwise the grid has silently stopped reaching them (groups that did not run in this session are asked for their names by a dry run)"""
    seen = set()
    for group in X.GROUPS:
        if group in SEEN and SEEN[group]:
            seen |= SEEN[group]
            continue
        for name in X.names_of(group):
            iops, _ = X.CASES[name][1](X.HostBackend())
            seen |= {cvgs.kernel_name(*iops, flags=f) for f in (capi.CHAIN_DEFAULT, capi.CHAIN_FORCE_GENERIC)}
    print("EXACT gpu kernels reached: %s" % sorted(seen))
    assert {"generic_inline8", "generic64_inline8"} <= seen, seen
    assert seen & {"generic_inline64", "generic_table"}, seen
    assert any(k.startswith("pointwise") for k in seen), seen
