"""K1's 2- and 4-rows-per-wave kernels held to the float64 model (tests/f64_model.py) on the small, ragged grid of tests/k1_rows_cases.py.

launch_k1 picks more than one row per wave only for large launches; the CVGS_K1_RPW hook asks for 1, 2 or 4 whatever the size.  The
library reads it once per process, so each setting runs in a fresh child (python -m tests.k1_rows_worker <outdir>), one after another.
A child that ends by a signal, a non-zero status or its timeout is the last one started: the remaining settings are reported as
failed, and nothing more is started on a card a child may have faulted.

One test item with one pytest subtest per (check, variant family): a failing subtest is reported under its own name
(SUBFAILED(check=..., family=...)), whatever it raised, and the others still run.  Per variant family: the "@rN" suffix of
cvgs_kernel_name equals the table of k1_rows_instantiated (k_k1_impl.hpp) under every setting and reaches N > 1 in every family; every model-covered output lies within the model's derived bound under every setting; the bytes under
settings 2 and 4 equal those under setting 1 (separate planes, the cvgs_execute_many ticks and the CircularTensor sequence included); the
separate-plane cases equal the CPU oracle bit for bit.  Canary bands: DeviceBackend.result() asserts them in every child.

A child takes about 3 s on an MI355X (WORKER_SECONDS; most of it the imports), the three together 8 s; the timeout is a safety net of
twenty times that.

Largest |kernel - model| / tolerance per family, measured on an MI355X (1 = at the bound), the same figure under CVGS_K1_RPW = 1 / 2 / 4
since the bytes are the same, and the CPU oracle's figure of tests/test_k1_rows_cases.py to four decimals: u8 planar 0.9999 / 0.9999 /
0.9999 (the 16-bit float outputs, whose tolerance IS one rounding of their format, which random inputs reach; fp32 outputs 0.43),
interpreted 0.3474 / 0.3474 / 0.3474, wide and few planar 0.4126 / 0.4126 / 0.4126, packed 0.9999 / 0.9999 / 0.9999 (16-bit floats;
integer outputs 0.50, their half step), windows 0.5000 / 0.5000 / 0.5000, tick 0.3493 / 0.3493 / 0.3493."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import f64_model as F
from tests import k1_rows_cases as K

pytestmark = pytest.mark.gpu

WORKER_SECONDS = 3                    # wall time of one child on the first good run
CHILD_TIMEOUT = 20 * WORKER_SECONDS   # a safety net, not a measurement
MODEL_FAMILIES = [f for f in K.FAMILIES if any(c.model for c in K.CASES.values() if c.family == f)]
_MODEL_CACHE = {}


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{setting: (status, npz or None)}: the three children, one after another; none is started behind one that did not end normally"""
    outdir = str(tmp_path_factory.mktemp("k1_rows"))
    res, stopped = {}, None
    for setting in K.SETTINGS:
        if stopped is not None:
            res[setting] = ("not started: the child of setting %d %s" % stopped, None)
            continue
        env = dict(os.environ, CVGS_K1_RPW=str(setting))
        try:
            p = subprocess.run([sys.executable, "-m", "tests.k1_rows_worker", outdir], env=env, cwd=K.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               timeout=CHILD_TIMEOUT)
            status = "ok" if p.returncode == 0 else "ended with status %d:\n%s" % (p.returncode, p.stdout[-3000:])
        except subprocess.TimeoutExpired as e:
            status = "did not end within %d s:\n%s" % (CHILD_TIMEOUT, (e.stdout or "")[-3000:] if isinstance(e.stdout, str) else "")
        if status != "ok":
            stopped = (setting, status)
            res[setting] = (status, None)
            continue
        res[setting] = ("ok", np.load(os.path.join(outdir, "k1_rows_rpw%d.npz" % setting)))
    return res


def _good(children):
    bad = ["CVGS_K1_RPW=%d: %s" % (s, children[s][0]) for s in K.SETTINGS if children[s][0] != "ok"]
    assert not bad, "\n".join(bad)
    return {s: children[s][1] for s in K.SETTINGS}


def _cases(family):
    return [c for c in K.CASES.values() if c.family == family]


def _outputs(rec, case):
    n = len(case.build) if case.kind == "tick" else 1
    return [rec["out::%s::%d" % (case.name, i)] for i in range(n)]


def model_of(tag, build):
    """the model's answer for a chain (the inputs are seeded: the same in every child), computed once"""
    if tag not in _MODEL_CACHE:
        iops, views = K.model_side(build)
        _MODEL_CACHE[tag] = (iops, F.evaluate(iops, views))
    return _MODEL_CACHE[tag]


def held_to_model(family, tag, res, iops, got, what):
    """tests/test_gpu_model.py's held_to_model for an output that arrives as bytes"""
    ok, ratio = K.check_against_model(res, iops, got.view(K.out_dtype(iops)))
    print("RATIO gpu %-10s %-40s %-8s %.4f" % (family, tag, what, float(np.nanmax(ratio))))
    if res.excluded is not None:
        assert (res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1) <= 0.01).all()
    assert ok.all(), "%s (%s): %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        tag, what, int((~ok).sum()), ok.size, float(np.nanmax(ratio)), np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))
    return float(np.nanmax(ratio))


def _check_rows(recs, family):
    top = 0
    for case in _cases(family):
        for setting in K.SETTINGS:
            for name in recs[setting]["kernel::" + case.name]:
                assert str(name) == "%s@r%d" % (case.kernel, case.rows[setting]), (case.name, setting, str(name))
            top = max(top, case.rows[setting])
    assert top == (1 if family == "interpreted" else 4), family  # non-vacuity: the family runs a multi-row kernel under some setting
    if family == "u8 planar":
        assert all(c.rows[2] == 2 for c in _cases(family))


def _check_model(recs, family):
    worst = {s: 0.0 for s in K.SETTINGS}
    for case in _cases(family):
        if not case.model:
            continue
        for i, (tag, build) in enumerate(K.chains_of(case)):
            iops, res = model_of(tag, build)
            for setting in K.SETTINGS:
                worst[setting] = max(worst[setting], held_to_model(family, tag, res, iops, _outputs(recs[setting], case)[i], "rpw%d@r%d" % (setting, case.rows[setting])))
    print("WORST gpu %-20s %s" % (family, " / ".join("%.4f" % worst[s] for s in K.SETTINGS)))


def _check_identity(recs, family):
    for case in _cases(family):
        base = _outputs(recs[1], case)
        assert all(b.size > 0 and b.any() for b in base), case.name
        for setting in (2, 4):
            for i, (a, b) in enumerate(zip(base, _outputs(recs[setting], case))):
                assert a.size == b.size and np.array_equal(a, b), "%s chain %d: %d bytes differ between CVGS_K1_RPW=1 and =%d (%s)" % (
                    case.name, i, int((a != b).sum()) if a.size == b.size else -1, setting, recs[setting]["kernel::" + case.name][i])


def _check_oracle(recs, family, oracle):
    for case in _cases(family):
        if not case.oracle_exact:
            continue
        want = np.ascontiguousarray(K.oracle_output(oracle, case.build)).reshape(-1).view(np.uint8)
        got = _outputs(recs[1], case)[0]
        assert got.size == want.size and np.array_equal(got, want), "%s: %d bytes differ from the oracle" % (case.name, int((got != want).sum()))


def test_k1_rows_per_wave(children, oracle, subtests):
    recs = _good(children)  # (a child that did not end normally fails the test here, with every setting's status)
    assert sum(c.oracle_exact for c in K.CASES.values()) == 5
    for family in K.FAMILIES:
        with subtests.test(check="rows instantiated", family=family):
            _check_rows(recs, family)
        with subtests.test(check="identity across settings", family=family):
            _check_identity(recs, family)
        if family in MODEL_FAMILIES:
            with subtests.test(check="model bound", family=family):
                _check_model(recs, family)
        if any(c.oracle_exact for c in _cases(family)):
            with subtests.test(check="oracle", family=family):
                _check_oracle(recs, family, oracle)
