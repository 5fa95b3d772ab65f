"""The grid of tests/k1_rows_cases.py without a GPU: every model-covered case runs on the CPU oracle and must lie within the float64
model's derived bound (tests/f64_model.py) -- the proof that the oracle stays inside the bound on these inputs, as
tests/test_model_vs_oracle.py gives it for its grid --, every case is one the product accepts and sends to K1, the grid holds what its
docstring says (every height and width, the workgroup's row count, window edges inside a row group), the rows-per-wave mapping agrees
with its table (tests/cpp/k1_rows_table.cpp) and with the "@rN" names the library reports under each CVGS_K1_RPW setting.

Largest |oracle - model| / tolerance per family on this grid (1 = at the bound): u8 planar 0.43 (fp32 outputs; 1.00 on the 16-bit float
outputs, whose tolerance IS one rounding of their format), interpreted 0.35, wide and few planar 0.41, packed 0.50 (the integer outputs' half
step; 1.00 on 16-bit floats), windows 0.50, tick 0.35."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cvgpuspeedup_amd import cvgs
from tests import f64_model as F
from tests import k1_rows_cases as K

ROOT = K.ROOT
CHAINS = [(tag, case.name) for case in K.CASES.values() if case.model for tag, _ in K.chains_of(case)]


def _build_of(tag, name):
    return dict(K.chains_of(K.CASES[name]))[tag]


@pytest.mark.parametrize("tag,name", CHAINS)
def test_oracle_within_the_model_bound(oracle, tag, name):
    build = _build_of(tag, name)
    iops, views = K.model_side(build)
    res = F.evaluate(iops, views)
    ok, ratio = K.check_against_model(res, iops, K.oracle_output(oracle, build))
    print("RATIO oracle %-10s %-40s %.4f" % (K.CASES[name].family, tag, float(np.nanmax(ratio))))
    if res.excluded is not None:  # (the cap of held_to_model: a condition on the inputs, not a measurement)
        assert (res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1) <= 0.01).all()
    assert np.isfinite(res.v).all() and res.v.std() > 0
    assert ok.all(), "%s: %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        tag, int((~ok).sum()), ok.size, float(np.nanmax(ratio)), np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


def test_every_case_is_one_k1_takes(lib):
    for case in K.CASES.values():
        for tag, build in K.chains_of(case):
            iops, _ = K.model_side(build)
            assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, tag
            assert cvgs.kernel_name(*iops) == case.kernel, (tag, cvgs.kernel_name(*iops))  # (no hook in this process: no "@rN")


def test_the_grid_covers_what_it_says():
    sizes = set()
    for case in K.CASES.values():
        for tag, build in K.chains_of(case):
            sizes.add(tuple(K.model_side(build)[0][0].dsize))
    assert {h for _, h in sizes} >= set(K.HEIGHTS) and {w for w, _ in sizes} >= set(K.WIDTHS)
    assert {(65, h) for h in K.HEIGHTS} | {(w, h) for w in K.WIDTHS for h in (5, 8)} <= sizes
    rows_per_workgroup = K.k1_waves() * 4
    assert {rows_per_workgroup - 1, rows_per_workgroup, rows_per_workgroup + 1} <= set(K.HEIGHTS)
    assert len(K.CASES) <= 130
    # every family reaches more than one row per wave under some setting -- except the one that is there for the rule "interpreted: always 1"
    for family in K.FAMILIES:
        top = max(max(c.rows.values()) for c in K.CASES.values() if c.family == family)
        assert top == (1 if family == "interpreted" else 4), family
    assert any(c.rows[2] == 2 for c in K.CASES.values())


def test_every_window_case_has_an_edge_inside_a_row_group():
    seen = 0
    for case in K.CASES.values():
        if case.family != "windows":
            continue
        crops, dst, ar = case.build.window
        iops, _ = K.model_side(case.build)  # (the builder asserts it from the lowered PlaneParams; restated here from the model's own window rule)
        used = iops[0].used_planes
        if used == 0:  # all background: the z >= used loop, over a row group that straddles the target's last row
            assert dst[1] % 4 != 0 and any(v != 0 for v in iops[0].background[:3])
        windows = [F.exact_window(c[2], c[3], dst[0], dst[1], ar) for c in crops[:used]]
        inside = [w for w in windows if 0 < w[1] and w[1] % 4 != 0 and (w[3] + 1) % 4 != 0 and w[3] < dst[1] - 1]
        assert len(inside) >= min(2, used) and len(K.edges_inside_a_row_group(K.plane_params(iops[0])[:used], dst[1])) >= min(2, used), case.name
        seen += 1
    assert seen == 16
    used = sorted(K.model_side(c.build)[0][0].used_planes for c in K.CASES.values() if "_used" in c.name)
    assert used == [0, 0, 3, 3]


def test_rows_mapping_matches_its_table():
    """tests/cpp/k1_rows_table.cpp: k1_rows_instantiated against the table, every combination of its arguments (host only)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/k1_rows_table"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "k1_rows_table")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "k1_rows_table passed!!" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("setting", K.SETTINGS)
def test_names_carry_the_instantiated_rows_under_the_hook(tmp_path, setting):
    """the library reads CVGS_K1_RPW once per process: a child reports every case's kernel name (a dry run, no GPU)"""
    env = dict(os.environ, CVGS_K1_RPW=str(setting))
    r = subprocess.run([sys.executable, "-m", "tests.k1_rows_worker", "--names", str(tmp_path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = np.load(os.path.join(str(tmp_path), "k1_rows_names_rpw%d.npz" % setting))
    for case in K.CASES.values():
        for name in rec["kernel::" + case.name]:
            assert str(name) == "%s@r%d" % (case.kernel, case.rows[setting]), (case.name, setting, str(name))
