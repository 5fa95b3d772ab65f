"""The refusals of the ten detector-side entry points (csrc/cvgs_detect.cpp), code and full text, held to the answers recorded from the
commit that still had them inside cvgs_api.cpp (tests/golden/detect_refusals.json; the cases and how they stay clear of any launch or
dereference: tests/detect_refusal_cases.py), and the host file itself in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/detect_asan.cpp)."""
import json
import os
import shutil
import subprocess

from tests import detect_refusal_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_every_refusal_equals_the_recorded_one(lib):
    """Every single defect of the five stages' tables, every pair of them (the pairs pin the order of the checks) and the defects of the
    call, on the device entry points and -- where the refusal comes before the first dereference -- on the host twins."""
    with open(G.GOLDEN) as f:
        doc = json.load(f)
    cases = G.cases()
    assert len(cases) == doc["cases"] == len(doc["case_answer"]) and G.ids_digest(cases) == doc["ids_sha256"], "the case list and the fixture disagree"
    assert G.left_out(cases) == G.LEFT_OUT
    assert len({c[0] for c in cases}) == len(cases) and len({c[1] for c in cases}) == 9  # (cvgs_plane_tables_from_boxes has no twin)
    got = G.replay(lib, cases)
    bad = [(c[0], a, doc["answers"][k]) for c, a, k in zip(cases, got, doc["case_answer"]) if list(a) != doc["answers"][k]]
    assert not bad, "%d of %d differ; the first: %r" % (len(bad), len(cases), bad[:3])
    refused = sum(1 for a in got if a[0])
    assert refused > 0.98 * len(cases) and (G.PASSES[0], G.PASSES[1]) in got  # almost everything is a refusal; cancelling pairs exist


def test_host_file_under_sanitizers(tmp_path):
    """tests/cpp/detect_asan.cpp (built by its rule in tests/cpp/Makefile, the one place that holds the flags): cvgs_detect.cpp compiled
    into a stand-alone program with -fsanitize=address,undefined and the engine's -ffp-contract=off (no HIP, no library), its launchers
    stubbed to keep the frames they are handed; the host twins run over heap buffers of exactly the contract's size and must write the
    bytes recorded from the parent commit's library for the same inputs."""
    cxx = next(shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c))
    subprocess.run(["make", "-C", CPP, "bin/detect_asan", "HOSTCXX=" + cxx], check=True, stdout=subprocess.DEVNULL)
    with open(G.GOLDEN) as f:
        want = G.recorded_twin_outputs(json.load(f))
    cases = G.twin_cases()
    assert len(cases) == len(want) == 51 and {c[0] for c in cases} == {"select", "head", "gather", "warp"}
    path = tmp_path / "twins.txt"
    path.write_text("".join(G.twin_line(c, w) + "\n" for c, w in zip(cases, want)))
    r = subprocess.run([os.path.join(CPP, "bin", "detect_asan"), str(path)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.endswith(" checks, 0 bad") and int(last.split()[0]) > 51 * 3, r.stdout[-2000:] + r.stderr[-3000:]
