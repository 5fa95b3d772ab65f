"""The decision that lets a captured tick run beside the ticks before it (cvgpuspeedup_amd/csrc/cvgs_tick_overlap.cpp), without a GPU.

tests/cpp/tick_overlap_model.cpp is a stand-alone program (its own main; it is never loaded into Python): it holds ticks_independent to a
brute-force byte-set model over seeded footprints inside a 4 KiB arena, and the two-lane bookkeeping (TickLanes) to an ordering model of a
capturing stream over random sequences of overlappable ticks, dependent ticks, foreign nodes and new capture ids.  It is built here with the
host compiler and -fsanitize=address,undefined from the two source files alone (no HIP header, no library) and run once; its summary
lines are printed, and the shares the generator must reach are asserted by the program AND read back here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "tick_overlap_model.cpp"), os.path.join(ROOT, "cvgpuspeedup_amd", "csrc", "cvgs_tick_overlap.cpp")]


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tick_overlap_model") / "tick_overlap_model")
    cxx = _host_compiler()
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if "clang" not in os.path.basename(cxx):  # gcc: the sanitizers' runtimes inside the program, as clang links them (nothing to load first)
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + ["-o", exe] + SOURCES, check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, "tick_overlap_model failed:\n%s\n%s" % (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith("OK")
    return run.stdout


def test_independence_matches_the_byte_set_model(report):
    m = re.search(r"independence: (\d+) cases, byte sets say independent (\d+) / not (\d+), (\d+) with an unknown range", report)
    assert m, report
    cases, indep, dep, unknown = map(int, m.groups())
    assert cases >= 2000 and indep + dep == cases
    assert 4 * indep >= cases and 4 * dep >= cases, "both outcomes in at least a quarter of the cases each"
    assert unknown >= cases // 5


def test_lanes_hold_the_ordering_model(report):
    m = re.search(r"lanes: (\d+) sequences, (\d+) captures, (\d+) ticks \((\d+) overlapped\), (\d+) foreign nodes", report)
    assert m, report
    sequences, captures, ticks, overlapped, foreign = map(int, m.groups())
    assert sequences >= 1000 and captures > sequences and foreign > 0
    assert 5 * overlapped >= ticks, "the sequences must exercise the overlap"
    for reason in ("not independent of the ticks it would run beside", "something else was captured since the previous tick", "no hull stated",
                   "no earlier tick of this capture"):
        assert reason in report, reason
