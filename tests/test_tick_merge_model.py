"""The decision that lets a captured tick ride in the previous tick's launch (cvgpuspeedup_amd/csrc/cvgs_tick_merge.cpp), without a GPU.

tests/cpp/tick_merge_model.cpp is a stand-alone program (its own main; it is never loaded into Python): over random sequences of ticks,
foreign nodes and new capture ids on a model of a capturing stream it holds the decision to an exact byte-set model (merged if and only if
the model says so), the node's bookkeeping to the call order (first segment, chain count within the cap, largest batch), every tick to the
ordering the stream had promised it, and ticks under the size floor to a plain TickLanes.  It is built here with the host compiler and
-fsanitize=address,undefined from three source files (no HIP header, no library) and run once; its summary is read back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvgpuspeedup_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "tick_merge_model.cpp"), os.path.join(CSRC, "cvgs_tick_merge.cpp"), os.path.join(CSRC, "cvgs_tick_overlap.cpp")]


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tick_merge_model") / "tick_merge_model")
    cxx = _host_compiler()
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if "clang" not in os.path.basename(cxx):  # gcc: the sanitizers' runtimes inside the program, as clang links them (nothing to load first)
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + ["-o", exe] + SOURCES, check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, "tick_merge_model failed:\n%s\n%s" % (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith("OK")
    return run.stdout


def test_the_decision_is_the_byte_set_models(report):
    m = re.search(r"merge: (\d+) sequences \((\d+) of small ticks only\), (\d+) captures, (\d+) ticks: (\d+) over the floor \((\d+) merged\), (\d+) under it "
                  r"\((\d+) overlapped, (\d+) plans compared\), (\d+) foreign nodes; most chains in a node (\d+), (\d+) nodes found full", report)
    assert m, report
    sequences, small_only, captures, ticks, big, merged, small, overlapped, compared, foreign, most, full = map(int, m.groups())
    assert sequences >= 2000 and captures > sequences and foreign > 0 and big + small == ticks
    assert 4 * merged >= big, "the sequences must exercise the merge"
    assert small_only > 0 and compared > 0 and 5 * overlapped >= small, "ticks under the floor: the lanes, compared with a plain TickLanes"
    assert 64 < most <= 128 and full > 0, "the cap is reached and never passed"


def test_every_refusal_occurs(report):
    for reason in ("no hull stated", "no earlier tick of this capture", "something else was captured since the previous tick",
                   "another kernel, program, target shape or geometry", "not independent of the ticks in the previous launch", "the previous launch is full"):
        assert reason in report, reason
