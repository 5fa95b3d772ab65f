"""The driver that takes a captured tick through the lane rule or the merge rule (cvgpuspeedup_amd/csrc/cvgs_tick_capture.h), without a GPU.

tests/cpp/tick_capture_model.cpp is a stand-alone program (its own main; it is never loaded into Python): it plays the driver on a fake
capturing stream -- a DAG with a frontier that can refuse the next set_deps, add_deps or rewrite_node -- over random sequences of ticks,
foreign nodes, new captures, eager ticks, failed launches and refused runtime calls, and holds every tick to the ordering the stream had
promised it, every unordered pair to an exact byte-set model, the frontier after every call, the counters, the lock and the notes.  It is
built here with the host compiler and -fsanitize=address,undefined from three source files (no HIP header, no library) and run once; its
summary is read back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvgpuspeedup_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "tick_capture_model.cpp"), os.path.join(CSRC, "cvgs_tick_merge.cpp"), os.path.join(CSRC, "cvgs_tick_overlap.cpp")]
N_LANE_REASONS, N_MERGE_REASONS = 11, 9  # TickOverlap, TickMerge


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tick_capture_model") / "tick_capture_model")
    cxx = _host_compiler()
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread"]
    if "clang" not in os.path.basename(cxx):  # gcc: the sanitizers' runtimes inside the program, as clang links them (nothing to load first)
        flags += ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx] + flags + ["-o", exe] + SOURCES, check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, "tick_capture_model failed:\n%s\n%s" % (run.stdout[-4000:], run.stderr[-4000:])
    assert run.stdout.strip().endswith("OK")
    return run.stdout


def test_the_driver_keeps_order_frontier_and_books(report):
    m = re.search(r"capture: (\d+) sequences, (\d+) captures, (\d+) ticks \((\d+) eager, (\d+) with a failed launch\): (\d+) over the floor \((\d+) merged\), "
                  r"(\d+) under it and admitted \((\d+) overlapped\), (\d+) not admitted \((\d+) never routed\), (\d+) foreign nodes; most chains in a node (\d+); "
                  r"refused calls: (\d+) sequences with one, (\d+) with two, (\d+) errors returned", report)
    assert m, report
    sequences, captures, ticks, eager, abandoned, big, merged, small, overlapped, not_admitted, unrouted, foreign, most, one, two, errors = map(int, m.groups())
    print(m.group(0))
    assert sequences >= 2000 and captures > sequences and foreign > 0 and eager > 0 and abandoned > 0 and unrouted > 0 and not_admitted > unrouted
    assert 4 * merged >= big > 0, "at least a quarter of the ticks over the floor merged"
    assert 5 * overlapped >= small > 0, "at least a fifth of the admitted ticks under the floor overlapped"
    assert most == 128, "the cap is reached and never passed"
    assert one > 0 and two > 0 and errors > 0, "sequences with one and with two refused calls, and the one error"


def test_every_reason_of_both_rules_occurs(report):
    lanes = re.findall(r"^  lanes +(\d+)  (.+)$", report, flags=re.M)
    merge = re.findall(r"^  merge +(\d+)  (.+)$", report, flags=re.M)
    print(lanes, merge)
    assert len(lanes) == N_LANE_REASONS and len(merge) == N_MERGE_REASONS and "?" not in [t for _, t in lanes + merge]
    for count, text in lanes + merge:
        assert int(count) > 0, text
    assert any("a capture-dependency call failed" in t for _, t in lanes) and any("could not be rewritten" in t for _, t in merge)


def test_the_pinned_notes_are_literal(report):
    assert "notes: 10 pinned notes compared" in report
