"""csrc/cvgs_boxwarp.cpp in a stand-alone program under AddressSanitizer + UBSan (tests/cpp/boxwarp_asan.cpp): no HIP, no library, no GPU.
Hostile boxes go through cvgs_warp_table_from_boxes_host over heap buffers of exactly the contract's size.  Built here with the flags of
tests/cpp/Makefile's detect_asan rule (a plain host compiler, the engine's -ffp-contract=off) and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_host_file_under_sanitizers(tmp_path):
    cxx = next(shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c))
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "boxwarp_asan")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    "-fno-omit-frame-pointer", "-Wall", os.path.join(CPP, "boxwarp_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.endswith(" checks, 0 bad") and int(last.split()[0]) > 200, r.stdout[-2000:] + r.stderr[-3000:]
