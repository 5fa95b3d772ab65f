"""cvGS::DeviceWarps on the C++ facade (tests/cpp/test_devicewarps.cpp): without a GPU the program COMPILES against the facade; on the GPU
it runs -- DeviceWarps::update + executeOperations over the device-built warp table against host-described cvGS::warp reads whose matrices
are the table's own floats, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "bin", "test_devicewarps")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CPP, "-j8"], check=True, stdout=subprocess.DEVNULL)


def test_devicewarps_program_compiles():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_devicewarps_program_passes():
    if not os.path.exists(EXE):
        _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_devicewarps passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
