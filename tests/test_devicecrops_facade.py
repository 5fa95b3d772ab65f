"""cvGS::DeviceCrops on the C++ facade (tests/cpp/test_devicecrops.cpp): without a GPU the program COMPILES against the facade and the
extension header stays plain C99; on the GPU it runs -- executeOperations, a ChainBatch tick and a recorded tick over device-built tables
against host-described crops, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "bin", "test_devicecrops")


def _build():
    subprocess.run(["make", "-C", os.path.join(ROOT, "cvgpuspeedup_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CPP, "-j8"], check=True, stdout=subprocess.DEVNULL)


def test_devicecrops_program_compiles():
    _build()
    assert os.path.exists(EXE)


def test_extension_header_is_plain_c99(tmp_path):
    """include/cvgs_hip_ext.h with the box-table struct: what a cgo / JNI / ctypes binding includes (gcc -std=c99 -pedantic)."""
    src = tmp_path / "ext.c"
    src.write_text('#include "include/cvgs_hip_ext.h"\n'
                   'int main(void) { cvgs_box_table_desc d; d.struct_size = (uint32_t)sizeof d; return d.struct_size == 96 ? 0 : 1; }\n')
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + ROOT, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0  # the layout the Python binding mirrors: 96 bytes


@pytest.mark.gpu
def test_devicecrops_program_passes():
    if not os.path.exists(EXE):
        _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_devicecrops passed!!" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_device_boxes_example_runs():
    """examples/device_boxes.cpp: producer -> DeviceCrops::update -> the tick, eight frames of two cameras on one stream, no host
    synchronisation before the end."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "examples", "bin", "device_boxes")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device boxes: ok" in r.stdout, r.stdout + r.stderr
