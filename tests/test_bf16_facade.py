"""The C++ facade's bf16 hand-off (cvgs/bfloat16.h, CV_16BF types in cvgs/cv_shim.h): cvgs::bfloat16_t against the host rounding the
GPU tests compare with, a bf16 chain compiling against the facade, and (GPU) the headline chain with convertTo<CV_32FC3, CV_16BFC3> +
split<CV_16BFC3> checked against its fp32 twin run through the same facade."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_bf16_types import _same_bits, rne_bf16, special_values, widen_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "cvgpuspeedup_amd", "include")
HIPCC = "/opt/rocm/bin/hipcc"

ROUNDTRIP = r"""
#include <cvgs/bfloat16.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
// the 65536 bf16 patterns -> float (raw, 4 bytes each) into argv[1]; the float32 patterns of argv[2] (raw) -> bf16 bits into argv[3]
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* o = std::fopen(argv[1], "wb");
    for (uint32_t b = 0; b < 65536; ++b) {
        const float f = (float)cvgs::bfloat16_t::from_bits((uint16_t)b);
        std::fwrite(&f, 4, 1, o);
    }
    std::fclose(o);
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    float f;
    while (std::fread(&f, 4, 1, in) == 1) {
        const cvgs::bfloat16_t h(f);
        std::fwrite(&h.bits, 2, 1, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
"""

CHAIN = r"""
#include <cvGPUSpeedup.h>
static_assert(std::is_same_v<CUDA_T(CV_16BFC1), cvgs::bfloat16_t>, "CUDA_T(CV_16BFC1)");
static_assert(cvGS::cv_type_of<CUDA_T(CV_16BFC3)> == CV_16BFC3, "the bf16 flag survives the type round trip");
static_assert(CV_16BFC3 == (CV_16FC3 | 0x1000), "CV_16BFC3 = CV_16FC3 | CVGS_TYPE_FLAG_BF16");
int main() {
    cv::cuda::Stream s;
    cv::cuda::GpuMat frame(720, 1280, CV_8UC3), out(4, 3 * 64 * 128, CV_16F);
    std::array<cv::cuda::GpuMat, 4> crops;
    for (auto& c : crops) c = frame(cv::Rect(0, 0, 100, 200));
    auto rd = cvGS::resize<CV_8UC3, cv::INTER_LINEAR, 4, cvGS::IGNORE_AR>(crops, cv::Size(64, 128), 4, cvGS::cvScalar_set<CV_32FC3>(0.f));
    cvGS::executeOperations(s, rd, cvGS::convertTo<CV_32FC3, CV_16BFC3>(), cvGS::split<CV_16BFC3>(out, cv::Size(64, 128)));
    cvGS::executeOperations(s, rd, cvGS::convertTo<CV_32FC3, CV_16BFC3>(1.f / 255.f, 0.5f), cvGS::write<CV_16BFC3>(out));
    auto t = cvGS::gpuMat2Tensor<cvgs::bfloat16_t>(out, cv::Size(64, 128), 3);
    (void)t;
    cvGS::CircularTensor<CV_8UC3, CV_16BFC1, 3, 4, fk::CircularTensorOrder::NewestFirst> ct(64, 128);
    return 0;
}
"""

PROGRAM = r"""
#include "common.h"
// the headline chain (resize -> swap -> mul -> sub -> div) into a bf16 NCHW tensor, and its fp32 twin: every bf16 element must be the
// round-to-nearest-even of the fp32 one (cvgs::bfloat16_t), bit for bit
int main() {
    constexpr int TI = CV_8UC3, TF = CV_32FC3, TB = CV_16BFC3, BATCH = 20;
    const cv::Size up(64, 128);
    cv::cuda::Stream stream;
    cv::Mat h_frame(720, 1280, TI);
    fill_random(h_frame, 0xB16ull);
    cv::cuda::GpuMat d_frame(h_frame);
    std::array<cv::cuda::GpuMat, BATCH> crops;
    for (int i = 0; i < BATCH; ++i) {
        const int w = 4 + (i * 41) % 400, h = 9 + (i * 59) % 600, x = (i * 97) % (1280 - w), y = (i * 71) % (720 - h);
        crops[i] = d_frame(cv::Rect(x, y, w, h));
    }
    const size_t n = (size_t)BATCH * 3 * up.width * up.height;
    cv::cuda::GpuMat d_bf(BATCH, up.width * up.height * 3, CV_16F), d_f32(BATCH, up.width * up.height * 3, CV_32F);
    const float alpha[3] = {0.3f, 0.3f, 0.3f};
    auto head = [&]() {
        return std::make_tuple(cvGS::resize<TI, cv::INTER_LINEAR, BATCH, cvGS::IGNORE_AR>(crops, up, BATCH, cvGS::cvScalar_set<TF>(0.f)),
                               cvGS::cvtColor<cv::COLOR_RGB2BGR, TF>(), cvGS::multiply<TF>(cv::Scalar(alpha[0], alpha[1], alpha[2])),
                               cvGS::subtract<TF>(cv::Scalar(40.f, 50.f, 60.f)), cvGS::divide<TF>(cv::Scalar(57.f, 58.f, 59.f)));
    };
    std::apply([&](const auto&... iops) { cvGS::executeOperations(stream, iops..., cvGS::convertTo<TF, TB>(), cvGS::split<TB>(d_bf, up)); }, head());
    std::apply([&](const auto&... iops) { cvGS::executeOperations(stream, iops..., cvGS::split<TF>(d_f32, up)); }, head());
    stream.waitForCompletion();
    const auto hb = fetch(d_bf.data, n * 2), hf = fetch(d_f32.data, n * 4);
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        float f;
        uint16_t b;
        std::memcpy(&f, hf.data() + 4 * i, 4);
        std::memcpy(&b, hb.data() + 2 * i, 2);
        bad += cvgs::bfloat16_t(f).bits != b;
    }
    CHECK(bad == 0, "bf16 NCHW hand-off == RNE(fp32 twin), " << bad << " of " << n << " differ");
    return report("bf16 facade");
}
"""


def _hipcc(src, out, extra=()):
    return subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I" + INC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           str(src), "-o", str(out)] + list(extra), capture_output=True, text=True)


@pytest.mark.parametrize("compiler", ["hipcc", "g++"])
def test_bfloat16_t_roundtrip(tmp_path, compiler):
    """cvgs::bfloat16_t == the host RNE helper: all 65,536 patterns back to float, the special classes + 10^6 random fp32 forward."""
    src = tmp_path / "rt.cpp"
    src.write_text(ROUNDTRIP)
    exe = tmp_path / "rt"
    cmd = [HIPCC, "-x", "c++"] if compiler == "hipcc" else ["g++"]
    r = subprocess.run(cmd + ["-std=c++17", "-O1", "-I" + INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(7)
    fwd = np.concatenate([special_values(), rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    (tmp_path / "in.bin").write_bytes(fwd.astype(np.float32).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "back.bin"), str(tmp_path / "in.bin"), str(tmp_path / "fwd.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    back = np.frombuffer((tmp_path / "back.bin").read_bytes(), np.float32)
    want_back = widen_bf16(np.arange(65536, dtype=np.uint16))
    assert np.array_equal(back.view(np.uint32), want_back.view(np.uint32))
    got = np.frombuffer((tmp_path / "fwd.bin").read_bytes(), np.uint16)
    assert _same_bits(got, rne_bf16(fwd))


def test_facade_compiles_bf16_chain(tmp_path):
    src = tmp_path / "chain.cpp"
    src.write_text(CHAIN)
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I" + INC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_facade_bf16_program_runs(tmp_path):
    lib = os.path.join(ROOT, "cvgpuspeedup_amd", "lib")
    src = tmp_path / "bf16_prog.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "bf16_prog"
    r = _hipcc(src, exe, ["-I" + os.path.join(ROOT, "tests", "cpp"), "-L" + lib, "-lcvgs_hip", "-L" + os.path.join(ROOT, "oracle"), "-lcvgs_oracle",
                          "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
