// device_boxes.cpp -- detector -> crops -> classifier input with no host in the loop (cvGS::DeviceCrops, cvgs_plane_tables_from_boxes).
//   every frame, all on ONE stream and with no host synchronisation in between:
//     1. the producer writes this frame's boxes and their count into device memory (here: a device-to-device copy on the stream stands in
//        for the detector's last kernel -- the host never sees the boxes of the frame it is working on),
//     2. DeviceCrops::update builds the plane tables of both cameras in one small kernel,
//     3. the tick: both cameras' resize -> normalize -> NCHW chains as ONE fused launch (cvGS::ChainBatch).
//   The host only waits at the very end, and prints how many boxes the LAST frame had from rects().
#include <cvGPUSpeedup.h>

#include <cstdio>
#include <vector>

int main() {
    constexpr int kMax = 50, kFrames = 8, kCams = 2;
    const cv::Size dsize(64, 128);
    cv::cuda::Stream stream;
    hipStream_t s = cv::cuda::StreamAccessor::getStream(stream);
    std::vector<cv::cuda::GpuMat> frames, tensors;
    std::vector<cvGS::DeviceCrops> crops;
    for (int c = 0; c < kCams; ++c) {
        frames.emplace_back(1080, 1920, CV_8UC3);
        (void)hipMemset(frames.back().data, 64 + 32 * c, frames.back().step * 1080);
        tensors.emplace_back(kMax, 3 * dsize.width * dsize.height, CV_32FC1);
        crops.emplace_back(kMax);
    }
    // the "detector": kFrames pre-computed outputs in device memory, (xa, ya, xb, yb) floats + one count per camera and frame
    std::vector<float> h_boxes((size_t)kFrames * kCams * kMax * 4);
    std::vector<int32_t> h_counts((size_t)kFrames * kCams);
    for (int f = 0; f < kFrames; ++f)
        for (int c = 0; c < kCams; ++c) {
            h_counts[(size_t)f * kCams + c] = 20 + 3 * f + c;
            for (int i = 0; i < kMax; ++i) {
                float* b = &h_boxes[(((size_t)f * kCams + c) * kMax + i) * 4];
                b[0] = 30.f * i - 40.f + f; b[1] = 17.f * i - 25.f; b[2] = b[0] + 60.5f + i; b[3] = b[1] + 121.25f + 2 * i; // some reach outside the frame
            }
        }
    float *d_detector = nullptr, *d_boxes = nullptr;
    int32_t *d_detector_counts = nullptr, *d_counts = nullptr;
    fk::hip_check(hipMalloc((void**)&d_detector, h_boxes.size() * sizeof(float)), "hipMalloc");
    fk::hip_check(hipMalloc((void**)&d_detector_counts, h_counts.size() * sizeof(int32_t)), "hipMalloc");
    fk::hip_check(hipMalloc((void**)&d_boxes, (size_t)kCams * kMax * 4 * sizeof(float)), "hipMalloc");
    fk::hip_check(hipMalloc((void**)&d_counts, kCams * sizeof(int32_t)), "hipMalloc");
    fk::hip_check(hipMemcpy(d_detector, h_boxes.data(), h_boxes.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
    fk::hip_check(hipMemcpy(d_detector_counts, h_counts.data(), h_counts.size() * sizeof(int32_t), hipMemcpyHostToDevice), "hipMemcpy");

    for (int f = 0; f < kFrames; ++f) {
        // 1. the producer, on the stream
        fk::hip_check(hipMemcpyAsync(d_boxes, d_detector + (size_t)f * kCams * kMax * 4, (size_t)kCams * kMax * 4 * sizeof(float), hipMemcpyDeviceToDevice, s), "producer");
        fk::hip_check(hipMemcpyAsync(d_counts, d_detector_counts + (size_t)f * kCams, kCams * sizeof(int32_t), hipMemcpyDeviceToDevice, s), "producer");
        // 2. both cameras' tables in one launch
        std::vector<cvGS::DeviceCrops::Job> jobs;
        for (int c = 0; c < kCams; ++c) jobs.push_back({&crops[(size_t)c], frames[(size_t)c], d_boxes + (size_t)c * kMax * 4, d_counts + c});
        cvGS::DeviceCrops::update(stream, jobs, CVGS_BOX_XYXY_F32, dsize);
        // 3. the tick
        cvGS::ChainBatch tick;
        for (int c = 0; c < kCams; ++c)
            tick.add(cvGS::resize<CV_8UC3, cv::INTER_LINEAR>(crops[(size_t)c]), cvGS::cvtColor<cv::COLOR_RGB2BGR, CV_32FC3>(),
                     cvGS::multiply<CV_32FC3>(cv::Scalar(1 / 255.0, 1 / 255.0, 1 / 255.0)), cvGS::subtract<CV_32FC3>(cv::Scalar(0.485, 0.456, 0.406)),
                     cvGS::divide<CV_32FC3>(cv::Scalar(0.229, 0.224, 0.225)), cvGS::split<CV_32FC3>(tensors[(size_t)c], dsize));
        tick.execute(stream);
    }
    stream.waitForCompletion();
    int ok = 1;
    for (int c = 0; c < kCams; ++c) {
        std::vector<int32_t> rects((size_t)kMax * 4);
        fk::hip_check(hipMemcpy(rects.data(), crops[(size_t)c].rects(), rects.size() * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy");
        int valid = 0;
        for (int i = 0; i < kMax; ++i) valid += rects[(size_t)i * 4 + 2] > 0;
        const int live = h_counts[(size_t)(kFrames - 1) * kCams + c];
        std::printf("camera %d: %d of %d boxes of the last frame lie inside it (count %d)\n", c, valid, kMax, live);
        ok = ok && valid > 0 && valid <= live;
    }
    (void)hipFree(d_detector); (void)hipFree(d_detector_counts); (void)hipFree(d_boxes); (void)hipFree(d_counts);
    std::printf(ok ? "device boxes: ok\n" : "device boxes: FAILED\n");
    return ok ? 0 : 1;
}
