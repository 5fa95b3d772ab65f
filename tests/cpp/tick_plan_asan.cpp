// plan_tick -- the admission of cvgs_execute_many's fused tick -- over the descriptor sets of tests/test_zz_gpu_tick_routes.py's route table,
// as a stand-alone host program for AddressSanitizer + UBSan:  make -C tests/cpp bin/tick_plan_asan && tests/cpp/bin/tick_plan_asan
// The C-ABI's host file is compiled INTO this program (its admission function lives in an anonymous namespace); the launchers plan_tick's
// neighbours call are stubbed and the rest of the file is dropped at link time (--gc-sections).  Nothing here launches, and without a GPU
// hipStreamIsCapturing fails, which plan_tick reads as "not capturing".
#include "../../cvgpuspeedup_amd/csrc/cvgs_api.cpp"

#include <cassert>
#include <memory>

namespace cvgs {
int launch_generic(const ChainArgs&, const PlaneParams*, int, const MirrorArgs&, void*, bool, LaunchInfo*) { return 0; }
int launch_generic64(const ChainArgs&, const Prog64Args&, const PlaneParams*, int, void*, bool, LaunchInfo*) { return 0; }
int launch_k1(const ChainArgs&, const PlaneParams*, int, LaunchCtx&, bool, LaunchInfo*, uint32_t) { return 0; }
int launch_nv12(const ChainArgs&, const PlaneParams*, int, int, LaunchCtx&, bool, LaunchInfo*, uint32_t) { return 0; }
int launch_yuv422(const ChainArgs&, const PlaneParams*, int, LaunchCtx&, bool, LaunchInfo*) { return 0; }
int launch_yuv444(const ChainArgs&, const PlaneParams*, int, LaunchCtx&, bool, LaunchInfo*) { return 0; }
bool k4_planes_eligible(const PlaneParams*, int, int, int) { return false; }
int launch_pointwise_many(const ChainArgs&, const PlaneParams*, int, const ManySeg*, int, int, uint32_t, void*, bool) { return 0; }
int launch_pointwise(const ChainArgs&, const PlaneParams*, int, uint32_t, void*, bool, LaunchInfo*) { return 0; }
} // namespace cvgs

namespace {
struct Set {
    std::vector<cvgs_chain_desc> chains;
    std::vector<std::vector<cvgs_image2d>> views;
    static constexpr size_t kArena = (size_t)1 << 26;
    std::unique_ptr<uint8_t[]> arena{new uint8_t[kArena]}; // every source and target lies in here, never read: chains_independent compares addresses only
    size_t at = 0;
    uint8_t* take(size_t bytes) {
        uint8_t* p = arena.get() + at;
        at += (bytes + 255) & ~(size_t)255;
        assert(at <= kArena);
        return p;
    }
    // a chain of `batch` views of a 97 x 61 frame (64 x 32 surface) into a planar fp32 tensor of 8 x 4
    void add(int kind, int batch, int cn = 3, bool table = false, int write_kind = CVGS_WRITE_TENSOR_SPLIT, uint32_t flags = 0) {
        cvgs_chain_desc c{};
        c.struct_size = sizeof(c);
        c.flags = flags;
        const bool yuv = kind == CVGS_READ_NV12_RESIZE_LINEAR;
        const int fw = yuv ? 64 : 97, fh = yuv ? 32 : 61, px = yuv ? 1 : cn;
        uint8_t* frame = take((size_t)fw * px * fh * 2);
        views.emplace_back();
        for (int k = 0; k < batch; ++k) views.back().push_back(cvgs_image2d{frame + (k % 8) * 2 * px, 8, 4, fw * px, 0});
        c.read.kind = kind;
        c.read.src_type = CVGS_MAKETYPE(CVGS_DEPTH_8U, yuv ? 1 : cn);
        c.read.src = views.back().data();
        c.read.batch = c.read.used_planes = batch;
        c.read.dst_width = 8;
        c.read.dst_height = 4;
        c.read.yuv_layout = yuv ? CVGS_YUV_NV12 : 0;
        if (table) {
            c.read.flags = CVGS_READ_FLAG_TABLE_ON_DEVICE | CVGS_READ_FLAG_TABLE_SOURCES_VOUCHED;
            c.read.src = frame; // (a device table: never looked at on the host)
        }
        c.write.kind = write_kind;
        c.write.dst_type = CVGS_MAKETYPE(CVGS_DEPTH_32F, write_kind == CVGS_WRITE_PIXEL_3D ? 3 : 1);
        c.write.width = 8;
        c.write.height = 4;
        c.write.data = take((size_t)(batch > 0 ? batch : 1) * 4 * 8 * 4 * 4);
        chains.push_back(c);
    }
    TickPlan plan() { return plan_tick(chains.data(), (int32_t)chains.size(), nullptr); }
};

int failures = 0;
void expect(const char* row, Set& s, TickFamily family, TickCarrier carrier, size_t planes, int max_batch) {
    const TickPlan p = s.plan();
    const bool ok = p.family == family && (family == TickFamily::none || (p.carrier == carrier && p.total_planes == planes && p.max_batch == max_batch));
    std::printf("%-52s family %d carrier %d planes %zu max_batch %d  %s\n", row, (int)p.family, (int)p.carrier, p.total_planes, p.max_batch, ok ? "ok" : "WRONG");
    failures += !ok;
}
} // namespace

int main() {
    const int K1 = CVGS_READ_RESIZE_LINEAR, K4 = CVGS_READ_NV12_RESIZE_LINEAR, PW = CVGS_READ_PIXEL;
    { Set s; for (int i = 0; i < 16; ++i) s.add(K1, 64); expect("1 k1 u8c3 host, 1024 planes", s, TickFamily::k1, TickCarrier::kernarg, 1024, 64); }
    { Set s; for (int i = 0; i < 16; ++i) s.add(K1, 64); s.add(K1, 1); expect("2 k1 u8c3 host, 1025 planes", s, TickFamily::k1, TickCarrier::host_table, 1025, 64); }
    { Set s; for (int b : {5, 3, 6}) s.add(K1, b, 1); expect("3 k1 u8c1 host", s, TickFamily::k1, TickCarrier::host_table, 14, 6); }
    { Set s; for (int b : {6, 4, 5}) s.add(K1, b, 3, true); expect("4 k1 u8c3 device tables, vouched", s, TickFamily::k1, TickCarrier::device_tables, 15, 6); }
    { Set s; s.add(K1, 6, 3, true); s.add(K1, 4); expect("5 k1 u8c3 table + host", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; for (int b : {3, 4, 3}) s.add(K4, b); expect("6 / 7 k4 nv12 (the narrow crop shows after lowering)", s, TickFamily::k4, TickCarrier::kernarg, 10, 4); }
    { Set s; for (int b : {5, 3, 6, 2}) s.add(K1, b); expect("8 k1 (integer arithmetic shows after lowering)", s, TickFamily::k1, TickCarrier::kernarg, 16, 6); }
    { Set s; for (int i = 0; i < 16; ++i) s.add(PW, 64, 3, false, CVGS_WRITE_PIXEL_3D); expect("9 pointwise, 1024 planes", s, TickFamily::pointwise, TickCarrier::kernarg, 1024, 64); }
    { Set s; for (int i = 0; i < 16; ++i) s.add(PW, 64, 3, false, CVGS_WRITE_PIXEL_3D); s.add(PW, 1, 3, false, CVGS_WRITE_PIXEL_3D); expect("10 pointwise, 1025 planes", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; for (int i = 0; i < 127; ++i) s.add(PW, 1, 3, false, CVGS_WRITE_PIXEL_3D); s.add(PW, 512, 3, false, CVGS_WRITE_PIXEL_3D); expect("11 pointwise, n * max_batch = 65536", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    // beside the table: the refusals plan_tick makes on its own
    { Set s; s.add(K1, 4); expect("one chain", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; s.add(K1, 4); s.add(K1, 0); expect("a chain of no planes", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; s.add(K1, 4); s.add(K1, 65536); expect("a batch beyond the grid", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; s.add(K4, 4, 3, true); s.add(K4, 4, 3, true); expect("k4 on device tables", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; s.add(K1, 4, 3, false, CVGS_WRITE_TENSOR_SPLIT, CVGS_CHAIN_FORCE_GENERIC); s.add(K1, 4, 3, false, CVGS_WRITE_TENSOR_SPLIT, CVGS_CHAIN_FORCE_GENERIC); expect("forced generic", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; s.add(K1, 4); s.add(K1, 4); s.chains[1].write.data = s.chains[0].write.data; expect("two chains, one target", s, TickFamily::none, TickCarrier::kernarg, 0, 0); }
    { Set s; for (int i = 0; i < CVGS_MAX_CHAINS; ++i) s.add(K1, 8); expect("CVGS_MAX_CHAINS chains", s, TickFamily::k1, TickCarrier::kernarg, 1024, 8); }
    std::printf(failures ? "FAILED: %d rows\n" : "all rows as expected\n", failures);
    return failures ? 1 : 0;
}
