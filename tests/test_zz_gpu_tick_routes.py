"""The routes of cvgs_execute_many's fused tick, as tables: which groups become ONE launch and which run chain by chain, that a tick refused
LATE (after its table slot was taken) gives the slot back, and what the queue's entry points refuse, word for word.

ROUTES (test_tick_routes, a subtest per row): the group is captured with tests/test_gpu_many._captured_kernel_nodes -- nothing is launched,
the graph is never replayed -- and the kernel nodes are counted; then the same descriptors run eagerly and every tensor is compared bit for
bit with the CPU oracle.
   1  K1 u8c3, host descriptors, 16 chains x 64 crops = 1024 planes (the large argument block's last fit)          1 node
   2  the same plus a 17th chain of one crop (1025 planes: a staged table, which a capture refuses)                17 nodes; eager: the ring
   3  K1 u8c1, host descriptors (not a family whose planes travel in the arguments), 3 chains                       3 nodes; eager: the ring
   4  K1 u8c3, a device table on every chain, vouched                                                              1 node
   5  K1 u8c3, chain 0 on a device table, chain 1 on host descriptors                                              2 nodes
   6  K4 NV12, 3 chains, the last one holding a crop 2 pixels wide (found after lowering: the LATE refusal)        3 nodes
   7  the same without that crop                                                                                   1 node
   8  K1 with a program whose arithmetic meets an integer-typed value (found on the lowered chain 0)               n nodes
   9  pointwise ticks of 1024 planes                                                                               1 node
  10  pointwise ticks of 1025 planes                                                                               n nodes
  11  pointwise ticks with n * max_batch = 65536: 127 chains of one plane and a last chain of 512                  n - 1 nodes + a refusal
Row 11 cannot be a plain node count: n <= 128 chains reach 65536 only with a chain of 512 planes, and a pointwise chain of more than 64
planes stages its table when it runs on its own, which a capture refuses.  The row therefore captures the call itself: the 127 small chains
are n - 1 kernel nodes and the last chain comes back CVGS_ERR_UNSUPPORTED with the staged upload's text -- the mark of the chain-by-chain
route (fused, the 639 planes travel in the kernel arguments: one node, no refusal).  Its eager run is held to the oracle like every row's.

RELEASE AFTER A LATE REFUSAL (test_a_late_refusal_gives_its_table_slot_back): in a fresh process per mode, the knobs are read once --
CVGS_MANY_INLINE=0 (the stream's table ring) and CVGS_MANY_INLINE=0 CVGS_MANY_PROGRESS_WORD=0 (the event-tracked scratch) -- 40 eager ticks on
one stream, nothing synchronised in between: row 6's tick, refused after its slot was taken, then a K4 tick that fuses with a different crop
list each time.  One synchronise, every tensor against the oracle.  The ring holds 8 fitting slots per stream: a slot leaked by the refusals
would be rewritten under a pending kernel or push the ticks into the scratch, not hang.

QUEUE REFUSALS (test_queue_refusals): AREA chains, NV12-write chains, a chain the server does not take and a dependent group through
cvgs_queue_submit / _submit_many / _submit_on / _submit_many_on: exact code, exact text (copied from cvgs_api.cpp), nothing submitted.

Shapes as tests/test_gpu_independence.py: frames of 97 x 61 (surfaces 64 x 32), targets of (8, 4) or (24, 16).  The module sorts behind
tests/test_zz_gpu_ring.py: its items are the last ones collected (tests/test_gpu_area.py says why)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FW, FH = 97, 61          # pixel frames
SW, SH = 64, 32          # 4:2:0 surfaces
FILL = -777.0

UPLOAD_UNDER_CAPTURE = "descriptor table upload during stream capture: pass a device plane table (cvgs_plane_table_build)"
# the queue's texts, copied from cvgpuspeedup_amd/csrc/cvgs_api.cpp
Q_AREA = "queue: INTER_AREA reads (CVGS_READ_RESIZE_AREA) are served by cvgs_execute / cvgs_execute_many only"
Q_NV12W = "queue: NV12 / NV21 surface writes (CVGS_WRITE_NV12) are served by cvgs_execute / cvgs_execute_many only"
Q_CHAIN = "queue: not a chain the server takes"
Q_CHAINS = "queue: not chains the server takes"
Q_DEPENDENT = "queue: the chains of one group must be independent (a chain writes what another chain reads or writes); submit them one by one"


class Group:
    """Chains on the device with their tensors, and the same chains over host arrays for the oracle."""

    def __init__(self):
        self.chains, self.host_chains, self.outs, self.refs, self.keep = [], [], [], [], []

    def add(self, build, src, src_type, shape, dev):
        """build(src_mat, out_mat) -> iops; `src` a numpy array; shape of the fp32 target"""
        import torch
        st = torch.from_numpy(src).to(dev)
        out = torch.full(shape, FILL, dtype=torch.float32, device=dev)
        ref = np.full(shape, FILL, np.float32)
        self.chains.append(build(cvgs.GpuMat.from_tensor(st, src_type), out))
        self.host_chains.append(build(cvgs.GpuMat.from_array(src, src_type), ref))
        self.outs.append(out)
        self.refs.append(ref)
        self.keep.append(st)
        return self

    def lowered(self):
        return [cvgs.lower(ops) for ops in self.chains]

    def check(self, oracle, what):
        for m, (host, out, ref) in enumerate(zip(self.host_chains, self.outs, self.refs)):
            ref.fill(FILL)
            oracle.execute(cvgs.lower(host))
            H.assert_bit_exact(out.cpu().numpy(), ref, "%s, chain %d" % (what, m))


def _wrap(out, cv_type=cvgs.CV_32FC1):
    return cvgs.GpuMat.from_array(out, cv_type) if isinstance(out, np.ndarray) else cvgs.GpuMat.from_tensor(out, cv_type)


def _crops(n, seed):
    return H.random_crops(n, FW, FH, seed=seed, wmin=4, wmax=48, hmin=4, hmax=30)


def k1_group(dev, sizes, cn=3, dst=(8, 4), seed=100, tables=(), vouched=False, mid=None):
    """K1 chains of sizes[m] crops of a 97 x 61 frame each.  tables: the chains that carry a device plane table; mid: the stages between the
    resize and the split (default: the reference's swap, multiply, subtract, divide)."""
    import torch
    g = Group()
    u, f = cvgs.make_type(cvgs.CV_8U, cn), cvgs.make_type(cvgs.CV_32F, cn)
    for m, n in enumerate(sizes):
        crops = _crops(n, seed + 50 + m)

        def build(src, out, crops=crops, m=m):
            if mid is not None:
                rd = cvgs.resize(u, cvgs.INTER_LINEAR, [src.roi(*c) for c in crops], dst, len(crops))
                ops = [rd] + mid() + [cvgs.split(f, _wrap(out), dst)]
            else:
                ops = H.k1_chain(src, crops, _wrap(out), dst, cn)
            if m in tables and not isinstance(out, np.ndarray):
                tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).to(dev)
                g.keep.append(tab)
                ops[0].table = tab.data_ptr()
                if vouched:
                    ops[0].mats, ops[0].table_vouched = None, True
            return ops
        g.add(build, H.random_u8((FH, FW, cn), seed=seed + m), u, (n, cn * dst[0] * dst[1]), dev)
    return g


def k4_group(dev, rect_lists, dst=(24, 16), seed=800):
    """K4 chains: crops (rect_lists[m]) of a 64 x 32 NV12 surface each -> swap, multiply, subtract, divide -> planar tensor."""
    g = Group()
    f = cvgs.CV_32FC3
    for m, rects in enumerate(rect_lists):
        def build(surf, out, rects=rects):
            luma = cvgs.GpuMat(SH, SW, cvgs.CV_8UC1, surf.data, surf.step, owner=surf.owner)
            return [cvgs.read_nv12([luma.nv12_roi(*r) for r in rects], dst, capi.YUV_LIMITED, capi.BT709, False),
                    cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]),
                    cvgs.split(f, _wrap(out), dst)]
        g.add(build, H.random_u8((SH + SH // 2, SW), seed=seed + m), cvgs.CV_8UC1, (len(rects), 3 * dst[0] * dst[1]), dev)
    return g


def k4_rects(n, seed):
    return [(x & ~1, y & ~1, max(4, w & ~1), max(2, h & ~1)) for (x, y, w, h) in H.random_crops(n, SW, SH, seed=seed, wmin=4, wmax=40, hmin=4, hmax=24)]


NARROW = (2, 2, 2, 4)  # 2 pixels wide: K4's chroma window needs 4 bytes


def late_refused_k4_rects(seed=850):
    return [k4_rects(3, seed), k4_rects(4, seed + 1), k4_rects(2, seed + 2) + [NARROW]]


def pointwise_group(dev, sizes, size=(8, 4), seed=2000):
    """Batched per-pixel chains: sizes[m] views of 8 x 4 pixels of a 97 x 61 frame -> convertTo, subtract, divide -> a dense fp32 tensor."""
    g = Group()
    u, f = cvgs.CV_8UC3, cvgs.CV_32FC3
    w, h = size
    for m, b in enumerate(sizes):
        rects = [((7 * i + 3 * m) % (FW - w), (5 * i + m) % (FH - h), w, h) for i in range(b)]

        def build(src, out, rects=rects, b=b):
            return [cvgs.ReadIOp(capi.READ_PIXEL, u, [src.roi(*r) for r in rects], b), cvgs.convertTo(u, f, 0.3), cvgs.subtract(f, H.K1_SUB[3]),
                    cvgs.divide(f, H.K1_DIV[3]), cvgs.write(f, _wrap(out, f), (w, h))]
        g.add(build, H.random_u8((FH, FW, 3), seed=seed + m), u, (b, w * h * 3), dev)
    return g


def _int_arith_mid():
    f, s16 = cvgs.CV_32FC3, cvgs.make_type(cvgs.CV_16S, 3)
    return [cvgs.convertTo(f, s16, 3.0, -300.0), cvgs.subtract(s16, [100, -100, 32000]), cvgs.convertTo(s16, f)]


def _captured(lib, arr, n):
    """(return code, kernel nodes) of ONE captured cvgs_execute_many call -- tests/test_gpu_many._captured_kernel_nodes for a call that may be
    refused part of the way (row 11)."""
    import torch
    hip = C.CDLL(None)
    if not hasattr(hip, "hipGraphGetNodes"):
        import glob
        hip = C.CDLL(sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))[0])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, count = C.c_void_p(), C.c_size_t(0)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 0) == 0
    rc = lib.cvgs_execute_many(arr, n, side.cuda_stream)
    text = lib.cvgs_last_error().decode() if rc else ""
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
    hip.hipGraphDestroy(graph)
    return rc, text, count.value


def rows(dev):
    """[(label, make_group, kernel nodes of the captured call)]"""
    full = [64] * 16
    return [
        ("1 k1 u8c3 host 1024 planes", lambda: k1_group(dev, full), 1),
        ("2 k1 u8c3 host 1025 planes", lambda: k1_group(dev, full + [1]), 17),
        ("3 k1 u8c1 host", lambda: k1_group(dev, [5, 3, 6], cn=1, dst=(24, 16), seed=300), 3),
        ("4 k1 u8c3 device tables, vouched", lambda: k1_group(dev, [6, 4, 5], dst=(24, 16), seed=400, tables=(0, 1, 2), vouched=True), 1),
        ("5 k1 u8c3 table + host", lambda: k1_group(dev, [6, 4], seed=500, tables=(0,), vouched=True), 2),
        ("6 k4 nv12 with a 2-pixel crop", lambda: k4_group(dev, late_refused_k4_rects()), 3),
        ("7 k4 nv12", lambda: k4_group(dev, [r[:2] for r in late_refused_k4_rects()]), 1),
        ("8 k1 integer-typed arithmetic", lambda: k1_group(dev, [5, 3, 6, 2], seed=600, mid=_int_arith_mid), 4),
        ("9 pointwise 1024 planes", lambda: pointwise_group(dev, full), 1),
        ("10 pointwise 1025 planes", lambda: pointwise_group(dev, full + [1], seed=2100), 17),
    ]


def test_tick_routes(oracle, device, lib, subtests):
    import torch
    from tests.test_gpu_many import _captured_kernel_nodes
    for label, make, want in rows(device):
        with subtests.test(row=label):
            g = make()
            low = g.lowered()
            arr = cvgs.pack_chains(low)
            nodes = _captured_kernel_nodes(lib, arr, len(low), device)
            print("%-36s %3d chains -> %3d nodes" % (label, len(low), nodes))
            assert nodes == want, "%s: %d kernel nodes, expected %d" % (label, nodes, want)
            for o in g.outs:
                assert float(o.min()) == FILL == float(o.max()), "%s: the captured call ran" % label
            capi.check(lib.cvgs_execute_many(arr, len(low), torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            g.check(oracle, label)
    with subtests.test(row="11 pointwise n * max_batch = 65536"):
        g = pointwise_group(device, [1] * 127 + [512], seed=2200)
        low = g.lowered()
        arr = cvgs.pack_chains(low)
        rc, text, nodes = _captured(lib, arr, len(low))
        print("%-36s %3d chains -> %3d nodes, rc %d (%s)" % ("11 pointwise n * max_batch = 65536", len(low), nodes, rc, text))
        assert (rc, text, nodes) == (capi.ERR_UNSUPPORTED, UPLOAD_UNDER_CAPTURE, 127)
        capi.check(lib.cvgs_execute_many(arr, len(low), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        g.check(oracle, "row 11")


_LATE_REFUSALS = r"""
import sys
sys.path.insert(0, %(root)r)
import torch
from cvgpuspeedup_amd import capi, cvgs
from oracle import oracle_binding
from tests import test_zz_gpu_tick_routes as T
oracle_binding.load_oracle()
lib = capi.load_library()
dev = torch.device("cuda:0")
ticks = []
for i in range(40):
    g = T.k4_group(dev, T.late_refused_k4_rects() if i %% 2 == 0 else [T.k4_rects(2 + (i + m) %% 4, 9000 + 10 * i + m) for m in range(3)], seed=900 + 3 * i)
    low = g.lowered()
    ticks.append((g, low, cvgs.pack_chains(low)))
s = torch.cuda.Stream()
torch.cuda.synchronize()
for g, low, arr in ticks:
    capi.check(lib.cvgs_execute_many(arr, len(low), s.cuda_stream))
s.synchronize()
for i, (g, _, _) in enumerate(ticks):
    g.check(oracle_binding, "tick %%d" %% i)
print("TICKS OK", len(ticks))
"""


def test_a_late_refusal_gives_its_table_slot_back(subtests):
    for mode, extra in (("ring", {"CVGS_MANY_INLINE": "0"}), ("events", {"CVGS_MANY_INLINE": "0", "CVGS_MANY_PROGRESS_WORD": "0"})):
        with subtests.test(mode=mode):
            env = dict(os.environ)
            env.update(extra)
            p = subprocess.run([sys.executable, "-c", _LATE_REFUSALS % {"root": ROOT}], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=300)
            assert p.returncode == 0 and "TICKS OK 40" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_queue_refusals(device, lib, subtests):
    """Every refusal comes back before anything is submitted; the AREA / NV12-write ones before the handle is even looked at."""
    import torch
    frame = torch.zeros((FH, FW, 3), dtype=torch.uint8, device=device)
    src = cvgs.GpuMat.from_tensor(frame, cvgs.CV_8UC3)
    f = cvgs.CV_32FC3
    dst, crops = (8, 4), _crops(3, 77)
    outs = [torch.zeros((3, 3 * 8 * 4), dtype=torch.float32, device=device) for _ in range(2)]
    surfs = [torch.zeros((6, 8), dtype=torch.uint8, device=device) for _ in range(3)]

    def k1(out, interp=cvgs.INTER_LINEAR, mid=None, write=None, flags=0):
        rd = cvgs.resize(cvgs.CV_8UC3, interp, [src.roi(*c) for c in crops], dst, 3)
        mid = [cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])] if mid is None else mid
        return cvgs.lower([rd] + mid + [write or cvgs.split(f, _wrap(out), dst)], flags)

    served = k1(outs[0])
    area = k1(outs[0], interp=cvgs.INTER_AREA)
    nv12w = k1(outs[0], mid=[], write=cvgs.write_nv12([cvgs.GpuMat(4, 8, cvgs.CV_8UC1, s.data_ptr(), 8, owner=s) for s in surfs]))
    both = k1(outs[0], interp=cvgs.INTER_AREA)
    both.desc.write.kind = capi.WRITE_NV12  # the AREA refusal is the earlier one
    forced = k1(outs[0], flags=capi.CHAIN_FORCE_GENERIC)
    int_arith = k1(outs[0], mid=_int_arith_mid())
    same_target = k1(outs[0])  # writes what `served` writes
    U, Q = capi.ERR_UNSUPPORTED, cvgs.Queue
    table = [  # (label, chains, code, {entry point: text})
        ("area", [area], U, dict.fromkeys(("submit", "submit_many", "submit_on", "submit_many_on"), Q_AREA)),
        ("area behind a served chain", [served, area], U, dict.fromkeys(("submit_many", "submit_many_on"), Q_AREA)),
        ("nv12 write", [nv12w], U, dict.fromkeys(("submit", "submit_many", "submit_on", "submit_many_on"), Q_NV12W)),
        ("nv12 write behind a served chain", [served, nv12w], U, dict.fromkeys(("submit_many", "submit_many_on"), Q_NV12W)),
        ("area and nv12 write", [both], U, dict.fromkeys(("submit", "submit_many", "submit_on", "submit_many_on"), Q_AREA)),
        ("forced generic", [forced], U, {"submit": Q_CHAIN, "submit_many": Q_CHAIN, "submit_on": Q_CHAIN, "submit_many_on": Q_CHAINS}),
        ("integer-typed arithmetic", [int_arith], U, {"submit": Q_CHAIN, "submit_many": Q_CHAIN, "submit_on": Q_CHAIN, "submit_many_on": Q_CHAINS}),
        ("integer-typed arithmetic in a group", [int_arith, k1(outs[1], mid=_int_arith_mid())], U, {"submit_many": Q_CHAIN, "submit_many_on": Q_CHAINS}),
        ("dependent group", [served, same_target], U, {"submit_many_on": Q_DEPENDENT}),
    ]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    q = cvgs.Queue()
    try:
        for label, chains, code, texts in table:
            ptrs = Q.chain_pointers(chains)
            calls = {"submit": lambda h: lib.cvgs_queue_submit(h, C.byref(chains[0].desc), C.byref(C.c_uint64())),
                     "submit_many": lambda h: lib.cvgs_queue_submit_many(h, ptrs, len(chains), C.byref(C.c_uint64())),
                     "submit_on": lambda h: lib.cvgs_queue_submit_on(h, C.byref(chains[0].desc), side.cuda_stream, 0, C.byref(C.c_uint64())),
                     "submit_many_on": lambda h: lib.cvgs_queue_submit_many_on(h, ptrs, len(chains), side.cuda_stream, Q.MIN_GROUP(2) if len(chains) > 1 else 0,
                                                                               C.byref(C.c_uint64()))}
            for entry, text in texts.items():
                with subtests.test(row=label, entry=entry):
                    rc = calls[entry](q.handle)
                    assert (rc, lib.cvgs_last_error().decode()) == (code, text)
                    if text in (Q_AREA, Q_NV12W):  # refused before the handle is looked at
                        rc = calls[entry](None)
                        assert (rc, lib.cvgs_last_error().decode()) == (code, text)
        side.synchronize()
        assert q.stats()["submitted"] == 0 and q.stats()["error"] == 0
    finally:
        q.destroy()
    for o in outs:
        assert float(o.abs().max()) == 0.0, "a refused submit ran"
