"""Consecutive independent K1 ticks captured on ONE stream run beside each other (cvgpuspeedup_amd/csrc/cvgs_tick_overlap.h, the capture code
in cvgs_api.cpp): the graph gets two lanes -- B behind what stood in front of A, C behind A, D behind B -- and everything that is not proven
independent, or is not this library's previous tick, keeps today's linear graph.

Shapes: 96 x 64 u8c3 frames; a chain is 3 crops (one up-scaled, one down-scaled, one of a single pixel) to an 8-wide x 16-high fp32 NCHW
target; a tick is 2 chains over device plane tables.  Graphs are captured with hipStreamBeginCapture through ctypes (as
tests/test_gpu_many._captured_kernel_nodes does); every tick's node is identified while it is captured (the stream's dependency set after
the call names it), the edges are read with hipGraphGetEdges.  Every graph is replayed at most twice.  Every GPU step runs under a
watchdog of its own (gpu_step: the process is ended if the step does not return in time, so nothing more is started on the device).

The reference of every tensor is computed once (the oracle) and shared; the eager launches of the same ticks, one by one, are the second.

The file's name makes it the suite's last (as the test_zz_* files before it): it captures graphs on side streams and ends its process on a
hung step, so it runs where no other test file is still to come, and it moves no existing test's place in the run."""
import contextlib
import ctypes as C
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cvgpuspeedup_amd import capi, cvgs  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

FW, FH, DST = 96, 64, (8, 16)
CROPS = [[(10, 8, 4, 6), (20, 5, 40, 50), (95, 63, 1, 1)],  # up-scaled, down-scaled, one pixel (the frame's last)
         [(0, 0, 3, 5), (30, 2, 66, 62), (0, 63, 1, 1)]]
PLANE = 3 * DST[0] * DST[1]
FILL = -777.0
STEP_S = 60

BESIDE = "captured beside the previous tick"
FIRST = "no earlier tick of this capture"
FOREIGN = "something else was captured since the previous tick"
DEPENDENT = "not independent of the ticks it would run beside"
NO_HULL = "no hull stated"
OTHER_STREAMS = "run on another stream as well"
OFF = "CVGS_TICK_OVERLAP=0"


@contextlib.contextmanager
def gpu_step(seconds=STEP_S):
    """One GPU step under its own time limit: a step that does not come back ends the process (nothing more is started on the device)."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


class KernelNodeParams(C.Structure):
    _fields_ = [("blockDim", C.c_uint * 3), ("extra", C.c_void_p), ("func", C.c_void_p), ("gridDim", C.c_uint * 3), ("kernelParams", C.c_void_p),
                ("sharedMemBytes", C.c_uint)]


_hip = None


def hip():
    global _hip
    if _hip is None:
        import torch
        h = C.CDLL(None)  # libamdhip64 came in with torch; its symbols are global in this process
        if not hasattr(h, "hipGraphGetEdges"):
            import glob
            h = C.CDLL(sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))[0])
        vp, sz = C.c_void_p, C.c_size_t
        h.hipStreamBeginCapture.argtypes = [vp, C.c_int]
        h.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
        h.hipStreamGetCaptureInfo_v2.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(vp), C.POINTER(C.POINTER(vp)), C.POINTER(sz)]
        h.hipGraphGetNodes.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
        h.hipGraphGetEdges.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz)]
        h.hipGraphNodeGetType.argtypes = [vp, C.POINTER(C.c_int)]
        h.hipGraphKernelNodeGetParams.argtypes = [vp, C.POINTER(KernelNodeParams)]
        h.hipKernelNameRefByPtr.argtypes = [vp, vp]
        h.hipKernelNameRefByPtr.restype = C.c_char_p
        h.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, C.POINTER(vp), C.c_char_p, sz]
        h.hipGraphLaunch.argtypes = [vp, vp]
        h.hipGraphExecDestroy.argtypes = [vp]
        h.hipGraphDestroy.argtypes = [vp]
        h.hipMemsetAsync.argtypes = [vp, C.c_int, sz, vp]
        _hip = h
    return _hip


class Tick:
    """Two chains over device tables: frames, crop lists, tensors, the lowered chains and their packed array."""

    def __init__(self, dev, seed, outs=None, hull=None, mode="stated", frame_views=None):
        import torch
        self.frames = [H.random_u8((FH, FW, 3), seed=seed + m) for m in range(2)]
        self.ft = [torch.from_numpy(f).to(dev) for f in self.frames]
        if frame_views is not None:  # the frames live where the caller says
            for view, f in zip(frame_views, self.ft):
                view.copy_(f)
            self.ft = list(frame_views)
        self.outs = outs or [torch.full((3, PLANE), FILL, dtype=torch.float32, device=dev) for _ in range(2)]
        self.tabs, self.low = [], []
        for m in range(2):
            g_src, g_out = cvgs.GpuMat.from_tensor(self.ft[m], cvgs.CV_8UC3), cvgs.GpuMat.from_tensor(self.outs[m], cvgs.CV_32FC1)
            ops = H.k1_chain(g_src, CROPS[m], g_out, dst=DST)
            tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).to(dev)
            self.tabs.append(tab)
            ops = H.k1_chain(g_src, CROPS[m], g_out, dst=DST, table=tab.data_ptr())
            if hull is not None:  # a stated hull of the caller's own: (lo, hi) or a function of the chain's computed one
                ops[0].table_hull = hull(m, cvgs.table_hull(ops[0])) if callable(hull) else hull
            if mode == "unstated":
                ops[0].mats = None  # no host views at hand: nothing stated, nothing vouched
            elif mode == "vouched":
                ops[0].mats = None
                ops[0].table_vouched = True
            self.low.append(cvgs.lower(ops))
        self.arr = cvgs.pack_chains(self.low)

    def launch(self, lib, stream):
        capi.check(lib.cvgs_execute_many(self.arr, 2, stream))
        return lib.cvgs_last_error().decode()

    def refs(self, oracle):
        res = []
        for m in range(2):
            ref = np.full((3, PLANE), FILL, np.float32)
            oracle.execute(cvgs.lower(H.k1_chain(cvgs.GpuMat.from_array(self.frames[m], cvgs.CV_8UC3), CROPS[m], cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), dst=DST)))
            res.append(ref)
        return res


class Captured:
    """A graph captured on a side stream, step by step: every step's new node (the stream's dependency set names it) and the note it left."""

    def __init__(self, stream):
        self.stream = C.c_void_p(stream.cuda_stream)
        self.graph = C.c_void_p()
        self.steps, self.notes, self.seen = [], [], set()

    def begin(self):
        assert hip().hipStreamBeginCapture(self.stream, 0) == 0  # hipStreamCaptureModeGlobal
        return self

    def deps(self):
        st, cid, g, arr, n = C.c_int(0), C.c_ulonglong(0), C.c_void_p(), C.POINTER(C.c_void_p)(), C.c_size_t(0)
        assert hip().hipStreamGetCaptureInfo_v2(self.stream, C.byref(st), C.byref(cid), C.byref(g), C.byref(arr), C.byref(n)) == 0
        assert st.value == 1  # hipStreamCaptureStatusActive
        return [arr[i] for i in range(n.value)]

    def _new_nodes(self):
        new = [d for d in self.deps() if d not in self.seen]
        self.seen.update(new)
        return new

    def tick(self, lib, t):
        note = t.launch(lib, self.stream.value)
        new = self._new_nodes()
        self.steps.append(new)  # one node for a fused tick; an un-fused one leaves its LAST launch here
        self.notes.append(note)
        return note

    def memset(self, tensor, value):
        assert hip().hipMemsetAsync(C.c_void_p(tensor.data_ptr()), value, tensor.numel() * tensor.element_size(), self.stream) == 0
        new = self._new_nodes()
        assert len(new) == 1
        self.steps.append(new)
        return new[0]

    def end(self):
        h = hip()
        assert h.hipStreamEndCapture(self.stream, C.byref(self.graph)) == 0
        n = C.c_size_t(0)
        assert h.hipGraphGetNodes(self.graph, None, C.byref(n)) == 0
        nodes = (C.c_void_p * n.value)()
        assert h.hipGraphGetNodes(self.graph, nodes, C.byref(n)) == 0
        self.nodes = list(nodes)
        self.kernels = []
        for nd in self.nodes:
            ty = C.c_int(-1)
            assert h.hipGraphNodeGetType(nd, C.byref(ty)) == 0
            if ty.value == 0:  # hipGraphNodeTypeKernel
                self.kernels.append(nd)
        e = C.c_size_t(0)
        assert h.hipGraphGetEdges(self.graph, None, None, C.byref(e)) == 0
        fr, to = (C.c_void_p * max(1, e.value))(), (C.c_void_p * max(1, e.value))()
        if e.value:
            assert h.hipGraphGetEdges(self.graph, fr, to, C.byref(e)) == 0
        self.edges = {(fr[i], to[i]) for i in range(e.value)}
        return self

    def kernel_identity(self, node):
        p = KernelNodeParams()
        assert hip().hipGraphKernelNodeGetParams(node, C.byref(p)) == 0
        name = hip().hipKernelNameRefByPtr(p.func, self.stream)
        return p.func, (name.decode() if name else None)

    def path(self, a, b):
        """is b ordered behind a?"""
        todo, seen = [a], set()
        while todo:
            x = todo.pop()
            for f, t in self.edges:
                if f == x and t not in seen:
                    if t == b:
                        return True
                    seen.add(t)
                    todo.append(t)
        return False

    def parents(self, n):
        return {f for f, t in self.edges if t == n}

    def replay(self, times=1):
        h = hip()
        import torch
        assert times <= 2
        ex = C.c_void_p()
        assert h.hipGraphInstantiate(C.byref(ex), self.graph, None, None, 0) == 0
        for _ in range(times):
            assert h.hipGraphLaunch(ex, self.stream) == 0
        torch.cuda.synchronize()
        h.hipGraphExecDestroy(ex)

    def destroy(self):
        if self.graph:
            hip().hipGraphDestroy(self.graph)
            self.graph = C.c_void_p()


def counts(note):
    """(overlapped, in order): the process-wide counters at the end of a note"""
    tail = note[note.rindex("[captured ticks:"):]
    a, b = [int(w) for w in tail.replace(",", " ").split() if w.isdigit()]
    return a, b


@pytest.fixture(scope="module")
def rig(device, lib, oracle):
    """Four independent ticks, their oracle tensors (computed once) and what the same ticks give launched eagerly one by one."""
    import torch
    ticks = [Tick(device, 7000 + 10 * k) for k in range(4)]
    refs = [t.refs(oracle) for t in ticks]
    with gpu_step():
        for t in ticks:
            note = t.launch(lib, torch.cuda.current_stream().cuda_stream)
            assert "eager launch" in note, note
        torch.cuda.synchronize()
        eager = [[o.cpu().numpy() for o in t.outs] for t in ticks]
    for k in range(4):
        for m in range(2):
            H.assert_bit_exact(eager[k][m], refs[k][m], "eager tick %d chain %d vs oracle" % (k, m))
    return {"ticks": ticks, "refs": refs, "eager": eager, "side": torch.cuda.Stream()}


def _refill(ticks):
    import torch
    for t in ticks:
        for o in t.outs:
            o.fill_(FILL)
    torch.cuda.synchronize()


def _check(ticks, refs, eager, what):
    for k, t in enumerate(ticks):
        for m in range(2):
            got = t.outs[m].cpu().numpy()
            H.assert_bit_exact(got, refs[k][m], "%s: tick %d chain %d vs oracle" % (what, k, m))
            if eager is not None:
                H.assert_bit_exact(got, eager[k][m], "%s: tick %d chain %d vs the eager launches" % (what, k, m))


def test_four_independent_ticks_take_two_lanes(rig, lib, device):
    ticks = rig["ticks"]
    with gpu_step():
        _refill(ticks)
        solo = Captured(rig["side"]).begin()  # a tick alone: the node "as before"
        solo.tick(lib, ticks[0])
        solo.end()
        assert len(solo.nodes) == 1 and len(solo.kernels) == 1 and FIRST in solo.notes[0]
        before = solo.kernel_identity(solo.kernels[0])
        solo.destroy()
        cap = Captured(rig["side"]).begin()
        before_counts = None
        for t in ticks:
            note = cap.tick(lib, t)
            before_counts = before_counts or counts(note)
        cap.end()
    print(cap.notes)
    assert FIRST in cap.notes[0] and all(BESIDE in n for n in cap.notes[1:]), cap.notes
    assert counts(cap.notes[-1]) == (before_counts[0] + 3, before_counts[1]), "three ticks overlapped, counted"
    assert all(len(s) == 1 for s in cap.steps), "each tick is exactly one node"
    a, b, c, d = [s[0] for s in cap.steps]
    assert len(cap.nodes) == 4 and sorted(cap.kernels) == sorted([a, b, c, d]), "four kernel nodes and nothing else"
    for n in (a, b, c, d):
        assert cap.kernel_identity(n) == before, "the tick's kernel is the one a tick has always launched"
    if before[1] is not None:
        assert "k1" in before[1].lower(), before
    assert not cap.path(a, b) and not cap.path(b, a), "B runs beside A"
    assert cap.parents(a) == set() and cap.parents(b) == set(), "B is captured behind what stood in front of A (nothing)"
    assert cap.parents(c) == {a} and not cap.path(b, c), "C depends on A, not on B"
    assert cap.parents(d) == {b} and not cap.path(c, d), "D depends on B, not on C"
    with gpu_step():
        cap.replay(2)
        _check(ticks, rig["refs"], rig["eager"], "two lanes")
    cap.destroy()


def test_write_after_write_keeps_its_order(rig, lib, device, oracle):
    """Tick 2 writes tick 1's tensors from other frames: an edge, and the tensors hold tick 2's values."""
    t1 = rig["ticks"][0]
    t2 = Tick(device, 7100, outs=t1.outs)
    with gpu_step():
        _refill([t1])
        cap = Captured(rig["side"]).begin()
        cap.tick(lib, t1)
        cap.tick(lib, t2)
        cap.end()
        a, b = cap.steps[0][0], cap.steps[1][0]
        assert DEPENDENT in cap.notes[1], cap.notes
        assert (a, b) in cap.edges and len(cap.nodes) == 2
        cap.replay(2)
        _check([t2], [t2.refs(oracle)], None, "write after write")
        assert not np.array_equal(t2.outs[0].cpu().numpy(), rig["refs"][0][0]), "the two ticks' values differ: the order shows"
    cap.destroy()


def test_read_after_write_through_an_aliasing_hull(rig, lib, device, oracle):
    """Tick 2 states source hulls that cover tick 1's output bytes.  One buffer holds [tick 2's frame 0 | tick 1's two tensors | tick 2's
    frame 1]; chain 0 of tick 2 states its own crops' range stretched up into tick 1's first tensor, chain 1 its own stretched down into
    it -- ranges a caller with a coarser idea of its sources would state.  Tick 2's own tensors lie elsewhere: it stays ONE launch."""
    import torch
    frame_bytes, out_bytes = FH * FW * 3, 3 * PLANE * 4
    arena = torch.zeros(3 * frame_bytes, dtype=torch.uint8, device=device)
    base = arena.data_ptr()
    assert base % 4 == 0
    outs1 = [arena[frame_bytes + m * out_bytes:frame_bytes + (m + 1) * out_bytes].view(torch.float32).view(3, PLANE) for m in range(2)]
    views = [arena[0:frame_bytes].view(FH, FW, 3), arena[2 * frame_bytes:3 * frame_bytes].view(FH, FW, 3)]
    t1 = Tick(device, 7200, outs=outs1)
    t2 = Tick(device, 7210, frame_views=views,
              hull=lambda m, own: (own[0], base + frame_bytes + out_bytes) if m == 0 else (base + frame_bytes + 16, own[1]))
    lo, hi = t2.low[0].desc.read.table_src_lo, t2.low[0].desc.read.table_src_hi
    assert lo < outs1[0].data_ptr() + out_bytes and outs1[0].data_ptr() < hi, "the stated hull meets tick 1's tensor"
    for o in t2.outs:  # (and not its own tick's: the tick stays ONE launch)
        assert not (lo < o.data_ptr() + out_bytes and o.data_ptr() < hi)
    with gpu_step():
        for o in outs1:
            o.fill_(FILL)
        _refill([t2])
        cap = Captured(rig["side"]).begin()
        cap.tick(lib, t1)
        cap.tick(lib, t2)
        cap.end()
        a, b = cap.steps[0][0], cap.steps[1][0]
        assert len(cap.nodes) == 2 and DEPENDENT in cap.notes[1], cap.notes
        assert (a, b) in cap.edges
        cap.replay(1)
        _check([t1, t2], [t1.refs(oracle), t2.refs(oracle)], None, "read after write")
    cap.destroy()


def test_a_foreign_node_between_two_ticks(rig, lib, device):
    import torch
    t1, t2 = rig["ticks"][0], rig["ticks"][1]
    other = torch.zeros(256, dtype=torch.uint8, device=device)
    with gpu_step():
        _refill([t1, t2])
        cap = Captured(rig["side"]).begin()
        cap.tick(lib, t1)
        m = cap.memset(other, 7)
        cap.tick(lib, t2)
        cap.end()
        a, b = cap.steps[0][0], cap.steps[2][0]
        assert FOREIGN in cap.notes[1], cap.notes
        assert cap.parents(m) == {a} and cap.parents(b) == {m}, "the memset behind the first tick, the second tick behind the memset"
        cap.replay(1)
        _check([t1, t2], rig["refs"][:2], rig["eager"][:2], "foreign node between")
        assert int(other.min()) == 7 == int(other.max())
    cap.destroy()


def test_a_foreign_node_after_two_overlapped_ticks(rig, lib, device):
    """A memset of the FIRST tick's tensor captured after two overlapped ticks waits for both; the tensor ends as the memset left it."""
    t1, t2 = rig["ticks"][0], rig["ticks"][1]
    with gpu_step():
        _refill([t1, t2])
        cap = Captured(rig["side"]).begin()
        cap.tick(lib, t1)
        cap.tick(lib, t2)
        m = cap.memset(t1.outs[0], 0)
        cap.end()
        a, b = cap.steps[0][0], cap.steps[1][0]
        assert BESIDE in cap.notes[1] and not cap.path(a, b) and not cap.path(b, a)
        assert cap.parents(m) == {a, b}, "the memset depends on both ticks"
        cap.replay(2)
        assert not t1.outs[0].cpu().numpy().any(), "the final bytes are the memset's"
        H.assert_bit_exact(t1.outs[1].cpu().numpy(), rig["refs"][0][1], "tick 1 chain 1")
        _check([t2], rig["refs"][1:2], rig["eager"][1:2], "foreign node after")
    cap.destroy()


def _linear(cap, nodes):
    return all(cap.parents(n) == ({nodes[i - 1]} if i else set()) for i, n in enumerate(nodes))


def test_chains_without_hulls_keep_the_linear_graph(rig, lib, device, oracle):
    """Vouched-for tables state no hull: the ticks are fused but nothing can be proven about them -- one node each, in order, and the note says
    why.  Tables that state nothing and are not vouched for are not fused at all; that is no longer silent either."""
    with gpu_step():
        ticks = [Tick(device, 7300 + 10 * k, mode="vouched") for k in range(3)]
        cap = Captured(rig["side"]).begin()
        for t in ticks:
            cap.tick(lib, t)
        cap.end()
        assert all(NO_HULL in n for n in cap.notes), cap.notes
        assert counts(cap.notes[2])[1] == counts(cap.notes[0])[1] + 2, "refusals are counted"
        nodes = [s[0] for s in cap.steps]
        assert len(cap.nodes) == 3 and _linear(cap, nodes), "the linear graph"
        cap.replay(1)
        _check(ticks, [t.refs(oracle) for t in ticks], None, "vouched")
        cap.destroy()
        ticks = [Tick(device, 7400 + 10 * k, mode="unstated") for k in range(2)]
        cap = Captured(rig["side"]).begin()
        for t in ticks:
            cap.tick(lib, t)
        cap.end()
        assert all(n.startswith("not fused:") and NO_HULL in n and "not vouched" in n for n in cap.notes), cap.notes
        assert len(cap.nodes) == 4 and len(cap.edges) == 3, "four launches, one by one"
        cap.replay(1)
        _check(ticks, [t.refs(oracle) for t in ticks], None, "unstated")
        cap.destroy()


def test_two_captures_in_a_row_share_no_state(rig, lib, device):
    """The second capture on the same stream starts over: its first tick has nothing to run beside (the first capture's nodes belong to a
    graph that may be gone), its second tick overlaps again."""
    ticks = rig["ticks"]
    with gpu_step():
        _refill(ticks)
        first = Captured(rig["side"]).begin()
        first.tick(lib, ticks[0])
        first.tick(lib, ticks[1])
        first.end()
        first.destroy()  # (its node handles are dead now)
        second = Captured(rig["side"]).begin()
        second.tick(lib, ticks[2])
        second.tick(lib, ticks[3])
        second.tick(lib, ticks[0])
        second.end()
        assert FIRST in first.notes[0] and BESIDE in first.notes[1]
        assert FIRST in second.notes[0] and BESIDE in second.notes[1] and BESIDE in second.notes[2], second.notes
        a, b, c = [s[0] for s in second.steps]
        assert len(second.nodes) == 3 and second.parents(a) == set() and second.parents(b) == set() and second.parents(c) == {a}
        second.replay(1)
        _check([ticks[2], ticks[3], ticks[0]], [rig["refs"][k] for k in (2, 3, 0)], [rig["eager"][k] for k in (2, 3, 0)], "second capture")
    second.destroy()


def test_ticks_the_caller_spread_over_two_streams_stay_where_they_are(rig, lib, device):
    """Ticks alternating over two streams of ONE capture are two lanes already: no stream's ticks are split again."""
    import torch
    ticks = rig["ticks"]
    s0, s1 = rig["side"], torch.cuda.Stream()
    with gpu_step():
        _refill(ticks)
        cap = Captured(s0).begin()
        s1.wait_stream(s0)  # (an event recorded and waited for: s1 joins the capture)
        notes = [t.launch(lib, (s0, s1)[k % 2].cuda_stream) for k, t in enumerate(ticks)]
        s0.wait_stream(s1)
        cap.end()
        print(notes)
        assert FIRST in notes[0] and FIRST in notes[1] and OTHER_STREAMS in notes[2] and OTHER_STREAMS in notes[3], notes
        assert len(cap.kernels) == 4
        between = [(f, t) for f, t in cap.edges if f in cap.kernels and t in cap.kernels]
        assert len(between) == 2 and len({f for f, t in between} | {t for f, t in between}) == 4, "two chains of two ticks"
        cap.replay(1)
        _check(ticks, rig["refs"], rig["eager"], "two streams")
    cap.destroy()


def _child():
    """CVGS_TICK_OVERLAP=0 (read once, at the first tick): four independent ticks captured in a fresh process."""
    import torch
    from oracle import oracle_binding
    oracle_binding.load_oracle()
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    ticks = [Tick(dev, 7000 + 10 * k) for k in range(4)]
    with gpu_step():
        cap = Captured(torch.cuda.Stream()).begin()
        for t in ticks:
            cap.tick(lib, t)
        cap.end()
        nodes = [s[0] for s in cap.steps]
        cap.replay(1)
        _check(ticks, [t.refs(oracle_binding) for t in ticks], None, "switched off")
    print(json.dumps({"notes": cap.notes, "nodes": len(cap.nodes), "linear": _linear(cap, nodes), "counts": counts(cap.notes[-1])}))


def test_switched_off_by_the_environment(rig):
    env = dict(os.environ, CVGS_TICK_OVERLAP="0")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["nodes"] == 4 and res["linear"], res
    assert all(OFF in n for n in res["notes"]), res
    assert res["counts"] == [0, 4], res


if __name__ == "__main__":
    _child()
