"""Consecutive independent, compatible K1 ticks captured on ONE stream ride in ONE kernel launch (cvgpuspeedup_amd/csrc/cvgs_tick_merge.h, the
capture code in cvgs_api.cpp): the previous tick's graph node takes the new tick's segments (gridDim.z grows by its chains, gridDim.y to the
larger batch); whatever is not proven mergeable becomes a node of its own, in order.

Shapes: 96 x 64 u8c3 frames, 8-wide x 16-high fp32 NCHW targets, the crop set of tests/test_zzz_gpu_tick_overlap.py (one up-scaled, one
down-scaled, the frame's last pixel); a tick is 2 chains of UNEQUAL batches (3 crops and 1 crop) over device plane tables.  Such ticks lie far
under the size floor (kTickMergeMinPixels), so every scenario runs in a CHILD process in which CVGS_TICK_MERGE_MIN_PIXELS=1 (read once)
lowers the floor; the cap (128 chains) is the product's.  One child runs all merge scenarios in turn, a second one runs with
CVGS_TICK_MERGE=0.  In a child every GPU step runs under a watchdog of its own (gpu_step), and the first failed scenario ends the child: no
step launches after a failed one.  Every graph is replayed at most twice.

Every tensor lies between two guard bands; outputs are compared bit for bit with the oracle (computed once per seed) and with eager
launches of the same chains.

The file's name makes it the suite's last: it moves no existing test's place in the run."""
import ctypes as C
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cvgpuspeedup_amd import capi, cvgs  # noqa: E402
from cvgpuspeedup_amd import workloads as W  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import test_zzz_gpu_tick_overlap as T  # noqa: E402  (Captured, gpu_step, hip: the capture rig of the lane tests)

pytestmark = pytest.mark.gpu

FW, FH = 96, 64
CROPS = [[(10, 8, 4, 6), (20, 5, 40, 50), (95, 63, 1, 1)],  # chain 0: up-scaled, down-scaled, one pixel (the frame's last)
         [(30, 2, 66, 62)]]                                 # chain 1: one crop -- the tick's batches are 3 and 1
FILL = -777.0
GUARD = 64  # floats in front of and behind every tensor

MERGED = "merged into the previous tick's launch"
FIRST = "not merged: no earlier tick of this capture"
FOREIGN = "not merged: something else was captured since the previous tick"
DEPENDENT = "not merged: not independent of the ticks in the previous launch"
DIFFERENT = "not merged: another kernel, program, target shape or geometry"
NO_HULL = "not merged: no hull stated"
FULL = "not merged: the previous launch is full"
CAP = 128
# A K4 (NV12) tick of 2 chains between two K1 ticks, one capture: each note up to the counters, three kernel nodes in a line.  Recorded from
# the commit before the capture driver moved into cvgs_tick_capture.h (the K4 tick takes the lane code and is never shown to the merge rule,
# whose node therefore stands: the K1 tick behind it finds a foreign node, not a first tick).
K4_BETWEEN = ["tick: in order, not merged: no earlier tick of this capture on the stream [merged ticks: ",
              "tick: in order: not a K1 tick over device tables, or pooled state rides on the launch [captured ticks: ",
              "tick: in order, not merged: something else was captured since the previous tick [merged ticks: "]
K4_BETWEEN_NODES = 3


def _chain(src, crops, out, dst, table=None, alpha=W.K1_ALPHA):
    """W.k1_chain's chain (resize -> RGB2BGR -> multiply -> subtract -> divide -> split) with the multiplier of the caller's choice."""
    src_type, f_type = cvgs.make_type(cvgs.CV_8U, 3), cvgs.make_type(cvgs.CV_32F, 3)
    rd = cvgs.resize(src_type, cvgs.INTER_LINEAR, [src.roi(*c) for c in crops], dst, len(crops), None, cvgs.IGNORE_AR)
    if table is not None:
        rd.table = table
    return [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f_type), cvgs.multiply(f_type, [alpha] * 3), cvgs.subtract(f_type, W.K1_SUB[3]),
            cvgs.divide(f_type, W.K1_DIV[3]), cvgs.split(f_type, out, dst)]


class Tick:
    """Two chains (3 crops, 1 crop) over device tables; each tensor between two guard bands of one buffer of its own."""

    def __init__(self, dev, seed, dst=(8, 16), alpha=W.K1_ALPHA, outs_of=None, hull=None, mode="stated", frame_views=None, out_views=None):
        import torch
        self.dst, self.alpha = dst, alpha
        self.plane = 3 * dst[0] * dst[1]
        self.frames = [H.random_u8((FH, FW, 3), seed=seed + m) for m in range(2)]
        self.ft = [torch.from_numpy(f).to(dev) for f in self.frames]
        if frame_views is not None:
            for view, f in zip(frame_views, self.ft):
                view.copy_(f)
            self.ft = list(frame_views)
        if outs_of is not None:  # another tick's tensors (and its guard bands)
            self.bufs, self.outs = outs_of.bufs, outs_of.outs
        elif out_views is not None:  # tensors where the caller says (no bands of their own)
            self.bufs, self.outs = [], list(out_views)
        else:
            self.bufs = [torch.full((2 * GUARD + len(CROPS[m]) * self.plane,), FILL, dtype=torch.float32, device=dev) for m in range(2)]
            self.outs = [b[GUARD:GUARD + len(CROPS[m]) * self.plane].view(len(CROPS[m]), self.plane) for m, b in enumerate(self.bufs)]
        self.tabs, self.low = [], []
        for m in range(2):
            g_src, g_out = cvgs.GpuMat.from_tensor(self.ft[m], cvgs.CV_8UC3), cvgs.GpuMat.from_tensor(self.outs[m], cvgs.CV_32FC1)
            ops = _chain(g_src, CROPS[m], g_out, dst, alpha=alpha)
            tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).to(dev)
            self.tabs.append(tab)
            ops = _chain(g_src, CROPS[m], g_out, dst, table=tab.data_ptr(), alpha=alpha)
            if hull is not None:
                ops[0].table_hull = hull(m, cvgs.table_hull(ops[0]))
            if mode == "vouched":  # no host views at hand, no hull stated: vouched for
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
            ref = np.full((len(CROPS[m]), self.plane), FILL, np.float32)
            oracle.execute(cvgs.lower(_chain(cvgs.GpuMat.from_array(self.frames[m], cvgs.CV_8UC3), CROPS[m], cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), self.dst,
                                             alpha=self.alpha)))
            res.append(ref)
        return res

    def refill(self):
        for b in self.bufs:
            b.fill_(FILL)

    def check(self, refs, what, eager=None):
        for m in range(2):
            got = self.outs[m].cpu().numpy()
            H.assert_bit_exact(got, refs[m], "%s: chain %d vs oracle" % (what, m))
            if eager is not None:
                H.assert_bit_exact(got, eager[m], "%s: chain %d vs the eager launches" % (what, m))
        for m, b in enumerate(self.bufs):
            bands = b.cpu().numpy()
            assert (bands[:GUARD] == FILL).all() and (bands[-GUARD:] == FILL).all(), "%s: chain %d wrote into a guard band" % (what, m)


class Nv12Tick(Tick):
    """A K4 tick: two chains (3 crops, 1 crop) of one 96 x 64 NV12 surface each, host descriptors in the kernel arguments."""
    RECTS = [[(0, 0, 96, 64), (10, 8, 40, 48), (32, 16, 32, 32)], [(2, 2, 64, 60)]]

    def __init__(self, dev, seed, dst=(8, 16)):
        import torch
        self.dst, self.plane = dst, 3 * dst[0] * dst[1]
        self.surfs = [H.random_u8((FH * 3 // 2, FW), seed=seed + m) for m in range(2)]
        self.st = [torch.from_numpy(s).to(dev) for s in self.surfs]
        self.bufs = [torch.full((2 * GUARD + len(self.RECTS[m]) * self.plane,), FILL, dtype=torch.float32, device=dev) for m in range(2)]
        self.outs = [b[GUARD:GUARD + len(self.RECTS[m]) * self.plane].view(len(self.RECTS[m]), self.plane) for m, b in enumerate(self.bufs)]
        self.low = [cvgs.lower(self._ops(cvgs.GpuMat.from_tensor(self.st[m], cvgs.CV_8UC1), m, cvgs.GpuMat.from_tensor(self.outs[m], cvgs.CV_32FC1))) for m in range(2)]
        self.arr = cvgs.pack_chains(self.low)

    def _ops(self, surf, m, out):
        f = cvgs.make_type(cvgs.CV_32F, 3)
        luma = cvgs.GpuMat(FH, FW, cvgs.CV_8UC1, surf.data, surf.step, owner=surf.owner)
        return [cvgs.read_nv12([luma.nv12_roi(*r) for r in self.RECTS[m]], self.dst, capi.YUV_FULL, capi.BT601, False), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
                cvgs.multiply(f, [W.K1_ALPHA] * 3), cvgs.subtract(f, W.K1_SUB[3]), cvgs.divide(f, W.K1_DIV[3]), cvgs.split(f, out, self.dst)]

    def refs(self, oracle):
        res = []
        for m in range(2):
            ref = np.full((len(self.RECTS[m]), self.plane), FILL, np.float32)
            oracle.execute(cvgs.lower(self._ops(cvgs.GpuMat.from_array(self.surfs[m], cvgs.CV_8UC1), m, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1))))
            res.append(ref)
        return res


def grid_of(node):
    p = T.KernelNodeParams()
    assert T.hip().hipGraphKernelNodeGetParams(node, C.byref(p)) == 0
    return list(p.gridDim), p.func


def merged_count(note):
    """the process-wide counter of merged ticks, in front of the two older counters"""
    tail = note[note.index("[merged ticks:"):]
    return int(tail[len("[merged ticks:"):tail.index("]")])


def _eager(lib, ticks):
    import torch
    for t in ticks:
        t.refill()
        assert "eager launch" in t.launch(lib, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = [[o.cpu().numpy() for o in t.outs] for t in ticks]
    for t in ticks:
        t.refill()
    torch.cuda.synchronize()
    return res


def _scenarios(lib, dev, oracle):
    """Generator of (name, facts): each scenario asserts what it can see itself and reports the graph's shape and the notes."""
    import torch
    side = torch.cuda.Stream()
    ticks = [Tick(dev, 8000 + 10 * k) for k in range(3)]
    refs = [t.refs(oracle) for t in ticks]
    with T.gpu_step():
        eager = _eager(lib, ticks)
    for k, t in enumerate(ticks):
        for m in range(2):
            H.assert_bit_exact(eager[k][m], refs[k][m], "eager tick %d chain %d vs oracle" % (k, m))

    def captured(seq, replays=1):
        """seq: ticks and ('memset', tensor, value) items, captured in order on the side stream and replayed"""
        with T.gpu_step():
            cap = T.Captured(side).begin()
            for item in seq:
                if isinstance(item, tuple):
                    cap.memset(item[1], item[2])
                else:
                    cap.tick(lib, item)
            cap.end()
            cap.grids = [grid_of(n) for n in cap.kernels]
            cap.replay(replays)
        return cap

    def facts(cap):
        tick_nodes = [s[0] for s in cap.steps if len(s) == 1 and s[0] in cap.kernels]
        return {"notes": cap.notes, "nodes": len(cap.nodes), "kernels": len(cap.kernels), "new_nodes": [len(s) for s in cap.steps],
                "grids": {str(n): grid_of(n)[0] for n in cap.kernels}, "order": [str(n) for n in tick_nodes], "linear": T._linear(cap, [s[0] for s in cap.steps if s])}

    # ---- three compatible independent ticks: one node, z = 6 chains, y = 3 crops --------------------------------------------------------
    solo = captured([ticks[0]])
    solo_grid, solo_func = grid_of(solo.kernels[0])
    ticks[0].check(refs[0], "a tick alone", eager[0])
    solo.destroy()
    ticks[0].refill()
    cap = captured(ticks, replays=1)
    f = facts(cap)
    assert f["kernels"] == 1 and f["nodes"] == 1 and f["new_nodes"] == [1, 0, 0], f
    (grid, func), = [grid_of(n) for n in cap.kernels]
    assert func == solo_func and grid == [solo_grid[0], 3, 6] and solo_grid[1:] == [3, 2], (grid, solo_grid)
    assert FIRST in cap.notes[0] and MERGED + " (4 chains)" in cap.notes[1] and MERGED + " (6 chains)" in cap.notes[2], cap.notes
    assert merged_count(cap.notes[2]) == merged_count(cap.notes[0]) + 2
    for k, t in enumerate(ticks):
        t.check(refs[k], "three merged ticks, tick %d" % k, eager[k])
    first = [[o.clone() for o in t.outs] for t in ticks]
    with T.gpu_step():
        for t in ticks:
            t.refill()
        cap.replay(1)
    for k, t in enumerate(ticks):
        t.check(refs[k], "three merged ticks replayed again, tick %d" % k, eager[k])
        assert all(torch.equal(a, b) for a, b in zip(first[k], t.outs))
    cap.destroy()
    yield "three_ticks", f

    # ---- refusals: one node per tick, in order, the reason in the note ------------------------------------------------------------------
    def refused(name, seq, reason, checks):
        for t in seq:
            if not isinstance(t, tuple):
                t.refill()
        cap = captured(seq)
        f = facts(cap)
        n_ticks = sum(1 for t in seq if not isinstance(t, tuple))
        assert f["kernels"] == n_ticks and f["nodes"] == len(seq) and f["linear"], (name, f)
        assert all(g[2] == 2 and g[1] == 3 for g in f["grids"].values()), (name, f)
        assert reason in cap.notes[-1] and "in order" in cap.notes[-1], (name, cap.notes)
        for t, r in checks:
            t.check(r, name)
        cap.destroy()
        return f

    waw = Tick(dev, 8100, outs_of=ticks[0])
    yield "write_after_write", refused("write after write", [ticks[0], waw], DEPENDENT, [(waw, waw.refs(oracle))])

    frame_bytes, out_bytes = FH * FW * 3, [len(c) * ticks[0].plane * 4 for c in CROPS]
    arena = torch.zeros(3 * frame_bytes, dtype=torch.uint8, device=dev)  # [tick 2's frame 0 | tick 1's two tensors | tick 2's frame 1]
    base = arena.data_ptr()
    o0 = arena[frame_bytes:frame_bytes + out_bytes[0]].view(torch.float32).view(3, -1)
    o1 = arena[frame_bytes + out_bytes[0]:frame_bytes + out_bytes[0] + out_bytes[1]].view(torch.float32).view(1, -1)
    t1 = Tick(dev, 8200, out_views=[o0, o1])
    t2 = Tick(dev, 8210, frame_views=[arena[0:frame_bytes].view(FH, FW, 3), arena[2 * frame_bytes:].view(FH, FW, 3)],
              hull=lambda m, own: (own[0], base + frame_bytes + out_bytes[0]) if m == 0 else (base + frame_bytes + 16, own[1]))
    yield "read_through_an_aliasing_hull", refused("read after write", [t1, t2], DEPENDENT, [(t1, t1.refs(oracle)), (t2, t2.refs(oracle))])

    other = torch.zeros(256, dtype=torch.uint8, device=dev)
    f = refused("memset between", [ticks[0], ("memset", other, 7), ticks[1]], FOREIGN, [(ticks[0], refs[0]), (ticks[1], refs[1])])
    assert int(other.min()) == 7 == int(other.max())
    yield "memset_between", f

    odd = Tick(dev, 8300, alpha=0.25)
    yield "different_operand", refused("different operand", [ticks[0], odd], DIFFERENT, [(ticks[0], refs[0]), (odd, odd.refs(oracle))])

    small = Tick(dev, 8400, dst=(8, 8))
    yield "different_target_size", refused("different target size", [ticks[0], small], DIFFERENT, [(ticks[0], refs[0]), (small, small.refs(oracle))])

    vouched = [Tick(dev, 8500 + 10 * k, mode="vouched") for k in range(2)]
    yield "no_stated_hull", refused("no stated hull", vouched, NO_HULL, [(t, t.refs(oracle)) for t in vouched])

    # ---- the cap: 64 ticks of 2 chains fill a node, the 65th opens a second one behind it ----------------------------------------------
    many = [Tick(dev, 8000) for _ in range(CAP // 2 + 1)]  # the same frames and crops, tensors of their own: one reference serves all
    cap = captured(many)
    f = facts(cap)
    a, b = f["order"]
    assert f["kernels"] == 2 and f["nodes"] == 2 and f["linear"] and f["grids"][a] == [solo_grid[0], 3, CAP] and f["grids"][b] == [solo_grid[0], 3, 2], f
    assert MERGED + " (%d chains)" % CAP in cap.notes[CAP // 2 - 1] and FULL in cap.notes[CAP // 2], cap.notes[-3:]
    for t in many:
        t.check(refs[0], "cap reached", eager[0])
    cap.destroy()
    f["notes"] = f["notes"][-2:]
    yield "cap_reached", f

    # ---- two captures in a row share no state -------------------------------------------------------------------------------------------
    for t in ticks:
        t.refill()
    one = captured(ticks[:2])
    one.destroy()  # (its node handles are dead now)
    two = captured([ticks[2], ticks[0]])
    f = facts(two)
    assert FIRST in one.notes[0] and MERGED in one.notes[1] and FIRST in two.notes[0] and MERGED + " (4 chains)" in two.notes[1], (one.notes, two.notes)
    assert f["kernels"] == 1 and list(f["grids"].values()) == [[solo_grid[0], 3, 4]], f
    for k in range(3):
        ticks[k].check(refs[k], "second capture, tick %d" % k, eager[k])
    two.destroy()
    yield "two_captures", f

    # ---- a K4 tick between two K1 ticks: in order through the lane code, and the merge rule's node stands --------------------------------
    nv = Nv12Tick(dev, 8600)
    nv_refs = nv.refs(oracle)
    with T.gpu_step():
        nv_eager, = _eager(lib, [nv])
    for t in ticks[:2]:
        t.refill()
    cap = captured([ticks[0], nv, ticks[1]])
    f = facts(cap)
    assert f["kernels"] == K4_BETWEEN_NODES == f["nodes"] and f["new_nodes"] == [1, 1, 1] and f["linear"], f
    assert all(note.startswith(want) for note, want in zip(cap.notes, K4_BETWEEN)) and len(cap.notes) == len(K4_BETWEEN), cap.notes
    for k in range(2):
        ticks[k].check(refs[k], "a K4 tick between, K1 tick %d" % k, eager[k])
    nv.check(nv_refs, "a K4 tick between, the K4 tick", nv_eager)
    cap.destroy()
    yield "k4_between", f


def _switched_off(lib, dev, oracle):
    """CVGS_TICK_MERGE=0: the graph of the lane rule -- four nodes in two lanes, the lane notes, no merged-tick counter."""
    import torch
    ticks = [Tick(dev, 8000 + 10 * k) for k in range(4)]
    with T.gpu_step():
        cap = T.Captured(torch.cuda.Stream()).begin()
        for t in ticks:
            cap.tick(lib, t)
        cap.end()
        a, b, c, d = [s[0] for s in cap.steps]
        lanes = cap.parents(a) == set() and cap.parents(b) == set() and cap.parents(c) == {a} and cap.parents(d) == {b}
        grids = [grid_of(n)[0][1:] for n in cap.kernels]
        cap.replay(1)
    for t in ticks:
        t.check(t.refs(oracle), "switched off")
    yield "switched_off", {"notes": cap.notes, "nodes": len(cap.nodes), "kernels": len(cap.kernels), "two_lanes": lanes, "grids": grids}


def _child(which):
    """Runs the scenarios in turn; the first failure ends the run.  Prints one JSON line: {scenario: facts, ..., "failed": text or null}."""
    import torch
    from oracle import oracle_binding
    oracle_binding.load_oracle()
    lib = capi.load_library()
    dev = torch.device("cuda:0")
    out = {"failed": None}
    try:
        for name, facts in (_switched_off if which == "off" else _scenarios)(lib, dev, oracle_binding):
            out[name] = facts
    except BaseException:  # nothing more is launched
        out["failed"] = traceback.format_exc()[-3000:]
    print(json.dumps(out))


def _run_child(which, env):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), which], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1)[:6000])
    return res


@pytest.fixture(scope="module")
def merged():
    return _run_child("merge", {"CVGS_TICK_MERGE_MIN_PIXELS": "1"})


def _scenario(res, name):
    assert name in res, "scenario %r did not run: %s" % (name, res["failed"])
    return res[name]


def test_three_compatible_independent_ticks_are_one_launch(merged):
    f = _scenario(merged, "three_ticks")
    assert f["kernels"] == 1 and f["new_nodes"] == [1, 0, 0]
    assert [g[1:] for g in f["grids"].values()] == [[3, 6]], "gridDim.y == 3 (the larger batch), gridDim.z == 6 (the chains of three ticks)"
    assert MERGED + " (6 chains)" in f["notes"][2]


@pytest.mark.parametrize("name,reason", [("write_after_write", DEPENDENT), ("read_through_an_aliasing_hull", DEPENDENT), ("memset_between", FOREIGN),
                                         ("different_operand", DIFFERENT), ("different_target_size", DIFFERENT), ("no_stated_hull", NO_HULL)])
def test_a_refusal_leaves_one_node_per_tick_in_order(merged, name, reason):
    f = _scenario(merged, name)
    assert f["kernels"] == 2 and f["linear"] and reason in f["notes"][-1], f
    assert MERGED not in " ".join(f["notes"])


def test_a_full_node_is_followed_by_a_second_one(merged):
    f = _scenario(merged, "cap_reached")
    assert f["kernels"] == 2 and f["linear"] and sorted(g[2] for g in f["grids"].values()) == [2, CAP], f
    assert FULL in f["notes"][-1]


def test_two_captures_in_a_row_share_no_state(merged):
    f = _scenario(merged, "two_captures")
    assert f["kernels"] == 1 and FIRST in f["notes"][0] and MERGED in f["notes"][1], f


def test_a_k4_tick_between_two_k1_ticks_leaves_the_merge_rule_alone(merged):
    f = _scenario(merged, "k4_between")
    assert f["kernels"] == K4_BETWEEN_NODES and f["linear"], f
    assert [n[:len(w)] for n, w in zip(f["notes"], K4_BETWEEN)] == K4_BETWEEN, f["notes"]


def test_every_scenario_ran(merged):
    assert merged["failed"] is None, merged["failed"]


def test_switched_off_by_the_environment():
    res = _run_child("off", {"CVGS_TICK_MERGE": "0", "CVGS_TICK_MERGE_MIN_PIXELS": "1"})
    assert res["failed"] is None, res["failed"]
    f = res["switched_off"]
    assert f["nodes"] == 4 and f["kernels"] == 4 and f["two_lanes"] and all(g == [3, 2] for g in f["grids"]), f
    assert T.FIRST in f["notes"][0] and all(T.BESIDE in n for n in f["notes"][1:]), f["notes"]
    assert not any("merged" in n for n in f["notes"]), "today's notes, without the third counter"


if __name__ == "__main__":
    _child(sys.argv[1] if len(sys.argv) > 1 else "merge")
