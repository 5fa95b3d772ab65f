"""Every CircularTensor update path of the gfx950 build held DIRECTLY to the independent ring model (tests/ring_model.py: which frame each
slot shows) and to tests/f64_model.py (what that frame's elements are), without the CPU oracle in between, over the grid of
tests/circular_cases.py.  The whole tensor at data() is read back and EVERY element is compared: slots that show a frame within the float64
model's derived bound, never-written slots bit-zero.

Default handles: BATCH + 3 eager updates (mirrored rings: 3 * BATCH), checked after each.  Capturable handles: 2 eager updates, BATCH + 2
updates captured into ONE graph (a linear sequence on one side stream), then: nothing ran -- replay -- one eager update -- replay, the
tensor checked at each of the four points against the model's plain sequence of updates.  Mirrored rings are read through data() and show
exactly BATCH distinct data() values over 3 * BATCH updates.

Largest |kernel - model| / tolerance per element type (1 = at the bound; the RATIO lines print them): NOT YET MEASURED on an MI355X when this
file was written -- the CPU oracle's figures on the same grid are 32f 0.58 (per-pixel pushes) / 0.40 (resize pushes), 64f 0.49, 8u 0.50 (the
integer output's half step), 16f / 16bf 1.00 (a 16-bit float's tolerance IS one rounding of its format).  The pass criterion is the model's
bound, not these figures."""
import ctypes as C

import pytest

from cvgpuspeedup_amd import cvgs
from tests import circular_cases as CC

pytestmark = pytest.mark.gpu

_MODEL_FRAMES = {}
_WORST = {}


def model_frame(case, i):
    if (case.name, i) not in _MODEL_FRAMES:
        _MODEL_FRAMES[(case.name, i)] = CC.model_frame(case, i)
    return _MODEL_FRAMES[(case.name, i)]


def _read_device(ptr, nbytes):
    import torch
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3) == 0
    return t.cpu().numpy()


class Run:
    """one handle, the model's ring beside it, and the frames on the device"""

    def __init__(self, case, n_frames):
        import torch
        CC.assert_preconditions(case)
        self.case, self.ring, self.ran, self.worst = case, CC.ring(case), 0, 0.0
        self.u8 = cvgs.make_type(cvgs.CV_8U, case.cn)
        self.frames_t = [torch.from_numpy(CC.frame(case, i)).to("cuda:0") for i in range(n_frames)]
        torch.cuda.synchronize()
        self.ct = cvgs.CircularTensor(self.u8, CC.elem_type(case), CC.color_planes(case), case.batch, CC.order_of(case), CC.mode_of(case), case.w, case.h,
                                      mirrored=case.mirrored, capturable=case.handle == "dev")
        assert self.ct.nbytes() == self.ring.nbytes()

    def update(self, i):
        """enqueue (or capture) the update that pushes frame i"""
        import torch
        ct, t = self.ct, CC.pixel_type(self.case)
        wr = {"std": ct.write_split, "tr": ct.write_splitT, "pk": ct.write_packed}[self.case.layout](t)
        ct.update(torch.cuda.current_stream(), *CC.chain(self.case, cvgs.GpuMat.from_tensor(self.frames_t[i], self.u8), wr))

    def ran_frames(self, indices):
        """the model's side of updates that have RUN"""
        for i in indices:
            self.ring.push(model_frame(self.case, i))
        self.ran += len(indices)

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        assert self.ct.updates() == self.ran, what
        bad, ratio, where = self.ring.check(_read_device(self.ct.data(), self.ct.nbytes()))
        self.worst = max(self.worst, ratio)
        assert bad == 0, "%s, %s: %s" % (self.case.name, what, where)

    def report(self):
        key = (self.case.handle, self.case.depth)
        _WORST[key] = max(_WORST.get(key, 0.0), self.worst)
        print("RATIO gpu ring %-5s %-62s %.4f   (worst so far, %s handles, %s elements: %.4f)" % (
            self.case.depth, self.case.name, self.worst, self.case.handle, self.case.depth, _WORST[key]))

    def eager_window(self, first, n, what):
        """n eager updates, each checked; returns the data() value after each"""
        seen = []
        for i in range(first, first + n):
            self.update(i)
            self.ran_frames([i])
            self.check("%s %d" % (what, i - first + 1))
            seen.append(self.ct.data())
        return seen


def _items(handle):
    """the cases that are test items of this module; CC.BESIDE_THE_JOB_LIMIT run as subtests of tests/test_zz_gpu_ring.py (the GPU suite's
    list of tests is kept from growing: tests/test_gpu_area.py says how), through the same two functions"""
    return [n for n, c in CC.CASES.items() if c.handle == handle and n not in CC.BESIDE_THE_JOB_LIMIT]


def run_cases_beside_the_job_limit(device, subtests):
    """Only a mismatch (AssertionError) lets the item go on to its next case: whatever else ends a case ends the item."""
    stopped = []
    for name in CC.BESIDE_THE_JOB_LIMIT:
        with subtests.test(case=name):
            assert not stopped, "not started: an earlier case ended with %s" % stopped[0]
            try:
                (test_default_handle_within_the_model if CC.CASES[name].handle == "def" else test_capturable_handle_within_the_model)(device, name)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise


@pytest.mark.parametrize("name", _items("def"))
def test_default_handle_within_the_model(device, name):
    case = CC.CASES[name]
    n = max(case.batch + 3, 3 * case.batch) if case.mirrored else case.batch + 3
    run = Run(case, n)
    try:
        run.check("before any update")
        seen = run.eager_window(0, n, "eager update")
        if case.mirrored:
            assert len(set(seen[:3 * case.batch])) == case.batch, seen
        else:
            assert len(set(seen)) == 1, seen
        run.report()
    finally:
        run.ct.release()


@pytest.mark.parametrize("name", _items("dev"))
def test_capturable_handle_within_the_model(device, name):
    import torch
    case = CC.CASES[name]
    B, N = case.batch, case.batch + 2
    graph = list(range(3, 3 + N))  # frames 0, 1, 2: the eager updates; 3 ..: the captured ones; behind them: the mirrored ring's last window
    run = Run(case, 3 + N + (3 * B if case.mirrored else 0))
    try:
        run.check("before any update")
        run.eager_window(0, 2, "eager update")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in graph:
                run.update(i)
        run.check("the capture itself must not run anything")
        g.replay()
        run.ran_frames(graph)
        run.check("first replay = updates 3..%d" % (2 + N))
        run.eager_window(2, 1, "eager update between the replays")
        g.replay()
        run.ran_frames(graph)
        run.check("second replay = the NEXT %d updates" % N)
        if case.mirrored:  # a mirrored ring's window moves with every update and comes round after BATCH of them
            seen = run.eager_window(3 + N, 3 * B, "eager update after the replays")
            assert len(set(seen)) == B, seen
        run.report()
        del g
    finally:
        torch.cuda.synchronize()
        run.ct.release()
