"""The one GPU item of tests/k4_x2_cases.py: both forms of K4's two-pixel kernel (csrc/k_nv12_x2.hip) -- above all the pipelined one,
two rows per wave with every store through one buffer descriptor -- on small, odd and batched targets, a subtest per case.

Per case the output tensor lies inside a larger allocation, 256 guard bytes of 0xA5 on both sides (and two more target rows of them
behind it), its payload prefilled with 0xFF bytes (a NaN no chain of the table produces).  After each of three launches -- as dispatched (the reported name must be the table's, "@r2"
included), CVGS_CHAIN_NO_THREAD_FUSION (k4_nv12_resize_*) and CVGS_CHAIN_FORCE_GENERIC -- the guard bytes are unchanged, every payload word
has been written, and the payload equals the CPU oracle's picture bit for bit; the dispatched picture also lies within the float64
model's derived bound (tests/f64_model.py), as tests/test_k4_x2_cases.py shows for the oracle's.  A store the kernel relies on the hardware
to drop (the second row of the last wave of an odd-height target) would land in a neighbouring plane, past the tensor (the guard band) or
nowhere (an unwritten word).

Only a mismatch (AssertionError) lets the item go on to its next case: anything else -- an error the library returns, a HIP error at the
synchronisation -- ends it, the remaining cases report "not started", and nothing more is started on a card that may have faulted.

The hook is set per case by a fixture (the library reads CVGS_K4_X2 on every call), restored when the item ends.

The 17 cases take 4.0 s on an MI355X, nearly all of it the float64 model and the oracle on the CPU."""
import os

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import k4_x2_cases as K

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = 0xA5        # guard bands
UNWRITTEN = 0xFF       # payload before every launch: 0xFFFFFFFF, a NaN
LAUNCHES = ((0, "as dispatched"), (capi.CHAIN_NO_THREAD_FUSION, "one-pixel kernel"), (capi.CHAIN_FORCE_GENERIC, "interpreted kernel"))


@pytest.fixture
def hook():
    """hook(True / False): CVGS_K4_X2=1 / unset for the calls that follow; the environment is put back when the item ends"""
    old = os.environ.get("CVGS_K4_X2")

    def set_(on):
        if on:
            os.environ["CVGS_K4_X2"] = "1"
        else:
            os.environ.pop("CVGS_K4_X2", None)
    yield set_
    if old is None:
        os.environ.pop("CVGS_K4_X2", None)
    else:
        os.environ["CVGS_K4_X2"] = old


class Out:
    """A device tensor of `nbytes` inside a larger allocation: [guard | payload | guard].  The band behind the tensor is GUARD bytes plus
    two target rows, all of it checked: a store of a row past the target that the hardware did NOT drop lands one or two rows behind the last
    plane, and must land in memory this test owns."""

    def __init__(self, torch, device, nbytes, row_bytes):
        self.torch, self.nbytes = torch, nbytes
        self.t = torch.full((GUARD + nbytes + GUARD + 2 * row_bytes,), SENTINEL, dtype=torch.uint8, device=device)
        self.ptr = self.t.data_ptr() + GUARD

    def prefill(self):
        self.t[GUARD:GUARD + self.nbytes] = UNWRITTEN

    def check(self, want, what):
        got = self.t.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all(), "%s: the guard band in front of the tensor changed" % what
        assert (got[GUARD + self.nbytes:] == SENTINEL).all(), "%s: the guard band behind the tensor changed" % what
        pay = got[GUARD:GUARD + self.nbytes].view(np.uint32)
        unwritten = np.flatnonzero(pay == 0xFFFFFFFF)
        assert unwritten.size == 0, "%s: %d elements never written, first at element %d" % (what, unwritten.size, unwritten[0])
        bad = np.flatnonzero(pay != want.view(np.uint32))
        assert bad.size == 0, "%s: %d of %d elements differ from the oracle, first at element %d (got %r, want %r)" % (
            what, bad.size, pay.size, bad[0], pay.view(np.float32)[bad[0]], want[bad[0]])
        return pay.view(np.float32)


_device_surfaces = {}


def _surface_on(torch, device, name):
    """the surface in an allocation of exactly its own size: it ends where the allocation ends"""
    if name not in _device_surfaces:
        _device_surfaces[name] = torch.from_numpy(K.surface(name)[2].copy()).to(device)
    return _device_surfaces[name]


def run_case(torch, device, oracle, hook, case):
    want = K.oracle_output(oracle, case)
    assert want.any() and want.size * 4 == K.tensor_bytes(case)
    st = _surface_on(torch, device, case.surface)
    o = Out(torch, device, K.tensor_bytes(case), case.dst[0] * 4)
    hook(case.hook)
    chain = K.ops(case, st.data_ptr(), o.ptr, keep=(st, o.t))
    for flags, what in LAUNCHES:
        name = cvgs.kernel_name(*chain, flags=flags)
        if flags == 0:
            assert name == case.want, "%s: dispatched to %s, the table says %s" % (case.name, name, case.want)
        elif flags == capi.CHAIN_NO_THREAD_FUSION:
            assert name.startswith("k4_nv12_resize_"), name
        else:
            assert "k4_" not in name, name
        o.prefill()
        cvgs.executeOperations(torch.cuda.current_stream(), *chain, flags=flags)
        torch.cuda.synchronize()
        got = o.check(want, "%s, %s (%s)" % (case.name, what, name))
        if flags == 0:
            ok, ratio = K.check_against_model(case, got)
            print("RATIO gpu %-40s %-32s %.4f" % (case.name, name, float(np.nanmax(ratio))))
            assert ok.all(), "%s (%s): %d of %d elements outside the model's bound, worst ratio %.3f" % (
                case.name, name, int((~ok).sum()), ok.size, float(np.nanmax(ratio)))


def test_k4_x2_both_forms_on_small_odd_and_batched_targets(device, oracle, hook, subtests):
    import torch
    cases = list(K.CASES.values())
    assert len(cases) == 17 and sum(c.want.endswith("@r2") for c in cases) >= 10
    stopped = []
    for case in cases:
        with subtests.test(case=case.name):
            assert not stopped, "not started: an earlier case ended with %s" % stopped[0]
            try:
                run_case(torch, device, oracle, hook, case)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise
