"""The fast warp kernels (k_warp.hip: k_warp_fast, and its bf16 twins of k_warp_bf16.hip) held to EXACT expectations at the source borders, on the
grid of tests/warp_edge_cases.py: integer and half-pixel translations, flips, scale 0.5 and their perspective twins over sources of 1, 2, 3, 5
and 13 pixels' width (the byte-gather branch, the first windowed row, the window clamped to the row end), dense and pitched, 0, 1, 3 and 5 bytes
into an aligned allocation, into targets around the 64-column tile and the 4 rows of a workgroup, with 1 to 53 planes (descriptors in the kernel
arguments, in the uploaded table, in a caller-owned device table) and `used` below the plane count.

Every case runs on the fast path and under CHAIN_FORCE_GENERIC, and a case is accepted only if, in this order,
  1. the kernel is the one the case names (fast path) / the interpreted warp kernel (generic),
  2. exact cases: the output's bytes EQUAL the exact expectation (no tolerance); modelled cases: every element lies within F.evaluate's bound,
  3. the fast path's bytes equal the interpreted path's,
  4. the canary bands of DeviceBackend are intact and every PADDING byte of the output buffer still holds its fill (the whole buffer is read back).

One test item with one pytest subtest per kernel family (transform x store), as tests/test_gpu_colour_model.py does, each naming every failing case.
The GPU suite's list of tests is kept from growing, so this module adds no item to it: its one item takes the place of test_gpu_warp.py's
70-plane test (descriptors uploaded as a table), whose body runs here unchanged as the FIRST subtest, before anything of this module.
Only a mismatch (AssertionError) lets a subtest go on to its next case and the item to its next subtest; whatever else ends a case -- an error the
library returns at launch, a HIP error at the synchronisation -- ends the item: nothing more is started on a card that may have faulted.

Largest |kernel - model| / tolerance per family on the modelled cases, measured on an MI355X (1 = at the bound; fast and interpreted path alike,
whose bytes are the same): affine fp32 0.2671, fp16 0.9944 (one rounding of the 16-bit format), packed 0.2663; perspective fp32 0.2243, fp16 0.9889,
packed 0.2238 -- the CPU oracle's figures of tests/test_warp_edge_cases.py to four decimals; the bf16 families hold exact cases only (0).  Exact
cases have no figure: they are equal or they fail.  No case needed a change to k_warp.hip.  The 152 cases (two runs each) take 0.8 s on an MI355X,
the module 2.9 s with its imports."""
import time

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import helpers as H
from tests import model_cases as MC
from tests import warp_edge_cases as W
from tests.test_gpu_chains import _both
from tests.test_warp_edge_cases import bits, held_to_model

pytestmark = pytest.mark.gpu

PATHS = (("fast", capi.CHAIN_DEFAULT), ("generic", capi.CHAIN_FORCE_GENERIC))


def _run(c, flags):
    """one run of a case on the GPU: (kernel name, backend, iops, views, the whole output buffer's bytes)"""
    import torch
    B = MC.DeviceBackend()
    iops, views = c.build(B)
    name = cvgs.kernel_name(*iops, flags=flags)
    cvgs.executeOperations(torch.cuda.current_stream(), *iops, flags=flags)
    torch.cuda.synchronize()
    whole = np.array(B.result(), copy=True).reshape(-1)  # (B.result() asserts the canary bands)
    return name, B, iops, views, whole


def _hold(c):
    """every acceptance condition of the module docstring on one case; returns the largest ratio against the model (modelled cases)"""
    first, worst = None, 0.0
    for what, flags in PATHS:
        name, B, iops, views, whole = _run(c, flags)
        want_name = c.kernel if what == "fast" else ("warp_perspective_interp" if c.persp else "warp_affine_interp")
        assert name == want_name, "%s: runs on %s, not on %s" % (what, name, want_name)
        got, moved = K.split_output(B.placed, whole)
        if c.cls == W.EXACT:
            want = c.expected(B)
            assert want.shape == got.shape and want.dtype == got.dtype
            bad = bits(want) != bits(got)
            at = np.unravel_index(int(np.argmax(bad)), bad.shape)
            assert not bad.any(), "%s (%s): %d of %d elements differ from the exact expectation, first at %r (%s order): %r, expected %r" % (
                what, name, int(bad.sum()), bad.size, at, c.write, got[at], want[at])
        else:
            ok, ratio, share, text = held_to_model(c, iops, views, got)
            assert share <= 0.01, "%s: the model excludes %.4f of a plane" % (what, share)
            assert ok, "%s (%s): %s" % (what, name, text)
            worst = max(worst, ratio)
        if first is None:
            first = whole
        else:
            assert np.array_equal(first, whole), "%s (%s): %d bytes differ from the fast path" % (what, name, int((first != whole).sum()))
        assert moved.size == 0, "%s (%s): %d padding bytes of the output buffer changed, first at byte %d (the samples start at %d, pitch %d, row %d)" % (
            what, name, moved.size, int(moved[0]), B.placed.origin, B.placed.pitch, B.placed.row_bytes)
    return worst


def _hold_all(cases, label):
    """Every case runs, also behind a mismatch; the test fails with the description of every case that did.  Anything but a mismatch -- an error
    returned at launch included -- is not caught here and ends the item (guarded)."""
    failed, worst, t0 = [], 0.0, time.perf_counter()
    for c in cases:
        try:
            worst = max(worst, _hold(c))
        except AssertionError as e:
            failed.append("%s: %s" % (c.name, str(e)[:400]))
    print("RATIO gpu %-20s %-12s %-8s %.4f" % (label, "%d cases" % len(cases), "2 paths", worst))
    print("SECONDS gpu %-20s %.2f" % (label, time.perf_counter() - t0))
    assert not failed, "%d of %d cases, the first: %s\n%s" % (len(failed), len(cases), failed[0].split(":")[0], "\n".join(failed))


def _warp_many_planes_uses_device_table():
    """More planes than travel in the kernel arguments (56): the descriptors are uploaded stream-ordered.  (from tests/test_gpu_warp.py, unchanged)"""
    import torch
    src = H.random_u8((90, 120, 3), 8)
    n = 70
    ms = [[[1.0, 0.02 * i, 0.5 * i], [-0.01 * i, 1.0, 0.25 * i]] for i in range(n)]

    def build(wrap, wrap_out, out):
        img = wrap(src, cvgs.CV_8UC3)
        return [cvgs.warp(cvgs.WARP_AFFINE, cvgs.CV_8UC3, [img] * n, ms, (64, 48)),
                cvgs.split(cvgs.CV_32FC3, wrap_out(out, cvgs.CV_32FC1), (64, 48))]

    gpu, ref = _both(build, (n, 3 * 64 * 48), np.float32)
    H.assert_bit_exact(gpu[0], ref[0], "70-plane warp")
    t = torch.zeros((90, 120, 3), dtype=torch.uint8, device="cuda:0")
    o = torch.zeros((n, 3 * 64 * 48), dtype=torch.float32, device="cuda:0")
    name = cvgs.kernel_name(cvgs.warp(cvgs.WARP_AFFINE, cvgs.CV_8UC3, [cvgs.GpuMat.from_tensor(t, cvgs.CV_8UC3)] * n, ms, (64, 48)),
                            cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_tensor(o, cvgs.CV_32FC1), (64, 48)))
    assert name == "warp_affine_u8c3_interp"


def test_fast_warp_kernels_at_source_borders(device, subtests):
    """one subtest for the 70-plane warp, one per transform and store"""
    stopped = []

    def guarded(body):
        assert not stopped, "not started: an earlier subtest ended with %s" % stopped[0]
        try:
            body()
        except AssertionError:
            raise
        except BaseException as e:  # not a mismatch: nothing more is started on the card
            stopped.append(repr(e)[:300])
            raise

    with subtests.test(family="70 planes, uploaded table"):
        guarded(_warp_many_planes_uses_device_table)
    assert len(W.FAMILIES) == 8
    for family in W.FAMILIES:
        with subtests.test(family=family):
            cases = W.cases_of(family)
            assert len(cases) >= 10
            guarded(lambda: _hold_all(cases, family))
