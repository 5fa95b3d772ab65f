"""The thread-fused pointwise kernels (k_pointwise.hip: k_pointwise4 and the tick kernel k_pointwise4_many, the bf16 twins of k_pointwise_bf16.hip)
held to EXACT bytes at their store edges, on the grid of tests/pointwise_edge_cases.py: widths around both narrow limits and around zero, one and
two full 256-pixel groups, heights around 1, 2 and 4 rows per wave and the 4, 8 and 16 rows of a workgroup, six source depths 0, 1, 3 and 5 bytes
(or one element) into an aligned allocation, dense and pitched, into fp32, fp16 and bf16 planar tensors, dense packed pixels, one pitched image
0 to 12 bytes behind an aligned address with 0 to 20 bytes of patterned row padding, and separate pitched planes; 1 to 65 planes (descriptors in
the kernel arguments and in the uploaded table) with `used` below the count; the named near-misses of the narrow dense path; three one-channel
planes that run two rows per thread and one just below that limit.

Every case runs on the default flags and under CHAIN_FORCE_GENERIC, and a case is accepted only if, in this order,
  1. the kernel is the one the case names (default) / an interpreted one (generic*),
  2. the output's bytes EQUAL the exact expectation (no tolerance),
  3. the default path's whole buffer equals the forced-generic path's whole buffer,
  4. the canary bands of DeviceBackend are intact and every PADDING byte of the output buffer still holds its fill: row padding, the bytes in front
     of the image, the space between separate planes, the tail of the allocation (the whole buffer is read back).
Cases of the shape the pointwise tick takes (u8 planes, an fp32 planar or dense packed tensor, descriptors in the kernel arguments) also go
through cvgs_execute_many as three chains of the case, each of which must leave the single launch's bytes in its whole buffer.

One test item with one pytest subtest per family (source depth x store), as tests/test_gpu_warp_edges.py does, each naming every failing case.
Only a mismatch (AssertionError) lets a subtest go on to its next case and the item to its next subtest; whatever else ends a case -- an error the
library returns at launch, a HIP error at the synchronisation -- ends the item: nothing more is started on a card that may have faulted.

Exact cases have no figure: they are equal or they fail.  No case needed a change to k_pointwise_body.hpp or k_pointwise.hip.  The 404 cases (two
runs each, 40 of them a three-chain tick as well) take 1.4 s on an MI355X, the module 4.0 s with its imports."""
import time

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import model_cases as MC
from tests import pointwise_edge_cases as P
from tests.test_pointwise_edge_cases import bits

pytestmark = pytest.mark.gpu

PATHS = (("default", capi.CHAIN_DEFAULT), ("generic", capi.CHAIN_FORCE_GENERIC))


def _run(c, flags):
    """one run of a case on the GPU: (kernel name, backend, the whole output buffer's bytes)"""
    import torch
    B = MC.DeviceBackend()
    iops, _ = c.build(B)
    name = cvgs.kernel_name(*iops, flags=flags)
    cvgs.executeOperations(torch.cuda.current_stream(), *iops, flags=flags)
    torch.cuda.synchronize()
    whole = np.array(B.result(), copy=True).reshape(-1)  # (B.result() asserts the canary bands)
    return name, B, whole


def _tick(c, single):
    """three chains of the case in one cvgs_execute_many: each buffer must hold the single launch's bytes"""
    import torch
    backends = [MC.DeviceBackend() for _ in range(3)]
    chains = [c.build(B)[0] for B in backends]
    held = cvgs.executeMany(torch.cuda.current_stream(), chains)
    torch.cuda.synchronize()
    del held
    for k, B in enumerate(backends):
        whole = np.array(B.result(), copy=True).reshape(-1)
        assert B.placed[0].origin == backends[0].placed[0].origin
        assert np.array_equal(whole, single), "tick, chain %d: %d bytes differ from the single launch, first at byte %d (the samples start at %d)" % (
            k, int((whole != single).sum()), int(np.argmax(whole != single)), B.placed[0].origin)


def _hold(c):
    """every acceptance condition of the module docstring on one case"""
    first = None
    for what, flags in PATHS:
        name, B, whole = _run(c, flags)
        assert (name == c.kernel) if what == "default" else name.startswith("generic"), "%s: runs on %s, not on %s" % (what, name, c.kernel if what == "default" else "generic*")
        got, moved = P.split_whole(B.placed, whole, c.write, c.n, c.cn)
        want = c.expected(B)
        assert want.shape == got.shape and want.dtype == got.dtype
        bad = bits(want) != bits(got)
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        assert not bad.any(), "%s (%s): %d of %d elements differ from the exact expectation, first at %r (%s order): %r, expected %r; store path %r" % (
            what, name, int(bad.sum()), bad.size, at, c.write, got[at], want[at], sorted(P.store_path(c).branches))
        if first is None:
            first = whole
        else:
            assert np.array_equal(first, whole), "%s (%s): %d bytes differ from the default path" % (what, name, int((first != whole).sum()))
        assert moved.size == 0, "%s (%s): %d padding bytes of the output buffer changed, first at byte %d (the samples start at %d, pitch %d, row %d); store path %r" % (
            what, name, moved.size, int(moved[0]), B.placed[0].origin, B.placed[0].pitch, B.placed[0].row_bytes, sorted(P.store_path(c).branches))
    if P.takes_tick(c):
        _tick(c, first)


def _hold_all(cases, label):
    """Every case runs, also behind a mismatch; the test fails with the description of every case that did.  Anything but a mismatch -- an error
    returned at launch included -- is not caught here and ends the item (guarded)."""
    failed, t0 = [], time.perf_counter()
    for c in cases:
        try:
            _hold(c)
        except AssertionError as e:
            failed.append("%s: %s" % (c.name, str(e)[:400]))
    print("SECONDS gpu %-10s %-10s %.2f" % (label, "%d cases" % len(cases), time.perf_counter() - t0))
    assert not failed, "%d of %d cases, the first: %s\n%s" % (len(failed), len(cases), failed[0].split(":")[0], "\n".join(failed))


def test_pointwise_kernels_at_store_edges(device, subtests):
    """one subtest per source depth and store"""
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

    assert len(P.FAMILIES) == 8
    for family in P.FAMILIES:
        with subtests.test(family=family):
            cases = P.cases_of(family)
            assert len(cases) >= 38
            guarded(lambda: _hold_all(cases, family))
