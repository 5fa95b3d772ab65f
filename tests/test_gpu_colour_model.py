"""The standalone colour-conversion kernels of k_cvtcolor_u8.hip (k_u8_permute16, k_u8_gray16 with its `ORD == 0` form, k_f32_colour4) held
DIRECTLY to the independent float64 model (tests/f64_model.py) on the grid of tests/colour_cases.py: tile edges (the last lane at the end of a
1024-pixel tile, a whole tile followed by a partial one), pitched source views and pitched output views, batches, gray orders and alphas
cvGS::cvtColor cannot say, and the ineligible neighbours of the host predicate.

Every case runs three times -- the default path, CHAIN_NO_THREAD_FUSION and CHAIN_FORCE_GENERIC -- and a run is accepted only if
  * the kernel is the one the case names (a fast kernel only where the chain is eligible for it),
  * channel permutations equal the model bit for bit (CV_32F by bit pattern, NaN at the same positions), gray lies within Result.check's bound,
  * the three runs wrote the same bytes,
  * the canary bands of DeviceBackend are intact and every PADDING byte of the output buffer -- between the rows of a pitched view, before the
    view, behind the last row -- still holds its fill: the whole buffer is read back, not the view.
Every eligible case runs once more with the SOURCE padding refilled with another pattern: not one output byte may change.

One test item with one pytest subtest per depth and kernel template and one for the ineligible neighbours (as tests/test_gpu_k1_rows.py does),
each naming every failing case: a failing subtest is reported under its own name and the others still run.  The GPU suite's list of tests is
kept from growing (tests/test_gpu_fuzz_layouts.py groups its seeds for the same reason), so this module adds no item to it: its one item takes
the place of test_gpu_chains.py's unaligned-crop test, whose body runs here unchanged as the FIRST subtest, before anything of this module.
Only a mismatch (AssertionError) lets a subtest go on to its next case and the item to its next subtest; whatever else ends a case -- an error
the library returns at launch, a HIP error at the synchronisation -- ends the item: nothing more is started on a card that may have faulted.

Largest |kernel - model| / tolerance per family, measured on an MI355X (1 = at the bound; the same figure on all three paths, whose bytes are
the same): permutations 0.0000 at every depth (bit for bit), gray 0.5000 on CV_8U and CV_16U (the integer outputs' half step) and 0.6474 on
CV_32F, the ineligible neighbours 0.6263 -- the CPU oracle's figures of tests/test_colour_cases.py to four decimals.  No case needed a change to
k_cvtcolor_u8.hip; the out-of-range alphas of CV_8U did not agree between pointwise4_u8_u8 and the generic kernel and are the generic kernel's now
(tests/colour_cases.py).  The 207 cases (four runs each where eligible) take 0.6 s on an MI355X, the module 2.7 s with its imports."""
import time

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import helpers as H
from tests import model_cases as MC

pytestmark = pytest.mark.gpu


def _run(c, flags, fill=0):
    """one run of a case on the GPU: (kernel name, iops, views, the whole output buffer's bytes)"""
    import torch
    B = MC.DeviceBackend()
    iops, views = c.build(B, fill)
    name = cvgs.kernel_name(*iops, flags=flags)
    cvgs.executeOperations(torch.cuda.current_stream(), *iops, flags=flags)
    torch.cuda.synchronize()
    whole = np.array(B.result(), copy=True).reshape(-1)  # (B.result() asserts the canary bands)
    return name, iops, views, whole, B.placed


def _hold(c):
    """every acceptance condition of the module docstring on one case; returns the largest ratio against the model"""
    first, worst, res = None, 0.0, None
    for what, flags in K.FLAGS:
        name, iops, views, whole, placed = _run(c, flags)
        assert name == (c.kernel if what == "default" else c.generic), "%s: runs on %s" % (what, name)
        assert name.startswith(K.FAST_PREFIXES) == (what == "default" and c.reason is None), "%s: runs on %s" % (what, name)
        got, moved = K.split_output(placed, whole)
        assert moved.size == 0, "%s (%s): %d padding bytes of the output buffer changed, first at byte %d (the view starts at %d, pitch %d, row %d)" % (
            what, name, moved.size, int(moved[0]), placed.origin, placed.pitch, placed.row_bytes)
        if res is None:
            res = K.model_of(c, iops, views)
        ok, ratio, text = K.compare(c, res, got)
        assert ok, "%s (%s): %s" % (what, name, text)
        worst = max(worst, ratio)
        if first is None:
            first = whole
        else:
            assert np.array_equal(first, whole), "%s (%s): %d bytes differ from the default path" % (what, name, int((first != whole).sum()))
    if c.reason is None:
        name, _, _, whole, placed = _run(c, capi.CHAIN_DEFAULT, fill=1)
        p = placed.src_padding[0]
        assert (K.pattern_bytes(p.size, 1) != K.pattern_bytes(p.size, 0))[p].mean() > 0.9  # (the second pattern IS another one)
        assert np.array_equal(first, whole), "%s: %d output bytes depend on source padding" % (name, int((first != whole).sum()))
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
    print("RATIO gpu %-12s %-40s %-8s %.4f" % (label, "%d cases" % len(cases), "3 paths", worst))
    print("SECONDS gpu %-12s %.2f" % (label, time.perf_counter() - t0))
    assert not failed, "%d of %d cases:\n%s" % (len(failed), len(cases), "\n".join(failed))


def _unaligned_crop_stays_interpreted(oracle):
    """a CV_8UC3 crop that starts 9 bytes into a row stays on the interpreted kernel and gives the oracle's bytes (from tests/test_gpu_chains.py, unchanged)"""
    import torch
    dev = torch.device("cuda:0")
    frame = H.random_u8((64, 200, 3), seed=17)
    ft = torch.from_numpy(frame).to(dev)
    out_t = torch.zeros((32, 64, 3), dtype=torch.uint8, device=dev)
    ref = np.zeros((32, 64, 3), np.uint8)

    def chain(m, out):
        return [cvgs.ReadIOp(capi.READ_PIXEL, cvgs.CV_8UC3, [m.roi(3, 5, 64, 32)], 1), cvgs.cvtColor(cvgs.COLOR_BGR2RGB, cvgs.CV_8UC3), cvgs.write(cvgs.CV_8UC3, out)]

    g_ops = chain(cvgs.GpuMat.from_tensor(ft, cvgs.CV_8UC3), cvgs.GpuMat.from_tensor(out_t, cvgs.CV_8UC3))
    assert cvgs.kernel_name(*g_ops).startswith("pointwise4_u8_u8")  # the crop starts 9 bytes into a row: no 16-byte loads
    cvgs.executeOperations(torch.cuda.current_stream(), *g_ops)
    torch.cuda.synchronize()
    oracle.execute(cvgs.lower(chain(cvgs.GpuMat.from_array(frame, cvgs.CV_8UC3), cvgs.GpuMat.from_array(ref, cvgs.CV_8UC3))))
    H.assert_bit_exact(out_t.cpu().numpy(), ref, "unaligned crop")


def test_colour_kernels_within_the_model_bound(device, oracle, subtests):
    """one subtest for the unaligned crop, one per depth and kernel template, one for the ineligible neighbours"""
    groups = [(K.family_name(d, t), K.cases_of(d, t, True), K.FAST[(d, t)]) for d, t in K.FAMILIES]
    groups.append(("ineligible", [c for c in K.CASES.values() if c.reason is not None], None))
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

    with subtests.test(family="unaligned crop"):
        guarded(lambda: _unaligned_crop_stays_interpreted(oracle))
    for label, cases, kernel in groups:
        with subtests.test(family=label):
            assert len(cases) >= (18 if kernel else 60) and all(kernel is None or c.kernel == kernel for c in cases)
            guarded(lambda: _hold_all(cases, label))
