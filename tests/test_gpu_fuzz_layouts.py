"""Seeded differential fuzzing of what tests/test_gpu_fuzz.py never draws: packed 4:2:2 and planar 4:4:4 reads, CV_16BF as the stored and
as the source type (generator: tests/fuzz_layout_cases.py, pinned on the CPU by tests/test_fuzz_layout_cases.py).  Every chain runs on the
GPU and is compared bit for bit with its exact expected value -- the oracle's, composed from two oracle runs for 4:2:2 / 4:4:4, the
oracle's fp32 twin rounded on the host for a CV_16BF store.  Every chain the generator spells is served: a refusal is a failure."""
import os

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import fuzz_layout_cases as G
from tests import helpers as H

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes of canary on both sides of every output buffer


def _on_gpu(c, flags, fill):
    """The chain of case `c` on the GPU.  4:2:2 / 4:4:4 sources: every byte that is no sample (row padding, the gaps between the planes,
    the guard bands) holds the `fill`-th pattern.  The output sits between canary bands that must come back untouched."""
    import torch
    outs = []

    def wrap_surface(src):
        if src.kind in ("yuv422", "yuv444"):
            src.fill_rest(G.rest_pattern(src.buf.size, fill))
        a = src.host(True)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        return src.mat(t.data_ptr(), t, True)

    def wrap_out(a, cvt):
        big = torch.full((a.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        big[GUARD:GUARD + a.nbytes].zero_()
        outs.append((big, a))
        return cvgs.GpuMat(a.shape[0], a.shape[1], cvt, big.data_ptr() + GUARD, a.strides[0], owner=big)

    ops = c.build(wrap_surface, wrap_out, c.out_array(True), True)
    cvgs.executeOperations(torch.cuda.current_stream(), *ops, flags=flags)
    torch.cuda.synchronize()
    big, a = outs[0]
    g = big.cpu().numpy()
    assert (g[:GUARD] == 0xA5).all() and (g[-GUARD:] == 0xA5).all(), "store outside the output: " + c.what
    return g[GUARD:-GUARD].view(a.dtype).reshape(a.shape)


def _nan(a, c):
    if c.bf16_store:
        return ((a & 0x7F80) == 0x7F80) & ((a & 0x7F) != 0)
    return np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)


def _run(seed, big, flags):
    c = G.case(seed, big=big)
    got = _on_gpu(c, flags, 0)
    gn, rn = _nan(got, c), _nan(c.ref, c)  # NaN payloads may differ; everything else must be the same bits
    assert np.array_equal(gn, rn), c.what
    H.assert_bit_exact(np.where(gn, 0, got).astype(got.dtype), np.where(rn, 0, c.ref).astype(got.dtype), c.what)
    if seed % 10 == 0 and c.read in ("yuv422", "yuv444"):  # other bytes around the samples: not one output bit may move
        again = _on_gpu(c, flags, 1)
        assert np.array_equal(again.view(np.uint8), got.view(np.uint8)), "the output depends on bytes that are no sample: " + c.what


def _run_seeds(seeds, big):
    """Every seed of a group runs, also behind a mismatch or a refusal (a GPU fault ends the group: nothing more is started on a faulted
    card); the group fails with the description of every seed that did."""
    failed = []
    for seed in seeds:
        try:
            _run(seed, big, 0 if big else G.FLAGS[seed % 4])
        except (AssertionError, capi.CvgsError) as e:
            failed.append("seed %d: %s" % (seed, str(e)[:400]))
    assert not failed, "%d of %d seeds:\n%s" % (len(failed), len(seeds), "\n".join(failed))


def _groups(base, n, size):
    """range(base, base + n) in groups of `size` seeds: one test per GROUP, so that the suite's list of tests stays short (a long hunt of
    20,000 seeds is 167 tests)"""
    return [range(a, min(a + size, base + n)) for a in range(base, base + n, size)]


def _id(seeds):
    return "seeds%d-%d" % (seeds[0], seeds[-1])


_BASE = int(os.environ.get("CVGS_FUZZ_LAYOUT_BASE", "0"))  # a long hunt in several runs: CVGS_FUZZ_LAYOUT_BASE=5000, 10000, ... with CVGS_FUZZ_LAYOUT_N=5000 each


@pytest.mark.parametrize("seeds", _groups(_BASE, int(os.environ.get("CVGS_FUZZ_LAYOUT_N", str(G.DEFAULT_N))), 120), ids=_id)
def test_random_layout_chain_matches_expectation(seeds):
    """flags by seed % 4: fast path, interpreted, fast path, no thread fusion"""
    _run_seeds(seeds, False)


@pytest.mark.parametrize("seeds", _groups(G.BIG_BASE, int(os.environ.get("CVGS_FUZZ_LAYOUT_BIG_N", str(G.DEFAULT_BIG_N))), 12), ids=_id)
def test_random_layout_chain_whole_frame_sizes(seeds):
    """frame sizes (four rows per wave, more than one block), the fast path only"""
    _run_seeds(seeds, True)
