"""The gfx950 kernels held DIRECTLY to the independent float64 model (tests/f64_model.py), without the CPU oracle in between: the grid of
tests/model_cases.py on the fast path and on the interpreted path (capi.CHAIN_FORCE_GENERIC), every output between canary bands, every
element within the model's derived bound; one cvgs_execute_many tick of K1 and one of K4.

Largest |kernel - model| / tolerance per family, measured on an MI355X, fast and interpreted path alike: the oracle's figures of
tests/test_model_vs_oracle.py to four decimals (K1 0.34 - 0.47, YUV 0.75 - 0.80, warp 0.33, chains 0.60, stores 1.00 = one rounding of the
16-bit format); the execute_many ticks 0.21 (K1) and 0.62 (K4)."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import model_cases as MC

pytestmark = pytest.mark.gpu

_MODEL_CACHE = {}


def model_of(name, iops, views):
    """the model's answer for a case (the inputs are seeded: the same for both paths)"""
    if name not in _MODEL_CACHE:
        _MODEL_CACHE[name] = F.evaluate(iops, views)
    return _MODEL_CACHE[name]


def held_to_model(name, res, iops, got, what):
    ok, ratio = res.check(res.logical(MC.widen_output(got, iops[-1].dst_type), iops[-1].kind))
    print("RATIO gpu %-10s %-40s %-8s %.4f" % (MC.CASES[name][0], name, what, float(np.nanmax(ratio))))
    if res.excluded is not None:
        assert (res.excluded.reshape(res.excluded.shape[0], -1).mean(axis=1) <= 0.01).all()
    assert ok.all(), "%s (%s, %s): %d of %d elements outside the bound, worst ratio %.3f at %r" % (
        name, what, cvgs.kernel_name(*iops), int((~ok).sum()), ok.size, float(np.nanmax(ratio)),
        np.unravel_index(int(np.nanargmax(ratio)), ratio.shape))


@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_kernel_within_the_model_bound(device, name, path):
    import torch
    family, build, kernel = MC.CASES[name]
    flags = capi.CHAIN_FORCE_GENERIC if path == "generic" else capi.CHAIN_DEFAULT
    B = MC.DeviceBackend()
    iops, views = build(B)
    kname = cvgs.kernel_name(*iops, flags=flags)
    if path == "generic":
        assert kname.startswith("generic") or kname.endswith("_interp"), kname
    elif kernel is not None:
        assert kname.startswith(kernel), (name, kname)
    cvgs.executeOperations(torch.cuda.current_stream(), *iops, flags=flags)
    torch.cuda.synchronize()
    held_to_model(name, model_of(name, iops, views), iops, B.result(), path)


@pytest.mark.parametrize("names,kernel", [(["k1_8uc3_up", "k1_8uc3_down", "k1_8uc3_up"], "k1_u8c3_swap_mul_sub_div"),
                                          (["yuv_up_nv12", "yuv_up_nv21", "yuv_up_i420", "yuv_up_nv12"], "k4_nv12_resize_swap_mul_sub_div")])
def test_execute_many_tick_within_the_model_bound(device, names, kernel):
    """one cvgs_execute_many tick of same-shape chains (each over its own sources and output tensor)"""
    import torch
    built = []
    for name in names:
        B = MC.DeviceBackend()
        iops, views = MC.CASES[name][1](B)
        assert cvgs.kernel_name(*iops) == kernel, cvgs.kernel_name(*iops)
        built.append((name, B, iops, views))
    keep = cvgs.executeMany(torch.cuda.current_stream(), [iops for _, _, iops, _ in built])
    torch.cuda.synchronize()
    del keep
    for name, B, iops, views in built:
        held_to_model(name, model_of(name, iops, views), iops, B.result(), "tick")
