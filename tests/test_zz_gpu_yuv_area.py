"""The one GPU test item of the INTER_AREA read of 4:2:0 decoder surfaces (CVGS_READ_NV12_RESIZE_AREA): every case of
tests/test_gpu_yuv_area.py (tests/test_gpu_area.py says why the item lives in a test_zz_* module, behind every other module of the suite)
as a subtest, bit-exact against the fp32 restatement of tests/yuv_area_model.py."""
import pytest

from tests import test_gpu_yuv_area as Y

pytestmark = pytest.mark.gpu


def test_yuv_area_kernels_equal_the_fp32_restatement_bit_for_bit(device, lib, subtests):
    Y.run_all(device, lib, subtests)
