"""The one GPU test item of the NV12 / NV21 surface write (CVGS_WRITE_NV12): every case of tests/test_gpu_nv12_write.py as a subtest, the stored
bytes bit-exact against the fp32 restatement of tests/nv12_write_model.py.  The module sorts behind tests/test_zz_gpu_area.py, so the item is
the last one collected and every existing item keeps its place."""
import pytest

from tests import test_gpu_nv12_write as W

pytestmark = pytest.mark.gpu


def test_nv12_write_kernels_store_the_fp32_restatement_bit_for_bit(device, lib, oracle, subtests):
    W.run_all(device, lib, oracle, subtests)
