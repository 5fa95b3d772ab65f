"""The one GPU test item of the INTER_AREA read kind: every case of tests/test_gpu_area.py (which says why the item lives here, behind every
other module of the suite) as a subtest, bit-exact against the fp32 restatement of tests/area_model.py."""
import pytest

from tests import test_gpu_area as A

pytestmark = pytest.mark.gpu


def test_area_kernels_equal_the_fp32_restatement_bit_for_bit(device, lib, subtests):
    A.run_all(device, lib, subtests)
