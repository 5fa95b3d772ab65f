"""The two GPU test items of the CircularTensor update's refusal table and of the ring model's cases beside the push launch's 64 copy jobs:
every handle of tests/test_gpu_circular_refusals.py and every case of tests/circular_cases.py's BESIDE_THE_JOB_LIMIT as a subtest.  The
module sorts behind tests/test_zz_gpu_nv12_write.py, so the items are the last ones collected and every existing item keeps its place
(tests/test_gpu_area.py says why)."""
import pytest

from tests import test_gpu_circular_model as M
from tests import test_gpu_circular_refusals as R

pytestmark = pytest.mark.gpu


def test_refused_circular_updates_say_why_and_leave_the_handle_alone(device, lib, subtests):
    R.run_all(device, lib, subtests)


def test_ring_cases_beside_the_push_job_limit_within_the_model(device, subtests):
    M.run_cases_beside_the_job_limit(device, subtests)
