"""The one GPU test item of tests/nv12_write_edge_cases.py: every case as a subtest -- windows, every read layout, the store's conversion edge,
targets inside a larger surface, the other sources, a mixed tick -- the stored bytes bit-exact against the fp32 restatement of
tests/nv12_write_model.py.  The module sorts behind tests/test_zz_gpu_tick_routes.py, so the item is the last one collected and every
existing item keeps its place."""
import pytest

from tests import nv12_write_edge_cases as E

pytestmark = pytest.mark.gpu


def test_nv12_write_kernels_on_every_read_window_and_placement(device, lib, oracle, subtests):
    E.run_all(device, lib, oracle, subtests)
