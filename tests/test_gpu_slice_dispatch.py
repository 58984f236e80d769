"""The nine <FIX, GATE> instantiations of the slicing kernels through the one dispatch, on the device: am_k_slice<FIX, GATE> behind
am_slicer_work and am_k_extract_slice_iq<2, FIX, GATE> behind am_process_iq, against the composed numpy definitions
(tests/dispatch_common.py)."""
import pytest

import dispatch_common as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return hip_lib


def test_slicer_block_nine_ways(lib):
    dc.check_slicer_block(lib)


def test_production_path_nine_ways(lib):
    dc.check_production_path(lib)
