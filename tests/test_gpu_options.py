"""The four opt-in decode options reach the context that does the work behind every handle kind, on the device
(tests/options_common.py)."""
import pytest

import options_common as oc

pytestmark = pytest.mark.gpu


def test_options_reach_every_handle(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"

    def to_device(f32):
        t = torch.from_numpy(f32).to("cuda:0")
        torch.cuda.synchronize()
        return t.data_ptr(), t

    oc.check_options_reach_every_handle(hip_lib, to_device)
