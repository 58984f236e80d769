"""The four opt-in decode options behind the three handle kinds, without a GPU: the product sources under the CPU emulation
(tests/options_common.py)."""
import pytest

import options_common as oc


@pytest.mark.parametrize("option", sorted(oc.OPTIONS))
@pytest.mark.parametrize("prefix", sorted(oc.KINDS))
def test_option_surface(emu_lib, prefix, option):
    oc.check_surface(emu_lib, prefix, option)


def test_options_reach_every_handle(emu_lib):
    oc.check_options_reach_every_handle(emu_lib, lambda f32: (f32.ctypes.data, f32))
