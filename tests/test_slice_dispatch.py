"""The nine <FIX, GATE> instantiations of the slicing kernels through the one dispatch, without a GPU: the product sources
under the CPU emulation against the composed numpy definitions (tests/dispatch_common.py)."""
import dispatch_common as dc


def test_slicer_block_nine_ways(emu_lib):
    dc.check_slicer_block(emu_lib)


def test_production_path_nine_ways(emu_lib):
    dc.check_production_path(emu_lib)
