"""The launch listing of tests/test_conv_routes_gpu.py on the CPU workgroup emulator: the routing is host code, the labels are the same."""
import os

import pytest

import conv_route_checks as K
from conftest import EMU_LIB


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="full-width network on the emulator (minutes); set SGMSE_SLOW=1")
def test_full_width_network_runs_on_the_recorded_kernel_families(emu):
    K.check_routes(emu, EMU_LIB)
