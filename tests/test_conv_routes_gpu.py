"""Every launch of the full-width network runs on the kernel family recorded before the routing moved into conv_route.h."""
import pytest

import conv_route_checks as K
from conftest import HIP_LIB

pytestmark = pytest.mark.gpu


def test_full_width_network_runs_on_the_recorded_kernel_families(hip):
    """fwd_nf128 at batch 1, default settings and SGMSE_WINO43=0: the launch labels of profile_forward, line for line."""
    K.check_routes(hip, HIP_LIB)
