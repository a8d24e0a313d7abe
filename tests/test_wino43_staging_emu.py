"""Staging schedule of the Winograd F(4,3) K loop (sgmse_amd/csrc/kernels_conv_wino43.h) on the CPU workgroup emulator."""
import pytest

import wino43_staging_checks as C


@pytest.mark.parametrize("args,kw", C.CASES, ids=[C.case_id(a, k) for a, k in C.CASES])
def test_wino43_staging_schedule_keeps_the_result(emu, args, kw):
    """1 .. 5 K-stages, guards and halo, the source switch at and inside the look-ahead, raw producer without residual, two utterances
    of different range: the per-op gate and the 4-row shape bit-equal to the 8-row shape."""
    C.check_case(emu, args, kw)


@pytest.mark.parametrize("c,y,x", C.ONE_HOT)
def test_wino43_staging_one_hot_input_lands_where_it_belongs(emu, c, y, x):
    C.check_one_hot(emu, c, y, x)
