"""Operand feed of the Winograd F(4,3) K loop (sgmse_amd/csrc/kernels_conv_wino43.h, SGMSE_WINO43_FEED) on the CPU workgroup emulator:
the waits are no-ops there, the order of the LDS reads and the weight offsets are what the kernel runs."""
import pytest

import wino43_feed_checks as C


@pytest.mark.parametrize("args,kw", C.CASES, ids=[C.case_id(a, k) for a, k in C.CASES])
def test_wino43_feed_keeps_the_result(emu, args, kw):
    C.check_case(emu, args, kw)


def test_wino43_feed_both_co_blocks(emu):
    C.check_co_blocks(emu)


def test_wino43_feed_repeated_launches_agree(emu):
    C.check_race(emu)
