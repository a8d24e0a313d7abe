"""Staging schedule of the Winograd F(4,3) K loop (sgmse_amd/csrc/kernels_conv_wino43.h) on the hardware."""
import pytest
import torch

import wino43_staging_checks as C
from test_wino43_gpu import SLACK      # value and derivation: tests/test_wino43_gpu.py

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("args,kw", C.CASES, ids=[C.case_id(a, k) for a, k in C.CASES])
def test_wino43_staging_schedule_keeps_the_result(hip, args, kw):
    """The emulator file's cases; on top of the per-op gate and the bit-equal 4-row shape, the error against fp64 within SLACK x the
    fp32-MFMA kernel's."""
    C.check_case(hip, args, kw, slack=SLACK)


@pytest.mark.parametrize("c,y,x", C.ONE_HOT)
def test_wino43_staging_one_hot_input_lands_where_it_belongs(hip, c, y, x):
    C.check_one_hot(hip, c, y, x)


def test_wino43_staging_is_free_of_races(hip):
    """Five K-stages, two utterances, 16 workgroups: a unit's LDS store that could pass the stage barrier, or a raw load that could
    overtake a unit reading the registers it fills, would make the three runs differ."""
    a, b, c = (C.race_output(hip) for _ in range(3))
    assert torch.equal(a, b) and torch.equal(a, c)
