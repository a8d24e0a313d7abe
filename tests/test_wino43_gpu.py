"""Winograd F(4,3) x fp16x2 (sgmse_amd/csrc/kernels_conv_wino43.h) on the hardware."""
import pytest

import wino43_checks as K

pytestmark = pytest.mark.gpu

# e_F43 <= SLACK x e_fp32MFMA, both against an fp64 convolution of the same operands.  F(2,3)'s slack of 2 does not fit by construction
# (the arithmetic model of F(4,3) predicts ~2x torch fp32).  Source of the number: the ratio was measured on the nine shapes below on an
# MI355X before the bound was set (profiles/r07_wino43_accuracy.txt: 0.67 ... 1.79, worst 1.786 at 48->128 @2x8x32 with inputs x 50);
# SLACK = worst measured ratio x 1.5 (room for another accumulation order on other inputs) = 2.68.  The hard gate is OP_TOL (1e-5).
SLACK = 2.68

SHAPES = [
    ((1, 32, 128, 9, 36), {}),
    ((2, 48, 128, 8, 32), dict(xmul=50.0)),
    ((1, 64, 256, 5, 40), dict(dual=32)),
    ((1, 16, 128, 12, 64), dict(xform=False, res=False)),
    ((1, 32, 128, 8, 32), dict(wmul=6)),
    ((2, 128, 128, 64, 96), {}),
    ((1, 384, 128, 32, 64), dict(dual=128)),
    ((1, 512, 256, 16, 32), dict(dual=256)),
    ((2, 256, 256, 64, 128), dict(wmul=4)),
]


def test_conv3x3_winograd_f43_kernel_has_fp32_accuracy(hip):
    """The emulator file's shapes and the shapes of test_conv3x3_winograd_fp16x2_kernel_has_fp32_accuracy whose width is a multiple
    of 4: per-op gate against torch fp32 (weights over decades: worst channel against fp64), 4-row shape bit-equal to the 8-row shape,
    error against fp64 within SLACK x the fp32-MFMA kernel's; the F(2,3) and fp32-MFMA kernels' errors are printed beside it."""
    for args, kw in SHAPES:
        K.check_conv_wino43(hip, *args, slack=SLACK, **kw)


def test_winograd_f43_block_end_with_unfolded_shortcut(hip):
    K.check_wino43_block_end_with_shortcut(hip, 1, 32, 64, 128, 9, 36)
    K.check_wino43_block_end_with_shortcut(hip, 2, 128, 256, 128, 64, 128)
