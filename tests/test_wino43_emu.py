"""Winograd F(4,3) x fp16x2 (sgmse_amd/csrc/kernels_conv_wino43.h) on the CPU workgroup emulator: the kernel's indexing and arithmetic
on shapes chosen for its geometry (column quads, 4-row position fragments)."""
import wino43_checks as K


def test_conv3x3_winograd_f43_kernel_has_fp32_accuracy(emu):
    """Widths that are not multiples of 32 (36, 40), heights that are not multiples of 8 or 4 (5, 9, 12), two sources, raw input
    without residual, inputs x 50 with one utterance x 0.01, weights over six decades with outliers; the 4-row shape bit-equal."""
    K.check_conv_wino43(emu, 1, 32, 128, 9, 36, beside=False)
    K.check_conv_wino43(emu, 2, 48, 128, 8, 32, xmul=50.0, beside=False)
    K.check_conv_wino43(emu, 1, 64, 256, 5, 40, dual=32, beside=False)
    K.check_conv_wino43(emu, 1, 16, 128, 12, 64, xform=False, res=False, beside=False)
    K.check_conv_wino43(emu, 1, 32, 128, 8, 32, wmul=6, beside=False)


def test_winograd_f43_block_end_with_unfolded_shortcut(emu):
    K.check_wino43_block_end_with_shortcut(emu, 1, 32, 64, 128, 9, 36)
