"""Raw-input instantiation of the split 1x1 kernel (conv1x1_split_kernel<S, XF = 0>, sgmse_amd/csrc/kernels_conv_split.h) on the CPU
workgroup emulator: its 16-byte staging on the shapes at which the item geometry can go wrong.  (Ragged launches of this kernel need
the full-width network: test_ragged_batch_full_width here under SGMSE_SLOW=1, tests/test_conv1x1_raw_gpu.py on the hardware.)"""
import pytest

import conv1x1_raw_checks as K

# B, C1, C2, Cout, H, W
SHAPES = [
    (2, 16, 16, 128, 12, 40),     # partial tile in both directions, a tile column 8 wide, two sources, two stages with clamped look-ahead
    (1, 48, 0, 128, 8, 32),       # odd stage count
    (1, 32, 0, 256, 4, 36),       # two output blocks, fewer rows than a tile
    (1, 32, 0, 128, 8, 34),       # width not a multiple of 4: the 4-byte staging, same bits
]


@pytest.mark.parametrize("split", ["fp16x2", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_raw_input_equals_the_identity_producer(emu, shape, split):
    K.check_raw_against_identity_producer(emu, *shape, split=split)


def test_conv1x1_raw_input_unaligned_sources_take_the_4_byte_staging(emu):
    K.check_raw_against_identity_producer(emu, 2, 16, 16, 128, 12, 40, unaligned=True)
