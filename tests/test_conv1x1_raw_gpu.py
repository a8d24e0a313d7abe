"""Raw-input instantiation of the split 1x1 kernel (conv1x1_split_kernel<S, XF = 0>, sgmse_amd/csrc/kernels_conv_split.h) on the hardware."""
import pytest

import conv1x1_raw_checks as K
import parity as P
from test_conv1x1_raw_emu import SHAPES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", ["fp16x2", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_raw_input_equals_the_identity_producer(hip, shape, split):
    K.check_raw_against_identity_producer(hip, *shape, split=split)


def test_conv1x1_raw_input_unaligned_sources_take_the_4_byte_staging(hip):
    K.check_raw_against_identity_producer(hip, 2, 16, 16, 128, 12, 40, unaligned=True)


def test_conv1x1_raw_input_ragged_batch_gives_single_run_bits(hip):
    """One batch of two utterances, 64 and 128 frames wide, through the full-width network (its residual shortcuts on the wide levels
    are this kernel's raw-input launches, 16-byte staging at widths 64 / 128 and 32 / 64): every utterance gets its single-run bits."""
    P.check_ragged_batch(hip, "fwd_nf128", frames=(64, 128), sampler=False, quick=True)
