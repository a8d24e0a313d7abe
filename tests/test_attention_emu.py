"""The attention kernel against float64 at every width, tile edge and logit range (attention_checks.py) on the CPU workgroup emulator."""
import pytest

import attention_checks as A


@pytest.mark.parametrize("gain, mode", A.LOGITS)
@pytest.mark.parametrize("S", A.LENGTHS)
@pytest.mark.parametrize("C", A.WIDTHS)
def test_attention_has_fp32_accuracy_against_fp64(emu, C, S, gain, mode):
    A.check_attention_fp64(emu, C, S, gain, mode)


@pytest.mark.parametrize("S", [1, 33, 97])
@pytest.mark.parametrize("C", A.WIDTHS)
def test_zero_queries_give_the_mean_of_v(emu, C, S):
    A.check_attention_uniform(emu, C, S)


@pytest.mark.parametrize("S", [33, 160])
@pytest.mark.parametrize("C", A.WIDTHS)
def test_an_utterance_alone_has_the_bits_it_has_in_a_batch(emu, C, S):
    A.check_attention_batch_independence(emu, C, S)
