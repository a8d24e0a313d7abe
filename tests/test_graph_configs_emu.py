"""Network graphs beyond the default ones (graph_config_checks.py) on the CPU workgroup emulator."""
import os

import pytest

import graph_config_checks as G

slow = pytest.mark.skipif(not os.environ.get("SGMSE_SLOW"), reason="more than 15 s of network evaluations on the emulator; set SGMSE_SLOW=1")


@pytest.mark.parametrize("name", [pytest.param(n, marks=[pytest.mark.slow, slow]) if n in G.FORWARD_SLOW_ON_EMULATOR else n for n in G.FORWARD])
def test_forward_matches_the_oracle(emu, name):
    G.check_config_forward(emu, name)


@pytest.mark.parametrize("name", [n if n == G.SAMPLER_GRAPH else pytest.param(n, marks=[pytest.mark.slow, slow]) for n in G.BITWISE])
def test_ragged_and_uniform_batches_equal_their_singles(emu, name):
    G.check_config_bitwise(emu, name)


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_attention_at_an_unsupported_width_is_refused_at_configuration(emu, name):
    G.check_refused(emu, name)


def test_same_graph_with_attention_at_a_supported_width_is_accepted(emu):
    G.check_same_graph_with_supported_attention_is_accepted(emu)
