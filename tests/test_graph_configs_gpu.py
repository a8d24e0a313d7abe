"""Network graphs beyond the default ones (graph_config_checks.py) on the hardware."""
import pytest

import graph_config_checks as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", G.FORWARD)
def test_forward_matches_the_oracle(hip, name):
    G.check_config_forward(hip, name)


@pytest.mark.parametrize("name", G.BITWISE)
def test_ragged_and_uniform_batches_equal_their_singles(hip, name):
    G.check_config_bitwise(hip, name)


def test_captured_sampler_step_equals_the_eager_step(hip):
    G.check_config_sampler_graph(hip)


@pytest.mark.parametrize("name", list(G.REFUSED))
def test_attention_at_an_unsupported_width_is_refused_at_configuration(hip, name):
    G.check_refused(hip, name)
