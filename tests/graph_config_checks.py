"""The network graphs sgmse_configure accepts, beyond the default ones of parity.NET_CASES: other level counts and channel multipliers,
block counts, attention resolutions, pyramids on and off, both variants -- what the engine's kernel routing, ragged tables, folded
shortcuts, pyramid branches and captured graph depend on.  The oracle (oracle/ncsnpp_oracle.py) restates the reference for every such
graph and is the reference here.  Shared by the emulator and the GPU module."""
import pytest
import torch

import parity
from conftest import rel_l2
from oracle import ncsnpp_oracle as NO
from oracle import synth

_n = lambda **kw: NO.NetCfg.for_variant("ncsnpp", nf=32, **kw)
_k = lambda **kw: NO.NetCfg.for_variant("ncsnpp_48k", nf=32, **kw)

# name -> (configuration, F); every input is F x 64 frames
CONFIGS = {
    "nf64": (NO.NetCfg.for_variant("ncsnpp", nf=64), 256),                       # 128-channel attention
    "nf96": (NO.NetCfg.for_variant("ncsnpp", nf=96), 256),                       # 192-channel attention, GroupNorm over 24 groups of 4 / 8
    "levels4_attn64": (_n(ch_mult=(1, 2, 2, 2), attn_resolutions=(64,)), 256),
    "levels4": (_n(ch_mult=(1, 2, 2, 2), attn_resolutions=()), 256),
    "blocks1": (_n(num_res_blocks=1), 256),
    "blocks3": (_n(num_res_blocks=3), 256),
    "no_output_pyramid": (_n(progressive="none"), 256),
    "no_input_pyramid": (_n(progressive_input="none"), 256),
    "attn32_16": (_n(attn_resolutions=(32, 16)), 256),
    "mult132_attn64": (_n(ch_mult=(1, 3, 2), attn_resolutions=(64,)), 256),     # a 96-channel level
    "mult1248_attn32": (_n(ch_mult=(1, 2, 4, 8), attn_resolutions=(32,)), 256),  # 32, 64, 128 and 256 channels in one graph
    "size128_levels6": (_n(image_size=128, ch_mult=(1, 1, 2, 2, 2, 2)), 128),
    "48k_attn16": (_k(attn_resolutions=(16,)), 256),
    "48k_blocks1_levels5": (_k(num_res_blocks=1, ch_mult=(1, 2, 2, 2, 2)), 192),
    # the graphs of the bitwise checks
    "levels4_attn64_blocks1": (_n(ch_mult=(1, 2, 2, 2), attn_resolutions=(64,), num_res_blocks=1), 256),
    "attn32_16_no_input_pyramid": (_n(attn_resolutions=(32, 16), progressive_input="none"), 256),
    "mult132_attn64_no_output_pyramid": (_n(ch_mult=(1, 3, 2), attn_resolutions=(64,), progressive="none"), 256),
    "48k_attn16_blocks3": (_k(attn_resolutions=(16,), num_res_blocks=3), 256),
}
FORWARD = tuple(CONFIGS)[:14]
FORWARD_SLOW_ON_EMULATOR = ("nf64", "nf96", "mult132_attn64", "mult1248_attn32")
BITWISE = tuple(CONFIGS)[14:]
SAMPLER_GRAPH = "levels4_attn64_blocks1"

# an attention block at a channel count the attention kernel has no instantiation for: refused when the engine is configured
REFUSED = {
    "attn_at_96_channels": NO.NetCfg(nf=32, ch_mult=(1, 3, 2), attn_resolutions=(128,)),
    "attn_at_160_channels": NO.NetCfg(nf=32, ch_mult=(1, 5, 2), attn_resolutions=(128,)),
}


def build(cfg, dev, P=None):
    """The module with its weights and its configured engine, as the first forward would create it."""
    net, P = parity.make_backbone(cfg, dev, P)
    net.engine(torch.device(dev))
    return net, P


def check_config_forward(dev, name):
    cfg, F_ = CONFIGS[name]
    net, P = build(cfg, dev)
    x = torch.randn(2, 2, F_, 64, dtype=torch.complex64, generator=parity.gen(11))
    t = torch.tensor([0.7, 0.2])
    with torch.no_grad():
        ref = NO.ncsnpp_forward(P, cfg, x, t)
    out = net(x.to(dev), t.to(dev))
    assert out.shape == ref.shape == (2, 1, F_, 64) and out.dtype == torch.complex64
    err = rel_l2(out.cpu(), ref)
    print(f"graph '{name}' on {dev}: rel_l2 vs the oracle = {err:.3e}")
    assert err < parity.NET_TOL, (name, err)


def check_config_bitwise(dev, name, frames=(128, 64)):
    """A ragged batch equals the single-utterance forwards, and a uniform batch of two equals its two singles, bit for bit."""
    cfg, F_ = CONFIGS[name]
    net, _ = build(cfg, dev)
    eng = net.engine(torch.device(dev))
    g = parity.gen(3)
    xs = [(torch.randn(2, F_, T, dtype=torch.complex64, generator=g) * 0.3).to(dev) for T in frames]
    t = torch.tensor([0.9, 0.4], device=dev)
    singles = [eng.forward(x[None], t[i:i + 1])[0] for i, x in enumerate(xs)]
    assert all(torch.isfinite(torch.view_as_real(s)).all() for s in singles)
    for a, b in zip(singles, eng.forward_ragged(xs, t)):
        assert a.shape == b.shape and torch.equal(a, b), name
    T = frames[-1]
    xb = torch.stack([xs[0][..., :T].contiguous(), xs[1]])
    both = eng.forward(xb, t)
    for i in range(2):
        assert torch.equal(eng.forward(xb[i:i + 1], t[i:i + 1])[0], both[i]), (name, i)


def check_config_sampler_graph(dev, name=SAMPLER_GRAPH):
    """The captured sampler step of a graph whose node count is not the default network's: equal to the eager step bit for bit."""
    cfg, F_ = CONFIGS[name]
    m, _ = parity.make_model(cfg, dev)
    y = synth.synth_spec(2, F_, 64, seed=4).to(dev)
    noise = parity.replay_noise(tuple(y.shape), 1 + 2 * 2).to(dev)
    run = lambda g: m.get_pc_sampler("reverse_diffusion", "ald", y, N=2, snr=0.5, noise=noise, use_graph=g)()
    (with_graph, nfe), (eager, nfe2) = run(True), run(False)
    assert nfe == nfe2 == 4 and torch.isfinite(torch.view_as_real(eager)).all()
    assert torch.equal(with_graph, eager)


def check_refused(dev, name):
    """Raised when the engine is configured -- where nf % 32 is refused -- with the level and its channel count in the message; not a
    RuntimeError out of the first forward, after the weights have been loaded."""
    with pytest.raises(ValueError, match=r"attention.*resolution 128.*(96|160) channels"):
        build(REFUSED[name], dev)


def check_same_graph_with_supported_attention_is_accepted(dev):
    """REFUSED's (1, 3, 2) graph with the attention at its 64-channel level instead still configures and takes its weights (its forward
    parity is the 'mult132_attn64' case of check_config_forward)."""
    net, P = build(CONFIGS["mult132_attn64"][0], dev)
    assert net.engine(torch.device(dev)).param_count() == sum(v.numel() for v in P.values())
