"""Checks of how the K loop of the Winograd F(4,3) kernel feeds its MFMAs (sgmse_amd/csrc/kernels_conv_wino43.h, SGMSE_WINO43_FEED: B
fragments read from LDS one fragment slot ahead, across taps; the weight ring loaded through a raw buffer view with the (stage, dy, k)
offset in a scalar register; the ring's first taps loaded in the prologue), shared by the emulator and the GPU test modules.  None of it
changes a value or an address, only when a read is issued and from which registers an address is formed: the shapes are the smallest at
which a fragment read from the wrong buffer or slot, a weight offset that drops a term, or a read that passes a barrier would show.

Every case runs wino43_checks.check_conv_wino43 (per-op gate against torch fp32, 4-row shape bit-equal to the 8-row shape) and gates the
error against the fp64 convolution it returns with the same OP_TOL."""
import math

import torch
import torch.nn.functional as F

import wino43_checks as K
import wino43_staging_checks as S
from conftest import rel_l2
from parity import OP_TOL

# (B, Cin, Cout, H, W), keywords of wino43_checks.check_conv_wino43
LOOK_AHEAD = [((1, ci, 128, 8, 32), {}) for ci in (16, 32, 48)]     # 1, 2, 3 K-stages: nothing to read ahead behind the only stage, the
#                                                                     first read across a stage barrier, steady state with the raw look-ahead
WEIGHT_OFFSETS = [((1, 512, 256, 8, 32), {}),                       # the largest stage count and weight offset of the network
                  ((1, 64, 128, 8, 32), dict(dual=32))]             # two sources
TWO_CO_BLOCKS = (1, 32, 256, 8, 32)                                 # (check_co_blocks: each block against the reference on its own)
WAITS = [((1, ci, 128, 8, 32), dict(xform=True, res=True)) for ci in (48, 64, 80)]      # fused producer + residual, 3 .. 5 K-stages
GUARDS = [((1, 48, 128, 12, 36), {})]                               # partly empty tiles: the look-ahead read of rows outside the image
CASES = LOOK_AHEAD + WEIGHT_OFFSETS + WAITS + GUARDS
RACE_RUNS = 5

case_id = S.case_id


def check_case(dev, args, kw):
    e_43 = K.check_conv_wino43(dev, *args, beside=False, **kw)[0]
    assert e_43 < OP_TOL, (args, kw, e_43)


def check_co_blocks(dev):
    """Two blocks of 128 output channels: the second block's weights lie one whole block (Cin / 16 stages) behind the first's.  Each
    block's output against the fp64 convolution within the per-op gate (a block computed from the other's weights is off by ~1), the
    4-row shape bit-equal."""
    from sgmse_amd import ops
    B, Ci, Co, H, W = TWO_CO_BLOCKS
    _, x, w, b, r, sc, sh, xin = K._operands(B, Ci, Co, H, W, True, True, 1.0, None, 7)
    ref64 = (F.conv2d(xin.double(), w.double(), b.double(), padding=1) + r.double()) / math.sqrt(2.0)
    mv = lambda t: t.to(dev)
    run = lambda f: ops.conv2d(mv(x), mv(w), mv(b), residual=mv(r), out_scale=1 / math.sqrt(2.0), in_scale=mv(sc), in_shift=mv(sh),
                               in_act=True, force_split=f).cpu()
    out8, out4 = run("wino43"), run("wino43_4")
    assert torch.equal(out8, out4), "the 4-row and 8-row Winograd F(4,3) shapes differ"
    for blk in range(Co // 128):
        ch = slice(128 * blk, 128 * (blk + 1))
        e = rel_l2(out8[:, ch].double(), ref64[:, ch])
        print(f"conv_wino43 {Ci}->{Co} @{B}x{H}x{W}: output channels {ch.start}..{ch.stop - 1}, error vs fp64 {e:.2e}")
        assert e < OP_TOL, (blk, e)


def check_race(dev):
    """The race shape of the staging checks (five K-stages, two utterances, 16 workgroups), launched five times: a fragment read that
    could pass the stage barrier, or a ring load consumed before it arrived, would make the outputs differ."""
    first = S.race_output(dev)
    for i in range(1, RACE_RUNS):
        assert torch.equal(first, S.race_output(dev)), f"launch {i} differs from launch 0"
