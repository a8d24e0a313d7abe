"""Checks of the K-loop staging schedule of the Winograd F(4,3) kernel (sgmse_amd/csrc/kernels_conv_wino43.h: the next stage's item cut
into units between the MFMAs of STG taps), shared by the emulator and the GPU test modules.  The schedule moves WHEN an element of the
item is produced, transformed, split and stored, never what is computed: the shapes are the smallest at which a unit in the wrong stage,
tap slot or k-group, a raw load issued too early or a store behind the stage barrier would show.

As a script -- python tests/wino43_staging_checks.py TREE_OR_LIBRARY [cuda|cpu] -- it prints one sha256 per case of the output that the
library of that tree computes (TREE/sgmse_amd/libsgmse_hip.so, or TREE/tests/emu/libsgmse_emu.so for cpu; a path ending in .so is taken
as the library itself).  Two builds that differ only in the schedule print the same listing on the same device."""
import hashlib
import math
import os
import sys

import torch
import torch.nn.functional as F

import wino43_checks as K
from conftest import rel_l2
from parity import OP_TOL

# (B, Cin, Cout, H, W), keywords of wino43_checks.check_conv_wino43
STAGE_COUNTS = [((1, ci, 128, 8, 32), {}) for ci in (16, 32, 48, 64, 80)]      # 1 .. 5 K-stages: nothing staged in the loop, no
#                                                                               look-ahead load, the first one, steady state, odd count
GUARDS = [((1, 48, 128, 12, 36), {}),                 # partial 8-row tile, second column tile mostly outside the image
          ((1, 32, 128, 5, 40), {})]
SOURCE_SWITCH = [((1, 48, 128, 8, 32), dict(dual=16)),      # second source from stage 2 on: the switch inside the look-ahead load
                 ((1, 64, 128, 8, 32), dict(dual=32))]      # ... at a stage boundary two stages ahead
RAW = [((1, 32, 128, 8, 32), dict(xform=False, res=False))]
RANGES = [((2, 48, 128, 8, 32), dict(xmul=50.0))]
CASES = STAGE_COUNTS + GUARDS + SOURCE_SWITCH + RAW + RANGES

ONE_HOT = [(0, 0, 0), (17, 3, 13), (34, 7, 31), (51, 4, 16), (63, 2, 3)]      # (channel, row, column) of the only non-zero input
RACE = (2, 80, 128, 16, 64)


def case_id(args, kw):
    return "%dx%d->%d@%dx%d" % args + "".join(f",{k}={v}" for k, v in kw.items())


def check_case(dev, args, kw, slack=None):
    K.check_conv_wino43(dev, *args, slack=slack, beside=False, **kw)


def _one_hot_operands(c, y, x):
    g = torch.Generator().manual_seed(4300 + c)
    w = torch.randn(128, 64, 3, 3, generator=g) / math.sqrt(64 * 9)
    inp = torch.zeros(1, 64, 8, 32)
    inp[0, c, y, x] = 1.5
    return inp, w


def one_hot_outputs(dev, c, y, x):
    from sgmse_amd import ops
    inp, w = _one_hot_operands(c, y, x)
    return [ops.conv2d(inp.to(dev), w.to(dev), None, force_split=f).cpu() for f in ("wino43", "wino43_4")]


def check_one_hot(dev, c, y, x):
    """Raw producer, no bias, no residual, one non-zero input: the output is the weights of channel c around (y, x) within the per-op
    gate and EXACTLY zero wherever the input cannot reach -- a unit written to the wrong stage, slot or k-group puts mass elsewhere.
    What the input can reach: rows y - 1 .. y + 1 (rows are not transformed), and in them the column quads 4 m .. 4 m + 3 whose input
    window 4 m - 1 .. 4 m + 4 holds x.  Inside such a quad, farther than one pixel from x, F(4,3) leaves the rounding of a sum that
    cancels only in exact arithmetic (y = M0 + M1 + ... of separately rounded transformed weights; 1.1e-8 here, on this kernel before
    and after the staging schedule changed), not a zero: there the bound is the per-op gate on the largest output."""
    inp, w = _one_hot_operands(c, y, x)
    out8, out4 = one_hot_outputs(dev, c, y, x)
    ref = F.conv2d(inp, w, padding=1)
    e = rel_l2(out8, ref)
    print(f"conv_wino43 one-hot channel {c} at ({y}, {x}): rel. L2 vs torch fp32 {e:.2e}")
    assert torch.equal(out8, out4), "the 4-row and 8-row Winograd F(4,3) shapes differ"
    assert e < OP_TOL, (c, y, x, e)
    near = torch.zeros(8, 32, dtype=torch.bool)
    near[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    reach = torch.zeros(8, 32, dtype=torch.bool)
    for m in range(8):
        if 4 * m - 1 <= x <= 4 * m + 4:
            reach[max(y - 1, 0):y + 2, 4 * m:4 * m + 4] = True
    assert bool((near & ~reach).sum() == 0)
    o = out8[0]
    assert bool((o[:, ~reach] == 0).all()), (c, y, x, float(o[:, ~reach].abs().max()))
    residue = float(o[:, reach & ~near].abs().max()) if bool((reach & ~near).any()) else 0.0
    print(f"   largest output inside the reached quads, farther than one pixel: {residue:.2e} (largest output {float(ref.abs().max()):.2e})")
    assert residue <= OP_TOL * float(ref.abs().max()), (c, y, x, residue)


def race_output(dev):
    from sgmse_amd import ops
    B, Ci, Co, H, W = RACE
    _, x, w, b, r, sc, sh, _ = K._operands(B, Ci, Co, H, W, True, True, 1.0, None, 7)
    mv = lambda t: t.to(dev)
    return ops.conv2d(mv(x), mv(w), mv(b), residual=mv(r), out_scale=1 / math.sqrt(2.0), in_scale=mv(sc), in_shift=mv(sh), in_act=True,
                      force_split="wino43").cpu()


def case_output(dev, args, kw):
    """The 8-row launch of check_conv_wino43 on the same operands (for the digest listing)."""
    from sgmse_amd import ops
    B, Ci, Co, H, W = args
    dual, xform, res = kw.get("dual", 0), kw.get("xform", True), kw.get("res", True)
    _, x, w, b, r, sc, sh, _ = K._operands(B, Ci, Co, H, W, xform, res, kw.get("xmul", 1.0), None, 7)
    x1, x2 = (x[:, :Ci - dual].contiguous(), x[:, Ci - dual:].contiguous()) if dual else (x, None)
    mv = lambda t: None if t is None else t.to(dev)
    return ops.conv2d(mv(x1), mv(w), mv(b), residual=mv(r), out_scale=1 / math.sqrt(2.0), x2=mv(x2), in_scale=mv(sc), in_shift=mv(sh),
                      in_act=xform, force_split="wino43").cpu()


def digests(dev):
    sha = lambda t: hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()
    for args, kw in CASES:
        yield case_id(args, kw), sha(case_output(dev, args, kw))
    for c, y, x in ONE_HOT:
        yield f"one-hot c={c} ({y},{x})", sha(one_hot_outputs(dev, c, y, x)[0])
    yield "race " + case_id(RACE, {}), sha(race_output(dev))


if __name__ == "__main__":
    target = os.path.abspath(sys.argv[1])
    device = sys.argv[2] if len(sys.argv) > 2 else "cuda"
    if target.endswith(".so"):
        library = target
    else:
        library = os.path.join(target, "sgmse_amd", "libsgmse_hip.so") if device == "cuda" else os.path.join(target, "tests", "emu", "libsgmse_emu.so")
    from sgmse_amd import _lib
    _lib.load_library(library)
    for name, digest in digests(device):
        print(f"{digest}  {name}")
