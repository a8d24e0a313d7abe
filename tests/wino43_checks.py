"""Checks of the Winograd F(4,3) x fp16x2 3x3 kernel (sgmse_amd/csrc/kernels_conv_wino43.h), shared by the emulator and the GPU test
modules.  Modelled on parity.check_conv_wino; the operands are drawn the same way."""
import math

import torch
import torch.nn.functional as F

from conftest import rel_l2
from parity import OP_TOL, R, gen


def _operands(B, Ci, Co, H, W, xform, res, xmul, wmul, seed_add):
    g = gen(B * 1000 + Ci + Co + H + W + seed_add)
    x = R(g, B, Ci, H, W) * xmul; w = R(g, Co, Ci, 3, 3) / math.sqrt(Ci * 9); b = R(g, Co) * xmul
    r = R(g, B, Co, H, W) * xmul if res else None
    if wmul:
        w = w * torch.logspace(-wmul / 2, wmul / 2, Co)[:, None, None, None]
        w[1, 0, 1, 1] *= 1e6; w[Co // 2, Ci - 1, 0, 2] *= 1e4
    if xmul != 1.0 and B > 1:
        x[0] *= 0.01          # utterances of one batch with very different ranges: the scale is per utterance
    sc = sh = None
    xin = x
    if xform:
        sc, sh = R(g, B, Ci), R(g, B, Ci)
        xin = x * sc[:, :, None, None] + sh[:, :, None, None]
        xin = xin * torch.sigmoid(xin)
    return g, x, w, b, r, sc, sh, xin


def check_conv_wino43(dev, B, Ci, Co, H, W, dual=0, xform=True, res=True, xmul=1.0, wmul=None, slack=None, beside=True):
    """Per-op gate against the fp32 oracle (with `wmul`: the worst output channel against fp64), the 4-row workgroup shape equal to the
    8-row shape bit for bit, and -- where `slack` is given -- an error against an fp64 convolution within `slack` x the fp32-MFMA
    kernel's on the same operands.  beside=False (emulator): the F(2,3) and fp32-MFMA kernels, which only supply the printed
    figures and the `slack` bound, are not run.  Returns (e_F43, e_F23, e_fp32MFMA, e_torch_fp32), all against fp64."""
    from sgmse_amd import ops
    g, x, w, b, r, sc, sh, xin = _operands(B, Ci, Co, H, W, xform, res, xmul, wmul, 7)
    fin = lambda t: (t + (r.to(t.dtype) if res else 0)) / math.sqrt(2.0)
    ref32 = fin(F.conv2d(xin, w, b, padding=1))
    ref64 = fin(F.conv2d(xin.double(), w.double(), b.double(), padding=1))
    x1, x2 = (x[:, :Ci - dual].contiguous(), x[:, Ci - dual:].contiguous()) if dual else (x, None)
    mv = lambda t: None if t is None else t.to(dev)
    kw = dict(residual=mv(r), out_scale=1 / math.sqrt(2.0), x2=mv(x2), in_scale=mv(sc), in_shift=mv(sh), in_act=xform)
    out8 = ops.conv2d(mv(x1), mv(w), mv(b), force_split="wino43", **kw).cpu()
    out4 = ops.conv2d(mv(x1), mv(w), mv(b), force_split="wino43_4", **kw).cpu()
    e_43, e_t = rel_l2(out8.double(), ref64), rel_l2(ref32.double(), ref64)
    e_23 = e_f32 = float("nan")
    if beside or slack is not None:
        out23 = ops.conv2d(mv(x1), mv(w), mv(b), force_split="wino", **kw).cpu()
        out_f32 = ops.conv2d(mv(x1), mv(w), mv(b), **kw).cpu()
        e_23, e_f32 = rel_l2(out23.double(), ref64), rel_l2(out_f32.double(), ref64)
    print(f"conv_wino43 {Ci}->{Co} @{B}x{H}x{W}: error vs fp64  F(4,3)-fp16x2 {e_43:.2e}  F(2,3)-fp16x2 {e_23:.2e}  fp32-MFMA {e_f32:.2e}  "
          f"torch-fp32 {e_t:.2e}  ratio F(4,3)/fp32-MFMA {e_43 / e_f32:.2f}")
    assert torch.equal(out8, out4), "the 4-row and 8-row Winograd F(4,3) shapes differ"
    if wmul:
        num = (out8.double() - ref64).pow(2).sum(dim=(0, 2, 3)).sqrt(); den = ref64.pow(2).sum(dim=(0, 2, 3)).sqrt()
        worst = float((num / den).max())
        print(f"conv_wino43 {Ci}->{Co} @{B}x{H}x{W} weights over {wmul} decades: worst per-channel error vs fp64 {worst:.2e}")
        assert worst < OP_TOL, worst
    else:
        assert rel_l2(out8, ref32) < OP_TOL, (B, Ci, Co, H, W, dual, xform, rel_l2(out8, ref32))
    if slack is not None:
        assert e_43 < slack * e_f32, (e_43, e_f32, slack)
    return e_43, e_23, e_f32, e_t


def check_wino43_block_end_with_shortcut(dev, B, Ci, Cs, Co, H, W):
    """The end of a residual block whose shortcut is a 1x1 convolution, as the engine runs it on the F(4,3) levels: the shortcut is its
    own launch (fp16x2 1x1 kernel on the raw block input) and enters the F(4,3) launch as the residual.
    (Conv3x3(SiLU(GroupNorm-affine(h))) + Conv1x1(x)) / sqrt 2 against torch within the per-op gate."""
    from sgmse_amd import ops
    g, h, w, b, _, sc, sh, hin = _operands(B, Ci, Co, H, W, True, False, 1.0, None, 13)
    xs = R(g, B, Cs, H, W); w1 = R(g, Co, Cs, 1, 1) / math.sqrt(Cs); b1 = R(g, Co)
    ref = (F.conv2d(hin, w, b, padding=1) + F.conv2d(xs, w1, b1)) / math.sqrt(2.0)
    mv = lambda t: t.to(dev)
    short = ops.conv2d(mv(xs), mv(w1), mv(b1), force_split="fp16x2")
    out = ops.conv2d(mv(h), mv(w), mv(b), residual=short, out_scale=1 / math.sqrt(2.0), in_scale=mv(sc), in_shift=mv(sh), in_act=True,
                     force_split="wino43").cpu()
    e = rel_l2(out, ref)
    print(f"conv_wino43 {Ci}->{Co} @{B}x{H}x{W} + unfolded 1x1 shortcut({Cs}): rel. L2 vs torch fp32 {e:.2e}")
    assert e < OP_TOL, e
