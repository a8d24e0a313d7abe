"""Checks of the raw-input instantiation of the split 1x1 kernel (conv1x1_split_kernel<S, XF = 0>, sgmse_amd/csrc/kernels_conv_split.h),
shared by the emulator and the GPU test modules.  A launch without a producer stages its input with no affine and no SiLU, and -- where
the width is a multiple of 4 and the sources are 16-byte aligned -- with 16-byte loads of aligned column quads.  Neither may change a
bit: the launch with a producer (XF = 1: 4-byte loads, affine, blend) given scale 1, shift 0 and no activation computes x * 1 + 0 = x."""
import math

import torch
import torch.nn.functional as F

from conftest import rel_l2
from parity import OP_TOL, R, gen

# e_split <= max(SLACK x e_fp32MFMA, 3e-7), both against an fp64 convolution of the same operands: the bounds the existing tests of this
# kernel apply (parity.check_conv_b3: 2.0 for bf16x3 by default, 3.0 for fp16x2 in test_conv1x1_fp16x2_kernel_scales_by_the_input_range)
SLACK = {"fp16x2": 3.0, "bf16x3": 2.0}
AMAX = 3.0


def _input(g, B, C, H, W):
    """Finite, both signs, no zeros (x * 1 + 0 would turn a -0 into +0), and max |x| = AMAX exactly in every utterance: the fp16x2 kernel
    scales by a power of two taken from a range bound, which is max |x| for a raw launch and max |x| * 1.0001 behind the identity producer
    (xform_bound_kernel) -- both in [2, 4), so both launches scale alike."""
    x = R(g, B, C, H, W).clamp(-AMAX, AMAX)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x)
    x[:, 0, 0, 0] = AMAX
    x[:, -1, -1, -1] = -AMAX
    assert bool((x != 0).all()) and bool(torch.isfinite(x).all()) and bool((x > 0).any()) and bool((x < 0).any())
    return x


def check_raw_against_identity_producer(dev, B, C1, C2, Co, H, W, split="fp16x2", unaligned=False):
    """Raw launch == launch with the identity producer, bit for bit; raw launch within the per-op gate and the kernel's fp64 bound.
    unaligned: the same operands from a source 4 bytes off a 16-byte boundary (4-byte staging) must give the aligned launch's bits."""
    from sgmse_amd import ops
    Ci = C1 + C2
    g = gen(B * 1000 + Ci + Co + H + W + 17)
    x = _input(g, B, Ci, H, W)
    w = R(g, Co, Ci, 1, 1) / math.sqrt(Ci); b = R(g, Co); r = R(g, B, Co, H, W)
    ref32 = (F.conv2d(x, w, b) + r) / math.sqrt(2.0)
    ref64 = (F.conv2d(x.double(), w.double(), b.double()) + r.double()) / math.sqrt(2.0)
    x1, x2 = (x[:, :C1].contiguous(), x[:, C1:].contiguous()) if C2 else (x, None)
    mv = lambda t: None if t is None else t.to(dev)
    kw = dict(residual=mv(r), out_scale=1 / math.sqrt(2.0), x2=mv(x2))
    raw = ops.conv2d(mv(x1), mv(w), mv(b), force_split=split, **kw).cpu()
    ident = ops.conv2d(mv(x1), mv(w), mv(b), force_split=split, in_scale=mv(torch.ones(B, Ci)), in_shift=mv(torch.zeros(B, Ci)),
                       in_act=False, **kw).cpu()
    out_f32 = ops.conv2d(mv(x1), mv(w), mv(b), **kw).cpu()
    e_raw, e_f32 = rel_l2(raw.double(), ref64), rel_l2(out_f32.double(), ref64)
    print(f"conv1x1 raw {split} {C1}+{C2}->{Co} @{B}x{H}x{W}: differing elements vs identity producer {int((raw != ident).sum())}, "
          f"error vs fp64 {e_raw:.2e}  fp32-MFMA {e_f32:.2e}  vs torch fp32 {rel_l2(raw, ref32):.2e}")
    assert torch.equal(raw, ident), "the raw-input launch and the identity-producer launch differ"
    assert rel_l2(raw, ref32) < OP_TOL, (B, C1, C2, Co, H, W, rel_l2(raw, ref32))
    assert e_raw < max(SLACK[split] * e_f32, 3e-7), (split, e_raw, e_f32)
    if unaligned:
        def off4(t):      # the same values, 4 bytes past a 16-byte boundary
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            return v
        kw_u = dict(kw, x2=None if x2 is None else off4(x2))
        raw_u = ops.conv2d(off4(x1), mv(w), mv(b), force_split=split, **kw_u).cpu()
        assert torch.equal(raw_u, raw), "unaligned sources (4-byte staging) and aligned sources (16-byte staging) differ"
