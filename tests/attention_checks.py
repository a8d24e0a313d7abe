"""The attention kernel (attn_core_kernel, kernels_attn_misc.h) at every width it is instantiated for, at the sequence lengths where its
key tiles, its four waves and its masked keys change behaviour, and over the logit range, against a float64 softmax-attention.  Shared by
the emulator and the GPU module."""
import torch

from conftest import rel_l2
from parity import gen, R

WIDTHS = (32, 64, 128, 192, 256)
# S: one key; a short single tile; a second tile with ONE valid key; three tiles (wave 3 idle); four tiles, one key in the last;
# a second round for wave 0; five full tiles
LENGTHS = (1, 31, 33, 96, 97, 129, 160)
LOGITS = ((1, "iid"), (40, "iid"), (40, "ramp"))
FLOOR = 3e-7          # as check_conv_b3 / check_conv_wino: "fp32 accuracy against fp64" = within 2x torch's own fp32 error, floor 3e-7
SLACK = 2.0


def _attention(q, k, v):
    """softmax_r(q^T k / sqrt C) v in the dtype of the operands ([B,C,S] each)."""
    w = torch.softmax(torch.einsum("bcs,bcr->bsr", q, k) * q.shape[1] ** -0.5, -1)
    return torch.einsum("bsr,bcr->bcs", w, v)


def _worst_query(a, ref):
    """max over (b, query) of the relative L2 over channels."""
    num = (a - ref).pow(2).sum(1).sqrt()
    return float((num / ref.pow(2).sum(1).sqrt().clamp_min(1e-300)).max())


def make_qkv(C, S, gain, mode, B=2):
    qkv = R(gen(1000 * C + 10 * S + gain), B, 3 * C, S)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    q *= gain ** 0.5
    k *= gain ** 0.5
    if mode == "ramp":       # every query's running maximum rises in every key tile and the last tile dominates
        k *= torch.linspace(0.2, 2.0, S)
        q.abs_()
        k.abs_()
    else:
        assert mode == "iid", mode
    return qkv


def check_attention_fp64(dev, C, S, gain, mode):
    """Global and worst-query error of the kernel against float64, each within 2x torch's fp32 evaluation of the same expression.

    Measured (kernel error / torch-fp32 error, global and worst query, maxima over the cases with an error above the floor):
      emulator, torch-fp32 on the same host   global <= 1.00 at every width; worst query 1.15 (C = 32), 1.11 (64), 1.02 (128), 1.86 (192), 1.25 (256)
      MI355X, torch-fp32 on its host          global <= 1.00 at every width; worst query 1.01 (C = 32), 1.11 (64), 1.02 (128), 1.86 (192), 1.74 (256)
    The two worst: C = 192, S = 96, ramp (worst query 4.70e-5 against torch's 2.53e-5) and, on the GPU host, C = 256, S = 97, gain 40
    (1.34e-5 against 7.68e-6).  The kernel's error on the hardware is the emulator's to three digits; torch's own fp32 error depends on
    the host: a BLAS that sums the 256 channels of q.k in blocks (the GPU host's) lands at 0.31 .. 0.74 of one that sums them
    sequentially, at K = 256 only.  Against that yardstick a kernel with ONE sequential 256-term chain per score stood at up to 3.25 / 2.86
    (nine C = 256 cases above 2 on the first hardware run), which is why the kernel sums the score per 64-channel chunk pair."""
    from sgmse_amd import ops
    qkv = make_qkv(C, S, gain, mode)
    out = ops.attention(qkv.to(dev)).cpu()
    assert out.shape == (2, C, S) and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    ref64 = _attention(q.double(), k.double(), v.double())
    ref32 = _attention(q, k, v).double()
    e_k, e_t = rel_l2(out.double(), ref64), rel_l2(ref32, ref64)
    w_k, w_t = _worst_query(out.double(), ref64), _worst_query(ref32, ref64)
    logit = float((torch.einsum("bcs,bcr->bsr", q, k) * C ** -0.5).abs().max())
    print(f"attention C={C} S={S} gain={gain} {mode} on {dev} (|logit| <= {logit:.0f}): error vs fp64  kernel {e_k:.2e}  torch-fp32 {e_t:.2e}  "
          f"ratio {e_k / max(e_t, 1e-30):.2f};  worst query  kernel {w_k:.2e}  torch-fp32 {w_t:.2e}  ratio {w_k / max(w_t, 1e-30):.2f}")
    assert e_k < max(SLACK * e_t, FLOOR), (C, S, gain, mode, e_k, e_t)
    assert w_k < max(SLACK * w_t, FLOOR), (C, S, gain, mode, w_k, w_t)
    return e_k / max(e_t, 1e-30), w_k / max(w_t, 1e-30)


def check_attention_uniform(dev, C, S):
    """q = 0: every weight is exactly 1/S, the output is the mean of v over the keys -- the masked keys of the last tile, the sum of the
    waves' partial sums and waves without a tile all show in it."""
    from sgmse_amd import ops
    qkv = R(gen(7 * C + S), 2, 3 * C, S)
    qkv[:, :C] = 0.0
    out = ops.attention(qkv.to(dev)).cpu()
    ref = qkv[:, 2 * C:].double().mean(-1, keepdim=True).expand(2, C, S)
    err = rel_l2(out.double(), ref)
    print(f"attention C={C} S={S} with q = 0 on {dev}: rel_l2 vs the fp64 mean of v = {err:.2e}")
    assert torch.isfinite(out).all() and err < 1e-6, (C, S, err)


def check_attention_batch_independence(dev, C, S):
    """An utterance alone has the bits it has inside a batch of three."""
    from sgmse_amd import ops
    qkv = make_qkv(C, S, 8, "iid", B=3).to(dev)
    full = ops.attention(qkv)
    for i in range(3):
        assert torch.equal(ops.attention(qkv[i:i + 1].contiguous())[0], full[i]), (C, S, i)
