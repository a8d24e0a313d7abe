"""Checks of the samplers' in-kernel noise (philox_cnormal / sampler_noise, the draw schedule of engine.h) against the host model
of the generator (philox_model.py), and of the element-wise update kernels (sampler_ald / revdiff / langevin_* / sb, kernels_attn_misc.h)
against a float64 restatement of the chain on a network whose score is a known constant.  Shared by the emulator and the GPU modules.

Every bound of the form "k x a deviation" takes that deviation from two host references inside the check, never from the library."""
import numpy as np
import torch

import philox_model as PM
from conftest import rel_l2
from ode_native_checks import _small_cfg
from oracle import synth
from parity import SAMPLER_TOL, make_model

F_, T_ = 64, 64                      # the smallest input the nf = 32 network accepts
PER = F_ * T_
SEED = 0x1234_5678_9ABC_DEF1         # (both words of the seed in use)
HI = 2 ** 32


def _std1(m):
    return float(m.sde._std(torch.ones(1))[0])


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dev is None else t.to(dev)


def small_model(dev):
    """The nf = 32 model of ode_native_checks._small_cfg with its synthetic weights."""
    return make_model(_small_cfg(), dev)[0]


def small_sb_model(dev, N=3):
    return make_model(_small_cfg("ncsnpp_v2"), dev, sde="sbve", k=2.6, c=0.4, N=N, loss_type="data_prediction")[0]


# ----------------------------------------------------------------------------------------------------------------------------
# the generator alone (no library)

def check_known_answers():
    """Philox4x32-10 of the model against the three known answers of Random123 (kat_vectors: philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = " ".join(f"{int(v):08x}" for v in PM.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, got, want)
    # vectorised evaluation = element by element
    ctr = [np.array([c[i] for c, _, _ in kat]) for i in range(4)]
    key = [np.array([k[i] for _, k, _ in kat]) for i in range(2)]
    out = PM.philox4x32_10(ctr, key)
    for j, (_, _, want) in enumerate(kat):
        assert " ".join(f"{int(v[j]):08x}" for v in out) == want


def check_stream_separation(n=2 ** 20):
    """n = 2^20 elements per stream: |correlation| < 5 / sqrt(n) between Re and Im, element i and i + 1, draw d and d + 1, stream s and
    s + 1, stream s and s + 2^32 (the high word goes into the key), seed and seed + 1, seed and seed + 2^32; every one of the four
    real-valued correlations (Re-Re, Im-Im, Re-Im, Im-Re) of a pair of streams is gated, and Var Re, Var Im = 1/2 within 5 sigma.
    No NaN or infinity in either flavour, including the ends of the 24-bit range of the radius' uniform:
      k = 2^24 - 1: fp32 u1 = (16777215 + 0.5f) * 2^-24 rounds to 1.0, radius 0 exactly (z = -0 - 0i at u2's k = 0);
                    fp64 u1 = 1 - 2^-25, radius 1.7263e-4;
      k = 0:        u1 = 2^-25 in both, radius sqrt(25 ln 2) = 4.162773, the largest value the generator can return."""
    seed, s, d = SEED, 5, 3
    idx = np.arange(n)
    base = PM.cnormal64(seed, idx, d, s)
    others = {"element i + 1": PM.cnormal64(seed, idx + 1, d, s), "draw d + 1": PM.cnormal64(seed, idx, d + 1, s),
              "stream s + 1": PM.cnormal64(seed, idx, d, s + 1), "stream s + 2^32": PM.cnormal64(seed, idx, d, s + HI),
              "seed + 1": PM.cnormal64(seed + 1, idx, d, s), "seed + 2^32": PM.cnormal64(seed + HI, idx, d, s)}
    bound = 5.0 / np.sqrt(n)

    def corr(a, b):
        return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
    worst = {"Re against Im": abs(corr(base.real, base.imag))}
    for name, o in others.items():
        assert np.isfinite(o.real).all() and np.isfinite(o.imag).all(), name
        worst[name] = max(abs(corr(a, b)) for a in (base.real, base.imag) for b in (o.real, o.imag))
    print(f"stream separation, n = {n}: bound {bound:.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v < bound, (name, v, bound)
    # Var of a variance estimate of N(0, 1/2) samples: 2 (1/2)^2 / n
    for part in (base.real, base.imag):
        assert abs(float(part.var()) - 0.5) < 5.0 * np.sqrt(0.5 / n) and abs(float(part.mean())) < 5.0 * np.sqrt(0.5 / n)
    f32 = PM.cnormal32(seed, idx, d, s)
    assert np.isfinite(f32.real).all() and np.isfinite(f32.imag).all()
    # the ends of the 24-bit range
    ends = np.array([0, 2 ** 24 - 1])
    e32, e64 = PM.box_muller32(ends, np.zeros(2, dtype=np.int64)), PM.box_muller64(ends, np.zeros(2, dtype=np.int64))
    assert np.isfinite(e32.real).all() and np.isfinite(e32.imag).all() and np.isfinite(e64.real).all() and np.isfinite(e64.imag).all()
    assert abs(abs(e32[0]) - np.sqrt(25.0 * np.log(2.0))) < 1e-6 and abs(abs(e64[0]) - np.sqrt(25.0 * np.log(2.0))) < 1e-14
    assert e32[1] == 0 and abs(abs(e64[1]) - 1.7263349e-4) < 1e-10
    every = PM.box_muller32(np.arange(2 ** 24), np.zeros(2 ** 24, dtype=np.int64)).real     # every radius the fp32 flavour can take
    assert np.isfinite(every).all() and every.max() == every[0] and every.min() == every[-1] == 0


# ----------------------------------------------------------------------------------------------------------------------------
# the device stream equals the model

STREAM_CASES = ["default", "explicit", "seed_high_word", "ragged"]


def _device_prior_z(m, dev, frames, seed, streams):
    """z of the prior draw, per utterance, recovered from get_pc_sampler('none', 'none', y = 0, N = 1, denoise=False): std(1) z, no
    network evaluation.  frames: a list of frame counts (ragged list) or (B, T)."""
    kw = dict(N=1, denoise=False, seed=seed, streams=streams)
    if isinstance(frames, list):
        y = [torch.zeros(1, F_, t, dtype=torch.complex64, device=dev) for t in frames]
        out, nfe = m.get_pc_sampler("none", "none", y, **kw)()
        assert [tuple(o.shape[-2:]) for o in out] == [(F_, t) for t in frames]
    else:
        y = torch.zeros(frames[0], 1, F_, frames[1], dtype=torch.complex64, device=dev)
        out, nfe = m.get_pc_sampler("none", "none", y, **kw)()
    return [o.cpu().numpy().astype(np.complex128).reshape(-1) / _std1(m) for o in out]


def check_device_stream(dev, m, case):
    """The in-kernel stream against the float64 model, utterance by utterance.  Gates: relative L2 <= 4 x the deviation of the fp32
    model from the fp64 model on the same counters (computed here from the two host models); element-wise |z_dev - z_fp64| <= 5e-4
    (worst case: u1 rounding to exactly 1.0 in fp32 moves the radius by 1.7e-4; a wrong counter gives O(1)).
    Measured over the 13 utterances of the four cases: the models' own deviation 1.95e-7 ... 2.08e-7 (bounds 7.8e-7 ... 8.3e-7);
    emulator rel L2 1.98e-7 ... 2.12e-7, element-wise at most 5.6e-6; MI355X rel L2 1.98e-7 ... 2.11e-7, element-wise at most 5.6e-6."""
    runs = {"default": [((3, T_), SEED, None)],
            "explicit": [((4, T_), SEED, [7, HI + 7, HI, 0])],
            "seed_high_word": [((2, T_), 0x1F, None), ((2, T_), 0x1F + HI, None)],
            "ragged": [([64, 128], SEED, [HI + 5, 3])]}[case]
    seen = []
    for frames, seed, streams in runs:
        zs = _device_prior_z(m, dev, frames, seed, streams)
        ids = list(range(len(zs))) if streams is None else streams
        for b, (z, sid) in enumerate(zip(zs, ids)):
            idx = np.arange(z.size)
            ref, f32 = PM.cnormal64(seed, idx, 0, sid), PM.cnormal32(seed, idx, 0, sid).astype(np.complex128)
            own = float(np.linalg.norm(f32 - ref) / np.linalg.norm(ref))
            err = float(np.linalg.norm(z - ref) / np.linalg.norm(ref))
            worst = float(np.abs(z - ref).max())
            print(f"in-kernel stream on {dev}, {case}: seed {seed:#x} stream {sid:#x} ({z.size} elements): rel_l2 vs the fp64 model {err:.3e} "
                  f"(fp32 model vs fp64 model {own:.3e}, bound {4 * own:.3e}), element-wise {worst:.3e} (bound 5e-4)")
            assert err <= 4.0 * own, (case, b, err, own)
            assert worst <= 5e-4, (case, b, worst)
            seen.append(z)
    # no two utterances of a case share a stream (ids that differ above bit 31 and seeds that differ in the high word included)
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            k = min(seen[i].size, seen[j].size)
            assert np.abs(seen[i][:k] - seen[j][:k]).max() > 1.0, (case, i, j)


def check_philox_noise_statistics(dev):
    """test_gpu_parity.test_philox_noise_statistics on either backend.  In-kernel Philox stream: complex standard normal (Re, Im ~
    N(0, 1/2)), different per draw, reproducible per seed."""
    m = make_model(synth_cfg_nf32(), dev)[0]
    y = torch.zeros(4, 1, 256, 64, dtype=torch.complex64, device=dev)
    s = m.get_pc_sampler("none", "none", y, N=1, seed=123, denoise=False)
    x1, _ = s()
    x2, _ = m.get_pc_sampler("none", "none", y, N=1, seed=123, denoise=False)()
    x3, _ = m.get_pc_sampler("none", "none", y, N=1, seed=124, denoise=False)()
    assert torch.equal(x1, x2) and not torch.equal(x1, x3)
    z = torch.view_as_real(x1).float() / float(m.sde._std(torch.ones(1))[0])   # prior = y + std(1) z with y = 0
    assert abs(float(z.mean())) < 0.01 and abs(float(z.var()) - 0.5) < 0.01
    assert abs(float((z[..., 0] * z[..., 1]).mean())) < 0.01


def synth_cfg_nf32():
    from oracle import ncsnpp_oracle as NO
    return NO.NetCfg.for_variant("ncsnpp", nf=32)


# ----------------------------------------------------------------------------------------------------------------------------
# a seeded run equals the replayed run of the model's noise

N_SCHED = 2
#        name: (kind, sampler arguments, draws the run consumes, adjacent pair swapped by the sensitivity control)
SCHEDULE_CASES = {
    "rd_ald_c1": ("pc", dict(predictor="reverse_diffusion", corrector="ald", corrector_steps=1), 1 + N_SCHED * 2, (1, 2)),
    "rd_ald_c2": ("pc", dict(predictor="reverse_diffusion", corrector="ald", corrector_steps=2), 1 + N_SCHED * 3, (1, 2)),
    "rd_none": ("pc", dict(predictor="reverse_diffusion", corrector="none", corrector_steps=1), 1 + N_SCHED, (1, 2)),
    "none_ald": ("pc", dict(predictor="none", corrector="ald", corrector_steps=1), 1 + N_SCHED, (1, 2)),
    "rd_langevin": ("pc", dict(predictor="reverse_diffusion", corrector="langevin", corrector_steps=1), 1 + N_SCHED * 2, (1, 2)),
    "ode_fixed": ("ode_fixed", {}, 1, (0, 1)),
    "ode_native": ("ode_native", {}, 1, (0, 1)),
    "sb_sde": ("sb", {}, 3, (0, 1)),
}


def check_seeded_equals_replayed(dev, m, case, use_graph=True):
    """The draw schedule, sampler by sampler, B = 2 on the real nf = 32 network: the run with seed= / streams= against the run of the
    same sampler with noise=Z, Z[d] = the fp32 model's draw d (philox_model.replay).  Gate: relative L2 < SAMPLER_TOL (expected
    ~1e-6: the two runs differ by the last-digit differences of the device's logf / sincosf from NumPy's).  Sensitivity control: Z with
    two adjacent draws swapped (a host-side permutation) must land more than 100 x SAMPLER_TOL from the seeded run; the prior-only
    samplers get one draw more than they consume for it, so that the swap puts draw 1 in the prior's place.
    Measured, seeded vs replayed: emulator 2.7e-7 (none_ald) ... 1.1e-6, MI355X 2.8e-7 (none_ald) ... 1.2e-6 (ode_native 4.3e-7);
    seeded vs swapped, the same on both: rd_ald_c1 0.56, rd_ald_c2 0.16, rd_none 0.71, none_ald 0.86, rd_langevin 0.58, ode_fixed 1.2,
    ode_native 1.3, sb_sde 0.23."""
    kind, args, ndraws, swap = SCHEDULE_CASES[case]
    streams = [7, HI + 7]                       # two ids that differ only above bit 31
    y = synth.synth_spec(2, F_, T_, seed=4).to(dev)
    Z = _t(PM.replay(SEED, streams, PER, range(max(ndraws, 2)))).reshape(-1, 2, 1, F_, T_)
    perm = list(range(Z.shape[0]))
    perm[swap[0]], perm[swap[1]] = perm[swap[1]], perm[swap[0]]

    def run(**noise_kw):
        if kind == "pc":
            out, nfe = m.get_pc_sampler(args["predictor"], args["corrector"], y, N=N_SCHED, snr=0.5, corrector_steps=args["corrector_steps"],
                                        use_graph=use_graph, **noise_kw)()
            assert nfe == N_SCHED * ((args["corrector_steps"] if args["corrector"] != "none" else 0) + 1)
        elif kind == "ode_fixed":
            out, nfe = m.get_ode_sampler(y, N=N_SCHED, use_graph=use_graph, **noise_kw)()
            assert nfe == N_SCHED
        elif kind == "ode_native":     # one accepted step of half the interval: 7 evaluations
            out, nfe = m.get_ode_sampler(y, denoise=False, solver="native", rtol=10.0, atol=10.0, first_step=0.5, eps=0.5, **noise_kw)()
            assert nfe == 7
        else:
            out, nfe = m.get_sb_sampler(m.sde, y, sampler_type="sde", N=3, n_steps=3, use_graph=use_graph, **noise_kw)()
            assert nfe == 3
        return out.cpu()

    seeded = run(seed=SEED, streams=streams)
    replayed = run(noise=Z.to(dev))
    swapped = run(noise=Z[perm].contiguous().to(dev))
    err, ctl = rel_l2(replayed, seeded), rel_l2(swapped, seeded)
    print(f"draw schedule {case} on {dev} (use_graph={use_graph}): seeded vs replayed model noise rel_l2 = {err:.3e} (gate {SAMPLER_TOL:.0e}); "
          f"control, draws {swap[0]} and {swap[1]} swapped: {ctl:.3e} (must exceed {100 * SAMPLER_TOL:.0e})")
    assert torch.isfinite(torch.view_as_real(seeded)).all()
    assert err < SAMPLER_TOL, (case, err)
    assert ctl > 100.0 * SAMPLER_TOL, (case, ctl)


# ----------------------------------------------------------------------------------------------------------------------------
# update kernels against a float64 closed form

def const_score_model(dev):
    """_small_cfg's model with output_layer.weight = 0 and the bias left as it is: the network exit yields the constant complex value
    c = bias for every element and every t, the score is -c.  Returns (model, c)."""
    m = small_model(dev)
    with torch.no_grad():
        m.dnn.output_layer.weight.zero_()
    m.dnn.mark_weights_changed()
    b = m.dnn.output_layer.bias.detach().cpu()
    assert float(b.abs().min()) > 0
    return m, b.clone()


def const_sb_model(dev):
    """The same for a data-prediction ncsnpp_v2 model on the Schroedinger-bridge SDE (N = 3): estimate = alpha(t) x + beta(t) c."""
    m = small_sb_model(dev, N=3)
    with torch.no_grad():
        m.dnn.output_layer.weight.zero_()
    m.dnn.mark_weights_changed()
    b = m.dnn.output_layer.bias.detach().cpu()
    assert float(b.abs().min()) > 0
    return m, b.clone()


def _inputs(dev, B):
    y = synth.synth_spec(B, F_, T_, seed=4)
    y[B - 1] *= 3.0                               # the utterances differ
    return y, y.to(dev)


def check_constant_score(dev, m, c):
    """One m(x, y, t) call: the score of the prepared model is -c for every element, whatever x, y and t are."""
    y, yd = _inputs(dev, 2)
    g = torch.Generator().manual_seed(3)
    x = y + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)
    s = torch.view_as_real(m(x.to(dev), yd, torch.tensor([0.9, 0.2], device=dev)).cpu())
    assert torch.equal(s, (-c).expand_as(s)), float((s + c).abs().max())


def check_constant_estimate(dev, m, c):
    """The same for the data-prediction model: estimate = alpha(t) x + beta(t) c with the scalars of score_affine (fp32, to 1e-6)."""
    y, yd = _inputs(dev, 2)
    g = torch.Generator().manual_seed(3)
    x = y + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)
    t = torch.tensor([0.9, 0.2])
    _, al, be = m.score_affine(t)
    want = al[:, None, None, None, None].double() * torch.view_as_real(x).double() + be[:, None, None, None, None].double() * c.double()
    got = torch.view_as_real(m(x.to(dev), yd, t.to(dev)).cpu()).double()
    assert rel_l2(got, want) < 1e-6, rel_l2(got, want)


def _pc_chain(rdt, y, Z, c, tab, theta, std1, snr, predictor, corrector, ncorr, pf, denoise):
    """The fused PC loop restated element by element in the real dtype rdt.  y: [B, PER, 2] (Re, Im), Z: [ndraws, B, PER, 2], c: [2];
    the per-step scalars are the fp32 values the library receives.  Returns x_mean (denoise) or x."""
    sc = lambda v: torch.as_tensor(v, dtype=torch.float32).to(rdt)
    y, Z, c = y.to(rdt), Z.to(rdt), c.to(rdt)
    theta, std1, snr = sc(theta), sc(std1), sc(snr)
    g = (-c).expand_as(y)                         # the score
    score_w = sc(0.5 if pf else 1.0)
    pred_noise = predictor == "reverse_diffusion" and not pf
    ncorr = ncorr if corrector != "none" else 0
    dps = ncorr + (1 if pred_noise else 0)
    x = y + Z[0] * std1
    xm = x.clone()
    for s in range(tab["t"].numel()):
        for cs in range(ncorr):
            z = Z[1 + cs + s * dps]
            if corrector == "ald":
                eps, ns = sc(tab["ald_eps"][s]), sc(tab["ald_noise"][s])
            else:                                 # Langevin: step size from the batch-mean norms of score and noise
                gn = g.pow(2).sum(dim=(1, 2)).sqrt().mean()
                zn = z.pow(2).sum(dim=(1, 2)).sqrt().mean()
                r = snr * zn / gn
                eps = r * r * 2
                ns = torch.sqrt(eps * 2)
            xm = x + eps * g
            x = xm + z * ns
        if predictor == "reverse_diffusion":
            dt, G, G2 = sc(tab["dt"][s]), sc(tab["G"][s]), sc(tab["G2"][s]) * score_w
            f = (theta * (y - x)) * dt - G2 * g
            xm = x - f
            x = xm + G * Z[1 + ncorr + s * dps] if pred_noise else xm
        elif ncorr > 0:
            xm = x
    return xm if denoise else x


def _sb_chain(rdt, y, Z, c, tab, aff):
    """The Schroedinger-bridge loop, product by product and sum by sum as the kernel (and the reference) evaluate it."""
    sc = lambda v: torch.as_tensor(v, dtype=torch.float32).to(rdt)
    y, c = y.to(rdt), c.to(rdt)
    x = y.clone()
    for s in range(tab["t"].numel()):
        al, be = sc(aff[1][s]), sc(aff[2][s])
        est = (be * c).expand_as(x)
        if float(al) != 0.0:
            est = est + al * x
        x = (sc(tab["w_prev"][s]) * x + sc(tab["w_est"][s]) * est) + sc(tab["w_y"][s]) * y
        if Z is not None:
            x = x + sc(tab["w_z"][s]) * Z[s].to(rdt)
    return x


N_CLOSED = 3
#       name: (predictor, corrector, B)
CLOSED_PC_CASES = {"rd_ald": ("reverse_diffusion", "ald", 2), "rd_none": ("reverse_diffusion", "none", 2),
                   "none_ald": ("none", "ald", 2), "none_none": ("none", "none", 2), "rd_langevin": ("reverse_diffusion", "langevin", 3)}


def _gate(what, dev, out, ref64, ref32):
    got = torch.view_as_real(out.cpu()).reshape(ref64.shape).double()
    own = rel_l2(ref32.double(), ref64)
    err = rel_l2(got, ref64)
    print(f"{what} on {dev}: rel_l2 vs the fp64 restatement = {err:.3e}; the fp32 restatement's own = {own:.3e} (bound 4x = {4 * own:.3e})")
    assert own > 0 and err < 4.0 * own, (what, err, own)


def check_closed_form_pc(dev, m, c, case, denoise):
    """prior -> N = 3 steps of the fused PC loop on the constant-score model, replayed noise from the generator model, against the
    float64 restatement _pc_chain.  Gate: relative L2 < 4 x the deviation of the same restatement evaluated in torch fp32 on the CPU
    (the factor covers the kernels' different, equally valid fp32 association and FMA contraction).  'rd_langevin': B = 3 with one
    utterance's y scaled by 3, so the three-pass reduction of the step size 2 (snr mean_b|z_b| / mean_b|g_b|)^2 is gated as tightly.
    Measured, fp32 restatement's own deviation (the bound is 4x) / emulator / MI355X: none_none (the prior) 3.1e-8 / 3.1e-8 / 2.5e-8;
    none_ald 6.2e-8 / 6.2e-8 / 5.8e-8; rd_none 7.6e-8, 8.0e-8 (denoise True, False) / the same / 6.8e-8, 7.2e-8; rd_ald 1.01e-7, 1.04e-7 /
    the same / 9.5e-8, 9.8e-8; rd_langevin 1.11e-7, 1.14e-7 / 1.23e-7, 1.26e-7 / 1.30e-7, 1.32e-7; probability flow (check_closed_form_pf)
    7.5e-8 / 7.5e-8 / 6.8e-8; sb sde (check_closed_form_sb) 4.0e-8 / 4.0e-8 / 4.0e-8.  (The emulator build does not contract, so it
    lands on the fp32 restatement except for Langevin's reduction order.)"""
    predictor, corrector, B = CLOSED_PC_CASES[case]
    y, yd = _inputs(dev, B)
    snr, N = 0.5, N_CLOSED
    ncorr = 1 if corrector != "none" else 0
    ndraws = 1 + N * (ncorr + (1 if predictor == "reverse_diffusion" else 0))
    Z = PM.replay(SEED, list(range(B)), PER, range(ndraws))
    out, nfe = m.get_pc_sampler(predictor, corrector, yd, N=N, snr=snr, denoise=denoise,
                                noise=_t(Z).reshape(ndraws, B, 1, F_, T_).to(dev))()
    assert nfe == N * (ncorr + 1)
    sde = m.sde.copy()
    tab = sde.step_table(m.t_eps, snr, N)
    args = (torch.view_as_real(y.reshape(B, PER)), torch.view_as_real(_t(Z)), c, tab, float(sde.theta), _std1(m), snr,
            predictor, corrector, ncorr, False, denoise)
    _gate(f"closed form {case} denoise={denoise}", dev, out, _pc_chain(torch.float64, *args), _pc_chain(torch.float32, *args))


def check_closed_form_pf(dev, m, c):
    """The fixed-step probability-flow sampler (score_w = 0.5, no predictor noise), N = 3, same construction and gate."""
    B, N = 2, N_CLOSED
    y, yd = _inputs(dev, B)
    Z = PM.replay(SEED, list(range(B)), PER, range(1))
    out, nfe = m.get_ode_sampler(yd, N=N, noise=_t(Z).reshape(1, B, 1, F_, T_).to(dev))()
    assert nfe == N
    sde = m.sde.copy()
    tab = sde.step_table(m.t_eps, 0.0, N)
    args = (torch.view_as_real(y.reshape(B, PER)), torch.view_as_real(_t(Z)), c, tab, float(sde.theta), _std1(m), 0.0,
            "reverse_diffusion", "none", 0, True, False)
    _gate("closed form probability flow", dev, out, _pc_chain(torch.float64, *args), _pc_chain(torch.float32, *args))


def check_closed_form_sb(dev, m, c, stype):
    """Schroedinger-bridge steps (N = 3) on the constant data-prediction model.
    'sde': against the float64 restatement under the 4 x fp32-restatement gate of the PC kernels.
    'ode': the kernel reproduces the reference's product-by-product rounding and the first step cancels two terms ~w_prev[0] |y| (see
    sampler_sb_kernel), so the float64 result is not what it aims at: compared with the torch-fp32 restatement of the same non-fused
    sequence instead.  Expected: within ONE ulp of the step's largest intermediate, ulp_fp32(|w_prev[0]| max|y|) = 9.8e-4 here (w_prev[0]
    = 5458.8 at N = 3, max|y| = 2.35), carried through the later steps by prod_s max(1, |w_prev[s]|) = 1 -- that bound is printed.
    The gate is tighter, because it can be: the estimate is the constant beta c = c exactly (alpha = 0, beta = 1), so both sides apply
    the same correctly rounded IEEE products and sums to the same operands, and the results must be EQUAL, bit for bit.
    Measured: emulator 0.  MI355X 1.67e-5 (1.5 quanta of the first step, scaled by w_prev[1] w_prev[2] = 0.0116) while drt_mul_rn /
    drt_add_rn were __fmul_rn / __fadd_rn, which the compiler contracted into v_fmac -- the defect this check found; 0 since."""
    B, N = 2, N_CLOSED
    y, yd = _inputs(dev, B)
    sde = m.sde.copy()
    sde.N = N
    tab = sde.sb_step_table(1e-4, stype, N)
    aff = m.score_affine(tab["t"])
    Z = PM.replay(SEED, list(range(B)), PER, range(N)) if stype == "sde" else None
    out, _ = m.get_sb_sampler(m.sde, yd, sampler_type=stype, N=N, n_steps=N,
                              noise=None if Z is None else _t(Z).reshape(N, B, 1, F_, T_).to(dev))()
    args = (torch.view_as_real(y.reshape(B, PER)), None if Z is None else torch.view_as_real(_t(Z)), c, tab, aff)
    ref32 = _sb_chain(torch.float32, *args)
    if stype == "sde":
        _gate("closed form sb sde", dev, out, _sb_chain(torch.float64, *args), ref32)
        return
    got = torch.view_as_real(out.cpu()).reshape(ref32.shape)
    big = np.float32(abs(float(tab["w_prev"][0])) * float(y.abs().max()))
    carry = float(np.prod([max(1.0, abs(float(w))) for w in tab["w_prev"][1:]]))
    bound = float(np.spacing(big)) * carry
    worst = float((got - ref32).abs().max())
    print(f"closed form sb ode on {dev}: max |library - fp32 non-fused restatement| = {worst:.3e}; w_prev[0] = {float(tab['w_prev'][0]):.1f}, "
          f"largest intermediate {float(big):.1f}, its ulp {float(np.spacing(big)):.3e}, carried by {carry:.3g}: bound {bound:.3e}; gate: equal")
    assert worst <= bound, (worst, bound)
    assert float(aff[1].abs().max()) == 0.0 and bool((aff[2] == 1).all())      # what makes the estimate exactly c
    assert torch.equal(got, ref32), worst
