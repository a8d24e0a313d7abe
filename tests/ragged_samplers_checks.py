"""Checks of ragged batches (sgmse_set_frames) through the Schroedinger-bridge sampler and the Langevin corrector with the step size
per utterance (sgmse_sampler_cfg.corrector = 3), and of replayed noise in ragged batches.  Shared by the emulator and the GPU modules.

Everything runs on the nf = 32 network of ode_native_checks._small_cfg at F = 64; frames [64, 128] is the smallest ragged composition
(utterances are multiples of 64 frames).  Every bound of the form "k x a deviation" takes that deviation from two host references
inside the check, never from the library."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import philox_model as PM
import sampler_noise_checks as K
from conftest import rel_l2
from ode_native_checks import _small_cfg
from oracle import ncsnpp_oracle as NO
from oracle import sde_oracle as SO
from oracle import synth
from parity import NET_CASES, SAMPLER_TOL, make_model, replay_noise

F_ = K.F_
SEED = K.SEED
HI = K.HI
FRAMES = [64, 128]
IDS = [HI + 5, 3]                     # noise-stream ids: one above bit 31


def _ragged_ys(dev, frames=FRAMES, scale_last=1.0):
    """One spectrogram [1,F,T_b] per frame count (the last one scaled, so that the utterances' norms differ)."""
    ys = [synth.synth_spec(1, F_, T, seed=3 + i)[0] for i, T in enumerate(frames)]
    ys[-1] = ys[-1] * scale_last
    return [y.to(dev) for y in ys]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. Schroedinger-bridge sampler: ragged = singles

def check_sb_ragged_equals_singles(dev, m, stype):
    """Ragged [64, 128] batch of the Schroedinger-bridge sampler (N = 2, seeded, stream ids [2^32 + 5, 3]): every utterance is
    torch.equal to its own [1,1,F,T_b] call with the same seed and stream id, in either batch order; a uniform call afterwards gives
    what it gave before.  'ode' includes the first step's large cancellation (sampler_sb_kernel).
    Measured: 0 differing elements on the emulator and on MI355X, 'sde' and 'ode', both orders."""
    ys = _ragged_ys(dev)
    make = lambda y, st: m.get_sb_sampler(m.sde, y, sampler_type=stype, N=2, n_steps=2, seed=SEED, streams=st)
    singles = [make(y[None], [IDS[i]])()[0][0] for i, y in enumerate(ys)]
    together, nfe = make(ys, IDS)()
    assert nfe == 2 and len(together) == 2
    rev, _ = make(ys[::-1], IDS[::-1])()
    bad = [int((a != b).sum()) if a.shape == b.shape else -1 for a, b in zip(singles + singles[::-1], list(together) + list(rev))]
    print(f"sb {stype} ragged {FRAMES} on {dev}: elements differing from the single-utterance runs (both orders) = {bad}")
    assert bad == [0, 0, 0, 0], bad
    assert all(torch.isfinite(torch.view_as_real(s)).all() for s in singles) and not torch.equal(singles[0], ys[0])
    assert _same(make(ys[0][None], [IDS[0]])()[0][0], singles[0])          # and back to uniform batches


# ----------------------------------------------------------------------------------------------------------------------------
# 2. per-utterance Langevin = the single-utterance run of the existing code path

def check_langevin_each_equals_singles(dev, m, ragged):
    """reverse_diffusion + langevin on the real nf = 32 network, seeded, N = 2.  With corrector_scope='utterance' utterance b of (a) a
    uniform B = 2 batch (sampler_noise_checks._inputs: one utterance scaled by 3) and (b) a ragged [64, 128] batch equals, bit for bit,
    its B = 1 run with the DEFAULT scope (the batch kernels, whose mean over one utterance is that utterance's norm).
    Control: the uniform B = 2 run with the default scope lies more than 100 x SAMPLER_TOL (relative L2) from those singles -- the
    coupling that the per-utterance form removes is real (the batch mean of norms that differ between the utterances moves each
    step size, and with it the corrector's move and its noise amplitude).
    Measured: (a), (b) 0 differing elements on the emulator and on MI355X; control, relative L2 per utterance: emulator 6.8e-2, 6.6e-2;
    MI355X 6.8e-2, 6.6e-2."""
    kw = dict(N=2, snr=0.5, seed=SEED)
    run = lambda y, st, **k: m.get_pc_sampler("reverse_diffusion", "langevin", y, streams=st, **kw, **k)()
    if ragged:
        _langevin_each_ragged(dev, run)
        return
    _, yd = K._inputs(dev, 2)
    singles = [run(yd[b:b + 1], [IDS[b]])[0][0] for b in range(2)]
    each, nfe = run(yd, IDS, corrector_scope="utterance")
    assert nfe == 4
    bad = [int((each[b] != singles[b]).sum()) for b in range(2)]
    coupled, _ = run(yd, IDS)
    ctl = [rel_l2(coupled[b].cpu(), singles[b].cpu()) for b in range(2)]
    print(f"langevin per utterance, uniform B = 2 on {dev}: elements differing from the singles = {bad}; control, batch scope vs singles "
          f"rel_l2 = {ctl[0]:.3e}, {ctl[1]:.3e} (must exceed {100 * SAMPLER_TOL:.0e})")
    assert bad == [0, 0], bad
    assert min(ctl) > 100.0 * SAMPLER_TOL, ctl


def _langevin_each_ragged(dev, run):
    ys = _ragged_ys(dev, scale_last=3.0)
    singles = [run(y[None], [IDS[i]])[0][0] for i, y in enumerate(ys)]
    together, _ = run(ys, IDS, corrector_scope="utterance")
    bad = [int((a != b).sum()) if a.shape == b.shape else -1 for a, b in zip(singles, together)]
    print(f"langevin per utterance, ragged {FRAMES} on {dev}: elements differing from the singles = {bad}")
    assert bad == [0, 0], bad
    assert all(torch.isfinite(torch.view_as_real(s)).all() for s in singles)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. closed form

NOISE_GAIN = [1.0, 2.0, 1.0]           # exact factors on the utterances' replayed draws (see check_closed_form_langevin_each)


def _chain_batch_mean(rdt, ys, Zs, c, tab, theta, std1, snr, denoise):
    """sampler_noise_checks._pc_chain for 'reverse_diffusion' + 'langevin' over utterances of DIFFERENT lengths with the batch-mean
    step size (what corrector = 2 would compute if it took a ragged batch): the control of the closed-form check."""
    sc = lambda v: torch.as_tensor(v, dtype=torch.float32).to(rdt)
    ys, Zs, c = [y.to(rdt) for y in ys], [Z.to(rdt) for Z in Zs], c.to(rdt)
    theta, std1, snr = sc(theta), sc(std1), sc(snr)
    gs = [(-c).expand_as(y) for y in ys]
    xs = [y + Z[0] * std1 for y, Z in zip(ys, Zs)]
    xms = [x.clone() for x in xs]
    for s in range(tab["t"].numel()):
        zs = [Z[1 + 2 * s] for Z in Zs]
        gn = torch.stack([g.pow(2).sum().sqrt() for g in gs]).mean()
        zn = torch.stack([z.pow(2).sum().sqrt() for z in zs]).mean()
        r = snr * zn / gn
        eps = r * r * 2
        ns = torch.sqrt(eps * 2)
        dt, G, G2 = sc(tab["dt"][s]), sc(tab["G"][s]), sc(tab["G2"][s])
        for b in range(len(ys)):
            xm = xs[b] + eps * gs[b]
            x = xm + zs[b] * ns
            f = (theta * (ys[b] - x)) * dt - G2 * gs[b]
            xms[b] = x - f
            xs[b] = xms[b] + G * Zs[b][2 + 2 * s]
    return xms if denoise else xs


def check_closed_form_langevin_each(dev, m, c, frames, denoise=True):
    """prior -> N = 3 steps of reverse_diffusion + langevin with corrector_scope='utterance' on the constant-score model, replayed
    noise from the generator model per utterance (PER_b = F T_b), against sampler_noise_checks._pc_chain called per utterance on B = 1
    slices (the mean over one utterance is its own norm) in fp64.  frames: (B, T) for a uniform batch or a list for a ragged one.
    Gate: sampler_noise_checks._gate, 4 x the deviation of the fp32 restatement from the fp64 one, per utterance.
    The score of this model is the same constant for every element, so ||score_b|| and ||z_b|| of raw generator draws both scale
    with sqrt(PER_b) and their ratio -- the step size -- comes out the same per utterance and per batch to within the draws' own
    fluctuation: with the raw draws the control below measures 3.9e-3, 2.7e-3 on the ragged case, under its threshold.  The inputs
    are therefore changed, not the threshold: utterance 1's replayed draws are the generator's times NOISE_GAIN[1] = 2 (exact in
    fp32 and fp64; replayed noise is an input like any other), which makes the two scopes differ by O(1) as they do on real data.
    Control (ragged case): the restatement with the batch-mean norms (_chain_batch_mean) lies more than 100 x SAMPLER_TOL from the
    per-utterance one.  The case controls the other direction too: with sampler_langevin_each_kernel reading lang[0..1] for every
    utterance the ragged case fails this gate (tried once on the emulator: utterance 1 lands 6.1e-1 from the fp64
    restatement against a bound of 3.1e-7, utterance 0 stays at 8.4e-8).
    Measured, per utterance, denoise=True; the fp32 restatement's own deviation (the bound is 4x) -> the library's: emulator uniform
    B = 3 9.4e-8 -> 8.6e-8, 8.2e-8 -> 8.4e-8, 1.13e-7 -> 8.8e-8; ragged [64, 128] 9.2e-8 -> 8.4e-8, 7.8e-8 -> 8.9e-8; MI355X uniform
    9.4e-8 -> 7.9e-8, 1.16e-7 -> 7.9e-8, 1.02e-7 -> 8.6e-8; ragged 9.2e-8 -> 7.8e-8, 1.51e-7 -> 7.6e-8 (the restatement is torch on the
    host: its own deviation varies with the host's thread count); control (ragged, host only) 1.05, 0.28."""
    ragged = isinstance(frames, list)
    Ts = frames if ragged else [frames[1]] * frames[0]
    B = len(Ts)
    if ragged:
        ys = _ragged_ys("cpu", Ts)
        yd = [y.to(dev) for y in ys]
    else:
        y, yd = K._inputs(dev, B)
        ys = [y[b] for b in range(B)]
    snr, N = 0.5, K.N_CLOSED
    ndraws = 1 + 2 * N
    Zs = [PM.replay(SEED, [b], F_ * T, range(ndraws)) * NOISE_GAIN[b] for b, T in enumerate(Ts)]           # [ndraws, 1, PER_b] each
    Zt = [K._t(Z).reshape(ndraws, 1, F_, T) for Z, T in zip(Zs, Ts)]
    noise = [z.to(dev) for z in Zt] if ragged else torch.stack(Zt, dim=1).to(dev)
    out, nfe = m.get_pc_sampler("reverse_diffusion", "langevin", yd, N=N, snr=snr, denoise=denoise, noise=noise,
                                corrector_scope="utterance")()
    assert nfe == 2 * N
    sde = m.sde.copy()
    tab = sde.step_table(m.t_eps, snr, N)
    rest = (c, tab, float(sde.theta), K._std1(m), snr)
    refs64 = []
    for b, T in enumerate(Ts):
        args = (torch.view_as_real(ys[b].reshape(1, F_ * T)), torch.view_as_real(K._t(Zs[b])), *rest, "reverse_diffusion", "langevin", 1,
                False, denoise)
        refs64.append(K._pc_chain(torch.float64, *args))
        K._gate(f"closed form langevin per utterance, {'ragged' if ragged else 'uniform'} {Ts}, utterance {b}, denoise={denoise}", dev,
                out[b], refs64[-1], K._pc_chain(torch.float32, *args))
    if ragged:
        mean = _chain_batch_mean(torch.float64, [torch.view_as_real(y.reshape(-1)) for y in ys], [torch.view_as_real(K._t(Z)[:, 0]) for Z in Zs],
                                 *rest, denoise)
        ctl = [rel_l2(a.reshape(-1), b.reshape(-1)) for a, b in zip(mean, refs64)]
        print(f"closed form langevin on {dev}: control, batch-mean step size vs per-utterance step size rel_l2 = "
              f"{', '.join(f'{v:.3e}' for v in ctl)} (must exceed {100 * SAMPLER_TOL:.0e})")
        assert min(ctl) > 100.0 * SAMPLER_TOL, ctl


# ----------------------------------------------------------------------------------------------------------------------------
# 4. against the oracle

def check_langevin_each_oracle(dev, use_graph=True):
    """Uniform B = 2, reverse_diffusion + langevin, N = 2, NoiseReplay noise as in parity.check_sampler_oracle, corrector_scope=
    'utterance': each utterance against oracle.sde_oracle.pc_sample run on that utterance ALONE with its slice of the draws (the
    reference's one-file-at-a-time loop).  Gate: parity.SAMPLER_TOL; equal NFE.  The same gate between the native run and the
    Python loop (force_python_loop=True, corrector_scope='utterance') on the same replayed noise.
    Measured, relative L2: vs the oracle emulator 1.47e-6, 1.27e-6 / MI355X 1.52e-6, 1.34e-6 (with and without the captured step);
    vs the Python loop 7.7e-7 / 1.17e-6."""
    cfg = _small_cfg()
    m, P = make_model(cfg, dev)
    N, snr, B = 2, 0.5, 2
    y, yd = K._inputs(dev, B)
    Z = replay_noise((B, 1, F_, K.T_), 1 + 2 * N)
    out, nfe = m.get_pc_sampler("reverse_diffusion", "langevin", yd, N=N, snr=snr, noise=Z.to(dev), use_graph=use_graph,
                                corrector_scope="utterance")()
    so = SO.OUVE(m.sde.theta, m.sde.sigma_min, m.sde.sigma_max, N)
    errs = []
    for b in range(B):
        draws = iter(Z[:, b:b + 1])
        ref, nfe_ref = SO.pc_sample(so, lambda a, bb, cc: NO.score_fn(P, cfg, a, bb, cc), y[b:b + 1], lambda like: next(draws), eps=0.03,
                                    snr=snr, corrector="langevin")
        assert nfe == nfe_ref
        errs.append(rel_l2(out[b:b + 1].cpu(), ref))
    draws = iter(Z.to(dev))
    orig = torch.randn_like
    torch.randn_like = lambda like, **kw: next(draws)
    try:
        loop, nfe_loop = m.get_pc_sampler("reverse_diffusion", "langevin", yd, N=N, snr=snr, force_python_loop=True,
                                          corrector_scope="utterance")()
    finally:
        torch.randn_like = orig
    e_loop = rel_l2(out.cpu(), loop.cpu())
    print(f"langevin per utterance on {dev}: rel_l2 vs the oracle on each utterance alone = {', '.join(f'{e:.3e}' for e in errs)}; "
          f"vs the Python loop with scope='utterance' = {e_loop:.3e} (gate {SAMPLER_TOL:.0e})")
    assert max(errs) < SAMPLER_TOL, errs
    assert nfe_loop == nfe and e_loop < SAMPLER_TOL, e_loop


# ----------------------------------------------------------------------------------------------------------------------------
# 5. replayed noise in ragged batches

#          name: (sampler arguments or None for the Schroedinger-bridge 'sde' sampler, draws of an N = 2 run, adjacent draws swapped by the control)
REPLAY_CASES = {"rd_ald": (dict(corrector="ald"), 5, (1, 2)),
                "rd_langevin_each": (dict(corrector="langevin", corrector_scope="utterance"), 5, (1, 2)),
                "sb_sde": (None, 2, (0, 1))}


def check_ragged_replayed_noise(dev, m, case):
    """Replayed noise of a ragged [64, 128] batch (a list of [ndraws,1,F,T_b]; packed draw-major by the host layer), N = 2.
    (a) every utterance of the replayed ragged run is bit-identical to its single-utterance run with its own draws;
    (b) the SEEDED ragged run (stream ids [2^32 + 5, 3]) against the replayed run of the generator model's draws (philox_model.replay
    per utterance: the element index runs inside the utterance, the stream id is the utterance's).  Gate: SAMPLER_TOL, as in
    sampler_noise_checks.check_seeded_equals_replayed (the two differ by the last digits of logf / sincosf); control: two adjacent
    draws swapped must land more than 100 x SAMPLER_TOL from the seeded run.  (b) pins the ragged draw schedule of the kernels to the
    host model.
    Measured, per utterance, seeded vs replayed / seeded vs swapped: emulator rd_ald 1.24e-6, 9.1e-7 / 0.51, 0.31; rd_langevin_each
    1.19e-6, 9.4e-7 / 0.57, 0.40; sb_sde 9.0e-7, 1.03e-6 / 0.44, 0.41; MI355X rd_ald 1.41e-6, 1.01e-6 / 0.51, 0.31; rd_langevin_each
    1.23e-6, 1.11e-6 / 0.57, 0.40; sb_sde 1.00e-6, 1.02e-6 / 0.44, 0.41; (a) 0 differing elements everywhere."""
    args, ndraws, swap = REPLAY_CASES[case]
    ys = _ragged_ys(dev, scale_last=3.0)
    Zs = [K._t(PM.replay(SEED, [sid], F_ * T, range(ndraws))).reshape(ndraws, 1, F_, T).to(dev) for sid, T in zip(IDS, FRAMES)]
    perm = list(range(ndraws))
    perm[swap[0]], perm[swap[1]] = perm[swap[1]], perm[swap[0]]

    def run(y, **noise_kw):
        if args is None:
            out, nfe = m.get_sb_sampler(m.sde, y, sampler_type="sde", N=2, n_steps=2, **noise_kw)()
        else:
            out, nfe = m.get_pc_sampler("reverse_diffusion", y=y, corrector_name=args["corrector"], N=2, snr=0.5,
                                        **{k: v for k, v in args.items() if k != "corrector"}, **noise_kw)()
            assert nfe == 4
        return out

    replayed = run(ys, noise=Zs)
    singles = [run(y[None], noise=z[:, None].contiguous())[0] for y, z in zip(ys, Zs)]
    bad = [int((a != b).sum()) if a.shape == b.shape else -1 for a, b in zip(singles, replayed)]
    seeded = run(ys, seed=SEED, streams=IDS)
    swapped = run(ys, noise=[z[perm].contiguous() for z in Zs])
    err = [rel_l2(a.cpu(), b.cpu()) for a, b in zip(replayed, seeded)]
    ctl = [rel_l2(a.cpu(), b.cpu()) for a, b in zip(swapped, seeded)]
    print(f"ragged replayed noise {case} on {dev}: elements differing from the single replayed runs = {bad}; seeded vs replayed model noise "
          f"rel_l2 = {err[0]:.3e}, {err[1]:.3e} (gate {SAMPLER_TOL:.0e}); control, draws {swap[0]} and {swap[1]} swapped: {ctl[0]:.3e}, {ctl[1]:.3e} "
          f"(must exceed {100 * SAMPLER_TOL:.0e})")
    assert bad == [0, 0], bad
    assert all(torch.isfinite(torch.view_as_real(s)).all() for s in seeded)
    assert max(err) < SAMPLER_TOL, (case, err)
    assert min(ctl) > 100.0 * SAMPLER_TOL, (case, ctl)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. captured step

def check_captured_step(dev, kind):
    """The captured step (use_graph=True) of the ragged Schroedinger-bridge sampler (kind 'sb') or of the ragged per-utterance Langevin
    corrector (kind 'langevin') under two compositions of one batch size in a row, [64, 128] then [128, 64]: each output equals its
    use_graph=False run bit for bit.  Returns graph_captures() + graph_updates() after each of the two captured calls, counted from
    before the first: as in parity.check_graph_update_path every new composition re-captures (an update in place or a new instance),
    so [1, 2] where graphs exist and [0, 0] on the eager path of the emulator.
    Measured: MI355X [1, 2] for both kinds, outputs equal; emulator [0, 0]."""
    m = K.small_sb_model(dev) if kind == "sb" else K.small_model(dev)
    eng = m.dnn.engine(torch.device(dev))

    def run(ys, g):
        if kind == "sb":
            return m.get_sb_sampler(m.sde, ys, sampler_type="sde", N=2, n_steps=2, seed=SEED, streams=IDS, use_graph=g)()[0]
        return m.get_pc_sampler("reverse_diffusion", "langevin", ys, N=2, snr=0.5, seed=SEED, streams=IDS, use_graph=g,
                                corrector_scope="utterance")()[0]

    base, hist = eng.graph_captures() + eng.graph_updates(), []
    for frames in ([64, 128], [128, 64]):
        ys = _ragged_ys(dev, frames, scale_last=3.0)
        with_graph = run(ys, True)
        hist.append(eng.graph_captures() + eng.graph_updates() - base)
        eager = run(ys, False)
        for a, b in zip(with_graph, eager):
            assert _same(a, b), (kind, frames)
    print(f"captured step, ragged {kind} on {dev}: captures + in-place updates after [64,128], [128,64] = {hist}")
    return hist


# ----------------------------------------------------------------------------------------------------------------------------
# 7. interfaces

def check_interfaces(dev, m, sb):
    """What the new arguments refuse: an invalid corrector_scope (ValueError, at every layer), corrector = 4 at the C ABI (EINVAL ->
    ValueError), a list given to the Schroedinger-bridge Python loop (TypeError), ragged noise given as a tensor or with wrong shapes
    (ValueError); a ragged batch with 'langevin' at the default scope still raises RuntimeError naming the Langevin corrector."""
    from sgmse_amd import _lib
    from sgmse_amd.sampling.correctors import LangevinCorrector
    ys = _ragged_ys(dev)
    with pytest.raises(ValueError, match="corrector_scope"):
        m.get_pc_sampler("reverse_diffusion", "langevin", ys, N=1, corrector_scope="file")
    with pytest.raises(ValueError, match="corrector_scope"):
        m.get_pc_sampler("reverse_diffusion", "ald", ys[0][None], N=1, corrector_scope=None)
    with pytest.raises(ValueError, match="scope"):
        LangevinCorrector(m.sde, m, snr=0.5, n_steps=1, scope="file")
    m.get_pc_sampler("reverse_diffusion", "ald", ys[0][None], N=1, corrector_scope="utterance")      # accepted with every corrector
    eng = m.dnn.engine(torch.device(dev))
    with pytest.raises(ValueError, match="corrector_scope"):
        eng.pc_sample(ys, m.sde.step_table(0.03, 0.5, 1), theta=1.5, std1=1.0, corrector="langevin", corrector_steps=1,
                      predictor="reverse_diffusion", probability_flow=False, denoise=True, noise=None, seed=1, corrector_scope="each")
    cfg = _lib.SamplerCfgC()
    cfg.N, cfg.corrector, cfg.corrector_steps, cfg.predictor = 1, 4, 1, 1
    y1 = ys[0].reshape(1, 1, F_, 64).contiguous()
    out = torch.empty_like(y1)
    rc = eng.lib.sgmse_pc_sample(eng.h, y1.data_ptr(), out.data_ptr(), 1, F_, 64, ctypes.byref(cfg), None, ctypes.c_ulonglong(0), None)
    assert rc == -1
    with pytest.raises(ValueError, match="corrector"):
        eng.check(rc)
    with pytest.raises(TypeError, match="ragged"):
        sb.get_sb_sampler(sb.sde, ys, sampler_type="sde", N=1, n_steps=1, force_python_loop=True)
    z = lambda n, T: torch.zeros(n, 1, F_, T, dtype=torch.complex64, device=dev)
    pc = lambda nz: m.get_pc_sampler("reverse_diffusion", "ald", ys, N=1, snr=0.5, noise=nz)()
    for nz in (z(3, 192), [z(3, 64)], [z(3, 64), z(3, 64)], [z(3, 64), z(4, 128)], [z(2, 64), z(2, 128)], [z(3, 64)[:, 0], z(3, 128)[:, 0]]):
        with pytest.raises(ValueError, match="noise"):
            pc(nz)
    for nz in (z(1, 192), [z(1, 128), z(1, 64)], [z(0, 64), z(0, 128)]):
        with pytest.raises(ValueError, match="noise"):
            sb.get_sb_sampler(sb.sde, ys, sampler_type="sde", N=1, n_steps=1, noise=nz)()
    with pytest.raises(RuntimeError, match="Langevin"):
        m.get_pc_sampler("reverse_diffusion", "langevin", ys, N=1, snr=0.5, seed=5)()
    out, nfe = m.get_pc_sampler("reverse_diffusion", "langevin", ys, N=1, snr=0.5, seed=5, corrector_scope="utterance")()      # and the context stays usable
    assert nfe == 2 and [tuple(o.shape) for o in out] == [(1, F_, 64), (1, F_, 128)]


# ----------------------------------------------------------------------------------------------------------------------------
# 8. directory job and enhance_batch

def _hparams(kind):
    from sgmse_amd.data_module import SpecsDataModule
    front = dict(data_module_cls=SpecsDataModule, n_fft=510, hop_length=128, spec_factor=0.15, spec_abs_exponent=0.5, t_eps=0.03, nf=32)
    if kind == "sbve":
        return dict(backbone="ncsnpp_v2", sde="sbve", k=2.6, c=0.4, N=1, loss_type="data_prediction", **front), NO.NetCfg.for_variant("ncsnpp_v2", nf=32)
    return dict(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30, **front), NET_CASES["fwd_nf32"]


def check_directory_job(dev, tmp_path, kind):
    """python -m sgmse_amd.enhancement on three files whose spectrograms pad to 64, 64 and 128 frames, for a Schroedinger-bridge
    checkpoint (kind 'sbve': --ragged) and an OUVE one (kind 'langevin': --corrector langevin --corrector_scope utterance --ragged):
    the run is planned as ONE ragged batch (the sampler receives a list of three spectrograms) with no fall-back warning, and writes
    files equal to those of the one-file-at-a-time run (--batch_size 1) with the same --seed.  'sbve': ScoreModel.enhance_batch on the
    list of waveforms equals the single-waveform calls bit for bit as well.  'langevin': --ragged with the batch scope still falls
    back to batches of one padded length, with the reworded warning."""
    from scipy.io import wavfile
    from sgmse_amd import enhancement as E
    from sgmse_amd.model import ScoreModel
    hp, cfg = _hparams("sbve" if kind == "sbve" else "ouve")
    src = ScoreModel(**hp)
    src.dnn.load_state_dict(synth.synth_params(cfg, seed=0))
    ckpt = tmp_path / "m.ckpt"
    torch.save({"state_dict": {"dnn." + k: v.clone() for k, v in src.dnn.state_dict().items()}, "hyper_parameters": hp}, ckpt)
    noisy = tmp_path / "noisy"
    (noisy / "sub").mkdir(parents=True)
    rng = torch.Generator().manual_seed(5)
    lengths = {"a.wav": 5000, "b.wav": 5100, "sub/c.wav": 8500}      # 40, 40 and 67 frames: padded to 64, 64 and 128 (reflection padding
    waves = {}                                                        # of the ncsnpp_v2 front end needs more frames than it adds)
    for name, L in lengths.items():
        waves[name] = 0.1 * torch.randn(L, generator=rng)
        wavfile.write(str(noisy / name), 16000, waves[name].numpy())
    base = ["--test_dir", str(noisy), "--ckpt", str(ckpt), "--device", str(dev), "--N", "1", "--seed", "7"]
    if kind == "langevin":
        base += ["--corrector", "langevin", "--corrector_scope", "utterance"]
    seen = []
    orig = E.build_sampler

    def spy(model, Y, *a, **k):
        seen.append([int(y.shape[-1]) for y in Y] if isinstance(Y, (list, tuple)) else (int(Y.shape[0]), int(Y.shape[-1])))
        return orig(model, Y, *a, **k)
    E.build_sampler = spy
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert E.main(base + ["--enhanced_dir", str(tmp_path / "one"), "--batch_size", "1"]) == 3
            assert seen == [(1, 64), (1, 64), (1, 128)], seen
            del seen[:]
            assert E.main(base + ["--enhanced_dir", str(tmp_path / "rag"), "--ragged", "--batch_size", "3"]) == 3
            assert seen == [[64, 64, 128]], seen
        fallback = [str(w.message) for w in caught if "batching by padded length" in str(w.message)]
        assert not fallback, fallback
        if kind == "langevin":
            del seen[:]
            with pytest.warns(UserWarning, match="langevin at batch scope.*batching by padded length"):
                E.main(base[:-2] + ["--enhanced_dir", str(tmp_path / "fb"), "--ragged", "--batch_size", "3"])
            assert seen == [(2, 64), (1, 128)], seen
    finally:
        E.build_sampler = orig
    for name, L in lengths.items():
        sr, x1 = wavfile.read(str(tmp_path / "one" / name))
        _, x2 = wavfile.read(str(tmp_path / "rag" / name))
        assert sr == 16000 and x1.shape == (L,) and np.isfinite(x1).all() and np.abs(x1).max() > 0
        assert np.array_equal(x1, x2), name
    if kind != "sbve":
        return
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # checkpoint without EMA weights
        m = ScoreModel.load_from_checkpoint(str(ckpt), map_location=dev)
    m.eval()
    m.to(dev)
    ws = [waves["a.wav"], waves["sub/c.wav"]]
    alone = [m.enhance_batch(w[None], seed=4, streams=[5 + i], pad_mode="reflection")[0][0] for i, w in enumerate(ws)]
    mixed, nfe = m.enhance_batch(ws, seed=4, streams=[5, 6], pad_mode="reflection")
    assert nfe == 50 and all(_same(a, b) for a, b in zip(alone, mixed))      # (get_sb_sampler reports its n_steps argument, like the reference)
    assert all(torch.isfinite(a).all() and float(a.abs().max()) > 0 for a in alone)
