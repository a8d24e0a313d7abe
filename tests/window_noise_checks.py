"""Checks of the noise geometry of the samplers' in-kernel Philox noise (sgmse_set_noise_frames, sampler_noise_index of
kernels_attn_misc.h) and of what it is for: ``ScoreModel.enhance_long(window_noise="recording")``, where the windows of a recording
draw ONE noise field, and ``python -m sgmse_amd.enhancement --window_noise``.  Shared by the emulator and the GPU modules.

An utterance with the geometry (first, total) is the frames first .. first + T_b - 1 of a recording of ``total`` frames: its element
(f, t) draws at the counter index f * total + first + t of its stream.  Shapes are those of sampler_noise_checks (nf = 32, F = 64, T of
64 or 128) and long_recording_checks (n_fft = 126, hop 32, windows of 128 frames overlapping by 32)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import long_recording_checks as L
import philox_model as PM
import sampler_noise_checks as K
from conftest import rel_l2
from ode_native_checks import _small_cfg
from oracle import synth
from parity import SAMPLER_TOL, make_model

F_, SEED, HI = K.F_, K.SEED, K.HI
N_STEPS = 2
UNIFORM = ((2, 64), [(0, 200), (136, 200)])               # (B, T) and one (first_frame, total_frames) per utterance
RAGGED = ([64, 128], [(5, 333), (205, 333)])              # frame counts ...
LAYOUTS = {"uniform": UNIFORM, "ragged": RAGGED}
L_WHOLE = 255 * L.HOP                                     # 256 frames: what pad_spec leaves alone

_t = K._t


def _frames_of(shape):
    return list(shape) if isinstance(shape, list) else [shape[1]] * shape[0]


def geometry_index(T, first, total):
    """Counter indices of an utterance [F, T] under the geometry (first, total), flattened as the utterance is stored."""
    return (np.arange(F_, dtype=np.int64)[:, None] * int(total) + int(first) + np.arange(T, dtype=np.int64)[None, :]).reshape(-1)


def model_noise(frames, streams, geom, draws, flavour=PM.cnormal32):
    """Per utterance [len(draws), F * T_b]: the host model's draws at the geometry's indices (geom None: the default geometry)."""
    geom = [(0, T) for T in frames] if geom is None else geom
    return [np.stack([flavour(SEED, geometry_index(T, a, tot), d, s) for d in draws]) for T, s, (a, tot) in zip(frames, streams, geom)]


def _zeros(dev, shape):
    if isinstance(shape, list):
        return [torch.zeros(1, F_, t, dtype=torch.complex64, device=dev) for t in shape]
    return torch.zeros(shape[0], 1, F_, shape[1], dtype=torch.complex64, device=dev)


def prior_z(m, dev, shape, streams=None, noise_frames=None, seed=SEED):
    """z of the prior draw per utterance, complex128 [F * T_b], as sampler_noise_checks._device_prior_z recovers it: the PC sampler
    'none' / 'none' on y = 0 with N = 1 returns std(1) z and evaluates no network."""
    out, _ = m.get_pc_sampler("none", "none", _zeros(dev, shape), N=1, denoise=False, seed=seed, streams=streams, noise_frames=noise_frames)()
    return [o.cpu().numpy().astype(np.complex128).reshape(-1) / K._std1(m) for o in out]


def _inputs(dev, shape):
    """y of a layout on the device: a tensor [B,1,F,T] or a ragged list of [1,F,T_b]; the utterances differ."""
    if isinstance(shape, list):
        return [synth.synth_spec(1, F_, t, seed=4 + i)[0].mul(1.0 + i).to(dev) for i, t in enumerate(shape)]
    y = synth.synth_spec(shape[0], F_, shape[1], seed=4)
    y[-1] *= 3.0
    return y.to(dev)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the device stream under a geometry equals the model

def check_device_stream_geometry(dev, m, layout):
    """The in-kernel stream under a non-trivial geometry against the float64 model evaluated at f * total + first + t, utterance by
    utterance, under check_device_stream's gates: relative L2 <= 4 x the deviation of the fp32 model from the fp64 model on the same
    counters, element-wise |z_dev - z_fp64| <= 5e-4 (a wrong counter gives O(1))."""
    shape, geom = LAYOUTS[layout]
    frames, streams = _frames_of(shape), [HI + 5, 3]
    zs = prior_z(m, dev, shape, streams, geom)
    ref64, ref32 = model_noise(frames, streams, geom, [0], PM.cnormal64), model_noise(frames, streams, geom, [0])
    for b, z in enumerate(zs):
        ref, f32 = ref64[b][0], ref32[b][0].astype(np.complex128)
        own = float(np.linalg.norm(f32 - ref) / np.linalg.norm(ref))
        err = float(np.linalg.norm(z - ref) / np.linalg.norm(ref))
        worst = float(np.abs(z - ref).max())
        print(f"in-kernel stream on {dev}, {layout}, utterance {b} geometry {geom[b]}: rel_l2 vs the fp64 model {err:.3e} (fp32 model vs fp64 "
              f"model {own:.3e}, bound {4 * own:.3e}), element-wise {worst:.3e} (bound 5e-4)")
        assert err <= 4.0 * own, (layout, b, err, own)
        assert worst <= 5e-4, (layout, b, worst)
    # the geometry matters: the same call without one is somewhere else
    plain = prior_z(m, dev, shape, streams)
    assert np.abs(plain[1] - zs[1]).max() > 1.0


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the explicit default geometry is no geometry

DEFAULT_CASES = ("pc_ald", "sb_sde", "ode_each")


def check_explicit_default(dev, m, case):
    """noise_frames=[(0, T_b)] and no noise_frames give torch.equal samples (f * T_b + 0 + t is the index inside the utterance): the PC
    sampler with 'ald' on the ragged batch [64, 128], the Schroedinger-bridge 'sde' sampler and ode_sample_each on a uniform one.  ``m``:
    the OUVE model, for 'sb_sde' the Schroedinger-bridge model."""
    shape = [64, 128] if case == "pc_ald" else (2, 64)
    y, frames = _inputs(dev, shape), _frames_of(shape)

    def run(**kw):
        if case == "pc_ald":
            out, _ = m.get_pc_sampler("none", "ald", y, N=1, snr=0.5, denoise=False, seed=SEED, streams=[7, HI + 7], **kw)()
            return torch.cat([o.reshape(-1) for o in out]).cpu()
        if case == "sb_sde":
            return m.get_sb_sampler(m.sde, y, sampler_type="sde", N=2, seed=SEED, streams=[7, HI + 7], **kw)()[0].cpu()
        return m.get_ode_sampler(y, denoise=False, solver="native", step_control="utterance", rtol=10.0, atol=10.0, first_step=0.5, eps=0.5,
                                 seed=SEED, streams=[7, HI + 7], **kw)()[0].cpu()
    plain, explicit = run(), run(noise_frames=[(0, T) for T in frames])
    assert torch.isfinite(torch.view_as_real(plain)).all() and torch.equal(plain, explicit)
    moved = run(noise_frames=[(1, T + 1) for T in frames])              # ... and the keyword does reach the kernels
    assert not torch.equal(plain, moved)


def _raw_set_noise_frames(ctx, pairs):
    """sgmse_set_noise_frames itself, past the host layer (which withdraws a table no call has consumed)."""
    n = len(pairs)
    first, total = (C.c_int * n)(*[p[0] for p in pairs]), (C.c_int * n)(*[p[1] for p in pairs])
    ctx.check(ctx.lib.sgmse_set_noise_frames(ctx.h, first, total, n))


def check_other_batch_size_ignores(dev, m):
    """A geometry set for batch size 2 and followed by a call of batch size 1: that call draws what it draws without (and consumes
    the table: a later call of batch size 2 draws the default too); n = 0 withdraws a pending table."""
    ctx = m.dnn.engine(torch.device(dev))
    one, two = prior_z(m, dev, (1, 64)), prior_z(m, dev, (2, 64))
    _raw_set_noise_frames(ctx, UNIFORM[1])
    assert np.array_equal(prior_z(m, dev, (1, 64))[0], one[0])
    assert all(np.array_equal(a, b) for a, b in zip(prior_z(m, dev, (2, 64)), two))
    _raw_set_noise_frames(ctx, UNIFORM[1])
    ctx.check(ctx.lib.sgmse_set_noise_frames(ctx.h, None, None, 0))
    assert all(np.array_equal(a, b) for a, b in zip(prior_z(m, dev, (2, 64)), two))
    _raw_set_noise_frames(ctx, UNIFORM[1])                            # (and a pending table of the call's size does apply)
    assert not np.array_equal(prior_z(m, dev, (2, 64))[1], two[1])


# ----------------------------------------------------------------------------------------------------------------------------
# 3. overlapping utterances of one stream share the draws of the frames they share

def check_overlaps_share_draws(dev, m):
    """Two utterances [128, 64] (ragged) with ONE stream id and the geometries (0, 160) and (96, 160): the prior z of utterance 0 at its
    frames 96 .. 127 is torch.equal to utterance 1's frames 0 .. 31.  With two stream ids nothing is shared."""
    geom = [(0, 160), (96, 160)]
    a, b = [torch.from_numpy(z) for z in prior_z(m, dev, [128, 64], [HI + 9, HI + 9], geom)]
    a, b = a.reshape(F_, 128), b.reshape(F_, 64)
    assert torch.equal(a[:, 96:128], b[:, 0:32]) and float(a[:, 96:128].abs().max()) > 1.0
    assert not torch.equal(a[:, 64:96], b[:, 0:32])
    a2, b2 = [torch.from_numpy(z) for z in prior_z(m, dev, [128, 64], [HI + 9, 9], geom)]
    assert torch.equal(a2.reshape(F_, 128), a) and float((a2.reshape(F_, 128)[:, 96:128] - b2.reshape(F_, 64)[:, 0:32]).abs().max()) > 1.0


# ----------------------------------------------------------------------------------------------------------------------------
# 4. every consumer of the noise follows the geometry

#            name: (kind, sampler arguments, number of draws, layouts)
CONSUMERS = {
    "rd_ald": ("pc", dict(corrector="ald"), 1 + N_STEPS * 2, ("uniform", "ragged")),
    "rd_langevin_utterance": ("pc", dict(corrector="langevin", corrector_scope="utterance"), 1 + N_STEPS * 2, ("uniform", "ragged")),
    "rd_langevin_batch": ("pc", dict(corrector="langevin"), 1 + N_STEPS * 2, ("uniform",)),
    "sb_sde": ("sb", {}, N_STEPS, ("uniform", "ragged")),
    "ode_batch": ("ode", dict(step_control="batch"), 1, ("uniform",)),
    "ode_utterance": ("ode", dict(step_control="utterance"), 1, ("uniform", "ragged")),
}
CONSUMER_CASES = [(c, lay) for c, v in CONSUMERS.items() for lay in v[3]]


def check_consumer(dev, m, case, layout, use_graph=True):
    """Seeded Philox under a non-trivial geometry against the same sampler replaying the fp32 host model's draws at the geometry's
    indices f * total + first + t, under check_seeded_equals_replayed's gates: relative L2 < SAMPLER_TOL (expected ~1e-6, the device's
    logf / sincosf against NumPy's), and the sensitivity control -- here the model's draws at the DEFAULT indices, what a consumer that
    ignored the geometry would have drawn -- more than 100 x SAMPLER_TOL away.  N = 2 steps; the native ODE takes one accepted step of
    half the interval (7 evaluations); a ragged ODE batch, which takes no replayed noise, gets the replayed prior as its start state.
    ``m``: the OUVE model, for 'sb_sde' the Schroedinger-bridge model.
    Measured over the ten cases, seeded vs replayed: emulator 3.4e-7 (ode) ... 1.1e-6, MI355X 3.4e-7 (ode) ... 1.14e-6 (rd_ald ragged, with and
    without the captured step); control: 0.39 (sb_sde ragged) ... 1.21 on both."""
    kind, args, ndraws, _ = CONSUMERS[case]
    shape, geom = LAYOUTS[layout]
    frames, streams = _frames_of(shape), [7, HI + 7]
    ragged = isinstance(shape, list)
    y = _inputs(dev, shape)

    def as_noise(Z):       # per-utterance [ndraws, F*T_b] -> what the sampler takes
        if ragged:
            return [_t(z).reshape(-1, 1, F_, T).to(dev) for z, T in zip(Z, frames)]
        return torch.stack([_t(z).reshape(-1, 1, F_, frames[0]) for z in Z], dim=1).to(dev)

    def run(Z=None, **kw):
        if Z is None:
            kw.update(seed=SEED, streams=streams)
        if kind == "pc":
            out, nfe = m.get_pc_sampler("reverse_diffusion", args["corrector"], y, N=N_STEPS, snr=0.5, corrector_steps=1, use_graph=use_graph,
                                        corrector_scope=args.get("corrector_scope", "batch"), noise=None if Z is None else as_noise(Z), **kw)()
            assert nfe == N_STEPS * 2
        elif kind == "sb":
            out, nfe = m.get_sb_sampler(m.sde, y, sampler_type="sde", N=N_STEPS, n_steps=N_STEPS, use_graph=use_graph,
                                        noise=None if Z is None else as_noise(Z), **kw)()
        else:
            sampler = lambda **nk: m.get_ode_sampler(y, denoise=False, solver="native", rtol=10.0, atol=10.0, first_step=0.5, eps=0.5,
                                                     step_control=args["step_control"], **nk, **kw)
            if Z is None:
                out, nfe = sampler()()
            elif ragged:
                x0 = [yb + K._std1(m) * _t(z[0]).reshape(1, F_, T).to(dev) for yb, z, T in zip(y, Z, frames)]
                out, nfe = sampler()(z=x0)
            else:
                out, nfe = sampler(noise=as_noise(Z))()
            assert nfe == 7
        return torch.cat([o.reshape(-1) for o in out]).cpu()

    seeded = run(noise_frames=geom)
    replayed = run(model_noise(frames, streams, geom, range(ndraws)))
    control = run(model_noise(frames, streams, None, range(ndraws)))
    err, ctl = rel_l2(replayed, seeded), rel_l2(control, seeded)
    print(f"noise geometry, {case} {layout} on {dev} (use_graph={use_graph}): seeded under {geom} vs replayed model noise at those indices "
          f"rel_l2 = {err:.3e} (gate {SAMPLER_TOL:.0e}); control, the model's noise at the default indices: {ctl:.3e} (must exceed "
          f"{100 * SAMPLER_TOL:.0e})")
    assert torch.isfinite(torch.view_as_real(seeded)).all()
    assert err < SAMPLER_TOL, (case, layout, err)
    assert ctl > 100.0 * SAMPLER_TOL, (case, layout, ctl)


# ----------------------------------------------------------------------------------------------------------------------------
# 5. without context the windowed run IS the whole run

def const_models(dev):
    """(OUVE model, Schroedinger-bridge model, N = 2) on long_recording_checks' F = 64 front end with output_layer.weight = 0: the
    network's output is a constant for every element, whatever x, y, t and the number of frames are."""
    def make():
        ms = (make_model(_small_cfg(), dev, **L.FRONT)[0],
              make_model(_small_cfg("ncsnpp_v2"), dev, sde="sbve", k=2.6, c=0.4, N=2, loss_type="data_prediction", **L.FRONT)[0])
        for m in ms:
            with torch.no_grad():
                m.dnn.output_layer.weight.zero_()
            m.dnn.mark_weights_changed()
            assert float(m.dnn.output_layer.bias.detach().abs().min()) > 0
        return ms
    return L._memo(("const_models", str(dev)), make)


def check_windowed_equals_whole(dev, kind):
    """A recording of 255 hops (256 frames, plan [0, 96, 192] x [128, 128, 64]) on the constant-score model, PC reverse_diffusion + ald
    with N = 2 ('pc') or the Schroedinger-bridge 'sde' sampler on the constant-estimate model ('sb'):
    enhance_long(window_noise="recording") is torch.equal to enhance_batch([y], streams=[stream]) of the whole recording.  256 frames
    need no padding, so both runs index the noise with f * 256 + k; every step is element-wise in (y, noise), so the two windows over a
    frame hold the same bits there and the cross-fade fmaf(w, b - a, a) of b = a is a.  With window_noise="window" the two differ.
    Measured, samples differing of 8160, 'pc' and 'sb', emulator and MI355X: 'recording' 0, 'window' 8160.  (On MI355X 5209 differed in
    'recording' mode while enhance_long divided the recording by its peak as a Python number -- torch multiplies by the reciprocal
    there -- where enhance_batch divides by a tensor; the windows themselves were equal to the whole run's frames throughout.)"""
    m = const_models(dev)[0 if kind == "pc" else 1]
    kw = L.PC if kind == "pc" else dict(sampler_type="sde")
    y, stream = L.wave(L_WHOLE), L.STREAM_HI
    whole, _ = m.enhance_batch([y], seed=SEED, streams=[stream], **kw)
    x, info = m.enhance_long(y, L.W, L.O, seed=SEED, stream=stream, window_noise="recording", **kw)
    assert info["starts"] == [0, 96, 192] and info["frames"] == [128, 128, 64]
    n = int((x != whole[0]).sum())
    xw, _ = m.enhance_long(y, L.W, L.O, seed=SEED, stream=stream, window_noise="window", **kw)
    nw = int((xw != whole[0]).sum())
    print(f"windowed vs whole run, {kind} on {dev}: samples differing of {x.numel()}: window_noise='recording' {n}, 'window' {nw}")
    assert x.shape == whole[0].shape == (L_WHOLE,) and torch.isfinite(x).all() and float(x.abs().max()) > 0
    assert n == 0
    assert nw > x.numel() // 2


# ----------------------------------------------------------------------------------------------------------------------------
# 6. batch-size independence, 10. how much the windows of the real network agree over their overlaps

def recording_run(dev, m, batch_size=2, use_graph=True):
    """enhance_long(window_noise="recording", return_windows=True) of long_recording_checks' 250-frame recording, once per argument set."""
    return L._memo(("long_rec", str(dev), batch_size, use_graph), lambda: m.enhance_long(
        L.wave(L.L_LONG), L.W, L.O, batch_size=batch_size, seed=SEED, stream=3, return_windows=True, use_graph=use_graph,
        window_noise="recording", **L.PC))


def check_batch_size_independence(dev, graphs=(True,)):
    """As long_recording_checks.check_batch_size_independence, in recording mode: batch_size 1 (three calls), 2 (a uniform call and the
    last window alone) and 3 (one ragged call) give torch.equal waveforms; on the GPU also with and without the captured step."""
    m = L.models(dev)[0]
    base = recording_run(dev, m, 2)[0]
    for g in graphs:
        for bs in (1, 2, 3):
            x, info = recording_run(dev, m, bs, g)
            assert len(info["nfe"]) == {1: 3, 2: 2, 3: 1}[bs]
            n = int((x != base).sum())
            print(f"enhance_long window_noise='recording' batch_size {bs} use_graph={g} on {dev}: samples differing from batch_size 2 = {n}")
            assert n == 0
    assert not torch.equal(base, L.long_run(dev, m, "pc", batch_size=2)[0])


def check_overlap_agreement(dev):
    """Reported, not gated: on the real nf = 32 network and the 250-frame recording (plan [0, 96, 186] x [128, 128, 64], PC
    reverse_diffusion + ald, N = 2), the relative L2 ||a - b|| / ||a|| between the two neighbouring windows' enhanced values (transformed
    domain) over the frames they share, per overlap, in both modes.  Nothing predicts how much of the agreement the network's dependence
    on context leaves, so no threshold: the figures go to DESIGN 7c.
    Measured (overlap 0/1: 32 frames, 1/2: 38 frames), emulator and MI355X alike: 'window' 1.340, 1.323; 'recording' 0.730, 0.698."""
    m = L.models(dev)[0]
    runs = {"window": L.long_run(dev, m, "pc", batch_size=2), "recording": recording_run(dev, m, 2)}
    for mode, (x, info) in runs.items():
        figs = []
        for i in range(len(info["starts"]) - 1):
            a0, a1, T0 = info["starts"][i], info["starts"][i + 1], info["frames"][i]
            n = a0 + T0 - a1
            a, b = info["windows"][i][:, a1 - a0:a1 - a0 + n].cpu(), info["windows"][i + 1][:, :n].cpu()
            figs.append((n, rel_l2(b, a)))
        print(f"overlap disagreement on {dev}, window_noise='{mode}': " + ", ".join(f"{n} frames rel_l2 {v:.3e}" for n, v in figs))
        assert all(np.isfinite(v) for _, v in figs) and torch.isfinite(x).all()


# ----------------------------------------------------------------------------------------------------------------------------
# 7. one captured step serves every geometry

def check_no_new_capture(dev, m):
    """Two seeded PC calls of one shape under two geometries replay ONE captured step: sgmse_graph_captures does not move between them
    (the geometry is device data behind the stream ids), nor for a call without a geometry; the samples differ."""
    ctx = m.dnn.engine(torch.device(dev))
    y = _inputs(dev, (2, 64))
    run = lambda g: m.get_pc_sampler("reverse_diffusion", "ald", y, N=N_STEPS, snr=0.5, seed=SEED, streams=[3, 3], use_graph=True, noise_frames=g)()[0]
    a = run([(0, 200), (136, 200)])
    n0 = ctx.graph_captures()
    b = run([(7, 300), (96, 300)])
    c = run(None)
    assert n0 >= 1 and ctx.graph_captures() == n0, (n0, ctx.graph_captures())
    assert not torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(b, c)


# ----------------------------------------------------------------------------------------------------------------------------
# 8. refusals

def check_refusals(dev, m, tmp_path):
    """Each a ValueError from the host layer, the context usable afterwards and nothing of the refused call left behind: a window that
    ends behind its recording, a negative first frame (the messages name the utterance), a geometry together with replayed noise (at
    the host layer and at the C boundary), an unknown window_noise, --window_noise without --window_frames."""
    from sgmse_amd import enhancement as E
    ctx = m.dnn.engine(torch.device(dev))
    base = prior_z(m, dev, (2, 64), [4, 5])
    usable = lambda: all(np.array_equal(a, b) for a, b in zip(prior_z(m, dev, (2, 64)), prior_z(m, dev, (2, 64), [0, 1]))) and \
        all(np.array_equal(a, b) for a, b in zip(prior_z(m, dev, (2, 64), [4, 5]), base))
    with pytest.raises(ValueError, match="utterance 1"):
        prior_z(m, dev, (2, 64), [4, 5], [(0, 64), (137, 200)])          # 137 + 64 > 200
    assert usable()
    with pytest.raises(ValueError, match="utterance 0"):
        prior_z(m, dev, [64, 128], [4, 5], [(-1, 333), (205, 333)])
    assert usable()
    prior_z(m, dev, [64, 128], [4, 5], [(0, 64), (205, 333)])            # (the ends themselves are inside)
    Z = torch.zeros(1, 2, 1, F_, 64, dtype=torch.complex64, device=dev)
    sampler = lambda **kw: m.get_pc_sampler("none", "none", _zeros(dev, (2, 64)), N=1, denoise=False, noise=Z, **kw)()
    with pytest.raises(ValueError, match="replayed noise"):
        sampler(noise_frames=UNIFORM[1])
    _raw_set_noise_frames(ctx, UNIFORM[1])
    with pytest.raises(ValueError, match="replayed noise"):
        sampler()
    assert float(sampler()[0].abs().max()) == 0.0 and usable()
    with pytest.raises(ValueError, match="noise_frames"):
        prior_z(m, dev, (2, 64), None, [(0, 64)])                        # one entry for two utterances
    fm = L.models(dev)[0]
    with pytest.raises(ValueError, match="window_noise"):
        fm.enhance_long(L.wave(L.L_LONG), L.W, L.O, seed=SEED, window_noise="frame", **L.PC)
    with pytest.raises(ValueError, match="window_frames"):
        E.main(["--test_dir", str(tmp_path), "--enhanced_dir", str(tmp_path / "out"), "--ckpt", str(tmp_path / "none.ckpt"), "--device", str(dev),
                "--window_noise", "recording"])
    assert usable()


# ----------------------------------------------------------------------------------------------------------------------------
# 9. directory job

def check_directory_job(dev, tmp_path):
    """python -m sgmse_amd.enhancement --window_frames 128 --window_overlap 32 --window_noise recording --seed 7 --N 1 on
    long_recording_checks.check_directory_job's two files: the 250-frame file holds the samples of enhance_long(window_noise="recording",
    stream = its index in the file list); --batch_size 1 and 3 write identical bytes; the file differs from the one --window_noise
    window writes (which is the one written without the switch); the 101-frame file is byte-equal in both modes."""
    from scipy.io import wavfile
    from sgmse_amd import enhancement as E
    from sgmse_amd.data_module import SpecsDataModule
    from sgmse_amd.model import ScoreModel
    cfg = _small_cfg()
    hp = dict(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30, data_module_cls=SpecsDataModule,
              spec_factor=0.15, spec_abs_exponent=0.5, t_eps=0.03, nf=cfg.nf, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks,
              attn_resolutions=cfg.attn_resolutions, image_size=cfg.image_size, progressive=cfg.progressive,
              progressive_input=cfg.progressive_input, **L.FRONT)
    src = ScoreModel(**hp)
    src.dnn.load_state_dict(synth.synth_params(cfg, seed=0))
    ckpt = tmp_path / "m.ckpt"
    torch.save({"state_dict": {"dnn." + k: v.clone() for k, v in src.dnn.state_dict().items()}, "hyper_parameters": hp}, ckpt)
    noisy = tmp_path / "noisy"
    noisy.mkdir()
    for name, n in {"a_short.wav": L.L_SHORT, "b_long.wav": L.L_LONG}.items():
        wavfile.write(str(noisy / name), 16000, L.wave(n).numpy())
    base = ["--test_dir", str(noisy), "--ckpt", str(ckpt), "--device", str(dev), "--N", "1", "--seed", "7", "--window_frames", str(L.W),
            "--window_overlap", str(L.O)]
    rec = ["--window_noise", "recording"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # checkpoint without EMA weights
        assert E.main(base + ["--enhanced_dir", str(tmp_path / "dflt"), "--batch_size", "1"]) == 2
        assert E.main(base + ["--window_noise", "window", "--enhanced_dir", str(tmp_path / "win"), "--batch_size", "1"]) == 2
        assert E.main(base + rec + ["--enhanced_dir", str(tmp_path / "r1"), "--batch_size", "1"]) == 2
        assert E.main(base + rec + ["--enhanced_dir", str(tmp_path / "r3"), "--batch_size", "3"]) == 2
        m = ScoreModel.load_from_checkpoint(str(ckpt), map_location=dev)
    m.eval()
    m.to(dev)
    raw = lambda d, name: open(str(tmp_path / d / name), "rb").read()
    assert raw("win", "a_short.wav") == raw("r1", "a_short.wav") == raw("r3", "a_short.wav")
    assert raw("r1", "b_long.wav") == raw("r3", "b_long.wav")
    assert raw("dflt", "b_long.wav") == raw("win", "b_long.wav") != raw("r1", "b_long.wav")
    y = torch.from_numpy(E.read_audio(str(noisy / "b_long.wav"))[0])
    x, info = m.enhance_long(y, L.W, L.O, batch_size=2, seed=7, stream=1, N=1, window_noise="recording")
    _, got = wavfile.read(str(tmp_path / "r1" / "b_long.wav"))
    assert info["frames"] == [128, 128, 64] and got.shape == (L.L_LONG,) and np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, x.cpu().numpy())
