"""Checks of the windowed enhancement of long recordings: sgmse_spec_split / sgmse_spec_merge (kernels_stft.h), ScoreModel.enhance_long
and ``python -m sgmse_amd.enhancement --window_frames``.  Shared by the emulator and the GPU modules.

Everything runs on the nf = 32 network of ode_native_checks._small_cfg with n_fft = 126, hop_length = 32 (F = 64), windows of W = 128
frames overlapping by O = 32, N = 2 sampler steps, seeded.  The long recording has 250 frames (plan [0, 96, 186] x [128, 128, 64]: two
full windows and a shorter last one pulled left), the short one 101.  Recordings and enhance_long results are computed once per
(device, model, arguments) and shared between the checks."""
import warnings

import numpy as np
import pytest
import torch

import sampler_noise_checks as K
from ode_native_checks import _small_cfg
from oracle import synth
from parity import make_model
from sgmse_amd import ops
from sgmse_amd.util.windows import plan_windows, window_stream

W, O = 128, 32
HOP, NFFT = 32, 126
FRONT = dict(n_fft=NFFT, hop_length=HOP)
L_LONG, L_SHORT = 249 * HOP, 100 * HOP          # 250 and 101 frames
SEED = K.SEED
STREAM_HI = 2 ** 31 + 9                         # a recording id above 2^31
XF = ("exponent", "log", "none")
PC = dict(N=2, snr=0.5, corrector="ald", predictor="reverse_diffusion", sampler_type="pc")

_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def models(dev):
    """(OUVE model, Schroedinger-bridge model) on the F = 64 front end."""
    return _memo(("models", str(dev)), lambda: (
        make_model(_small_cfg(), dev, **FRONT)[0],
        make_model(_small_cfg("ncsnpp_v2"), dev, sde="sbve", k=2.6, c=0.4, N=2, loss_type="data_prediction", **FRONT)[0]))


def wave(L):
    return _memo(("wave", L), lambda: 0.1 * synth.synth_waveform(L, seed=11 + L % 7)[0])


def long_run(dev, m, kind, batch_size=2, stream=3, use_graph=True):
    """enhance_long of the 250-frame recording (return_windows=True), once per argument set."""
    kw = PC if kind == "pc" else {}
    return _memo(("long", str(dev), kind, batch_size, stream, use_graph), lambda: m.enhance_long(
        wave(L_LONG), W, O, batch_size=batch_size, seed=SEED, stream=stream, return_windows=True, use_graph=use_graph, **kw))


def _rand_spec(F_, T, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(F_, T, generator=g), torch.randn(F_, T, generator=g)).mul(0.25).to(dev)


# ----------------------------------------------------------------------------------------------------------------------------
# 2. split

def check_split(dev, F_, Kf):
    """Every window of ops.spec_split is torch.equal to the slice [:, a : a + T] of ops.spec_transform (spec_fwd) of the whole
    spectrogram, for the three transform types; the windows are views of one packed buffer.
    Measured: 0 differing elements, emulator and MI355X, (F, K) = (3, 203) and (64, 250)."""
    S = _rand_spec(F_, Kf, 5, dev)
    starts, frames = plan_windows(Kf, W, O)
    assert len(starts) > 1
    for tt in XF:
        wins = ops.spec_split(S, starts, frames, tt, 0.15, 0.5)
        ref = ops.spec_transform(S, tt, 0.15, 0.5, inverse=False)
        assert [tuple(w.shape) for w in wins] == [(F_, T) for T in frames]
        bad = [int((w != ref[:, a:a + T]).sum()) for w, a, T in zip(wins, starts, frames)]
        print(f"split {tt} F={F_} K={Kf} on {dev}: plan {starts} x {frames}, elements differing from the slices of spec_fwd = {bad}")
        assert bad == [0] * len(starts)
        assert wins[1].data_ptr() == wins[0].data_ptr() + 8 * F_ * frames[0]


# ----------------------------------------------------------------------------------------------------------------------------
# 3. merge

def check_merge_roundtrip(dev, F_, Kf):
    """Split then merge with transform 'none' returns the input bit for bit (in an overlap b - a = 0 and fmaf(w, 0, a) = a).
    Measured: torch.equal on the emulator and on MI355X."""
    S = _rand_spec(F_, Kf, 6, dev)
    starts, frames = plan_windows(Kf, W, O)
    back = ops.spec_merge(ops.spec_split(S, starts, frames, "none", 1.0, 1.0), starts, frames, Kf, "none", 1.0, 1.0)
    assert back.shape == S.shape and torch.equal(back, S)


def check_merge_blend(dev, F_, Kf, tt):
    """Independent random windows.  A frame under one window is torch.equal to ops.spec_transform(inverse=True) of that window; a
    frame under two is compared with an fp64 host blend a + w (b - a), w = (k - start[j+1] + 0.5) / O_j, of the existing op's two
    outputs a, b: per real component |out - ref| <= 2^-21 max(|a|, |b|).  The bound is derived: the rounding of w (one division,
    2^-24 relative, times |b - a| <= 2 max), of b - a (2^-24 |b - a| <= 2^-23 max) and of the fma (2^-24 |out| <= 2^-24 max) add up to
    (2^-23 + 2^-23 + 2^-24) max < 2^-21 max.
    Measured, largest |out - ref| / max(|a|, |b|) in units of 2^-21 (the bound is 1), exponent / log / none: (F, K) = (3, 203) emulator
    0.357 / 0.212 / 0.264, MI355X 0.357 / 0.201 / 0.264; (64, 250) emulator and MI355X 0.327 / 0.389 / 0.288; frames under one window: 0
    elements differing from spec_back everywhere."""
    starts, frames = plan_windows(Kf, W, O)
    wins = [_rand_spec(F_, T, 20 + i, dev) for i, T in enumerate(frames)]
    out = torch.view_as_real(ops.spec_merge(wins, starts, frames, Kf, tt, 0.15, 0.5).cpu())
    backs = [torch.view_as_real(ops.spec_transform(w, tt, 0.15, 0.5, inverse=True).cpu()) for w in wins]
    cover = [[j for j, (a, T) in enumerate(zip(starts, frames)) if a <= k < a + T] for k in range(Kf)]
    assert all(1 <= len(c) <= 2 for c in cover) and any(len(c) == 2 for c in cover)
    worst, nbad = 0.0, 0
    for k, c in enumerate(cover):
        if len(c) == 1:
            nbad += int((out[:, k] != backs[c[0]][:, k - starts[c[0]]]).sum())
            continue
        i, j = c
        assert j == i + 1
        a, b = backs[i][:, k - starts[i]].double(), backs[j][:, k - starts[j]].double()
        w = (k - starts[j] + 0.5) / (starts[i] + frames[i] - starts[j])
        ref = a + w * (b - a)
        scale = torch.maximum(a.abs(), b.abs())
        err = (out[:, k].double() - ref).abs()
        ok = scale > 0
        worst = max(worst, float((err[ok] / scale[ok]).max()))
        assert bool((err <= 2.0 ** -21 * scale).all()), (k, float((err / scale.clamp_min(1e-300)).max()))
    print(f"merge {tt} F={F_} K={Kf} on {dev}: elements under one window differing from spec_back = {nbad}; largest blend error / "
          f"max(|a|,|b|) = {worst / 2.0 ** -21:.3f} x 2^-21")
    assert nbad == 0


BAD_PLANS = {"starts not increasing": ([0, 0], [100, 200]),
             "outside": ([0, 100], [128, 128]),
             "gap": ([0, 130], [128, 70]),
             "three windows": ([0, 50, 90], [100, 100, 110])}


def check_merge_refusals(dev):
    """The four refused plans over K = 200 frames (SGMSE_EINVAL) surface as ValueError from both ops; a valid plan afterwards works."""
    F_, Kf = 3, 200
    S = _rand_spec(F_, Kf, 7, dev)
    for name, (starts, frames) in BAD_PLANS.items():
        with pytest.raises(ValueError, match="invalid argument"):
            ops.spec_split(S, starts, frames, "none", 1.0, 1.0)
        with pytest.raises(ValueError, match="invalid argument"):
            ops.spec_merge(torch.zeros(F_ * sum(frames), dtype=torch.complex64, device=dev), starts, frames, Kf, "none", 1.0, 1.0)
    starts, frames = plan_windows(Kf, W, O)
    assert torch.equal(ops.spec_merge(ops.spec_split(S, starts, frames, "none", 1.0, 1.0), starts, frames, Kf, "none", 1.0, 1.0), S)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. a window is its own run

def check_window_equals_own_run(dev, kind, stream):
    """enhance_long(return_windows=True) of the 250-frame recording, PC sampler (reverse_diffusion + ald, N = 2) or the
    Schroedinger-bridge model: window i is torch.equal to the sampler called alone on spec_fwd(S)[:, a_i : a_i + T_i] with the same
    seed and the stream id stream + (i << 32).
    Measured: 0 differing elements in every window, emulator and MI355X, both samplers, stream 3 and 2^31 + 9."""
    m = models(dev)[0 if kind == "pc" else 1]
    x, info = long_run(dev, m, kind, stream=stream)
    assert info["starts"] == [0, 96, 186] and info["frames"] == [128, 128, 64] and x.shape == (L_LONG,)
    y = wave(L_LONG).reshape(1, -1).to(dev)
    Sf = m._forward_transform(m._stft(y / float(y.abs().max()))[0])
    bad = []
    for i, (a, T) in enumerate(zip(info["starts"], info["frames"])):
        Y = Sf[:, a:a + T].contiguous()[None, None]
        sid = [window_stream(stream, i)]
        if kind == "pc":
            alone = m.get_pc_sampler("reverse_diffusion", "ald", Y, N=2, corrector_steps=1, snr=0.5, seed=SEED, streams=sid)()[0]
        else:
            alone = m.get_sb_sampler(m.sde, Y, sampler_type="ode", seed=SEED, streams=sid)()[0]
        bad.append(int((alone[0, 0] != info["windows"][i]).sum()))
    print(f"enhance_long {kind} stream {stream} on {dev}: elements of each window differing from its own run = {bad}")
    assert bad == [0, 0, 0]
    assert all(torch.isfinite(torch.view_as_real(w)).all() for w in info["windows"]) and torch.isfinite(x).all() and float(x.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------------
# 5. batch-size independence, 6. composition

def check_batch_size_independence(dev, graphs=(True,)):
    """The 250-frame recording with batch_size 1 (three calls), 2 (a uniform call of two and the last window alone) and 3 (ONE ragged
    call [128, 128, 64]) gives torch.equal waveforms; on the GPU also with and without the captured step.
    Measured: 0 differing samples, emulator and MI355X."""
    m = models(dev)[0]
    base = long_run(dev, m, "pc", batch_size=2)[0]
    for g in graphs:
        for bs in (1, 2, 3):
            x, info = long_run(dev, m, "pc", batch_size=bs, use_graph=g)
            assert len(info["nfe"]) == {1: 3, 2: 2, 3: 1}[bs]
            n = int((x != base).sum())
            print(f"enhance_long batch_size {bs} use_graph={g} on {dev}: samples differing from batch_size 2 = {n}")
            assert n == 0


def check_composition(dev, kind):
    """The returned waveform is torch.equal to istft(merge_windows(returned windows)) * peak built from the public pieces.
    Measured: equal on the emulator (pc) and on MI355X (pc, sb)."""
    m = models(dev)[0 if kind == "pc" else 1]
    x, info = long_run(dev, m, kind)
    peak = float(wave(L_LONG).abs().max())
    X = m.data_module.merge_windows(info["windows"], info["starts"], info["frames"], L_LONG // HOP + 1)
    assert torch.equal(x, m._istft(X, L_LONG) * peak)


# ----------------------------------------------------------------------------------------------------------------------------
# 7. short input

def check_short_input(dev, kind):
    """A recording of 101 frames (K <= W) through enhance_long is torch.equal to enhance_batch([y], seed=..., streams=[stream])."""
    m = models(dev)[0 if kind == "pc" else 1]
    kw = PC if kind == "pc" else {}
    y = wave(L_SHORT)
    x, info = m.enhance_long(y, W, O, seed=SEED, stream=STREAM_HI, return_windows=True, **kw)
    ref, nfe = m.enhance_batch([y], seed=SEED, streams=[STREAM_HI], **kw)
    assert info["starts"] == [0] and info["frames"] == [101] and info["nfe"] == [nfe] and info["windows"] is None
    assert x.shape == (L_SHORT,) and torch.equal(x, ref[0])


# ----------------------------------------------------------------------------------------------------------------------------
# 8. refusals

COUPLED = {"langevin": dict(sampler_type="pc", corrector="langevin", N=1, snr=0.5),
           "ode_scipy": dict(sampler_type="ode", adaptive=True, rtol=0.5, atol=0.5),
           "ode_native_batch": dict(sampler_type="ode", adaptive=True, solver="native", rtol=0.5, atol=0.5)}
ALTERNATIVE = {"langevin": "corrector_scope='utterance'", "ode_scipy": "step_control='utterance'", "ode_native_batch": "step_control='utterance'"}


def check_refusal(dev, case):
    """A configuration that couples the utterances of a batch raises ValueError (naming the per-utterance alternative) on the
    250-frame recording, before anything runs, and is accepted on the 101-frame one (rtol = atol = 0.5 keeps the solvers short)."""
    m = models(dev)[0]
    with pytest.raises(ValueError, match=ALTERNATIVE[case]):
        m.enhance_long(wave(L_LONG), W, O, seed=SEED, **COUPLED[case])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # scipy's solver: seed / streams do not apply
        x, info = m.enhance_long(wave(L_SHORT), W, O, seed=SEED, **COUPLED[case])
    assert x.shape == (L_SHORT,) and torch.isfinite(x).all() and info["frames"] == [101]


# ----------------------------------------------------------------------------------------------------------------------------
# 9. directory job

def check_directory_job(dev, tmp_path):
    """python -m sgmse_amd.enhancement --window_frames 128 --window_overlap 32 --seed 7 --N 1 on a 101-frame and a 250-frame file (a
    temporary checkpoint of the small model): the short file equals, byte for byte, the one written without --window_frames; the long
    file equals ScoreModel.enhance_long with stream = its index in the file list; --batch_size 1 and 3 write identical files; without
    the switch the long file is a different one (the windows are real).
    Measured: all comparisons byte-equal / 0 differing samples on the emulator and on MI355X."""
    from scipy.io import wavfile
    from sgmse_amd import enhancement as E
    from sgmse_amd.data_module import SpecsDataModule
    from sgmse_amd.model import ScoreModel
    cfg = _small_cfg()
    hp = dict(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30, data_module_cls=SpecsDataModule,
              spec_factor=0.15, spec_abs_exponent=0.5, t_eps=0.03, nf=cfg.nf, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks,
              attn_resolutions=cfg.attn_resolutions, image_size=cfg.image_size, progressive=cfg.progressive,
              progressive_input=cfg.progressive_input, **FRONT)
    src = ScoreModel(**hp)
    src.dnn.load_state_dict(synth.synth_params(cfg, seed=0))
    ckpt = tmp_path / "m.ckpt"
    torch.save({"state_dict": {"dnn." + k: v.clone() for k, v in src.dnn.state_dict().items()}, "hyper_parameters": hp}, ckpt)
    noisy = tmp_path / "noisy"
    noisy.mkdir()
    lengths = {"a_short.wav": L_SHORT, "b_long.wav": L_LONG}
    for name, L in lengths.items():
        wavfile.write(str(noisy / name), 16000, wave(L).numpy())
    base = ["--test_dir", str(noisy), "--ckpt", str(ckpt), "--device", str(dev), "--N", "1", "--seed", "7"]
    win = ["--window_frames", str(W), "--window_overlap", str(O)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # checkpoint without EMA weights
        assert E.main(base + ["--enhanced_dir", str(tmp_path / "plain"), "--batch_size", "1"]) == 2
        assert E.main(base + win + ["--enhanced_dir", str(tmp_path / "w1"), "--batch_size", "1"]) == 2
        assert E.main(base + win + ["--enhanced_dir", str(tmp_path / "w3"), "--batch_size", "3"]) == 2
        m = ScoreModel.load_from_checkpoint(str(ckpt), map_location=dev)
    m.eval()
    m.to(dev)
    raw = lambda d, name: open(str(tmp_path / d / name), "rb").read()
    assert raw("plain", "a_short.wav") == raw("w1", "a_short.wav") == raw("w3", "a_short.wav")
    assert raw("w1", "b_long.wav") == raw("w3", "b_long.wav")
    assert raw("plain", "b_long.wav") != raw("w1", "b_long.wav")
    y = torch.from_numpy(E.read_audio(str(noisy / "b_long.wav"))[0])
    x, info = m.enhance_long(y, W, O, batch_size=2, seed=7, stream=1, N=1)
    _, got = wavfile.read(str(tmp_path / "w1" / "b_long.wav"))
    assert info["frames"] == [128, 128, 64] and got.shape == (L_LONG,) and np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, x.cpu().numpy())
