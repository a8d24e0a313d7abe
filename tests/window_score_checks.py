"""Checks of the windowed score of long recordings: ONE reverse process over the recording, only the network evaluated on windows
(sgmse_set_windows, sgmse_window_gather / sgmse_window_blend of kernels_stft.h, ``get_pc_sampler(windows=...)``,
``ScoreModel.enhance_long(window_blend="score")`` and ``python -m sgmse_amd.enhancement --window_blend score``).  Shared by the emulator
and the GPU modules.

Shapes are those of long_recording_checks: the nf = 32 network, F = 64 (n_fft 126, hop 32), windows of W = 128 frames overlapping by
O = 32, at most 256 frames and three windows, PC N <= 2.  Recordings of 240 frames have the uniform plan [0, 96, 112] (frames 112-127
under three windows), 250 frames [0, 96, 122], 256 frames [0, 96, 128].  Runs are computed once per argument set and shared."""
import warnings

import numpy as np
import pytest
import torch

import long_recording_checks as L
import sampler_noise_checks as K
import window_noise_checks as WN
from conftest import rel_l2
from ode_native_checks import _small_cfg
from oracle import synth
from parity import SAMPLER_TOL
from sgmse_amd import _lib, ops
from sgmse_amd.util.windows import plan_windows, plan_windows_uniform

W, O, F_ = L.W, L.O, 64
SEED = L.SEED
L_WHOLE = WN.L_WHOLE                        # 256 frames
f32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the plan

PLAN_CASES = [(k, w, o) for w, o in ((128, 32), (128, 0), (128, 31), (64, 0), (256, 96), (512, 64), (512, 224))
              for k in sorted({1, w - 1, w, w + 1, w + o, 2 * w - o - 1, 2 * w - o, 2 * w - o + 1, 2 * w, 3 * w - 2 * o - 1, 3 * w - 2 * o,
                               3 * w - 2 * o + 1, 3 * w - 2 * o + o // 2, 5 * w + 7, 240, 250, 256, 75001})]


def check_plan(Kf, Wf, Of):
    """plan_windows_uniform over (K, W, O): K <= W gives [0]; otherwise all windows have W frames inside [0, K), the starts strictly
    increase from 0, the windows cover [0, K) (last end = K, no gap), every overlap is at least O, no frame lies under more than three
    windows and the count is plan_windows'."""
    starts = plan_windows_uniform(Kf, Wf, Of)
    ref_starts, _ = plan_windows(Kf, Wf, Of)
    assert len(starts) == len(ref_starts)
    if Kf <= Wf:
        assert starts == [0]
        return
    n = len(starts)
    assert n == -(-(Kf - Of) // (Wf - Of)) and starts[0] == 0 and starts[-1] + Wf == Kf
    assert all(b > a for a, b in zip(starts, starts[1:]))
    assert all(a + Wf - b >= Of for a, b in zip(starts, starts[1:]))                   # every overlap >= O (so no gap)
    assert all(starts[j] >= starts[j - 3] + Wf for j in range(3, n))                    # at most three windows over a frame
    assert starts[:-1] == ref_starts[:-1]


def check_plan_refusals():
    for bad in ((0, 128, 32), (300, 100, 10), (300, 128, 33), (300, 128, -1), (300, 0, 0)):
        with pytest.raises(ValueError):
            plan_windows_uniform(*bad)


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the kernels against a NumPy model

def _rand_windows(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(n, F_, W, generator=g), torch.randn(n, F_, W, generator=g)).mul(0.25).to(dev)


def np_weights(starts, j, t):
    """w_j of sgmse_window_blend at the local frames t (int array), in float32 as the kernel evaluates it."""
    n = len(starts)
    w = np.ones(len(t), f32)
    if j > 0:
        w = np.minimum(w, (t.astype(f32) + f32(0.5)) / f32(starts[j - 1] + W - starts[j]))
    if j < n - 1:
        w = np.minimum(w, ((W - t).astype(f32) - f32(0.5)) / f32(starts[j] + W - starts[j + 1]))
    return w


def np_blend(wins, Kf, starts):
    """The blend of sgmse_window_blend over windows [n, F, W] (complex NumPy): the weights, their sum S (ascending j) and the ratios
    w_j / S in float32, exactly as the kernel has them; the blend a + sum_j (w_j / S)(v_j - a) itself in float64 (what
    long_recording_checks.check_merge_blend does for the fused multiply-adds).  Returns (ref complex128 [F, K], cover: windows per
    frame, scale float64 [F, K, 2]: the largest |real component| among the frame's windows)."""
    wins = np.asarray(wins).astype(np.complex128)
    ref = np.zeros((wins.shape[1], Kf), np.complex128)
    scale = np.zeros((wins.shape[1], Kf, 2))
    cover = []
    for k in range(Kf):
        js = [j for j, a in enumerate(starts) if a <= k < a + W]
        cover.append(js)
        ws = [np_weights(starts, j, np.array([k - starts[j]]))[0] for j in js]
        S = ws[0]
        for w in ws[1:]:
            S = f32(S + w)
        vs = [wins[j][:, k - starts[j]] for j in js]
        out = vs[0].copy()
        for w, v in zip(ws[1:], vs[1:]):
            out = out + float(f32(w / S)) * (v - vs[0])
        ref[:, k] = out
        scale[:, k, 0] = np.max([np.abs(v.real) for v in vs], axis=0)
        scale[:, k, 1] = np.max([np.abs(v.imag) for v in vs], axis=0)
    return ref, cover, scale


def check_kernels(dev, Kf):
    """sgmse_window_gather / sgmse_window_blend on the uniform plan of Kf frames (240: frames 112-127 under three windows; 256).
    gather: torch.equal to slicing.  blend of independent random windows: a frame under one window is torch.equal to that window's
    element; the others against np_blend under check_merge_blend's gate, per real component |out - ref| <= 2^-21 max_j |v_j|: the model
    holds the kernel's own float32 ratios r_j = w_j / S (IEEE operations), so what is left is, per later window, the rounding of
    v_j - a (2^-24 |v_j - a| <= 2^-23 max) and of the fma (2^-24 |out| <= 2^-24 max): 3 x 2^-24 max for two windows, 6 x 2^-24 max
    = 0.75 x 2^-21 max for three.  Windows that agree over their overlaps blend to the common value bit for bit.
    Measured, largest |out - ref| / max_j |v_j| in units of 2^-21 (the bound is 1), emulator and MI355X alike: K = 240 0.295, K = 256
    0.307; 0 elements under one window differing; agreeing windows: torch.equal."""
    starts = plan_windows_uniform(Kf, W, O)
    n = len(starts)
    S = L._rand_spec(F_, Kf, 31, dev)
    g = ops.window_gather(S, W, starts)
    assert g.shape == (n, F_, W) and all(torch.equal(g[j], S[:, a:a + W]) for j, a in enumerate(starts))
    assert torch.equal(ops.window_blend(g, Kf, starts), S)                    # windows that agree: their common value, bit for bit
    wins = _rand_windows(n, 40 + Kf, dev)
    out = ops.window_blend(wins, Kf, starts).cpu()
    ref, cover, scale = np_blend(wins.cpu().numpy(), Kf, starts)
    counts = sorted({len(c) for c in cover})
    assert counts == ([1, 2, 3] if Kf == 240 else [1, 2]), counts
    nbad, worst = 0, 0.0
    got = torch.view_as_real(out).numpy().astype(np.float64)
    want = np.stack([ref.real, ref.imag], axis=-1)
    for k, c in enumerate(cover):
        if len(c) == 1:
            nbad += int((out[:, k] != wins[c[0]][:, k - starts[c[0]]].cpu()).sum())
            continue
        err = np.abs(got[:, k] - want[:, k])
        ok = scale[:, k] > 0
        worst = max(worst, float((err[ok] / scale[:, k][ok]).max()))
        assert bool((err <= 2.0 ** -21 * scale[:, k]).all()), (k, c, float((err / np.maximum(scale[:, k], 1e-300)).max()))
    print(f"window_blend K={Kf} plan {starts} on {dev}: elements under one window differing from the window = {nbad}; largest blend error / "
          f"max|v| = {worst / 2.0 ** -21:.3f} x 2^-21")
    assert nbad == 0
    same = _rand_windows(1, 50, dev)[0, :, :1].expand(F_, W).contiguous()     # every window the same row-constant values
    const = ops.window_blend(same[None].expand(n, F_, W).contiguous(), Kf, starts)
    assert torch.equal(const, same[:, :1].expand(F_, Kf))


BAD_PLANS = {"strictly increasing": (200, [0, 0]), "inside": (200, [0, 100]), "gap": (300, [0, 172]), "four windows": (160, [0, 8, 16, 32])}


def check_kernel_refusals(dev):
    """The refused plans (SGMSE_EINVAL) surface as ValueError from both ops; a valid plan afterwards works."""
    for name, (Kf, starts) in BAD_PLANS.items():
        S = L._rand_spec(3, Kf, 7, dev)
        with pytest.raises(ValueError, match=name):
            ops.window_gather(S, W, starts)
        with pytest.raises(ValueError, match=name):
            ops.window_blend(torch.zeros(len(starts), 3, W, dtype=torch.complex64, device=dev), Kf, starts)
    S = L._rand_spec(3, 240, 7, dev)
    starts = plan_windows_uniform(240, W, O)
    assert torch.equal(ops.window_blend(ops.window_gather(S, W, starts), 240, starts), S)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. one window is the plain run

def _spec(dev, Kf, seed=4):
    return synth.synth_spec(1, F_, Kf, seed=seed).to(dev)


def check_one_window_is_plain(dev, kind):
    """K = W = 128 with the explicit one-window plan (128, [0]) through get_pc_sampler(windows=...) ('pc': reverse_diffusion + ald,
    N = 1) or get_sb_sampler(windows=...) ('sb': the 'sde' sampler, N = 2) is torch.equal to the same call without a plan: the gather is
    a copy, a frame under one window gets that window's score."""
    m = L.models(dev)[0 if kind == "pc" else 1]
    y = _spec(dev, W)

    def run(**kw):
        if kind == "pc":
            return m.get_pc_sampler("reverse_diffusion", "ald", y, N=1, snr=0.5, seed=SEED, streams=[5], **kw)()
        return m.get_sb_sampler(m.sde, y, sampler_type="sde", seed=SEED, streams=[5], **kw)()
    (plain, nfe0), (win, nfe1) = run(), run(windows=(W, [0]), window_batch=1)
    assert nfe0 == nfe1 and plain.shape == win.shape == (1, 1, F_, W)
    assert torch.isfinite(torch.view_as_real(plain)).all() and torch.equal(plain, win)
    assert torch.equal(run()[0], plain)                                       # (and the plan is gone again)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. / 7. without context the windowed score IS the whole score

CONTEXT_FREE = {"pc": L.PC, "sb": dict(sampler_type="sde"),
                "langevin": dict(N=2, snr=0.5, corrector="langevin", predictor="reverse_diffusion", sampler_type="pc")}


def check_context_free(dev, kind):
    """The 256-frame recording (uniform plan [0, 96, 128]) on window_noise_checks' constant-score models: enhance_long(window_blend=
    "score") is torch.equal to the one-spectrogram enhance_batch run with the same seed and stream -- PC reverse_diffusion + ald N = 2
    ('pc'), the Schroedinger-bridge 'sde' sampler ('sb') and the 'langevin' corrector at batch scope ('langevin': refused by
    window_blend="output" for more than one window; the batch is the recording here, so its norms are the whole run's).  Every window's
    score is the constant, the blend of equal values is that value, state and noise are the recording's own.
    Measured: 0 of 8160 samples differ, all three, emulator and MI355X."""
    m = WN.const_models(dev)[1 if kind == "sb" else 0]
    kw = CONTEXT_FREE[kind]
    y, stream = L.wave(L_WHOLE), L.STREAM_HI
    if kind == "langevin":
        with pytest.raises(ValueError, match="corrector_scope='utterance'"):
            m.enhance_long(y, W, O, seed=SEED, stream=stream, **kw)
        whole, nfe = m.enhance_batch(y[None], seed=SEED, streams=[stream], **kw)
    else:
        whole, nfe = m.enhance_batch([y], seed=SEED, streams=[stream], **kw)
    x, info = m.enhance_long(y, W, O, batch_size=2, seed=SEED, stream=stream, window_blend="score", **kw)
    assert info["starts"] == [0, 96, 128] and info["frames"] == [W] * 3 and info["nfe"] == [nfe]
    n = int((x != whole[0]).sum())
    print(f"window_blend='score' vs the whole run, context-free {kind} on {dev}: samples differing of {x.numel()} = {n}")
    assert x.shape == whole[0].shape == (L_WHOLE,) and torch.isfinite(x).all() and float(x.abs().max()) > 0
    assert n == 0


# ----------------------------------------------------------------------------------------------------------------------------
# 5. chunking never matters

def score_run(dev, m, batch_size=2, use_graph=True, seed=SEED):
    """enhance_long(window_blend="score") of the 250-frame recording on the real network, once per argument set."""
    return L._memo(("score_run", str(dev), batch_size, use_graph, seed), lambda: m.enhance_long(
        L.wave(L.L_LONG), W, O, batch_size=batch_size, seed=seed, stream=3, use_graph=use_graph, window_blend="score", **L.PC))


def check_chunking(dev, graphs=(True,)):
    """The 250-frame recording (plan [0, 96, 122]) on the real random-init network with batch_size 1 (three chunks of one window), 2
    (two chunks of two: the last one's second slot is a filler that evaluates window 2 again) and 3 (one chunk) gives torch.equal
    waveforms, with and without the captured step.  A second recording under one plan does not capture again: captures + in-place
    updates grow by exactly one over two runs of batch_size 2 (N = 2 steps, four evaluations of two chunks each).
    Measured: 0 differing samples, emulator and MI355X; one capture."""
    m = L.models(dev)[0]
    ctx = m.dnn.engine(torch.device(dev))
    captured = lambda: ctx.graph_captures() + ctx.graph_updates()
    c0 = captured()
    base, info = score_run(dev, m, 2)
    c1 = captured()
    other = score_run(dev, m, 2, seed=SEED + 1)[0]
    assert captured() == c1 and c1 - c0 == (0 if _lib.is_emulator() else 1), (c0, c1, captured())
    assert info["starts"] == [0, 96, 122] and info["nfe"] == [4] and not torch.equal(other, base)
    assert torch.isfinite(base).all() and float(base.abs().max()) > 0
    for g in graphs:
        for bs in (1, 2, 3):
            x, _ = score_run(dev, m, bs, g)
            n = int((x != base).sum())
            print(f"window_blend='score' batch_size {bs} use_graph={g} on {dev}: samples differing from batch_size 2 = {n}")
            assert n == 0
    assert not torch.equal(base, L.long_run(dev, m, "pc", batch_size=2)[0])   # (and it is not the cross-faded windows)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. wiring against a host composition

def check_wiring(dev):
    """One predictor step ('reverse_diffusion' / 'none', N = 1, denoise=False, replayed noise) on a 240-frame spectrogram under the plan
    [0, 96, 112], window_batch 2 (a filler slot), against the composition of public pieces: x0 = y + std(1) z0; the score of each of its
    windows from the model's own forward (ncsnpp_forward + the score wrapper), one window at a time; np_blend of the three; the
    predictor update of sampler_noise_checks._pc_chain in float64 with the blended score.  Relative L2 <= parity.SAMPLER_TOL, the
    project's sampler gate.  A wrong gather offset, a filler's score in the blend or y taken from the wrong window gives O(1).
    Measured: emulator 5.1e-8 (its fp32 arithmetic is the host's), MI355X 1.1e-6."""
    m = L.models(dev)[0]
    Kf = 240
    starts = plan_windows_uniform(Kf, W, O)
    y = _spec(dev, Kf, seed=9)
    g = torch.Generator().manual_seed(12)
    Z = torch.complex(torch.randn(2, 1, 1, F_, Kf, generator=g), torch.randn(2, 1, 1, F_, Kf, generator=g)).mul(0.5 ** 0.5).to(dev)
    out, nfe = m.get_pc_sampler("reverse_diffusion", "none", y, N=1, snr=0.5, denoise=False, noise=Z, windows=(W, starts), window_batch=2)()
    assert nfe == 1 and out.shape == (1, 1, F_, Kf)
    sde = m.sde.copy()
    sde.N = 1
    tab = sde.step_table(m.t_eps, 0.5, 1)
    x0 = y + K._std1(m) * Z[0]
    t = tab["t"][:1].to(dev)
    with torch.no_grad():
        scores = [m(x0[..., a:a + W].contiguous(), y[..., a:a + W].contiguous(), t)[0, 0].cpu().numpy() for a in starts]
    score = np_blend(np.stack(scores), Kf, starts)[0]
    d = lambda v: v.cpu().numpy().astype(np.complex128).reshape(F_, Kf)
    sc = lambda v: float(torch.as_tensor(v, dtype=torch.float32))
    yd, xd = d(y), d(x0)
    f = (sc(sde.theta) * (yd - xd)) * sc(tab["dt"][0]) - sc(tab["G2"][0]) * score
    ref = (xd - f) + sc(tab["G"][0]) * d(Z[1])
    err = rel_l2(d(out), ref)
    ctl = rel_l2(d(out), xd)
    print(f"windowed predictor step on {dev}: rel_l2 vs the host composition = {err:.3e} (gate {SAMPLER_TOL:.0e}); the step itself moved "
          f"the state by {ctl:.3e}")
    assert err <= SAMPLER_TOL and ctl > 100.0 * SAMPLER_TOL


# ----------------------------------------------------------------------------------------------------------------------------
# 8. refusals

def check_refusals(dev):
    """Each a ValueError, the context usable afterwards and no plan left behind: a plan with a ragged context, with a pending noise
    geometry, with B != 1, with T != K; W not a multiple of 2^(levels-1) = 64; starts that do not increase, a window outside [0, K), a
    gap, window_batch < 1; the adaptive solver (both step controls) with a plan in force ("not supported"); and from the host layer an
    unknown window_blend, windows= on a configuration that runs the Python loop and on the adaptive ODE sampler."""
    m = L.models(dev)[0]
    ctx = m.dnn.engine(torch.device(dev))
    Kf = 256
    starts = plan_windows_uniform(Kf, W, O)
    zeros = lambda B, T: torch.zeros(B, 1, F_, T, dtype=torch.complex64, device=dev)
    prior = lambda Y, **kw: m.get_pc_sampler("none", "none", Y, N=1, denoise=False, seed=SEED, **kw)()[0]
    plain = prior(zeros(1, Kf))
    usable = lambda: ctx._windows is None and torch.equal(prior(zeros(1, Kf)), plain)
    # the recording's own field: the plan changes nothing in a run that evaluates no network
    assert torch.equal(prior(zeros(1, Kf), windows=(W, starts), window_batch=2), plain) and usable()
    cases = [("exclude each other", lambda: prior([zeros(1, Kf)[0]], windows=(W, starts))),
             ("noise geometry", lambda: prior(zeros(1, Kf), windows=(W, starts), noise_frames=[(0, Kf)])),
             ("B must be 1", lambda: prior(zeros(2, Kf), windows=(W, starts))),
             ("not the window plan's K", lambda: prior(zeros(1, 192), windows=(W, starts))),
             ("multiple of", lambda: prior(zeros(1, 160), windows=(96, [0, 64]))),
             ("strictly increasing", lambda: prior(zeros(1, Kf), windows=(W, [0, 96, 96]))),
             ("inside", lambda: prior(zeros(1, Kf), windows=(W, [0, -5, 128]))),
             ("gap", lambda: prior(zeros(1, 384), windows=(W, [0, 256]))),
             ("max_batch", lambda: prior(zeros(1, Kf), windows=(W, starts), window_batch=0))]
    for what, call in cases:
        with pytest.raises(ValueError, match=what):
            call()
        assert usable(), what
    sb = L.models(dev)[1]
    with pytest.raises(ValueError, match="B must be 1"):
        sb.get_sb_sampler(sb.sde, zeros(2, Kf), sampler_type="ode", seed=SEED, windows=(W, starts))()
    assert sb.dnn.engine(torch.device(dev))._windows is None
    ode = dict(denoise=False, solver="native", rtol=10.0, atol=10.0, first_step=0.5, eps=0.5, seed=SEED)
    for sc in ("batch", "utterance"):
        ctx.set_windows((W, starts), 2)
        with pytest.raises(ValueError, match="not supported"):
            m.get_ode_sampler(zeros(1, Kf), step_control=sc, **ode)()
        ctx.set_windows(None)
        assert usable()
    with pytest.raises(ValueError, match="window_blend"):
        m.enhance_long(L.wave(L.L_LONG), W, O, seed=SEED, window_blend="state", **L.PC)
    with pytest.raises(ValueError, match="Python loop"):
        m.get_pc_sampler("reverse_diffusion", "ald", zeros(1, Kf), N=1, windows=(W, starts), force_python_loop=True)
    with pytest.raises(ValueError, match="Python loop"):
        sb.get_sb_sampler(sb.sde, zeros(1, Kf), windows=(W, starts), force_python_loop=True)
    for kw in (dict(adaptive=True), dict(denoise=False, solver="native"), dict(denoise=False, solver="native", step_control="utterance")):
        with pytest.raises(ValueError, match="adaptive ODE"):
            m.get_ode_sampler(zeros(1, Kf), windows=(W, starts), **kw)
    with pytest.raises(ValueError, match="adaptive ODE"):
        m.enhance_long(L.wave(L.L_LONG), W, O, seed=SEED, window_blend="score", sampler_type="ode", adaptive=True, solver="native",
                       step_control="utterance")
    assert usable()


# ----------------------------------------------------------------------------------------------------------------------------
# 9. directory job

def check_directory_job(dev, tmp_path):
    """python -m sgmse_amd.enhancement --window_frames 128 --window_overlap 32 --window_blend score --seed 7 --N 1 on
    long_recording_checks.check_directory_job's two files: the 250-frame file holds the samples of enhance_long(window_blend="score",
    stream = its index in the file list), the 101-frame file (one window: the existing path) those of enhance_long as well -- and the
    bytes written without --window_blend; --batch_size 1 and 3 write identical bytes; the long file differs from --window_blend output's."""
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
    base = ["--test_dir", str(noisy), "--ckpt", str(ckpt), "--device", str(dev), "--N", "1", "--seed", "7", "--window_frames", str(W),
            "--window_overlap", str(O)]
    score = ["--window_blend", "score"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # checkpoint without EMA weights
        assert E.main(base + ["--window_blend", "output", "--enhanced_dir", str(tmp_path / "out"), "--batch_size", "1"]) == 2
        assert E.main(base + score + ["--enhanced_dir", str(tmp_path / "s1"), "--batch_size", "1"]) == 2
        assert E.main(base + score + ["--enhanced_dir", str(tmp_path / "s3"), "--batch_size", "3"]) == 2
        m = ScoreModel.load_from_checkpoint(str(ckpt), map_location=dev)
        with pytest.raises(ValueError, match="window_frames"):
            E.main(["--test_dir", str(noisy), "--enhanced_dir", str(tmp_path / "no"), "--ckpt", str(ckpt), "--device", str(dev)] + score)
    m.eval()
    m.to(dev)
    raw = lambda d, name: open(str(tmp_path / d / name), "rb").read()
    assert raw("out", "a_short.wav") == raw("s1", "a_short.wav") == raw("s3", "a_short.wav")
    assert raw("s1", "b_long.wav") == raw("s3", "b_long.wav") != raw("out", "b_long.wav")
    for g, (name, n) in enumerate((("a_short.wav", L.L_SHORT), ("b_long.wav", L.L_LONG))):
        y = torch.from_numpy(E.read_audio(str(noisy / name))[0])
        x, info = m.enhance_long(y, W, O, batch_size=2, seed=7, stream=g, N=1, window_blend="score")
        _, got = wavfile.read(str(tmp_path / "s1" / name))
        assert got.shape == (n,) and np.isfinite(got).all() and np.abs(got).max() > 0
        assert np.array_equal(got, x.cpu().numpy()), name
    assert info["starts"] == [0, 96, 122] and info["frames"] == [W] * 3


# ----------------------------------------------------------------------------------------------------------------------------
# 10. reported, not gated

def check_distance_to_whole(dev):
    """Reported, not gated: on the real random-init nf = 32 network and the 256-frame recording (PC reverse_diffusion + ald, N = 2, one
    seed and stream), the relative L2 between each windowed waveform and the one-spectrogram enhance_batch run: window_blend="score",
    and window_blend="output" with window_noise "window" and "recording".  Nothing predicts what the network's dependence on context
    leaves, and no trained checkpoint exists here, so no threshold: the figures go to DESIGN 7c.
    Measured, 'score' / 'output' + 'window' / 'output' + 'recording': 0.270 / 1.358 / 0.295, emulator and MI355X to the digits shown."""
    m = L.models(dev)[0]
    y, stream = L.wave(L_WHOLE), 3
    whole = m.enhance_batch([y], seed=SEED, streams=[stream], **L.PC)[0][0]
    figs = {}
    for name, kw in (("score", dict(window_blend="score")), ("output/window", dict(window_noise="window")),
                     ("output/recording", dict(window_noise="recording"))):
        x, _ = m.enhance_long(y, W, O, batch_size=2, seed=SEED, stream=stream, **kw, **L.PC)
        figs[name] = rel_l2(x.cpu(), whole.cpu())
    print(f"distance to the one-spectrogram run on {dev}, rel_l2: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert all(np.isfinite(v) for v in figs.values())
