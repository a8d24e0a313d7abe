"""Checks of the native adaptive probability-flow sampler (get_ode_sampler(solver="native") -> sgmse_ode_sample: Dormand-Prince 5(4)
with scipy's RK45 step control inside the library, sgmse_amd/csrc/kernels_ode.h), shared by the emulator and the GPU test modules."""
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import ncsnpp_oracle as NO, synth
from parity import SAMPLER_TOL, load, make_model, replay_noise

EPS = 0.03


def _engine(m, dev):
    return m.dnn.engine(torch.device(dev))


def _small_cfg(variant="ncsnpp"):
    """The nf = 32 test network built for 64 frequency bins: [B, 1, 64, 64] is then the smallest input it accepts (seven levels)."""
    return NO.NetCfg.for_variant(variant, nf=32, image_size=64)


def _zero_score_model(dev):
    """nf = 32 test model whose output convolution is zero: the score is exactly 0 and the probability-flow drift is theta (y - x)."""
    cfg = _small_cfg()
    m, _ = make_model(cfg, dev)
    with torch.no_grad():
        m.dnn.output_layer.weight.zero_()
        m.dnn.output_layer.bias.zero_()
    m.dnn.mark_weights_changed()
    return m


CLOSED_FORM_CASES = [(1e-5, None), (1e-3, None), (1e-5, 0.5), (1e-3, 0.9)]      # (rtol = atol, first_step)


def check_closed_form(dev, m, tol, first_step):
    """Controller and stage kernels against scipy.integrate.solve_ivp on the drift theta (y - x) written in NumPy (no network):
    same evaluation count, same accepted / rejected step counts, end state within rtol (relative L2), last accepted time = eps exactly,
    accepted times within 1e-2 of scipy's (fp32 rounding of the state moves the step size of this nearly linear problem a little)."""
    from scipy import integrate
    theta = 1.5
    y = synth.synth_spec(2, 64, 64, seed=4)
    y[1] *= 3.0                                   # two different utterances: one error norm over both
    g = torch.Generator().manual_seed(3)
    z = y + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)
    yn = y.numpy().reshape(-1).astype(np.complex128)
    kw = {} if first_step is None else dict(first_step=first_step)
    sol = integrate.solve_ivp(lambda t, x: theta * (yn - x), (1.0, EPS), z.numpy().reshape(-1), rtol=tol, atol=tol, method="RK45", **kw)
    assert sol.status == 0
    acc_ref = len(sol.t) - 1
    rej_ref = (sol.nfev - 1 - (1 if first_step is None else 0)) // 6 - acc_ref
    sampler = m.get_ode_sampler(y.to(dev), denoise=False, rtol=tol, atol=tol, method="RK45", solver="native", eps=EPS, **kw)
    out, nfe = sampler(z=z.to(dev))
    st = _engine(m, dev).ode_stats()
    ref = torch.from_numpy(sol.y[:, -1]).reshape(y.shape)
    err = rel_l2(out.cpu().to(torch.complex128), ref)
    dt = max(abs(a - b) for a, b in zip(st["t"], sol.t[1:])) if st["accepted"] == acc_ref else float("nan")
    print(f"closed form rtol=atol={tol:g} first_step={first_step}: nfe {nfe} (scipy {sol.nfev}), accepted {st['accepted']} ({acc_ref}), "
          f"rejected {st['rejected']} ({rej_ref}), end state rel_l2 vs scipy {err:.2e}, accepted times within {dt:.1e}")
    assert nfe == sol.nfev, (nfe, sol.nfev)
    assert (st["accepted"], st["rejected"]) == (acc_ref, rej_ref), (st["accepted"], st["rejected"], acc_ref, rej_ref)
    assert err < tol, err
    assert st["t"][-1] == EPS and sol.t[-1] == EPS
    assert dt < 1e-2, dt
    if first_step == 0.5:
        assert st["rejected"] >= 1        # (this setting exists to exercise a rejection)


def check_fixture(dev, name, compare_scipy=True):
    """tests/golden/<name>.npz (the reference's own get_ode_sampler(denoise=False) run) with solver='native' and the replayed prior
    noise, under the gates parity.check_ode_rk45 applies to the scipy-driven path: |nfe - reference| <= 12; end state within 5x the
    fixture's oracle_vs_reference at rtol = 1e-3, within SAMPLER_TOL at the default 1e-5."""
    z = load(name)
    cfg = NO.NetCfg.for_variant("ncsnpp", nf=32)
    m, _ = make_model(cfg, dev)
    y = torch.from_numpy(z["y"]).to(dev)
    noise = replay_noise(tuple(y.shape), 1).to(dev)
    kw = dict(denoise=False, rtol=float(z["rtol"]), atol=float(z["atol"]), method="RK45", noise=noise)
    out, nfe = m.get_ode_sampler(y, solver="native", **kw)()
    st = _engine(m, dev).ode_stats()
    err = rel_l2(out.cpu(), torch.from_numpy(z["out"]))
    own = float(z["oracle_vs_reference"])
    bound = SAMPLER_TOL if float(z["rtol"]) <= 1e-5 else 5.0 * own
    print(f"{name} native on {dev}: evaluations {nfe} (reference {int(z['nfe'])}), accepted {st['accepted']}, rejected {st['rejected']}, "
          f"end state rel_l2 vs the reference's = {err:.3e} (the oracle's own: {own:.3e}; bound {bound:.1e})")
    if compare_scipy:
        out_s, nfe_s = m.get_ode_sampler(y, **kw)()
        print(f"{name} native vs the scipy-driven path on {dev}: rel_l2 = {rel_l2(out.cpu(), out_s.cpu()):.3e} (scipy-driven: {nfe_s} evaluations, "
              f"{rel_l2(out_s.cpu(), torch.from_numpy(z['out'])):.3e} from the reference)")
    assert nfe == 2 + 6 * (st["accepted"] + st["rejected"])
    assert abs(nfe - int(z["nfe"])) <= 12 and err < bound, (nfe, err, bound)


def check_bit_stability_and_interface(dev, quick=False):
    """Same seed -> same bytes and same nfe; `streams` ties an utterance's prior to its stream id, not its batch slot; a tiny max_nfe
    raises and the next call works; unsupported requests raise the documented exceptions.  quick (emulator, seconds per evaluation):
    the runs are one accepted step of one utterance (7 evaluations) instead of a whole integration of two."""
    from sgmse_amd import sampling
    cfg = _small_cfg()
    m, _ = make_model(cfg, dev)
    y = synth.synth_spec(2, 64, 64, seed=4).to(dev)
    kw = dict(denoise=False, solver="native", **(dict(rtol=10.0, atol=10.0, first_step=0.5, eps=0.5) if quick else dict(rtol=1e-2, atol=1e-2)))
    yb, ids = (y[:1], [5]) if quick else (y, [5, 9])
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # no "do not apply" warning: seed and streams DO apply to the native solver
        a, nfe_a = m.get_ode_sampler(yb, seed=11, streams=ids, **kw)()
    b, nfe_b = m.get_ode_sampler(yb, seed=11, streams=ids, **kw)()
    assert nfe_a == nfe_b and torch.equal(a, b) and nfe_a >= 7
    c, _ = m.get_ode_sampler(yb, seed=12, streams=ids, **kw)()
    assert not torch.equal(a, c)
    # the prior draw of an utterance depends on (seed, stream id), not on its batch slot: one utterance twice under one stream id
    # draws the same prior in both slots (and then follows the same trajectory); under two ids it does not
    same_y = torch.cat([y[:1], y[:1]])
    d, _ = m.get_ode_sampler(same_y, seed=11, streams=[5, 5], **kw)()
    assert torch.equal(d[0], d[1])
    e, _ = m.get_ode_sampler(same_y, seed=11, streams=[5, 6], **kw)()
    assert not torch.equal(e[0], e[1])
    # a cap on evaluations ends the call with an error, and the context stays usable
    with pytest.raises(RuntimeError, match="max_nfe"):
        m.get_ode_sampler(yb, seed=11, streams=ids, **kw)(max_nfe=5)
    again, nfe_again = m.get_ode_sampler(yb, seed=11, streams=ids, **kw)()
    assert nfe_again == nfe_a and torch.equal(again, a)
    pc, _ = m.get_pc_sampler("reverse_diffusion", "ald", yb, N=1, snr=0.5, seed=3)()
    assert torch.isfinite(torch.view_as_real(pc)).all()
    # what the native solver does not do raises, naming it
    with pytest.raises(ValueError, match="RK23"):
        m.get_ode_sampler(y, method="RK23", **kw)
    with pytest.raises(ValueError, match="t_eval"):
        m.get_ode_sampler(y, t_eval=[0.5], **kw)
    with pytest.raises(TypeError, match="ragged"):
        m.get_ode_sampler([y[0], y[1]], **kw)
    with pytest.raises(ValueError, match="solver"):
        m.get_ode_sampler(y, denoise=False, solver="cvode")
    with pytest.raises(ValueError, match="HIP backbone"):
        sampling.get_ode_sampler(m.sde.copy(), lambda x, yy, t: yy - x, y, denoise=False, solver="native")
    # a ragged context refuses the library call itself
    ctx = _engine(m, dev)
    ctx.set_frames([64, 64])
    try:
        with pytest.raises(RuntimeError, match="ragged"):
            ctx.check(ctx.lib.sgmse_ode_sample(ctx.h, y.data_ptr(), torch.empty_like(y).data_ptr(), 2, 64, 64,
                                               _ode_cfg(), None, None, 0, None))
    finally:
        ctx.set_frames([])


def _ode_cfg():
    import ctypes as C
    from sgmse_amd import _lib
    c = _lib.OdeCfgC()
    c.theta, c.sigma_min, c.sigma_max, c.std1, c.t_end, c.eps, c.rtol, c.atol, c.max_nfe = 1.5, 0.05, 0.5, 0.3, 1.0, EPS, 1e-2, 1e-2, 1000
    return C.byref(c)


def check_scipy_default_unchanged(dev):
    """solver='scipy' and the default are the scipy-driven path: equal to a solve_ivp run written here over the same device drift
    (half the interval in one step: 7 evaluations per run)."""
    from scipy import integrate
    cfg = _small_cfg()
    m, _ = make_model(cfg, dev)
    y = synth.synth_spec(1, 64, 64, seed=4).to(dev)
    g = torch.Generator().manual_seed(3)
    z = (y.cpu() + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)).to(dev)
    kw = dict(denoise=False, rtol=10.0, atol=10.0, method="RK45", first_step=0.5, eps=0.5)
    a, nfe_a = m.get_ode_sampler(y, **kw)(z=z)
    b, nfe_b = m.get_ode_sampler(y, solver="scipy", **kw)(z=z)
    rsde = m.sde.copy().reverse(m, probability_flow=True)

    def f(t, xf):
        xt = torch.from_numpy(xf.reshape(tuple(y.shape))).to(dev).type(torch.complex64)
        with torch.no_grad():
            return rsde.sde(xt, y, torch.ones(1, device=dev) * t)[0].cpu().numpy().reshape(-1)
    sol = integrate.solve_ivp(f, (1, 0.5), z.cpu().numpy().reshape(-1), rtol=10.0, atol=10.0, method="RK45", first_step=0.5)
    want = torch.tensor(sol.y[:, -1]).reshape(y.shape).type(torch.complex64)
    assert nfe_a == nfe_b == sol.nfev == 7 and torch.equal(a, b) and torch.equal(a.cpu(), want)
    with pytest.warns(UserWarning, match="do not apply"):
        m.get_ode_sampler(y, seed=3, **kw)


def _dopri_step(m, dev, y, z, hh):
    """One Dormand-Prince step of size hh from (t = 1, z), formed in complex128 from ScoreModel.forward-based drifts: (z, the end point)."""
    C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
    A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
         [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]]
    Bw = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
    rsde = m.sde.copy().reverse(m, probability_flow=True)
    f = lambda t, x: rsde.sde(x.type(torch.complex64), y, torch.ones(y.shape[0], device=dev) * t)[0].to(torch.complex128)
    with torch.no_grad():
        x = z.to(torch.complex128)
        K = [f(1.0, x)]
        for s in range(1, 6):
            K.append(f(1.0 + C[s] * hh, x + sum(a * k for a, k in zip(A[s], K)) * hh))
        return x, x + hh * sum(b * k for b, k in zip(Bw, K))


V2_WRAP = dict(loss_type="denoiser", network_scaling="1/sigma", c_in="edm", c_out="1", c_skip="0", sigma_data=0.1)


def check_v2_callback(dev):
    """ncsnpp_v2 ('denoiser', network scaling 1/sigma, c_in 'edm'): the host callback receives each attempt's six stage times, its rows
    reach the device table, and ONE attempted step (first_step given, a tolerance under which it is accepted) equals the
    Dormand-Prince step formed from ScoreModel.forward-based drifts at the same stage times, within the drift gate of
    check_ode_rk45 (1e-5) on the step's increment."""
    cfg = _small_cfg("ncsnpp_v2")
    m, _ = make_model(cfg, dev, **V2_WRAP)
    y = synth.synth_spec(1, 64, 64, seed=4).to(dev)
    g = torch.Generator().manual_seed(3)
    z = (y.cpu() + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)).to(dev)
    seen = []
    orig = m.score_affine

    def spy(ts):
        seen.append([float(v) for v in ts])
        return orig(ts)
    m.score_affine = spy
    h = 1.0 - 0.9                                  # (so that eps = 0.9 below is one step of exactly this size)
    hh = (1.0 - h) - 1.0                           # the step as the solver forms it: t_new - t
    # one attempt exactly: first_step = h, and max_nfe = 1 + 6 lets the first attempt run and refuses a second one
    sampler = m.get_ode_sampler(y, denoise=False, rtol=1e3, atol=1e3, solver="native", first_step=h, max_step=h)
    with pytest.raises(RuntimeError, match="max_nfe"):
        sampler(z=z, max_nfe=7)
    m.score_affine = orig
    st = _engine(m, dev).ode_stats()
    assert st["accepted"] == 1 and st["t"][0] == 1.0 - h
    C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
    want_t = [float(np.float32(1.0))] + [float(np.float32(1.0 + c * hh)) for c in C[1:5]] + [float(np.float32(1.0 + C[5] * hh)), float(np.float32(1.0 + hh))]
    got_t = [t for call in seen for t in call]
    assert got_t[1:8] == want_t, (got_t, want_t)      # (got_t[0]: the probe that asks whether the model has an affine wrapper)
    x, want = _dopri_step(m, dev, y, z, hh)
    # the accepted state is not returned by a failed call: run the same single step to completion by integrating to eps = 1 - h
    out, nfe = m.get_ode_sampler(y, denoise=False, rtol=1e3, atol=1e3, solver="native", first_step=h, eps=0.9)(z=z)
    step = (want - x).cpu()
    err = rel_l2((out.to(torch.complex128) - x).cpu(), step)
    print(f"v2 wrapper on {dev}: one Dormand-Prince step of size {h}: increment rel_l2 vs ScoreModel.forward-based drifts = {err:.3e}")
    assert nfe == 7 and err < 1e-5, (nfe, err)


def check_batch_control_step(dev):
    """Batch control with MORE THAN ONE utterance on a network whose time-embedding rows matter: the construction of check_v2_callback
    at B = 2 (the second utterance three times the first).  One accepted attempt under step_control="batch": 7 evaluations; the host
    callback sees ONE time for the start and the SIX stage times of the attempt (one controller group: not 2 and 12); the increment
    is within the one-step gate of check_v2_callback (1e-5, relative L2) of the Dormand-Prince step formed from ScoreModel.forward-
    based drifts on the two-utterance batch."""
    m, _ = make_model(_small_cfg("ncsnpp_v2"), dev, **V2_WRAP)
    y = synth.synth_spec(2, 64, 64, seed=4)
    y[1] *= 3.0
    g = torch.Generator().manual_seed(3)
    z = (y + 0.3 * torch.randn(y.shape, dtype=torch.complex64, generator=g)).to(dev)
    y = y.to(dev)
    h = 1.0 - 0.9
    hh = (1.0 - h) - 1.0
    seen = []
    orig = m.score_affine

    def spy(ts):
        seen.append([float(v) for v in ts])
        return orig(ts)
    m.score_affine = spy
    try:
        out, nfe = m.get_ode_sampler(y, denoise=False, rtol=1e3, atol=1e3, solver="native", step_control="batch", first_step=h, eps=0.9)(z=z)
    finally:
        m.score_affine = orig
    C = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
    stage_t = [float(np.float32(1.0 + c * hh)) for c in C[:4]] + [float(np.float32(1.0 + C[4] * hh)), float(np.float32(1.0 + hh))]
    assert nfe == 7, nfe
    assert seen[1:] == [[1.0], stage_t], (seen, stage_t)       # (seen[0]: the probe that asks whether the model has an affine wrapper)
    x, want = _dopri_step(m, dev, y, z, hh)
    err = rel_l2((out.to(torch.complex128) - x).cpu(), (want - x).cpu())
    print(f"batch control, two utterances, v2 wrapper on {dev}: one Dormand-Prince step of size {h}: increment rel_l2 vs "
          f"ScoreModel.forward-based drifts = {err:.3e}")
    assert err < 1e-5, err


def check_enhancement_flag(dev):
    """enhancement.build_sampler: --ode_solver selects the adaptive solver of --sampler_type ode (seed and streams only reach the native
    one), leaving it unset keeps the fixed-step loop, and a ragged list is refused at once with a message that names the flag."""
    from types import SimpleNamespace
    from sgmse_amd.enhancement import build_sampler
    cfg = _small_cfg()
    m, _ = make_model(cfg, dev)
    y = synth.synth_spec(2, 64, 64, seed=4).to(dev)
    calls = []
    real = m.get_ode_sampler
    m.get_ode_sampler = lambda Y, **kw: calls.append(kw) or real(Y, **kw)
    args = SimpleNamespace(sampler_type="ode", N=3, corrector="ald", corrector_steps=1, snr=0.5)
    try:
        for solver in ("native", "scipy", None):
            args.ode_solver = solver
            assert callable(build_sampler(m, y, args, seed=5, streams=[7, 8]))
        with pytest.raises(TypeError, match="--ode_solver native.*rectangular"):
            args.ode_solver = "native"
            build_sampler(m, [y[0], y[1]], args, seed=5, streams=[7, 8])
    finally:
        m.get_ode_sampler = real
    assert calls[0] == dict(adaptive=True, denoise=False, solver="native", seed=5, streams=[7, 8])
    assert calls[1] == dict(adaptive=True, denoise=False, solver="scipy")
    assert calls[2] == dict(N=3, seed=5, streams=[7, 8])
    assert len(calls) == 3
