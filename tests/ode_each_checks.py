"""Checks of the native adaptive sampler's per-utterance step control (get_ode_sampler(solver="native", step_control="utterance") ->
sgmse_ode_sample_each, sgmse_amd/csrc/kernels_ode.h with one controller group per utterance), shared by the emulator and the GPU test modules.  The defining property:
utterance b of any batch, uniform or ragged, in any slot, is bit-identical to the existing solver's run on that utterance alone, with
the same evaluation count, accepted / rejected counts and accepted time points."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import ncsnpp_oracle as NO, synth
from parity import load, make_model, replay_noise
import ode_native_checks as N

EPS = N.EPS
OFFSETS = (0.003, 0.3, 30.0)          # prior offsets a_b of the three utterances: three different step sequences
# the emulator takes seconds per evaluation: half the interval in one attempt that every utterance accepts on the random-weight network
# (7 evaluations).  Tolerances under which that network makes one utterance reject the attempt make it reject many in a row (measured:
# offset 0.003 at rtol = atol = 3e-3 rejects seven times and is not done after 43 evaluations), minutes on the emulator; the mixed
# round -- one utterance accepts the attempt the other rejects -- runs there on the zero-score network (QUICK_MIXED: 7 and 19
# evaluations in scipy), and on the random-weight network on the GPU.
QUICK = dict(rtol=1.0, atol=1.0, first_step=0.5, eps=0.5)
QUICK_MIXED = dict(rtol=1e-5, atol=1e-5, first_step=0.5, eps=0.5)
QUICK_OFFSETS = (0.003, 30.0)


def _engine(m, dev):
    return m.dnn.engine(torch.device(dev))


def _inputs(dev, offsets=OFFSETS):
    """y = synth_spec(B, 64, 64, seed=4), z_b = y_b + a_b n with n drawn as in ode_native_checks.check_closed_form (generator seed 3)."""
    y = synth.synth_spec(len(offsets), 64, 64, seed=4)
    g = torch.Generator().manual_seed(3)
    n = torch.randn(y.shape, dtype=torch.complex64, generator=g)
    z = y + torch.tensor(offsets, dtype=torch.float32)[:, None, None, None] * n
    return y.to(dev), z.to(dev)


def _alone(m, dev, y_b, kw, call_kw):
    """The existing solver (one error norm over the batch) on ONE utterance [1,1,F,T]: (sample, nfe, ode_stats)."""
    out, nfe = m.get_ode_sampler(y_b, denoise=False, solver="native", **kw)(**call_kw)
    return out, nfe, _engine(m, dev).ode_stats()


def _assert_same_as_alone(tag, b, got, st_b, alone):
    out_a, nfe_a, st_a = alone
    print(f"{tag}: utterance {b}: nfe {st_b['nfe']} (alone {nfe_a}), accepted {st_b['accepted']} ({st_a['accepted']}), rejected {st_b['rejected']} "
          f"({st_a['rejected']}), bytes equal: {torch.equal(got.reshape(-1), out_a.reshape(-1))}")
    assert torch.equal(got.reshape(-1), out_a.reshape(-1))
    assert (st_b["nfe"], st_b["accepted"], st_b["rejected"]) == (nfe_a, st_a["accepted"], st_a["rejected"])
    assert st_b["t"] == st_a["t"]


CLOSED_FORM_CASES = [(1e-5, None), (1e-5, 0.5), (1e-3, None)]      # (rtol = atol, first_step)


def check_closed_form_each(dev, m, tol, first_step):
    """Zero-score model (drift theta (y - x), theta = 1.5): every utterance of a batch of three against ITS OWN scipy.integrate.solve_ivp
    run, under the gates of ode_native_checks.check_closed_form: same nfev, accepted and rejected counts, end state within tol (relative
    L2), accepted times within 1e-2, last time == eps.  The three prior offsets give three different step sequences (asserted: a batch
    whose utterances march in lockstep would show nothing), and the returned nfe is the largest."""
    from scipy import integrate
    theta = 1.5
    y, z = _inputs(dev)
    kw = {} if first_step is None else dict(first_step=first_step)
    sols = []
    for b in range(3):
        yn = y[b].cpu().numpy().reshape(-1).astype(np.complex128)
        sol = integrate.solve_ivp(lambda t, x: theta * (yn - x), (1.0, EPS), z[b].cpu().numpy().reshape(-1), rtol=tol, atol=tol, method="RK45", **kw)
        assert sol.status == 0
        sols.append(sol)
    nfevs = [s.nfev for s in sols]
    assert len(set(nfevs)) > 1, nfevs
    out, nfe = m.get_ode_sampler(y, denoise=False, rtol=tol, atol=tol, method="RK45", solver="native", step_control="utterance", eps=EPS, **kw)(z=z)
    st = _engine(m, dev).ode_stats_each()
    assert len(st["utterances"]) == 3
    for b, (sol, u) in enumerate(zip(sols, st["utterances"])):
        acc_ref = len(sol.t) - 1
        rej_ref = (sol.nfev - 1 - (1 if first_step is None else 0)) // 6 - acc_ref
        err = rel_l2(out[b].cpu().to(torch.complex128), torch.from_numpy(sol.y[:, -1]).reshape(out[b].shape))
        dt = max(abs(a - c) for a, c in zip(u["t"], sol.t[1:])) if u["accepted"] == acc_ref else float("nan")
        print(f"closed form each rtol=atol={tol:g} first_step={first_step} utterance {b}: nfe {u['nfe']} (scipy {sol.nfev}), accepted "
              f"{u['accepted']} ({acc_ref}), rejected {u['rejected']} ({rej_ref}), end state rel_l2 vs scipy {err:.2e}, times within {dt:.1e}")
        assert u["nfe"] == sol.nfev, (b, u["nfe"], sol.nfev)
        assert (u["accepted"], u["rejected"]) == (acc_ref, rej_ref), (b, u, acc_ref, rej_ref)
        assert err < tol, (b, err)
        assert u["t"][-1] == EPS and sol.t[-1] == EPS
        assert dt < 1e-2, (b, dt)
    assert nfe == max(nfevs), (nfe, nfevs)
    rounds = (max(nfevs) - 1 - (1 if first_step is None else 0)) // 6
    assert st["rounds"] == rounds and st["wasted"] == sum(max(nfevs) - v for v in nfevs), st


def check_bit_identity_uniform(dev, quick=False, zero_model=None):
    """Real (random-weight) nf = 32 model: the batch under step_control="utterance" equals the B = 1 runs of the existing solver, byte
    for byte and count for count -- with the start states given, with the utterances permuted, and with the prior drawn from (seed,
    stream id), where an utterance's result follows its stream id and not its slot.  quick (emulator): two utterances and one accepted
    attempt on that model, then on the zero-score model a first attempt that one utterance accepts and the other rejects (asserted)."""
    m, _ = make_model(N._small_cfg(), dev)
    offsets = QUICK_OFFSETS if quick else OFFSETS
    y, z = _inputs(dev, offsets)
    B = len(offsets)
    kw = dict(QUICK) if quick else dict(rtol=1e-2, atol=1e-2)
    alone = [_alone(m, dev, y[b:b + 1], kw, dict(z=z[b:b + 1])) for b in range(B)]
    each = lambda yy, **skw: m.get_ode_sampler(yy, denoise=False, solver="native", step_control="utterance", **kw, **skw)
    out, nfe = each(y)(z=z)
    st = _engine(m, dev).ode_stats_each()
    for b in range(B):
        _assert_same_as_alone("z given", b, out[b], st["utterances"][b], alone[b])
    assert nfe == max(a[1] for a in alone)
    if quick:
        alone0 = [_alone(zero_model, dev, y[b:b + 1], QUICK_MIXED, dict(z=z[b:b + 1])) for b in range(B)]
        out0, nfe0 = zero_model.get_ode_sampler(y, denoise=False, solver="native", step_control="utterance", **QUICK_MIXED)(z=z)
        u = _engine(zero_model, dev).ode_stats_each()["utterances"]
        for b in range(B):
            _assert_same_as_alone("mixed round", b, out0[b], u[b], alone0[b])
        assert sorted(min(v["rejected"], 1) for v in u) == [0, 1], u      # one accepts the attempt the other rejects
        assert nfe0 == max(a[1] for a in alone0)
    perm = [1, 0] if quick else [2, 0, 1]
    out_p, nfe_p = each(y[perm].contiguous())(z=z[perm].contiguous())
    st_p = _engine(m, dev).ode_stats_each()
    for slot, b in enumerate(perm):
        _assert_same_as_alone("permuted", b, out_p[slot], st_p["utterances"][slot], alone[b])
    assert nfe_p == nfe
    if quick:      # (the prior from seed and stream ids: check_bit_identity_ragged, which the emulator runs too)
        return
    # the prior from (seed, stream id)
    ids = [5, 9, 2]
    alone_s = [_alone(m, dev, y[b:b + 1], dict(kw, seed=11, streams=[ids[b]]), {}) for b in range(B)]
    out_s, _ = each(y, seed=11, streams=ids)()
    st_s = _engine(m, dev).ode_stats_each()
    for b in range(B):
        _assert_same_as_alone("seed + streams", b, out_s[b], st_s["utterances"][b], alone_s[b])
    out_sp, _ = each(y[perm].contiguous(), seed=11, streams=[ids[b] for b in perm])()
    for slot, b in enumerate(perm):
        assert torch.equal(out_sp[slot], out_s[b])


def check_bit_identity_ragged(dev, quick=False):
    """A ragged list of 64 and 128 frames with seed and streams: each result is bit-identical to its own B = 1 run, with equal counts;
    the same list under the default step control is still refused."""
    m, _ = make_model(N._small_cfg(), dev)
    ys = [synth.synth_spec(1, 64, 64, seed=4)[0].to(dev), synth.synth_spec(1, 64, 128, seed=5)[0].to(dev)]      # [1,F,T_b]
    kw = dict(QUICK) if quick else dict(rtol=1e-2, atol=1e-2)
    ids = [5, 9]
    alone = [_alone(m, dev, ys[b][None], dict(kw, seed=11, streams=[ids[b]]), {}) for b in range(2)]
    outs, nfe = m.get_ode_sampler(ys, denoise=False, solver="native", step_control="utterance", seed=11, streams=ids, **kw)()
    st = _engine(m, dev).ode_stats_each()
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(1, 64, 64), (1, 64, 128)]
    for b in range(2):
        _assert_same_as_alone("ragged", b, outs[b], st["utterances"][b], alone[b])
    assert nfe == max(a[1] for a in alone)
    with pytest.raises(TypeError, match="ragged"):
        m.get_ode_sampler(ys, denoise=False, solver="native", step_control="batch", seed=11, streams=ids, **kw)
    # a uniform call afterwards is uniform again
    again, _ = m.get_ode_sampler(ys[0][None], denoise=False, solver="native", step_control="utterance", seed=11, streams=[5], **kw)()
    assert torch.equal(again.reshape(-1), alone[0][0].reshape(-1))


def check_fixture_each(dev, name="ode_rk45"):
    """B = 1 on tests/golden/ode_rk45.npz (the reference's own run, 92 evaluations): step_control="utterance" gives the bytes and the
    nfe of step_control="batch", and so passes the gates of ode_native_checks.check_fixture against the reference."""
    z = load(name)
    m, _ = make_model(NO.NetCfg.for_variant("ncsnpp", nf=32), dev)
    y = torch.from_numpy(z["y"]).to(dev)
    noise = replay_noise(tuple(y.shape), 1).to(dev)
    kw = dict(denoise=False, rtol=float(z["rtol"]), atol=float(z["atol"]), method="RK45", noise=noise, solver="native")
    a, nfe_a = m.get_ode_sampler(y, step_control="batch", **kw)()
    st_a = _engine(m, dev).ode_stats()
    b, nfe_b = m.get_ode_sampler(y, step_control="utterance", **kw)()
    u = _engine(m, dev).ode_stats_each()["utterances"][0]
    err = rel_l2(b.cpu(), torch.from_numpy(z["out"]))
    print(f"{name} per-utterance control on {dev}: evaluations {nfe_b} (batch control {nfe_a}, reference {int(z['nfe'])}), rel_l2 vs the reference's {err:.3e}")
    assert torch.equal(a, b) and nfe_a == nfe_b == u["nfe"]
    assert (u["accepted"], u["rejected"], u["t"]) == (st_a["accepted"], st_a["rejected"], st_a["t"])
    assert abs(nfe_b - int(z["nfe"])) <= 12 and err < 5.0 * float(z["oracle_vs_reference"])


def check_v2_callback_each(dev):
    """ncsnpp_v2 wrapper (the model of ode_native_checks.check_v2_callback), two utterances with different prior offsets, ONE attempt
    (first_step given, accepted by both): the host callback sees B times for the start and 6 B stage times for the round, stage-major
    (t[stage * B + b]), and each utterance equals its B = 1 run bit for bit."""
    wrap = dict(loss_type="denoiser", network_scaling="1/sigma", c_in="edm", c_out="1", c_skip="0", sigma_data=0.1)
    m, _ = make_model(N._small_cfg("ncsnpp_v2"), dev, **wrap)
    y, z = _inputs(dev, (0.003, 0.3))
    h = 1.0 - 0.9
    hh = (1.0 - h) - 1.0
    kw = dict(rtol=1e3, atol=1e3, first_step=h, eps=0.9)
    seen = []
    orig = m.score_affine

    def spy(ts):
        seen.append([float(v) for v in ts])
        return orig(ts)
    m.score_affine = spy
    try:
        out, nfe = m.get_ode_sampler(y, denoise=False, solver="native", step_control="utterance", **kw)(z=z)
    finally:
        m.score_affine = orig
    C = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
    stage_t = [float(np.float32(1.0 + c * hh)) for c in C[:4]] + [float(np.float32(1.0 + C[4] * hh)), float(np.float32(1.0 + hh))]
    assert seen[1] == [1.0, 1.0], seen[1]                            # (seen[0]: the probe that asks whether the model has an affine wrapper)
    assert seen[2] == [t for t in stage_t for _ in range(2)], (seen[2], stage_t)
    assert len(seen) == 3 and nfe == 7
    st = _engine(m, dev).ode_stats_each()
    for b in range(2):
        _assert_same_as_alone("v2 wrapper", b, out[b], st["utterances"][b], _alone(m, dev, y[b:b + 1], kw, dict(z=z[b:b + 1])))


def check_interface_each(dev, zero_model, quick=False):
    """step_control: only 'batch' / 'utterance', 'utterance' only with the native solver; a per-utterance max_nfe that only the slowest
    utterance exceeds raises RuntimeError naming it, and the next call on the context reproduces the bytes; ode_stats_each is
    consistent; enhancement.build_sampler forwards the flag and a ragged list, and without the attribute calls exactly what it did."""
    m = zero_model
    offsets = QUICK_OFFSETS if quick else OFFSETS
    y, z = _inputs(dev, offsets)
    B = len(offsets)
    with pytest.raises(ValueError, match="step_control"):
        m.get_ode_sampler(y, denoise=False, solver="scipy", step_control="utterance")
    with pytest.raises(ValueError, match="step_control"):
        m.get_ode_sampler(y, denoise=False, step_control="utterance")
    with pytest.raises(ValueError, match="step_control"):
        m.get_ode_sampler(y, denoise=False, solver="native", step_control="file")
    # zero-score drift: quick -- the far utterance rejects the half-interval attempt at this tolerance and the near one accepts it;
    # else the automatic first step at 1e-5, where the three utterances need different numbers of attempts
    kw = dict(rtol=1e-5, atol=1e-5, first_step=0.5, eps=0.5) if quick else dict(rtol=1e-5, atol=1e-5)
    sampler = m.get_ode_sampler(y, denoise=False, solver="native", step_control="utterance", **kw)
    a, nfe = sampler(z=z)
    st = _engine(m, dev).ode_stats_each()
    nfes = [u["nfe"] for u in st["utterances"]]
    print(f"interface: per-utterance nfe {nfes}, rounds {st['rounds']}, wasted {st['wasted']}")
    assert len(nfes) == B and nfe == max(nfes) and nfes[-1] == max(nfes) and sorted(nfes)[-2] < max(nfes), nfes
    first = 1 if quick else 2
    for u in st["utterances"]:
        assert u["nfe"] == first + 6 * (u["accepted"] + u["rejected"]) and len(u["t"]) == u["accepted"] and u["t"][-1] == kw.get("eps", EPS)
    assert st["rounds"] == (nfe - first) // 6 and st["wasted"] == sum(nfe - v for v in nfes)
    with pytest.raises(RuntimeError, match=f"utterance {B - 1} needs more than max_nfe"):
        sampler(z=z, max_nfe=max(nfes) - 1)
    again, nfe_again = sampler(z=z)
    assert nfe_again == nfe and torch.equal(again, a)
    # enhancement.build_sampler
    from types import SimpleNamespace
    from sgmse_amd.enhancement import build_sampler
    calls = []
    real = m.get_ode_sampler
    m.get_ode_sampler = lambda Y, **k: calls.append((Y, k)) or real(Y, **k)
    args = SimpleNamespace(sampler_type="ode", N=3, corrector="ald", corrector_steps=1, snr=0.5, ode_solver="native")
    ragged = [y[0], synth.synth_spec(1, 64, 128, seed=5)[0].to(dev)]
    try:
        assert callable(build_sampler(m, y, args, seed=5, streams=list(range(B))))          # no attribute: today's call
        args.ode_step_control = "batch"
        assert callable(build_sampler(m, y, args, seed=5, streams=list(range(B))))
        with pytest.raises(TypeError, match="--ode_solver native.*rectangular"):
            build_sampler(m, ragged, args, seed=5, streams=[7, 8])
        args.ode_step_control = "utterance"
        assert callable(build_sampler(m, ragged, args, seed=5, streams=[7, 8]))
        args.ode_solver = "scipy"                                                             # the flag is the native solver's
        with pytest.raises(TypeError, match="--ode_solver scipy.*rectangular"):
            build_sampler(m, ragged, args, seed=5, streams=[7, 8])
    finally:
        m.get_ode_sampler = real
    today = dict(adaptive=True, denoise=False, solver="native", seed=5, streams=list(range(B)))
    assert calls[0][1] == today and calls[1][1] == today
    assert calls[2][0] is ragged and calls[2][1] == dict(adaptive=True, denoise=False, solver="native", seed=5, streams=[7, 8], step_control="utterance")
    assert len(calls) == 3
