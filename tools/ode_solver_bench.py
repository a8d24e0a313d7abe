#!/usr/bin/env python3
"""Adaptive probability-flow sampler: the scipy-driven path (solve_ivp over host memory, one network evaluation per callback) against
the native solver (sgmse_ode_sample: the same RK45 step control, state and slopes on the device) on one GPU.

Seeded full-width synthetic weights, the same spectrogram and the same prior draw for both; the two paths alternate, --runs each
(after one untimed warm-up run of each at --warmup-tol).  Per (batch, tolerance): wall time, nfe, ms per evaluation of every run, the
relative L2 between the two end states, the fixed-step probability-flow loop's ms per evaluation at the same shape, and the verdict
of the pass condition: the native path's median ms per evaluation is no worse than the scipy-driven path's median plus that path's
own run-to-run spread (max - min over its runs).  The native run of a pair goes first and is capped at --max-nfe evaluations, so a
problem the solver cannot finish ends the row with a message before the uncapped scipy run starts.

    python tools/ode_solver_bench.py [--batches 32 1] [--tols 1e-3 1e-5] [--runs 3] [--seconds 4] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--tols", type=float, nargs="+", default=[1e-3, 1e-5])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--nf", type=int, default=128)
    ap.add_argument("--fixed-N", type=int, default=30)
    ap.add_argument("--warmup-tol", type=float, default=1e-3)
    ap.add_argument("--max-nfe", type=int, default=3000)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--test-emulator", type=str, default=None, metavar="LIB",
                    help="TEST ONLY: run this script's logic on CPU tensors with the workgroup-emulator build of the kernels; never a measurement")
    a = ap.parse_args()
    import torch
    from sgmse_amd import _lib
    from sgmse_amd.util.other import pad_spec
    from sgmse_amd.model import ScoreModel
    emu = a.test_emulator is not None
    if emu:
        _lib.load_library(a.test_emulator)
        dev, sync, name = torch.device("cpu"), (lambda: None), "workgroup emulator (not a measurement)"
    else:
        if not torch.cuda.is_available():
            raise SystemExit("ode_solver_bench.py needs an MI355X: sgmse_amd has no CPU path")
        _lib.load_library()
        dev, sync, name = torch.device("cuda", 0), torch.cuda.synchronize, torch.cuda.get_device_name(0)
    torch.manual_seed(0)
    model = ScoreModel("ncsnpp", "ouve", nf=a.nf, theta=1.5, sigma_min=0.05, sigma_max=0.5)      # random init, seeded (as bench.py)
    model.to(dev).eval()
    rel = lambda p, q: float((p - q).norm() / q.norm())
    rows = []
    for B in a.batches:
        g = torch.Generator().manual_seed(1000)
        wav = torch.randn(B, int(a.seconds * 16000), generator=g).to(dev)
        wav = wav / wav.abs().amax(dim=1, keepdim=True)
        Y = pad_spec(model._forward_transform(model._stft(wav)).unsqueeze(1), mode="zero_pad")
        gz = torch.Generator().manual_seed(7)
        noise = torch.randn(Y.shape, dtype=torch.complex64, generator=gz).to(dev)

        def run(solver, tol):
            extra = dict(max_nfe=a.max_nfe) if solver == "native" else {}
            sync()
            t0 = time.perf_counter()
            out, nfe = model.get_ode_sampler(Y, denoise=False, rtol=tol, atol=tol, noise=noise, solver=solver)(**extra)
            sync()
            return out, nfe, time.perf_counter() - t0
        for s in ("native", "scipy"):
            run(s, a.warmup_tol)
        # fixed-step probability-flow loop (captured graph) at the same shape: what one evaluation costs without a solver around it
        fixed = model.get_ode_sampler(Y, N=a.fixed_N, noise=noise.unsqueeze(0), seed=1)
        fixed()
        sync()
        t0 = time.perf_counter()
        fixed()
        sync()
        fixed_ms = (time.perf_counter() - t0) * 1e3 / a.fixed_N
        for tol in a.tols:
            rec = dict(batch=B, shape=list(Y.shape), rtol=tol, atol=tol, fixed_step_ms_per_eval=fixed_ms, scipy=[], native=[])
            outs = {}
            try:
                for _ in range(a.runs):
                    for s in ("native", "scipy"):
                        out, nfe, sec = run(s, tol)
                        outs[s] = out
                        rec[s].append(dict(seconds=sec, nfe=nfe, ms_per_eval=sec * 1e3 / nfe))
                        print(f"  batch {B} rtol=atol={tol:g} {s}: {sec:.2f} s, {nfe} evaluations", flush=True)
            except RuntimeError as e:
                rec["failed"] = str(e)
                rows.append(rec)
                print(f"batch {B} rtol=atol={tol:g}: {e}", flush=True)
                continue
            rec["native_vs_scipy_rel_l2"] = rel(outs["native"], outs["scipy"])
            st = model.dnn.engine(dev).ode_stats()
            rec["native_accepted"], rec["native_rejected"] = st["accepted"], st["rejected"]
            per = {s: [r["ms_per_eval"] for r in rec[s]] for s in ("scipy", "native")}
            med = {s: statistics.median(v) for s, v in per.items()}
            spread = max(per["scipy"]) - min(per["scipy"])
            rec.update(scipy_median_ms_per_eval=med["scipy"], native_median_ms_per_eval=med["native"], scipy_spread_ms_per_eval=spread,
                       native_no_worse_than_scipy=bool(med["native"] <= med["scipy"] + spread),
                       native_over_fixed_step=med["native"] / fixed_ms)
            rows.append(rec)
            f = lambda s: " ".join(f"{v:.2f}" for v in per[s])
            print(f"batch {B} {tuple(Y.shape)} rtol=atol={tol:g}: scipy nfe {rec['scipy'][0]['nfe']} ms/eval [{f('scipy')}]  native nfe "
                  f"{rec['native'][0]['nfe']} ms/eval [{f('native')}]  fixed-step loop {fixed_ms:.2f} ms/eval  end states rel_l2 "
                  f"{rec['native_vs_scipy_rel_l2']:.2e}  native no worse than scipy: {rec['native_no_worse_than_scipy']}", flush=True)
    res = dict(device=name, nf=a.nf, runs=a.runs, seconds=a.seconds, rows=rows)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if any("failed" in r or not r["native_no_worse_than_scipy"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
