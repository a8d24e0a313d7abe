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

--step_control utterance measures the native solver's per-utterance step control (sgmse_ode_sample_each) instead: per (batch,
tolerance) the wall time of the batched run against the same utterances integrated one by one with the existing B = 1 path (the two
alternate, --runs each, in this process; utterances of different levels, priors from one seed and the utterance's stream id), the
rounds, the utterance-evaluations wasted on finished utterances, and whether the outputs are byte-equal between the two (required).
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
    ap.add_argument("--step_control", type=str, choices=("batch", "utterance"), default="batch")
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
    if a.step_control == "utterance":
        return each_rows(a, model, dev, sync, name)
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


def each_rows(a, model, dev, sync, name):
    """--step_control utterance: batched per-utterance step control against the one-by-one B = 1 runs."""
    import torch
    from sgmse_amd.util.other import pad_spec
    rows = []
    for B in a.batches:
        g = torch.Generator().manual_seed(1000)
        wav = torch.randn(B, int(a.seconds * 16000), generator=g)
        level = torch.logspace(-1.5, 0, B)[torch.randperm(B, generator=g)]            # a corpus is not one level: the step sequences differ
        wav = (wav / wav.abs().amax(dim=1, keepdim=True) * level[:, None]).to(dev)
        Y = pad_spec(model._forward_transform(model._stft(wav)).unsqueeze(1), mode="zero_pad")
        ids = list(range(B))

        def batched(tol):
            sync()
            t0 = time.perf_counter()
            out, nfe = model.get_ode_sampler(Y, denoise=False, rtol=tol, atol=tol, solver="native", step_control="utterance", seed=7,
                                             streams=ids)(max_nfe=a.max_nfe)
            sync()
            return out, nfe, time.perf_counter() - t0

        def one_by_one(tol):
            sync()
            t0 = time.perf_counter()
            outs, nfes = [], []
            for b in range(B):
                o, n = model.get_ode_sampler(Y[b:b + 1], denoise=False, rtol=tol, atol=tol, solver="native", seed=7, streams=[ids[b]])(max_nfe=a.max_nfe)
                outs.append(o)
                nfes.append(n)
            sync()
            return torch.cat(outs), nfes, time.perf_counter() - t0
        batched(a.warmup_tol)
        model.get_ode_sampler(Y[:1], denoise=False, rtol=a.warmup_tol, atol=a.warmup_tol, solver="native", seed=7, streams=[0])()
        for tol in a.tols:
            rec = dict(batch=B, shape=list(Y.shape), rtol=tol, atol=tol, batched_seconds=[], one_by_one_seconds=[])
            for _ in range(a.runs):
                out_b, nfe, sec = batched(tol)
                st = model.dnn.engine(dev).ode_stats_each()
                rec["batched_seconds"].append(sec)
                out_1, nfes, sec1 = one_by_one(tol)
                rec["one_by_one_seconds"].append(sec1)
                print(f"  batch {B} rtol=atol={tol:g}: batched {sec:.2f} s ({nfe} batch evaluations), one by one {sec1:.2f} s", flush=True)
            per = [u["nfe"] for u in st["utterances"]]
            mb, m1 = statistics.median(rec["batched_seconds"]), statistics.median(rec["one_by_one_seconds"])
            rec.update(batch_evaluations=nfe, rounds=st["rounds"], wasted_utterance_evaluations=st["wasted"],
                       wasted_share=st["wasted"] / float(B * nfe), nfe_per_utterance=per, nfe_one_by_one=nfes,
                       byte_equal=bool(torch.equal(out_b, out_1)) and per == nfes, batched_median_seconds=mb, one_by_one_median_seconds=m1,
                       speedup=m1 / mb, utterances_per_second_batched=B / mb, utterances_per_second_one_by_one=B / m1)
            rows.append(rec)
            print(f"batch {B} {tuple(Y.shape)} rtol=atol={tol:g}: batched {mb:.2f} s, one by one {m1:.2f} s, speed-up {rec['speedup']:.2f}x; "
                  f"rounds {st['rounds']}, nfe per utterance {min(per)}..{max(per)}, wasted {st['wasted']} of {B * nfe} utterance-evaluations "
                  f"({100 * rec['wasted_share']:.1f} %); byte-equal: {rec['byte_equal']}", flush=True)
    res = dict(device=name, nf=a.nf, runs=a.runs, seconds=a.seconds, step_control="utterance", rows=rows)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not all(r["byte_equal"] for r in rows):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
