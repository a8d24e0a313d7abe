#!/usr/bin/env python3
"""Headline benchmark: utterances/s (and RTF) of the reverse-SDE enhancement path on MI355X.

One "step" = one pass of the hot path over one batch of synthetic 16 kHz utterances already resident in HBM:
STFT -> spec_fwd -> pad -> PC sampler (reverse_diffusion + ALD, N=30, snr=0.5 => 60 NCSN++ evaluations, captured as a
hipGraph step replayed N times) -> spec_back -> iSTFT.  Workload = BASELINE.json configs[1] (batch 32, 4 s utterances,
full 65.6 M-parameter NCSN++, fp32, random-init weights).  N > 1: one process per GPU (torch.distributed, RCCL), every
rank enhances its own batch (weak scaling), the only collective is one weight broadcast before the timed region.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the headline (metric, value,
unit, higher_is_better, dtype, ms_per_step, config).  --dump-outputs DIR writes what the last timed step returned (the
enhanced waveforms, float32, and its NFE count) as DIR/<name>.npy; the inputs are seeded, so two builds compare output for
output.  --full adds the extra objects (each can still be left out with its --no-* flag):
  power        socket power and shader clock sampled during the timed region
  roofline     dominant kernel = the 3x3 convolution of the wide U-Net levels.  By default that is conv3x3_wino_kernel
               (kernels_conv_wino.h): 1-D Winograd F(2,3) along the frame axis on top of the fp16x2 operand split (fp32
               operands as two fp16 terms, three partial products on the f16 MFMA pipe, fp32 accumulate).  achieved =
               ALGORITHMIC fp32 FLOPs of its launches / their HIP-event time, measured by one instrumented (eager)
               network evaluation on the same batch right after the timed region; peak = the ceiling of THE FORM THAT
               RUNS: dense f16 MFMA peak / MFMA multiplies issued per algorithmic multiply = 2500/2 (Winograd fp16x2: 12
               K-steps per output pair where the direct form has 18, x 3 partial products), 2500/3 (direct fp16x2),
               2500/6 (bf16x3), 157.3 (fp32 MFMA) TFLOP/s (MI355X_MICROARCH.md) -- so frac <= 1 by construction;
               frac_of_the_direct_form keeps the 2500/3 yardstick of rounds 1-4 beside it.  traffic / mfma_busy: PMC
               passes of THIS command at batch 32 when profiles/ holds them (tools/gpu_visit.sh STEPS=pmcbench)
  cpu_baseline the CPU oracle (oracle/, a torch-fp32 restatement of the reference) timed on this box's host cores on
               a bounded sample, extrapolated to the 60-evaluation run
  other_workloads  configs[2], configs[3], batch 1, and configs[1] again under SGMSE_CONV_SPLIT=0 (exact fp32 MFMA
               everywhere: the arithmetic of the reference itself, BASELINE.md section 3's ceiling applies to it)
  parity       rel. L2 of this build against the reference's own run of configs[1] (tests/golden/pc16k_full.npz, one
               utterance, replayed noise) under the default kernels and under SGMSE_CONV_SPLIT=0
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_EVAL = 1.064686e12       # algorithmic FLOPs of one NCSN++ evaluation at [1,4,256,512]
FP32_PEAK_TFLOPS = 157.3
MFMA16_PEAK_TFLOPS = 2500.0       # dense bf16 / f16 MFMA
DOMINANT = {   # conv split mode -> (kernel, effective peak, how the peak is derived, kernel-name prefix in rocprof output)
    0: ("conv_mfma_pipe_kernel<3,2,2,4> (3x3 fp32 MFMA implicit GEMM, 128 co x 256 px tile)", FP32_PEAK_TFLOPS,
        "fp32 MFMA peak", "void sgmse::conv_mfma_kernel<3, 2, 2, 4"),
    1: ("conv3x3_split_kernel<SplitB3> (3x3 implicit GEMM, exact 3-way bf16 operand split, 6 partial products, fp32 accumulate)",
        MFMA16_PEAK_TFLOPS / 6, "dense bf16 MFMA peak 2500 TFLOP/s / 6 partial products per multiply", "void sgmse::conv3x3_split_kernel<sgmse::SplitB3, 0, 1, 0"),
    2: ("conv3x3_split_kernel<SplitH2> (3x3 implicit GEMM, fp16x2 operand split, 3 partial products, fp32 accumulate)",
        MFMA16_PEAK_TFLOPS / 3, "dense f16 MFMA peak 2500 TFLOP/s / 3 partial products per multiply", "void sgmse::conv3x3_split_kernel<sgmse::SplitH2, 0, 1, 0"),
    # split mode 2 with the Winograd kernel on the wide levels (the default since round 4).  `peak` is the ceiling of the form that
    # actually runs (F(2,3) along T: 12 instead of 18 K-steps per output pair, i.e. 2 MFMA multiplies per algorithmic multiply instead
    # of 3), so `frac` is a real fraction; the direct form's 2500/3 (the yardstick of rounds 1-4) rides along as frac_of_the_direct_form
    3: ("conv3x3_wino_kernel<8,...> (3x3 implicit GEMM, 1-D Winograd F(2,3) along T x fp16x2 operand split, fp32 accumulate; the levels "
        "below 64 x 128 stay on conv3x3_split_kernel<SplitH2>)",
        MFMA16_PEAK_TFLOPS / 2, "dense f16 MFMA peak 2500 TFLOP/s / 2 MFMA multiplies per algorithmic multiply (3 partial products x 12/18 "
                                "K-steps of the F(2,3) form)",
        "void sgmse::conv3x3_wino_kernel<8, 1, 0"),
}
HBM_PEAK_GBS = 8000.0
# how much slower the reference's own NCSNpp module is than the oracle port timed by cpu_baseline (see there)
PORT_VS_REFERENCE = {"factor": 1.70, "calibration": "tools/port_vs_reference.py in the build container, 2026-09-30: reference / port seconds per "
                     "[1,4,256,512] evaluation = 4.01 / 2.42 and 4.23 / 2.35 (8 threads), 6.64 / 3.90 (4 threads); /root/reference is not on the GPU box",
                     "threads_of_the_calibration": [8, 4], "reference_path": "sgmse/backbones/ncsnpp.py:256-419"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32, help="utterances per GPU per step")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--workload", choices=("pc16k", "ode16k", "pc48k"), default="pc16k",
                    help="BASELINE.json configs[1] (default, the headline), configs[2] (fixed-step PF-ODE) or configs[3] (48 kHz)")
    ap.add_argument("--sampler", choices=("pc", "ode"), default=None)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--snr", type=float, default=None)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: power, roofline / per-class profile, cpu_baseline, other_workloads, parity")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-others", action="store_true", help="headline only: skip the configs[2] / configs[3] / batch-1 measurements attached as other_workloads")
    ap.add_argument("--cpu-evals", type=int, default=8, help="timed CPU score evaluations for the baseline sample")
    ap.add_argument("--test-emulator", type=str, default=None, metavar="LIB",
                    help="TEST ONLY (tests/test_host_api.py): run the launcher / collective / reporting logic of this script on CPU "
                         "tensors with the workgroup-emulator build of the kernels and gloo, reduced-width network; never a measurement")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


DUMP_LIMIT_BYTES = 60 * 10**6          # (under the 64 MB cap with the .npy headers)


def dump_outputs(out_dir, arrays, rank, world):
    """Writes {name: array} as out_dir/<name>.npy (float64 stays float64, everything else becomes float32); rank r > 0 adds a
    _rank<r> suffix.  Each rank keeps to its share of DUMP_LIMIT_BYTES: an array that does not fit is replaced by a fixed, seeded
    sample of its flattened elements (the same indices for the same shape in every run)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_LIMIT_BYTES // world
    conv = {}
    for name, v in arrays.items():
        arr = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
        conv[name] = arr.astype(np.float64 if arr.dtype == np.float64 else np.float32)
    for name, arr in sorted(conv.items(), key=lambda kv: kv[1].nbytes):        # the small ones first: the largest takes the rest
        if arr.nbytes > budget:
            keep = budget // arr.itemsize
            idx = np.sort(np.random.default_rng(0).choice(arr.size, size=keep, replace=False))
            arr = arr.reshape(-1)[idx]
        np.save(os.path.join(out_dir, (name if rank == 0 else f"{name}_rank{rank}") + ".npy"), arr)
        budget -= arr.nbytes


class PowerSampler:
    """Socket power and shader clock from rocm-smi, sampled in a background thread during the timed region (rank 0, N = 1).
    Evidence for the clock the path actually ran at: the direct fp16x2 kernel of rounds 2-3 sat at the 1400 W cap at 1.5-1.7 GHz
    (profiles/r02_power_probe.txt); the Winograd kernel runs below the cap at 1.9-2.0 GHz (profiles/r04_power_probe.txt), and the
    share of the NOMINAL (2.4 GHz) MFMA peak in `roofline` is bounded by that clock too."""

    def __init__(self, period=0.5):
        import threading
        self.period, self.rows = period, []
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import subprocess
        while not self._stop.is_set():
            try:
                r = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=5)
                card = next(iter(json.loads(r.stdout).values()))
                p = next((float(v) for k, v in card.items() if "Power" in k and "(W)" in k), None)
                c = next((float(v.strip("()").lower().replace("mhz", "")) for k, v in card.items() if k.lower().startswith("sclk clock speed")), None)
                if p is not None:
                    self.rows.append((p, c))
            except Exception:       # noqa: BLE001 -- rocm-smi missing or busy: no power evidence, the benchmark goes on
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._th.join(timeout=10)

    def summary(self):
        if not self.rows:
            return None
        ps = [r[0] for r in self.rows]
        cs = [r[1] for r in self.rows if r[1]]
        return {"samples": len(ps), "socket_power_w_mean": sum(ps) / len(ps), "socket_power_w_max": max(ps),
                "sclk_mhz_mean": (sum(cs) / len(cs)) if cs else None,
                "note": "rocm-smi during the timed region; the MI355X socket power cap is 1400 W and the maximum shader clock 2400 MHz"}


def spawn_ranks(a):
    """`bench.py --gpus N` started by hand (no torchrun around it): start the N ranks ourselves, one per GPU, exactly as the
    driver does (python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...), and hand their exit code back."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def usable_cpus():
    """CPUs this process may actually use: affinity mask, capped by a cgroup quota if one is set."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per))))
    except Exception:
        pass
    return n


def cpu_baseline(state, n_evals, N, snr, frames=512):
    """Oracle (port of the reference's CPU path) on the host cores, B=1.  Bounded sample (~10-20 s of CPU work): the score
    network is timed on `n_evals` full [1,4,256,512] evaluations (a shorter `frames` slice would be scaled linearly: the
    network is fully convolutional in T and attention is 0.08 % of the FLOPs); 60 evaluations extrapolated."""
    import torch
    from oracle import ncsnpp_oracle as NO, sde_oracle as SO, stft_oracle as FO
    cores = min(usable_cpus(), 32)      # torch's intra-op pool stops scaling (and oversubscribes) far below 256 threads
    torch.set_num_threads(cores)
    cfg = NO.NetCfg.for_variant("ncsnpp")
    P = {k: v.detach().cpu().float() for k, v in state.items()}
    fc = FO.FrontCfg()
    g = torch.Generator().manual_seed(0)
    y = torch.randn(1, 64000, generator=g)
    with torch.no_grad():
        t0 = time.perf_counter()
        Y = FO.pad_spec(FO.spec_fwd(FO.stft(y / y.abs().max(), fc), fc)[None], "zero_pad")
        sde = SO.OUVE(1.5, 0.05, 0.5, N)
        rep = SO.NoiseReplay(7)
        x = sde.prior(Y, rep)
        t_front = time.perf_counter() - t0
        tvec = torch.ones(1)
        xs, Ys = x[..., :frames].contiguous(), Y[..., :frames].contiguous()
        NO.score_fn(P, cfg, xs, Ys, tvec)                     # warm-up (thread pools, oneDNN primitives)
        t0 = time.perf_counter()
        for _ in range(n_evals):
            s = NO.score_fn(P, cfg, xs, Ys, tvec)
        t_eval = (time.perf_counter() - t0) / n_evals * (Y.shape[-1] / frames)
        s = torch.zeros_like(x)
        t0 = time.perf_counter()
        x2, _ = SO.ald_update(sde, lambda a, b, c: s, x, Y, tvec, snr, rep)
        x3, xm = SO.revdiff_update(sde, lambda a, b, c: s, x2, Y, tvec, torch.tensor(1.0 / N), rep)
        t_glue = time.perf_counter() - t0
        t0 = time.perf_counter()
        FO.istft(FO.spec_back(xm[0, 0], fc), fc, 64000)
        t_back = time.perf_counter() - t0
    per_utt = t_front + t_back + 2 * N * t_eval + N * t_glue
    # Calibration of the port against the module it restates (tools/port_vs_reference.py: the imported reference NCSNpp and the port
    # on the same [1,4,256,512] evaluation, interleaved runs, build container, 2026-09-30): 8 threads 4.01 s vs 2.42 s (1.66), repeat
    # 4.23 vs 2.35 (1.80); 4 threads 6.64 vs 3.90 (1.70).  The ratio does not move with the thread count (the container has 8 CPUs:
    # 16 threads cannot be measured there), so the same factor is applied to the box's `cores` threads.
    factor = PORT_VS_REFERENCE["factor"]
    return {"value": 1.0 / per_utt, "unit": "utterances/s", "cores": cores, "kind": "port",
            "sample": f"{n_evals} timed NCSN++ evaluations at [1,4,256,{frames}] after 1 warm-up, scaled x{512 // frames} to the "
                      f"512-frame utterance ({t_eval:.2f} s per full evaluation on {cores} threads) + front-end + one PC step of "
                      f"sampler glue, extrapolated to {2 * N} evaluations; B=1, 4 s utterance",
            "seconds_per_eval": t_eval, "rtf": per_utt / 4.0,
            "reference_equivalent": {"value": 1.0 / (per_utt * factor), "unit": "utterances/s", "rtf": per_utt * factor / 4.0,
                                     "seconds_per_eval": t_eval * factor, **PORT_VS_REFERENCE},
            "port_vs_reference": f"the port is {factor:.2f}x FASTER than the reference module it restates (no autograd bookkeeping, fused padding, "
                                 "FIR as closed-form taps instead of upfirdn2d_native's single-channel convolutions): the reference's own CPU "
                                 "rate on this box is reference_equivalent.value"}


def hbm_traffic_of_dominant_kernel(prefix):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE in
    separate passes, read side calibrated x2 in the same run; tools/summarize_hbm.py).  rocprofv3 --pmc segfaults on the
    full bench command, so the counters are collected on the kernel micro-benchmark at the dominant layer shape."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*hbm_traffic*.json")))
    for f in reversed(files):
        d = json.load(open(f))
        for k, v in d.items():
            if k.startswith(prefix):
                alg = d.get("_algorithmic_bytes_per_launch_of_the_benchmarked_conv")
                note = f"{os.path.basename(f)}: 3x3 128->128 @256x512, B=8, fused producer+residual epilogue, median {v.get('median_duration_us_under_pmc')} us under the counters"
                return v["hbm_bytes_per_launch"], note + (f"; algorithmic bytes of that launch = {alg:.4g}" if alg else "")
    return None, "no committed PMC profile holds the dominant kernel"


def pmc_of_the_bench_run(prefix, batch, workload):
    """COMMITTED counters of this command's launches of the dominant kernel (tools/gpu_visit.sh STEPS=pmcbench: rocprofv3 --pmc passes over
    `bench.py --batch B --steps 1 --warmup 0 --N 2 --no-graph ...`, one pass per counter group, summarised by
    tools/summarize_pmc_bench.py into profiles/*pmc_bench_b<batch>.json).  They are counters of an EARLIER execution of the command, not of
    the process that prints the line, so the summary's `_meta` (command, workload, batch, git commit, hash of the kernel sources) decides
    whether they apply: only a file of the same workload and batch is used, and `pmc_matches_this_build` says whether the kernel sources
    have changed since.  `traffic` = calibrated FETCH_SIZE + WRITE_SIZE per launch (the calibration rows of the same pass, `_meta` /
    `fetch_calibration`); `attention` = the same passes' rows of attn_core_kernel (MFMA utilisation of the QK^T / PV contractions)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*pmc_bench_b{batch}.json")))
    for f in reversed(files):
        d = json.load(open(f))
        meta = d.get("_meta") or {}
        if meta.get("workload", "pc16k") != workload or int(meta.get("batch", batch)) != batch:
            continue
        row = next((v for k, v in d.items() if k.startswith(prefix.replace("void ", ""))), None)
        if not row:
            continue
        src = (f"{os.path.basename(f)}: committed rocprofv3 --pmc passes over `{meta.get('command', 'bench.py --batch %d --N 2 --no-graph' % batch)}` "
               f"at commit {meta.get('commit', '?')} ({row.get('launches')} launches of the dominant kernel instantiation)")
        upd = {"pmc_source": src, "pmc_source_hash": meta.get("source_hash"), "pmc_matches_this_build": meta.get("source_hash") == source_hash()}
        if row.get("hbm_bytes_per_launch") is not None:
            upd["traffic"] = row["hbm_bytes_per_launch"]
            upd["traffic_source"] = src
            upd["traffic_note"] = (f"calibrated FETCH_SIZE + WRITE_SIZE per launch, mean over the run's launches; raw counters "
                                   f"{row.get('fetch_bytes_per_launch_raw')} + {row.get('write_bytes_per_launch_raw')}; algorithmic bytes per "
                                   f"launch (mean) {row.get('algorithmic_bytes_per_launch')}")
            upd["fetch_calibration"] = d.get("_calibration")
        for k in ("mfma_busy", "effective_clock_ghz", "valu_per_mfma", "lds_conflict_frac"):
            if row.get(k) is not None:
                upd[k] = row[k]
        att = next((v for k, v in d.items() if "attn_core_kernel" in k), None)
        if att:
            upd["attention"] = {k: att.get(k) for k in ("launches", "mean_duration_us_under_pmc", "mfma_busy", "effective_clock_ghz", "valu_per_mfma",
                                                         "lds_conflict_frac") if att.get(k) is not None}
            upd["attention"]["kernel"] = "attn_core_kernel (QK^T and PV on v_mfma_f32_32x32x2_f32; layerspp.py:82-88)"
        return upd
    return {}


CALIB_BYTES = 1 << 30


def pmc_calibration_launches(dev):
    """SGMSE_PMC_CALIB=1 (tools/gpu_visit.sh STEPS=pmcbench): four launches of known size -- a coalesced 1 GiB read and write stream at
    8 and at 16 bytes per lane (calib_stream_kernel) -- in front of the run, so that the FETCH_SIZE / WRITE_SIZE pass over THIS command
    holds its own calibration rows (tools/summarize_pmc_bench.py divides the known bytes by what the counter reported for them)."""
    from sgmse_amd import _lib
    ctx = _lib.Context(str(dev))
    for mode in (0, 1):
        for width in (8, 16):
            ms = ctx.calib_stream(mode, width, CALIB_BYTES)
            print(f"[pmc-calib] {'write' if mode else 'read'} {width} B/lane: {CALIB_BYTES} bytes in {ms:.3f} ms = {CALIB_BYTES / ms / 1e9:.2f} TB/s", file=sys.stderr)
    del ctx


def source_hash():
    """sha256 over the kernel sources the library is built from: ties a committed counter summary to the build it was taken on."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "sgmse_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "sgmse_amd", "csrc", "*.hip"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def parity_leg(env):
    """CHECKER LEG (like cpu_baseline: the only other place this script touches oracle/ and tests/): configs[1] on ONE utterance with
    replayed noise against the reference's own run (tests/golden/pc16k_full.npz, written by oracle/make_golden_full.py from the imported
    reference), under the default kernels and under SGMSE_CONV_SPLIT=0 (exact fp32 MFMA everywhere).  ~3 s of GPU time."""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import parity as TP
    res = {"fixture": "tests/golden/pc16k_full.npz (the reference's NCSNpp + OUVESDE + pc_sampler, 60 NFE, one 4 s utterance, replayed noise)",
           "gate": {"spectrogram": TP.SAMPLER_TOL, "waveform": TP.WAVE_TOL}}
    saved = os.environ.get("SGMSE_CONV_SPLIT")
    try:
        for key, mode in (("default kernels", None), ("SGMSE_CONV_SPLIT=0 (exact fp32 MFMA everywhere)", "0")):
            if mode is None:
                os.environ.pop("SGMSE_CONV_SPLIT", None)
                if saved is not None:
                    os.environ["SGMSE_CONV_SPLIT"] = saved
            else:
                os.environ["SGMSE_CONV_SPLIT"] = mode
            e_spec, e_wave, nfe = TP.run_full_config(str(env.dev), "pc16k_full")
            res[key] = {"rel_l2_spectrogram": e_spec, "rel_l2_waveform": e_wave, "nfe": nfe}
    finally:
        os.environ.pop("SGMSE_CONV_SPLIT", None)
        if saved is not None:
            os.environ["SGMSE_CONV_SPLIT"] = saved
    return res


WORKLOADS = {
    "pc16k": dict(backbone="ncsnpp", sr=16000, sampler="pc", N=30, snr=0.5, batch=32, sde=dict(theta=1.5, sigma_min=0.05, sigma_max=0.5),
                  front=dict(), pad="zero_pad", F=256, flop=FLOP_PER_EVAL, cfg="configs[1]"),
    "ode16k": dict(backbone="ncsnpp", sr=16000, sampler="ode", N=30, snr=0.5, batch=32, sde=dict(theta=1.5, sigma_min=0.05, sigma_max=0.5),
                   front=dict(), pad="zero_pad", F=256, flop=FLOP_PER_EVAL, cfg="configs[2]"),
    "pc48k": dict(backbone="ncsnpp_48k", sr=48000, sampler="pc", N=50, snr=0.33, batch=16, sde=dict(theta=2.0, sigma_min=0.1, sigma_max=1.0),
                  front=dict(n_fft=1534, hop_length=384, spec_factor=0.065, spec_abs_exponent=0.667), pad="reflection", F=768,
                  flop=3.187556e12, cfg="configs[3]"),
}


class Env:
    """What every measurement of this process shares: device, ranks, fences."""

    def __init__(self, a):
        import torch
        import torch.distributed as dist
        from sgmse_amd import _lib
        self.torch, self.dist = torch, dist
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != a.gpus and self.rank == 0:
            print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={self.world}; reporting n_gpus={self.world}", file=sys.stderr)
        self.emu = a.test_emulator is not None
        if self.emu:
            self.dev = torch.device("cpu")
            _lib.load_library(a.test_emulator)
        else:
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs an MI355X: sgmse_amd has no CPU path")
            if self.local >= torch.cuda.device_count():
                raise SystemExit(f"rank {self.rank}: LOCAL_RANK {self.local} but only {torch.cuda.device_count()} GPU(s) visible")
            torch.cuda.set_device(self.local)
            self.dev = torch.device("cuda", self.local)
            _lib.load_library()
        if self.world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if self.emu:
                dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
            else:
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev)   # "nccl" is RCCL on ROCm
        self.sync = (lambda: None) if self.emu else torch.cuda.synchronize

    def barrier(self):
        if self.world > 1:
            self.dist.barrier(**({} if self.emu else {"device_ids": [self.local]}))

    def fence(self):
        self.barrier()
        self.sync()


def measure(env, a, workload, batch, steps, warmup, sampler=None, N=None, snr=None, seconds=4.0, want_power=False, profile=False):
    """W untimed + K timed steps of one workload on every rank of `env`; returns (JSON object on rank 0 / None elsewhere, model,
    {name: output of the last timed step}).  `profile`: one instrumented evaluation after the timed region (roofline objects)."""
    torch, dist = env.torch, env.dist
    from sgmse_amd.model import ScoreModel
    from sgmse_amd.parallel import broadcast_backbone_weights
    wl = WORKLOADS[workload]
    sampler = sampler or wl["sampler"]
    N = N or wl["N"]
    snr = snr if snr is not None else wl["snr"]
    world, rank, dev, emu = env.world, env.rank, env.dev, env.emu
    L = int(seconds * wl["sr"])
    torch.manual_seed(0)
    net_kw = dict(nf=32) if emu else {}                                                    # full-size network unless --test-emulator
    model = ScoreModel(wl["backbone"], "ouve", N=N, sr=wl["sr"], **wl["sde"], **wl["front"], **net_kw)   # random init
    model.to(dev).eval()
    bcast_ms = comm_setup_ms = None
    if world > 1:
        # The first collective of a process carries RCCL's lazy communicator set-up (0.5-3 s at 8 ranks): one 4-byte broadcast takes
        # it (reported apart), so that weight_broadcast_ms is the 262 MB transfer over xGMI the north star names and nothing else.
        env.sync()
        t0 = time.perf_counter()
        dist.broadcast(torch.zeros(1, device=dev), src=0)
        env.sync()
        comm_setup_ms = (time.perf_counter() - t0) * 1e3
        env.fence()
        t0 = time.perf_counter()
        broadcast_backbone_weights(model.dnn, src=0)
        env.sync()
        bcast_ms = (time.perf_counter() - t0) * 1e3

    g = torch.Generator().manual_seed(1000 + rank)
    y = torch.randn(batch, L, generator=g).to(dev)            # resident in HBM before the timed region

    def step(i):
        return model.enhance_batch(y, N=N, snr=snr, sampler_type=sampler, seed=17 + i, use_graph=not a.no_graph, pad_mode=wl["pad"])

    nfe = 0
    for i in range(warmup):
        _, nfe = step(i)
    env.fence()
    power = PowerSampler() if (want_power and rank == 0 and world == 1 and not emu) else None
    if power:
        power.__enter__()
    t0 = time.perf_counter()
    for i in range(steps):
        x_hat, nfe = step(warmup + i)
    env.fence()
    elapsed = time.perf_counter() - t0
    if power:
        power.__exit__()
    per_rank = [elapsed]
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(every, tt)
        per_rank = [float(t.item()) for t in every]
        elapsed = max(per_rank)                               # the job is done when its slowest rank is
    assert torch.isfinite(x_hat).all()
    last = {"x_hat": x_hat, "nfe": torch.tensor(float(nfe), dtype=torch.float64)}
    if rank != 0:
        return None, model, last

    ctx = model.dnn.engine(dev)
    utts = world * batch * steps
    hop = wl["front"].get("hop_length", 128)
    T = ((L // hop + 1) + 63) // 64 * 64
    flop_eval = wl["flop"] * (T / 512.0)
    out = {
        "metric": ("utterances/sec, SGMSE+ NCSN++ PC N=30 (reverse_diffusion + ALD, 60 NFE), 16 kHz 4 s utterances"
                   if (workload == "pc16k" and sampler == "pc" and N == 30)
                   else f"utterances/sec, {wl['backbone']} {sampler.upper()} N={N}, {wl['sr'] // 1000} kHz {seconds:g} s utterances"),
        "value": utts / elapsed, "unit": "utterances/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": {0: "f32", 1: "f32 (bf16x3-split products, fp32 accumulate)",
                  2: "f32 (fp16x2-split products, fp32 accumulate)"}[ctx.conv_split_mode()],
        "dtype_note": {0: "exact fp32 MFMA everywhere",
                       1: "fp32 operands and accumulation; wide 3x3 / 1x1 conv products formed from exact 3-way bf16 operand splits on the bf16 MFMA pipe",
                       2: "fp32 operands and accumulation; wide 3x3 / 1x1 conv products formed from fp16x2 operand splits (exact per-utterance power-of-two "
                          "scaling from the data's own range) on the f16 MFMA pipe; error vs fp64 measured at or below the fp32-MFMA kernels' "
                          "(DESIGN.md section 3)"}[ctx.conv_split_mode()],
        "data": "synthetic (N(0,1) waveforms, random-init weights of the full architecture)",
        "config": {"workload": f"BASELINE {wl['cfg']}: {wl['backbone']} ({ctx.param_count() / 1e6:.1f}M params) "
                               f"{sampler.upper()} sampler N={N}, batch={batch} x {seconds:g} s @{wl['sr'] // 1000} kHz per GPU, "
                               f"hipGraph-captured step",
                   "batch_per_gpu": batch, "F": wl["F"], "T": T, "nfe": nfe, "sampler": sampler, "snr": snr,
                   "arena_gb": ctx.arena_bytes() / 1e9,
                   "parallelism": f"utterance-sharded x{world} (weights broadcast once over RCCL)"},
        "rtf": elapsed / (utts * seconds),
        "seconds_per_utterance_batch": elapsed / steps,
        "path_tflops": batch * steps * nfe * flop_eval / elapsed / 1e12,
        "path_frac_of_fp32_peak": batch * steps * nfe * flop_eval / elapsed / 1e12 / FP32_PEAK_TFLOPS,
    }
    if power and power.summary():
        out["power"] = power.summary()
    out["graph_captures_rank0"] = ctx.graph_captures()   # 1: the seed changes per step, the captured step does not
    if world > 1:
        out["weight_broadcast_ms"] = bcast_ms
        out["weight_broadcast_gbps"] = ctx.param_count() * 4 / (bcast_ms * 1e-3) / 1e9 if bcast_ms else None
        out["communicator_setup_ms"] = comm_setup_ms     # the 4-byte warm-up broadcast: RCCL's lazy init, once per process
        out["per_rank_utt_per_s"] = [batch * steps / t for t in per_rank]
        out["collective_backend"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                                     "note": "the only collective: one weight broadcast before the timed region"}
    if emu:
        out["data"] = "TEST ONLY: CPU workgroup emulator, reduced-width network -- not a measurement"
    if profile and not emu:
        Y = torch.randn(batch, 2, wl["F"], T, dtype=torch.complex64, device=dev) * 0.3
        tt = torch.full((batch,), 0.5, device=dev)
        prof, _ = ctx.profile_forward(Y, tt)
        dom = prof["conv3x3_wide"]
        ach = dom["work"] / (dom["ms"] * 1e-3) / 1e12 if dom["ms"] > 0 else 0.0
        wino = ctx.conv_split_mode() == 2 and ctx.conv_winograd()
        kname, peak, peak_note, prefix = DOMINANT[3 if wino else ctx.conv_split_mode()]
        traffic, traffic_note = hbm_traffic_of_dominant_kernel(prefix)
        out["roofline"] = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                           "frac": ach / peak, "traffic": traffic, "traffic_note": traffic_note,
                           "traffic_source": "committed rocprofv3 PMC passes over the kernel micro-benchmark at the dominant layer shape "
                                             "(not counters of this run: rocprofv3 --pmc does not survive the full bench command)",
                           "kernel": kname, "peak_note": peak_note, "achieved_vs_fp32_mfma_peak": ach / FP32_PEAK_TFLOPS,
                           "launches_per_eval": dom["launches"],
                           "avg_launch_us": dom["ms"] * 1e3 / max(dom["launches"], 1),
                           "flop_per_launch_avg": dom["work"] / max(dom["launches"], 1)}
        if wino:
            out["roofline"]["peak_of_the_direct_form"] = MFMA16_PEAK_TFLOPS / 3
            out["roofline"]["frac_of_the_direct_form"] = ach / (MFMA16_PEAK_TFLOPS / 3)
        out["roofline"].update(pmc_of_the_bench_run(prefix, batch, workload))
        classes = {}
        for k, v in prof.items():
            rate = v["work"] / (v["ms"] * 1e-3) if v["ms"] > 0 else 0.0
            classes[k] = {"ms": round(v["ms"], 3), "launches": v["launches"],
                          ("tflops" if v["unit"] == "flop" else "gbps"): rate / (1e12 if v["unit"] == "flop" else 1e9)}
        out["kernel_classes_one_eval"] = classes
    return out, model, last


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(a))
    wl = WORKLOADS[a.workload]
    if a.batch == 32 and wl["batch"] != 32:
        a.batch = wl["batch"]
    env = Env(a)
    if os.environ.get("SGMSE_PMC_CALIB") and env.rank == 0 and not env.emu:
        pmc_calibration_launches(env.dev)
    out, model, last = measure(env, a, a.workload, a.batch, a.steps, a.warmup, sampler=a.sampler, N=a.N, snr=a.snr, seconds=a.seconds,
                               want_power=a.full, profile=a.full and not a.no_profile)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, last, env.rank, env.world)
    del last
    headline = (a.workload == "pc16k" and a.batch == 32 and a.sampler in (None, "pc") and a.N in (None, 30) and a.seconds == 4.0)
    if a.full and env.rank == 0 and not a.no_cpu_baseline and env.world == 1 and a.workload == "pc16k" and not env.emu:
        out["cpu_baseline"] = cpu_baseline(model.dnn.state_dict(), a.cpu_evals, a.N or wl["N"], a.snr if a.snr is not None else wl["snr"])
    if a.full and env.world == 1 and headline and not a.no_others and not env.emu:
        # The other BASELINE.json configurations one GPU holds, and the per-file (batch 1) latency of the drop-in path, in the same
        # line, each with its own roofline object: 1 warm-up + 1 (batch 1: 3) timed steps after the headline's timed region.
        del model
        import gc
        others = {}
        exact_key = "configs[1] under SGMSE_CONV_SPLIT=0: exact fp32 MFMA everywhere (the reference's own arithmetic; BASELINE.md section 3's ceiling)"
        for key, (wname, batch, steps, envs) in {
                "configs[2] ode16k": ("ode16k", 32, 1, {}), "configs[3] pc48k": ("pc48k", 16, 1, {}),
                "configs[0] shape on the GPU: pc16k batch 1 (per-file loop of enhancement.py)": ("pc16k", 1, 3, {}),
                exact_key: ("pc16k", 32, 1, {"SGMSE_CONV_SPLIT": "0"})}.items():
            gc.collect()
            env.torch.cuda.empty_cache()
            saved = {k: os.environ.get(k) for k in envs}
            os.environ.update(envs)                       # (the engine re-reads its switches when a model is built)
            try:
                o, m, _ = measure(env, a, wname, batch, steps, 1, profile=not a.no_profile)
                del m
                others[key] = {k: o[k] for k in ("metric", "value", "unit", "ms_per_step", "rtf", "steps", "warmup", "dtype", "config", "roofline",
                                                 "kernel_classes_one_eval", "graph_captures_rank0") if k in o}
            except Exception as e:      # noqa: BLE001 -- the headline stands on its own
                others[key] = {"error": f"{type(e).__name__}: {e}"}
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        out["other_workloads"] = others
        gc.collect()
        env.torch.cuda.empty_cache()
        try:
            out["parity"] = parity_leg(env)
        except Exception as e:          # noqa: BLE001
            out["parity"] = {"error": f"{type(e).__name__}: {e}"}
    if env.rank == 0:
        print(json.dumps(out), flush=True)
    if env.world > 1:
        env.barrier()
        env.dist.destroy_process_group()


if __name__ == "__main__":
    main()
