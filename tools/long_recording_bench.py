#!/usr/bin/env python3
"""Windowed enhancement of one long recording against the bench rate: a synthetic recording (default 10 minutes at 16 kHz) through
ScoreModel.enhance_long (random-init full-width ncsnpp, PC N=30, W = 512 frames, O = 64, 32 windows per sampler call) on one GPU,
next to the same process's plain batch-32 x 4 s step (the tools/dir_job_bench.py pattern).  Reports seconds of audio per second for
both, their ratio (arithmetic alone says 1 / (W / (W - O)) = 0.875) and the activation arena.  Every GPU step runs under its own
time limit: when one runs out the process ends there and starts nothing more.  Prints one JSON object per ``--window_blend`` mode
('output': every window its own reverse process, cross-faded; 'score': one reverse process, the network windowed); several modes
run one after the other in the one process, next to the one plain step.

    python tools/long_recording_bench.py [--minutes 10] [--window_frames 512] [--window_overlap 64] [--batch 32] [--N 30]
                                         [--window_blend output [score]] [--out FILE]
"""
import argparse
import contextlib
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextlib.contextmanager
def limit(seconds, what):
    def stop(*_):
        raise SystemExit(f"{what}: time limit of {seconds} s ran out")
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--window_frames", type=int, default=512)
    ap.add_argument("--window_overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--window_blend", type=str, nargs="+", choices=("output", "score"), default=["output"])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from sgmse_amd.data_module import SpecsDataModule
    from sgmse_amd.model import ScoreModel

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, N=30, t_eps=0.03,
                       data_module_cls=SpecsDataModule, n_fft=510, hop_length=128, spec_factor=0.15, spec_abs_exponent=0.5)
    model.to(dev).eval()
    eng = model.dnn.engine(dev)
    sync = torch.cuda.synchronize
    kw = dict(N=a.N, snr=0.5)

    # the bench step: batch x 4 s, waveforms resident in HBM (warm-up: arena plan + graph capture, then two timed calls)
    y = torch.randn(a.batch, 64000, generator=torch.Generator().manual_seed(1)).to(dev)
    with limit(240, "plain step"):
        model.enhance_batch(y, seed=1, **kw)
        sync()
        t0 = time.perf_counter()
        for i in range(2):
            model.enhance_batch(y, seed=2 + i, **kw)
        sync()
        plain_s = (time.perf_counter() - t0) / 2
    arena_plain = eng.arena_bytes()

    L = int(a.minutes * 60 * 16000)
    rec = 0.1 * torch.randn(L, generator=torch.Generator().manual_seed(2))
    P = a.window_frames - a.window_overlap
    lines = []
    for mode in a.window_blend:
        win = dict(window_frames=a.window_frames, overlap_frames=a.window_overlap, batch_size=a.batch, window_blend=mode)
        with limit(120, f"windowed warm-up ({mode})"):          # one sampler call's worth of windows
            warm = min(L, (a.batch * P + a.window_overlap - 1) * 128)
            model.enhance_long(rec[:warm], seed=3, **win, **kw)
            sync()
        captures = eng.graph_captures()
        with limit(600, f"windowed run ({mode})"):
            t0 = time.perf_counter()
            x, info = model.enhance_long(rec, seed=4, **win, **kw)
            sync()
            long_s = time.perf_counter() - t0
        ok = bool(torch.isfinite(x).all()) and x.shape == (L,)
        plain_rate = a.batch * 4.0 / plain_s
        long_rate = (L / 16000) / long_s
        res = {"window_blend": mode, "minutes": a.minutes, "frames": L // 128 + 1, "windows": len(info["starts"]),
               "last_window_frames": info["frames"][-1],
               "sampler_calls": len(info["nfe"]), "window_frames": a.window_frames, "window_overlap": a.window_overlap, "batch": a.batch,
               "N": a.N, "finite": ok, "wall_s_windowed": long_s, "audio_s_per_s_windowed": long_rate,
               "wall_s_plain_step": plain_s, "audio_s_per_s_plain_step_same_process": plain_rate,
               "windowed_over_plain": long_rate / plain_rate, "expected_from_arithmetic": P / a.window_frames,
               "arena_bytes_plain_step": arena_plain, "arena_bytes_windowed": eng.arena_bytes(),
               "graph_captures": eng.graph_captures(), "graph_captures_timed_run": eng.graph_captures() - captures,
               "graph_updates": eng.graph_updates()}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

if __name__ == "__main__":
    main()
