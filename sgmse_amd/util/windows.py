"""The window plan of a long recording: how a spectrogram of K frames is cut into windows of at most ``window_frames`` frames that
overlap their neighbours by at least ``overlap_frames`` (``ScoreModel.enhance_long``, ``python -m sgmse_amd.enhancement
--window_frames``).  Pure host arithmetic; not in the reference, which enhances every recording as one spectrogram."""
from __future__ import annotations

from typing import List, Tuple


def _ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


def plan_windows(K: int, window_frames: int, overlap_frames: int) -> Tuple[List[int], List[int]]:
    """(starts, frames) of the windows over K frames, W = window_frames, O = overlap_frames, P = W - O.

    K <= W: the one window (0, K) -- the caller takes the ordinary path (``pad_spec`` and the model's pad mode).
    K > W:  n = ceil((K - O) / P) windows; window j < n - 1 starts at j P and has W frames; the last one covers the LAST
            ceil64(K - (n - 1) P) frames of the recording: it is pulled left instead of padded, so it overlaps its neighbour by
            O .. O + 63 frames.  Every window is a multiple of 64 frames (what the network takes) and none is padded.
    W % 64 == 0 and 0 <= O <= W / 2 - 32 (else ValueError): the last window then starts behind the end of window n - 3
    (K - T_last > (n - 1) P - 64 >= (n - 3) P + W  <=>  W - 2 O >= 64), so no frame lies under three windows."""
    K, W, O = int(K), int(window_frames), int(overlap_frames)
    if K < 1:
        raise ValueError(f"a spectrogram has at least one frame, got {K}")
    if W < 64 or W % 64 != 0:
        raise ValueError(f"window_frames must be a positive multiple of 64, got {W}")
    if not 0 <= O <= W // 2 - 32:
        raise ValueError(f"overlap_frames must lie in [0, window_frames / 2 - 32] = [0, {W // 2 - 32}] (every frame under at most two "
                         f"windows), got {O}")
    if K <= W:
        return [0], [K]
    P = W - O
    n = -(-(K - O) // P)
    T_last = _ceil64(K - (n - 1) * P)
    return [j * P for j in range(n - 1)] + [K - T_last], [W] * (n - 1) + [T_last]


def plan_windows_uniform(K: int, window_frames: int, overlap_frames: int) -> List[int]:
    """Starts of the windows of ``enhance_long(window_blend="score")`` over K frames: ALL of exactly W = window_frames frames
    (the network runs at one shape), W = window_frames, O = overlap_frames, P = W - O; the argument checks of ``plan_windows``.

    K <= W: [0] -- one window; the caller takes the ordinary path, as with ``plan_windows``.
    K > W:  n = ceil((K - O) / P) windows (``plan_windows``' count); window j < n - 1 starts at j P, the last one at K - W: pulled
            left, never padded.  K - (n - 1) P lies in (O, W], so the starts strictly increase and the last overlap is at least O.
            The last window starts inside the overlap of windows n - 3 and n - 2 when K - (n - 1) P < 2 O: a frame may lie under
            THREE windows (never four: K - W > (n - 2) P >= (n - 4) P + W, as W >= 2 O), which sgmse_window_blend handles."""
    K, W, O = int(K), int(window_frames), int(overlap_frames)
    plan_windows(K, W, O)                                     # (the argument checks)
    if K <= W:
        return [0]
    P = W - O
    n = -(-(K - O) // P)
    return [j * P for j in range(n - 1)] + [K - W]


def window_stream(stream: int, i: int) -> int:
    """Noise-stream id of window i of the recording whose own id is ``stream``: window 0 keeps the recording's id, so a recording
    of one window draws the noise it draws without windows; the window index goes into the id's high word."""
    return (int(stream) + (int(i) << 32)) & (2 ** 64 - 1)


WINDOW_NOISE = ("window", "recording")


def window_noise_plan(stream: int, starts: List[int], K: int, window_noise: str):
    """(stream ids, noise geometry) of the windows starting at ``starts`` of a recording of K frames whose id is ``stream``.
    'window': window i draws from ``window_stream(stream, i)`` at the index inside the window (geometry None: the default).
    'recording': every window draws from the recording's own id at the index of the recording's frame -- geometry (starts[i], K),
    ``Context.set_noise_frames`` -- so the windows over a frame share its draws."""
    if window_noise not in WINDOW_NOISE:
        raise ValueError(f"window_noise must be 'window' or 'recording', got {window_noise!r}")
    if window_noise == "recording":
        return [window_stream(stream, 0)] * len(starts), [(int(a), int(K)) for a in starts]
    return [window_stream(stream, i) for i in range(len(starts))], None
