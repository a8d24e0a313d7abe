"""The window plan of long recordings (sgmse_amd/util/windows.py): pure host arithmetic, no library."""
import pytest

from sgmse_amd.util.windows import plan_windows, window_stream

WS = (64, 128, 192, 256, 512)


def _overlaps(W):
    return sorted({o for o in (0, 1, 7, 32, W // 4, W // 2 - 32) if 0 <= o <= W // 2 - 32})


def test_plan_properties_over_the_grid():
    """W in {64,128,192,256,512}, O in {0, 1, 7, 32, W/4, W/2 - 32} where allowed, every K < 3000: every frame under one or two windows
    and no gap, starts strictly increasing, every window a multiple of 64 frames and at most W, all but the last exactly W, no window
    outside the recording (none is padded); K <= W is the one window (0, K)."""
    plans = 0
    for W in WS:
        for O in _overlaps(W):
            for K in range(1, 3000):
                starts, frames = plan_windows(K, W, O)
                if K <= W:
                    assert (starts, frames) == ([0], [K])
                    continue
                plans += 1
                n = len(starts)
                assert n == len(frames) >= 2 and starts[0] == 0 and starts[-1] + frames[-1] == K
                assert all(b > a for a, b in zip(starts, starts[1:]))
                assert all(T % 64 == 0 and 0 < T <= W for T in frames) and all(T == W for T in frames[:-1])
                assert all(starts[j] == j * (W - O) for j in range(n - 1))
                assert all(starts[j + 1] <= starts[j] + frames[j] for j in range(n - 1))                    # no gap
                assert all(starts[j + 2] >= starts[j] + frames[j] for j in range(n - 2))                    # at most two windows per frame
                assert all(starts[j + 1] + frames[j + 1] > starts[j] + frames[j] for j in range(n - 1))
                last = starts[-2] + frames[-2] - starts[-1]
                assert O <= last <= O + 63 and all(starts[j] + frames[j] - starts[j + 1] == O for j in range(n - 2))
    assert plans > 60000


@pytest.mark.parametrize("args, starts, frames", [((250, 128, 32), [0, 96, 186], [128, 128, 64]),
                                                   ((300, 128, 32), [0, 96, 172], [128, 128, 128]),
                                                   ((129, 128, 32), [0, 65], [128, 64])])
def test_example_plans(args, starts, frames):
    assert plan_windows(*args) == (starts, frames)


@pytest.mark.parametrize("args", [(300, 100, 10), (300, 0, 0), (300, 128, 33), (300, 128, -1), (300, 64, 1), (0, 128, 32)])
def test_refused_arguments(args):
    with pytest.raises(ValueError):
        plan_windows(*args)


def test_window_stream_ids():
    """Window 0 keeps the recording's id; the window index goes into the high word."""
    assert window_stream(5, 0) == 5 and window_stream(5, 2) == 5 + (2 << 32) and window_stream(2 ** 31 + 9, 1) == 2 ** 31 + 9 + 2 ** 32
    assert len({window_stream(s, i) for s in range(40) for i in range(40)}) == 1600
