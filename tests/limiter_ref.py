"""The oracle of the limiter tests: the true-peak meter and the look-ahead limiter as DESIGN 4.22 defines them, restated in fp64
with numpy and scipy -- scipy.signal.upfirdn for the oversampling, numpy windows for the hold and the average, a plain recurrence
for the release.  Nothing here is shared with the product code (csrc/limiter.h, gsv_tts_lite_amd/limiter.py)."""
import functools
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.signal import upfirdn

TILE = 1024                 # LIM_TILE: the tests sit on its edges; the oracle itself knows no tile


@functools.lru_cache(maxsize=None)
def taps():
    """the 49-tap table: sinc(k / 4) * kaiser(49, beta = 8), k = -24 .. 24"""
    return np.sinc(np.arange(-24, 25) / 4.0) * np.kaiser(49, 8.0)


def phase_sum():
    """S: the largest per-phase sum of |tap|"""
    return max(float(np.abs(taps()[p::4]).sum()) for p in range(4))


def envelope(x):
    """e[n] = max |u[4n-3 .. 4n+3]|, u = x oversampled 4x, zeros outside the clip"""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0)
    u = np.abs(upfirdn(taps(), x, up=4))            # u[i] sits at index i + 24
    a = u[21: 4 * (n - 1) + 28]                     # u[-3 .. 4(n-1)+3]
    return sliding_window_view(a, 7)[::4].max(axis=1)


def true_peak(x):
    e = envelope(x)
    return float(e.max()) if len(e) else 0.0


def times(rate, lookahead_ms=1.5, release_ms=50.0):
    return max(1, int(round(lookahead_ms * rate / 1000.0))), max(1, int(round(release_ms * rate / 1000.0)))


class Limited:
    """every stage of the definition for one clip: e, c, h, r, g, y1, t, y; true_peak_in, true_peak_y1"""

    def __init__(self, x, ceiling_db, L, R):
        x = np.asarray(x, np.float64)
        n = len(x)
        self.T = T = 10.0 ** (ceiling_db / 20.0)
        self.e = e = envelope(x)
        self.true_peak_in = float(e.max()) if n else 0.0
        with np.errstate(divide="ignore"):
            self.c = c = np.minimum(1.0, T / e)
        self.h = h = sliding_window_view(np.concatenate([c, np.ones(L - 1)]), L).min(axis=1) if n else c
        r = np.empty(n)
        s = 1.0 / R
        prev = math.inf
        for i in range(n):
            prev = min(h[i], prev + s)
            r[i] = prev
        self.r = r
        if n:
            padded = np.concatenate([np.full(L - 1, r[0]), r])
            self.g = np.minimum(c, sliding_window_view(padded, L).sum(axis=1) / L)
        else:
            self.g = r
        self.y1 = self.g * x
        self.true_peak_y1 = true_peak(self.y1)
        self.t = min(1.0, T / self.true_peak_y1) if self.true_peak_y1 > 0 else 1.0
        self.y = self.t * self.y1


# the grid both the CPU and the GPU test walk: every length with every signal
LENGTHS = [0, 1, 11, 12, 13, 47, 48, 49, 95, 97, TILE - 1, TILE, TILE + 1, 2 * TILE + 47]
KINDS = ("sine997", "quarter", "click_first", "click_last", "click_tile", "noise", "zeros", "quiet", "nan")


@functools.lru_cache(maxsize=None)
def grid_signal(kind, n, rate):
    t = np.arange(n)
    if kind == "sine997":
        x = 1.2 * np.sin(2.0 * np.pi * 997.0 * t / rate)
    elif kind == "quarter":             # fs / 4 at phase pi / 4: every sample +-0.7071, the peaks between them
        x = np.sin(2.0 * np.pi * t / 4.0 + np.pi / 4.0)
    elif kind in ("click_first", "click_last", "click_tile"):
        x = np.zeros(n)
        if n:
            x[{"click_first": 0, "click_last": n - 1, "click_tile": TILE if n > TILE else n // 2}[kind]] = 1.5
    elif kind == "noise":
        x = np.random.default_rng(1000 + n).standard_normal(n) * 0.5
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "quiet":
        x = 0.3 * np.sin(2.0 * np.pi * 997.0 * t / rate)
    elif kind == "nan":
        x = np.random.default_rng(2000 + n).standard_normal(n) * 0.5
        if n:
            x[n // 3] = np.nan
    else:
        raise KeyError(kind)
    return x.astype(np.float32)
