"""The oracle of the loudness tests: ITU-R BS.1770 integrated loudness as DESIGN 4.20 defines it, restated in fp64 with
numpy alone -- a plain loop for the two biquads, numpy sums for the blocks, math.log10 for the gates.  Nothing here is shared
with the product code (csrc/loudness.h, gsv_tts_lite_amd/loudness.py)."""
import functools
import math

import numpy as np

TG, STEP = 0.4, 0.25


def coefficients(rate):
    """[(b0, b1, b2, a1, a2)] of the high shelf and the high pass, each normalised by its a0"""
    out = []
    A = 10.0 ** (4.0 / 40.0)
    w0 = 2.0 * math.pi * 1500.0 / rate
    alpha = math.sin(w0) / (2.0 * (1.0 / math.sqrt(2.0)))
    c = math.cos(w0)
    b0 = A * ((A + 1) + (A - 1) * c + 2 * math.sqrt(A) * alpha)
    b1 = -2 * A * ((A - 1) + (A + 1) * c)
    b2 = A * ((A + 1) + (A - 1) * c - 2 * math.sqrt(A) * alpha)
    a0 = (A + 1) - (A - 1) * c + 2 * math.sqrt(A) * alpha
    a1 = 2 * ((A - 1) - (A + 1) * c)
    a2 = (A + 1) - (A - 1) * c - 2 * math.sqrt(A) * alpha
    out.append((b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0))
    w0 = 2.0 * math.pi * 38.0 / rate
    alpha = math.sin(w0) / (2.0 * 0.5)
    c = math.cos(w0)
    a0 = 1 + alpha
    out.append(((1 + c) / 2 / a0, -(1 + c) / a0, (1 + c) / 2 / a0, -2 * c / a0, (1 - alpha) / a0))
    return out


def k_filter(x, rate):
    y = [float(v) for v in np.asarray(x, np.float32)]
    for b0, b1, b2, a1, a2 in coefficients(rate):
        s1 = s2 = 0.0
        o = [0.0] * len(y)
        for n, xn in enumerate(y):
            yn = b0 * xn + s1
            s1 = b1 * xn - a1 * yn + s2
            s2 = b2 * xn - a2 * yn
            o[n] = yn
        y = o
    return np.asarray(y, np.float64)


def block_count(n, rate):
    """None: no measurement"""
    if n < int(TG * rate):
        return None
    T = n / rate
    return int(round((T - TG) / (TG * STEP))) + 1


def block_values(x, rate):
    n = len(x)
    nb = block_count(n, rate)
    if nb is None:
        return None
    y = k_filter(x, rate)
    z = np.empty(nb)
    for j in range(nb):
        lo, hi = int(TG * (j * STEP) * rate), int(TG * (j * STEP + 1) * rate)
        z[j] = np.sum(y[lo:min(hi, n)] ** 2) / (TG * rate)
    return z


class Measurement:
    """lufs (-inf: none), zbar, blocks, above_abs, kept, and the block loudnesses l with the relative threshold (None when no
    block passed the absolute gate) for the margin checks; ungated: the mean over all blocks"""

    def __init__(self, x, rate):
        self.lufs, self.zbar, self.blocks, self.above_abs, self.kept = -math.inf, 0.0, 0, 0, 0
        self.l, self.rel, self.ungated = None, None, -math.inf
        if not np.all(np.isfinite(np.asarray(x, np.float32))):
            nb = block_count(len(x), rate)
            self.blocks = nb or 0
            return
        z = block_values(x, rate)
        if z is None:
            return
        self.blocks = len(z)
        with np.errstate(divide="ignore"):
            self.l = -0.691 + 10.0 * np.log10(z)
        if z.mean() > 0:
            self.ungated = -0.691 + 10.0 * math.log10(z.mean())
        a = self.l >= -70.0
        self.above_abs = int(a.sum())
        if not a.any():
            return
        self.rel = -0.691 + 10.0 * math.log10(z[a].mean()) - 10.0
        k = (self.l > self.rel) & (self.l > -70.0)
        self.kept = int(k.sum())
        if not k.any():
            return
        self.zbar = float(z[k].mean())
        self.lufs = -0.691 + 10.0 * math.log10(self.zbar)

    def margin(self):
        """the least distance in LU of any block from either gate threshold"""
        m = np.abs(self.l + 70.0).min()
        if self.rel is not None:
            m = min(m, np.abs(self.l - self.rel).min())
        return float(m)

    def gain(self, target):
        return math.sqrt(10.0 ** ((target + 0.691) / 10.0) / self.zbar)


def sine(freq, seconds, rate, amp=0.5):
    t = np.arange(int(seconds * rate)) / rate
    return (amp * np.sin(2.0 * np.pi * freq * t)).astype(np.float32)


def noise(n, seed=0, amp=0.3):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, n) * amp).astype(np.float32)


GATING_RATES = (8000, 32000, 44100)


@functools.lru_cache(maxsize=None)
def _gating_signals():
    """One default_rng(7) draws the signals for 8000, 32000 and 44100 Hz in this order.  That is the draw DESIGN 4.20's figures
    belong to (-13.31 LUFS gated at 32 kHz, every block at least 5 LU from both gate thresholds at all three rates); a generator
    restarted per rate gives other signals, and at 44.1 kHz one whose first quiet block sits 0.6 LU from the absolute gate."""
    rng = np.random.default_rng(7)
    out = {}
    for r in GATING_RATES:
        seg = lambda s, a: rng.uniform(-1.0, 1.0, int(s * r)) * a
        out[r] = np.concatenate([seg(0.8, 0.3), seg(0.8, 1e-5), seg(0.8, 0.3 * 10 ** (-25 / 20)), seg(0.63, 0.3)]).astype(np.float32)
    return out


def gating_signal(rate):
    """0.8 s of noise at +-0.3, 0.8 s at +-1e-5, 0.8 s at +-0.3 * 10^(-25/20), 0.63 s at +-0.3"""
    return _gating_signals()[rate]


# the grid both the CPU and the GPU test walk: every length with every signal
SPAN = 512 * 16             # samples of one pass of the filter block (LOUD_SPAN); two make a chunk
LENGTHS = {
    32000: [0, 1, 12799, 12800, 14400, 17600, 20800, 22400, 2 * SPAN, 2 * SPAN + 1, 16400],
    8000: [0, 1, 3199, 3200, 3600, 4400, 5200, 5600, SPAN, SPAN - 1, 2 * SPAN + 77, 24000],
    44100: [17639, 17640, 30000],
}
KINDS = ("noise", "sine997", "sine60", "zeros")


@functools.lru_cache(maxsize=None)
def grid_signal(kind, n, rate):
    if kind == "noise":
        return noise(n, seed=n % 1000)
    if kind == "sine997":
        return sine(997.0, n / rate + 1, rate)[:n]
    if kind == "sine60":
        return sine(60.0, n / rate + 1, rate)[:n]
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "gating":
        return gating_signal(rate)
    raise KeyError(kind)
