"""The oracle of the equaliser tests: DESIGN 4.24's definition restated in fp64 -- the cookbook designs with `math`, and each
section as a plain serial transposed direct form II recurrence from zero state (scipy.signal.lfilter's, which `cascade_loop`
restates as a Python loop and test_eq_cpu.py holds against it), fp64 between the sections, one rounding to fp32 at the end,
saturating at +-FLT_MAX.  Nothing here is shared with the product code (csrc/eq.h, gsv_tts_lite_amd/eq.py)."""
import functools
import math

import numpy as np
from scipy.signal import lfilter

FLT_MAX = float(np.finfo(np.float32).max)


def section(kind, f0, q, gain_db, rate):
    """(b0, b1, b2, a1, a2) normalised by a0: the RBJ Audio-EQ-Cookbook, shelves in the Q form"""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * f0 / rate
    alpha = math.sin(w0) / (2.0 * q)
    c = math.cos(w0)
    if kind == "highpass":
        b0, b1, b2 = (1 + c) / 2, -(1 + c), (1 + c) / 2
        a0, a1, a2 = 1 + alpha, -2 * c, 1 - alpha
    elif kind == "lowpass":
        b0, b1, b2 = (1 - c) / 2, 1 - c, (1 - c) / 2
        a0, a1, a2 = 1 + alpha, -2 * c, 1 - alpha
    elif kind == "peak":
        b0, b1, b2 = 1 + alpha * A, -2 * c, 1 - alpha * A
        a0, a1, a2 = 1 + alpha / A, -2 * c, 1 - alpha / A
    elif kind == "lowshelf":
        r = 2 * math.sqrt(A) * alpha
        b0, b1, b2 = A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r)
        a0, a1, a2 = (A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r
    elif kind == "highshelf":
        r = 2 * math.sqrt(A) * alpha
        b0, b1, b2 = A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)
        a0, a1, a2 = (A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r
    else:
        raise KeyError(kind)
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def voice(rate):
    """the three filters of the reference WebUI's enhance_audio"""
    return [("highpass", 80.0, 1.0 / math.sqrt(2.0), 0.0), ("peak", 300.0, 1.0, 2.5), ("peak", min(7000.0, 0.45 * rate), 2.0, -3.0)]


def six(rate):
    """six sections, among them the double-pole high pass at 20 Hz of the issue's sketch"""
    return [("highpass", 20.0, 0.5, 0.0), ("lowshelf", 120.0, 0.7, 4.0), ("peak", 300.0, 1.0, 2.5), ("peak", min(2500.0, 0.3 * rate), 4.0, -6.0),
            ("highshelf", min(6000.0, 0.4 * rate), 0.8, 3.0), ("lowpass", 0.45 * rate, 1.0 / math.sqrt(2.0), 0.0)]


def bands_for(count, rate):
    return {1: [("peak", 1000.0, 2.0, 6.0)], 3: voice(rate), 6: six(rate)}[count]


def coefficients(bands, rate):
    return [section(k, f, q, g, rate) for k, f, q, g in bands]


def cascade64(x, coefs):
    """the cascade in fp64, not yet rounded"""
    y = np.asarray(x, np.float32).astype(np.float64)
    for b0, b1, b2, a1, a2 in coefs:
        y = lfilter([b0, b1, b2], [1.0, a1, a2], y) if len(y) else y
    return y


def cascade_loop(x, coefs):
    """the same as a Python loop: the definition's three lines per section"""
    y = [float(v) for v in np.asarray(x, np.float32)]
    for b0, b1, b2, a1, a2 in coefs:
        z0 = z1 = 0.0
        o = [0.0] * len(y)
        for n, xn in enumerate(y):
            yn = b0 * xn + z0
            z0 = b1 * xn - a1 * yn + z1
            z1 = b2 * xn - a2 * yn
            o[n] = yn
        y = o
    return np.asarray(y, np.float64)


def to_f32(y64):
    return np.clip(y64, -FLT_MAX, FLT_MAX).astype(np.float32)


def equalise(x, coefs):
    return to_f32(cascade64(x, coefs))


def ulps(a, b):
    """the distance of two finite fp32 arrays in units in the last place"""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# the grid both the CPU and the GPU test walk: every length with every signal, per rate and section count
RUN, SPAN, CHUNK = 16, 512 * 16, 2 * 512 * 16
RATES = (8000, 32000, 44100, 192000)
COUNTS = (1, 3, 6)
LENGTHS = (0, 1, RUN - 1, RUN, RUN + 1, SPAN - 1, SPAN, SPAN + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
KINDS = ("noise", "sine997", "sine60", "zeros", "impulse")


@functools.lru_cache(maxsize=None)
def _noise():
    """one default_rng(7) draws the noise of every length, in LENGTHS' order"""
    rng = np.random.default_rng(7)
    return {n: rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in LENGTHS}


@functools.lru_cache(maxsize=None)
def grid_signal(kind, n, rate):
    if kind == "noise":
        return _noise()[n]
    if kind in ("sine997", "sine60"):
        f = 997.0 if kind == "sine997" else 60.0
        return (0.5 * np.sin(2.0 * np.pi * f * np.arange(n) / rate)).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "impulse":
        x = np.zeros(n, np.float32)
        x[:1] = 1.0
        return x
    raise KeyError(kind)


def grid(rate):
    """[(length, kind, signal)] of one rate"""
    return [(n, k, grid_signal(k, n, rate)) for n in LENGTHS for k in KINDS]


@functools.lru_cache(maxsize=None)
def grid_expected(rate, count):
    """the oracle's fp32 output of every grid signal of (rate, count), computed once"""
    co = coefficients(bands_for(count, rate), rate)
    out = []
    for _, _, x in grid(rate):
        y = equalise(x, co)
        y.setflags(write=False)
        out.append(y)
    return out
