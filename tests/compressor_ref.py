"""The oracle of the compressor tests: DESIGN 4.26's definition restated in fp64 as a plain serial loop -- the smooth decoupled peak
detector from zero state, the hard-knee gain with libm's log2 and exp2 (`math`), one rounding to fp32 at the end, saturating at
+-FLT_MAX -- and the grid both the CPU and the GPU test walk.  Nothing here is shared with the product code (csrc/compressor.h,
gsv_tts_lite_amd/compressor.py)."""
import functools
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
RUN, SPAN, CHUNK = 16, 512 * 16, 2 * 512 * 16
RATES = (8000, 32000, 48000)
LENGTHS = (1, RUN - 1, RUN, RUN + 1, SPAN - 1, SPAN + 1, CHUNK + 1, 3 * CHUNK + 5)
LONGEST = max(LENGTHS)
# (threshold_db, ratio, attack_ms, release_ms, makeup_db)
SETS = {"voice": (-18.0, 3.5, 1.0, 100.0, 0.0), "fast": (-30.0, 20.0, 0.1, 5.0, 0.0), "slow": (-6.0, 2.0, 30.0, 1000.0, 3.0),
        "inf": (-18.0, math.inf, 1.0, 100.0, 0.0)}
KINDS = ("noise", "gated220", "square", "quiet")
GATE = 3001             # samples of half a gate period: no divisor of a span, so attacks and releases cross span and chunk edges
DENORMAL = dict(rate=8000, params=(-18.0, 3.5, 1.0, 1.0, 0.0), burst=64, n=6000)


def coefficients(params, rate):
    """(aA, aR, T, s, M): what the call takes"""
    thr, ratio, att, rel, mk = params
    return (math.exp(-2.0 * math.pi * 1000.0 / (rate * att)), math.exp(-2.0 * math.pi * 1000.0 / (rate * rel)), 10.0 ** (thr / 20.0),
            1.0 / ratio - 1.0, 10.0 ** (mk / 20.0))


def detector(x, co):
    """e[n] of the definition as a list of Python floats"""
    a_a, a_r = co[0], co[1]
    p = e = 0.0
    out = [0.0] * len(x)
    for n, v in enumerate(np.abs(np.asarray(x, np.float32)).astype(np.float64).tolist()):
        t = a_r * p + (1.0 - a_r) * v
        p = t if t > v else v
        e = a_a * e + (1.0 - a_a) * p
        out[n] = e
    return out


def gains(e, co):
    """g[n] of the definition, fp64"""
    T, s = co[2], co[3]
    inv = 1.0 / T
    exp2 = getattr(math, "exp2", None) or (lambda t: math.pow(2.0, t))     # math.exp2: Python 3.11
    return np.array([1.0 if v <= T else exp2(s * math.log2(v * inv)) for v in e], np.float64)


def to_f32(y64):
    return np.clip(y64, -FLT_MAX, FLT_MAX).astype(np.float32)


def compress(x, co):
    """-> (y fp32, g fp64)"""
    x = np.asarray(x, np.float32)
    g = gains(detector(x, co), co)
    return to_f32(co[4] * g * x.astype(np.float64)), g


def ulps(a, b):
    """the distance of two finite fp32 arrays in units in the last place"""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@functools.lru_cache(maxsize=None)
def _longest(kind, rate, name):
    """the signal of a cell at the grid's longest length; the shorter ones are its beginnings"""
    n = LONGEST
    if kind == "noise":
        x = np.random.default_rng(7).uniform(-1.0, 1.0, n)
    elif kind == "gated220":
        amp = np.where((np.arange(n) // GATE) % 2 == 0, 0.9, 0.01)
        x = amp * np.sin(2.0 * np.pi * 220.0 * np.arange(n) / rate)
    elif kind == "square":
        x = np.where((np.arange(n) // 32) % 2 == 0, 1.0, -1.0)
    elif kind == "quiet":           # 26 dB under the set's threshold
        x = 10.0 ** ((SETS[name][0] - 26.0) / 20.0) * np.random.default_rng(8).uniform(-1.0, 1.0, n)
    else:
        raise KeyError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def grid_signal(kind, n, rate, name):
    return _longest(kind, rate, name)[:n]


def grid(rate):
    """[(set name, length, kind, signal)] of one rate"""
    return [(name, n, k, grid_signal(k, n, rate, name)) for name in SETS for n in LENGTHS for k in KINDS]


@functools.lru_cache(maxsize=None)
def _expected_longest(kind, rate, name):
    y, g = compress(_longest(kind, rate, name), coefficients(SETS[name], rate))
    y.setflags(write=False)
    g.setflags(write=False)
    return y, g


def grid_expected(rate):
    """the oracle's (y, g) of every grid cell of a rate; the compressor is causal, so a shorter cell is the beginning of the
    longest one's and every (set, signal) is computed once"""
    out = []
    for name, n, k, _ in grid(rate):
        y, g = _expected_longest(k, rate, name)
        out.append((y[:n], g[:n]))
    return out


@functools.lru_cache(maxsize=None)
def denormal_clip():
    """a loud burst, then zeros under a 1 ms release at 8 kHz: p and e fall through the fp64 denormals to 0 -> (x, coefficients)"""
    d = DENORMAL
    x = np.zeros(d["n"], np.float32)
    x[: d["burst"]] = 0.9 * np.where(np.arange(d["burst"]) % 2 == 0, 1.0, -1.0)
    x.setflags(write=False)
    return x, coefficients(d["params"], d["rate"])
