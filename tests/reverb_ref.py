"""The oracle of the reverb tests: Freeverb as one serial loop over the samples in plain Python floats (IEEE fp64),
rounded to fp32 once, and the grid of parameter sets, lengths and signals the CPU and the GPU tests share.  Nothing here comes from
the product's code: the constants, the delays and the loop are written out again.

    u = gin v;  comb k: o = b[n - D];  l = o (1 - d) + l d;  b[n] = u + l fb;  s = o_0 + ... + o_7 from the left
    all-pass j in order: t = a[n - E];  a[n] = s + 0.5 t;  s = t - s;   y = fp32(s gw + v gd), saturating"""
import functools

import numpy as np

COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (556, 441, 341, 225)
FLT_MAX = 3.4028234663852886e38


def parameter_set(room_size, damping, wet_level, dry_level, width, rate):
    """-> (comb delays, all-pass delays, d, fb, gin, gw, gd)"""
    combs = tuple(rate * t // 44100 for t in COMB_TUNING)
    aps = tuple(rate * t // 44100 for t in ALLPASS_TUNING)
    return combs, aps, 0.4 * damping, 0.28 * room_size + 0.7, 0.015, 1.5 * wet_level * (1.0 + width), 2.0 * dry_level


VOICE = (0.1, 0.5, 0.03, 0.97, 1.0)       # room_size, damping, wet_level, dry_level, width
HALL = (1.0, 0.0, 1.0, 0.0, 1.0)
# name -> (the parameter set, the rate its tone is made at)
SETS = {
    "voice8": (parameter_set(*VOICE, 8000), 8000),
    "voice32": (parameter_set(*VOICE, 32000), 32000),
    "voice48": (parameter_set(*VOICE, 48000), 48000),
    "hall": (parameter_set(*HALL, 32000), 32000),
    "tiny": (((1, 2, 3, 5, 7, 64, 65, 257), (1, 3, 63, 130)) + parameter_set(*VOICE, 32000)[2:], 32000),
}
LONG = parameter_set(*VOICE, 768000)        # the longest legal line: 28 160 samples
LONG_N = 2 * 28160 + 5
KINDS = ("noise", "impulse", "gated220", "quiet")


def lengths(ps):
    delays = ps[0] + ps[1]
    lo, hi = min(delays), max(delays)
    return sorted({0, 1, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 2 * hi + 1, 3 * hi + 7})


def signal(kind, n, rate, seed=0):
    if kind == "impulse":
        x = np.zeros(n, np.float32)
        x[:1] = 1.0
        return x
    if kind == "gated220":      # a 220 Hz tone, on for 20 ms of every 50
        t = np.arange(n, dtype=np.float64) / rate
        return (0.8 * np.sin(2 * np.pi * 220.0 * t) * ((t % 0.05) < 0.02)).astype(np.float32)
    x = np.random.default_rng(1000 + seed).uniform(-1, 1, n).astype(np.float32)
    return x * np.float32(1e-30) if kind == "quiet" else x


def gain_bound(ps):
    """the largest |y| a clip of peak 1 can reach: the sum of the magnitudes of the impulse response.  A comb's is gin / (1 - fb)
    at most (its damping filter's response is positive and sums to 1), an all-pass's is 1 + 1 + 1/2 + 1/4 + ... = 3"""
    _, _, d, fb, gin, gw, gd = ps
    return abs(gd) + abs(gw) * 8.0 * abs(gin) / (1.0 - fb) * 3.0 ** 4


def reverb(x, ps):
    """the serial loop -> fp32 [len(x)]"""
    combs, aps, d, fb, gin, gw, gd = ps
    n = len(x)
    y = np.empty(n, np.float32)
    bk = [[0.0] * D for D in combs]
    lk = [0.0] * 8
    ak = [[0.0] * E for E in aps]
    xs = [float(v) for v in x]
    for i in range(n):
        v = xs[i]
        u = gin * v
        s = 0.0
        for k in range(8):
            buf = bk[k]
            at = i % combs[k]
            o = buf[at]
            l = o * (1 - d) + lk[k] * d
            lk[k] = l
            buf[at] = u + l * fb
            s = o if k == 0 else s + o
        for j in range(4):
            buf = ak[j]
            at = i % aps[j]
            t = buf[at]
            buf[at] = s + 0.5 * t
            s = t - s
        w = s * gw + v * gd
        y[i] = np.float32(min(max(w, -FLT_MAX), FLT_MAX))
    return y


@functools.lru_cache(maxsize=None)
def grid(name):
    """[(name, n, kind, x, oracle y)] of one parameter set: every length with every signal; computed once, never written to"""
    ps, rate = SETS[name]
    cells = []
    for n in lengths(ps):
        for k, kind in enumerate(KINDS):
            x = signal(kind, n, rate, seed=k)
            y = reverb(x, ps)
            x.setflags(write=False)
            y.setflags(write=False)
            cells.append((name, n, kind, x, y))
    return tuple(cells)


@functools.lru_cache(maxsize=None)
def long_cell(with_oracle=True):
    x = signal("noise", LONG_N, 768000, seed=9)
    y = reverb(x, LONG) if with_oracle else None
    x.setflags(write=False)
    return x, y
