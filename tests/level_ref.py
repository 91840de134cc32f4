"""The oracle of the leveller tests: the running BS.1770 gain as DESIGN 4.21 defines it, restated in fp64 with numpy alone -- the
plain loop of loudness_ref.k_filter over the whole stream, numpy sums in plain order for the hops and the gates, ** and log10 for
the constants.  Nothing here is shared with the product code (csrc/level.h, gsv_tts_lite_amd/level.py); only the K-filter's
coefficients and the test signals come from loudness_ref."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as LR  # noqa: E402

TG, STEP = LR.TG, LR.STEP


def knot(h, rate):
    return int(TG * (h * STEP) * rate)


class Run:
    """the whole stream x levelled in one go.  Per knot h = 0 .. hops + 1: A[h].  Per decided knot h + 1 (h = 1 .. hops): blocks,
    above_abs, kept, zbar, margin (the least distance in LU of any block then measured from either threshold then in force).
    out: the levelled samples (float32), clamped: how many were set to +-peak_limit; nonfinite / full: why the measure froze."""

    def __init__(self, x, rate, target, seed=None, seed_blocks=10, slew_db_s=10.0, max_gain_db=20.0, peak_limit=1.0, max_seconds=600):
        x = np.asarray(x, np.float32)
        n = len(x)
        k = 10.0 ** ((target + 0.691) / 10.0)
        G = 10.0 ** (max_gain_db / 20.0)
        r = 10.0 ** (slew_db_s * 0.1 / 20.0)
        w = float(seed_blocks) if seed is not None else 0.0
        seed_z = 10.0 ** ((seed + 0.691) / 10.0) if seed is not None else 0.0
        cap_blocks = int(round((max_seconds - TG) / (TG * STEP))) + 1
        A0 = min(max(math.sqrt(k / seed_z), 1.0 / G), G) if seed is not None else 1.0
        y = LR.k_filter(x, rate)
        finite = np.isfinite(x)
        self.A, self.knots = [A0], []
        self.nonfinite = self.full = False
        S, z, peak = [], [], 0.0
        h = 0
        self.A.append(self._next(A0, 0, 0.0, 0.0, k, w, seed_z, G, r, peak_limit))
        self.margin = math.inf
        self.zbar, self.blocks, self.above_abs, self.kept = 0.0, 0, 0, 0
        while True:
            lo, hi = knot(h, rate), knot(h + 1, rate)
            if hi > n:
                break
            if not finite[lo:hi].all():
                self.nonfinite = True
                break
            S.append(float(np.sum(y[lo:hi] ** 2)))
            peak = max(peak, float(np.abs(x[lo:hi]).max()))
            h += 1
            if h >= 4:
                z.append((S[h - 4] + S[h - 3] + S[h - 2] + S[h - 1]) / (TG * rate))
            zz = np.asarray(z, np.float64)
            above, kept, zbar = 0, 0, 0.0
            if len(zz):
                with np.errstate(divide="ignore"):
                    l = -0.691 + 10.0 * np.log10(zz)
                a = l >= -70.0
                above = int(a.sum())
                m = float(np.abs(l + 70.0).min())
                if above:
                    rel = -0.691 + 10.0 * math.log10(zz[a].mean()) - 10.0
                    m = min(m, float(np.abs(l - rel).min()))
                    keep = (l > rel) & (l > -70.0)
                    kept = int(keep.sum())
                    if kept:
                        zbar = float(zz[keep].mean())
                self.margin = min(self.margin, m)
            self.knots.append((len(zz), above, kept, zbar))
            self.zbar, self.blocks, self.above_abs, self.kept = zbar, len(zz), above, kept
            self.A.append(self._next(self.A[h], kept, zbar, peak, k, w, seed_z, G, r, peak_limit))
            if len(zz) == cap_blocks:
                self.full = True
                break
        self.hops, self.peak = h, peak
        self.lufs = -0.691 + 10.0 * math.log10(self.zbar) if self.kept else -math.inf
        # apply
        K = len(self.A) - 1
        gains = np.empty(n, np.float32)
        for hh in range(K):
            lo, hi = knot(hh, rate), min(knot(hh + 1, rate), n)
            if lo >= n:
                break
            frac = np.arange(hi - lo, dtype=np.float64) / float(knot(hh + 1, rate) - knot(hh, rate))
            gains[lo:hi] = (self.A[hh] + (self.A[hh + 1] - self.A[hh]) * frac).astype(np.float32)
        if knot(K, rate) < n:
            gains[knot(K, rate):] = np.float32(self.A[K])
        self.gains = gains
        with np.errstate(invalid="ignore", over="ignore"):
            out = x * gains
            over = np.abs(out) > np.float32(peak_limit)
        self.clamped = int(over.sum())
        out[over] = np.copysign(np.float32(peak_limit), out[over])
        self.out = out

    @staticmethod
    def _next(A, kept, zbar, peak, k, w, seed_z, G, r, peak_limit):
        d = 1.0
        if w + kept > 0:
            d = math.sqrt(k / ((w * seed_z + kept * zbar) / (w + kept)))
        d = min(max(d, 1.0 / G), G)
        if peak > 0:
            d = min(d, peak_limit / peak)
        return min(max(d, A / r), A * r)


RATES = (8000, 11025, 32000, 44100)
KINDS = ("noise", "sine997", "sine60", "zeros", "gating")
SECONDS = {8000: 4.0, 11025: 3.05, 32000: 2.5, 44100: 2.03}       # none a whole number of hops but the first


@functools.lru_cache(maxsize=None)
def signal(kind, rate):
    """the streams both the CPU and the GPU test walk"""
    if kind == "gating":
        # the stepped signal of DESIGN 4.20 -- 0.8 s at +-0.3, 0.8 s at +-1e-5, 0.8 s at +-0.3 * 10^(-25/20), 0.63 s at +-0.3 --, drawn
        # per rate here (loudness_ref's draw has no 11 025 Hz)
        rng = np.random.default_rng(700 + rate)
        seg = lambda s, a: rng.uniform(-1.0, 1.0, int(s * rate)) * a
        return np.concatenate([seg(0.8, 0.3), seg(0.8, 1e-5), seg(0.8, 0.3 * 10 ** (-25 / 20)), seg(0.63, 0.3)]).astype(np.float32)
    n = int(SECONDS[rate] * rate)
    if kind == "noise":
        return LR.noise(n, seed=rate % 1000)
    if kind == "sine997":
        return LR.sine(997.0, n / rate + 1, rate)[:n]
    if kind == "sine60":
        return LR.sine(60.0, n / rate + 1, rate)[:n]
    if kind == "zeros":
        return np.zeros(n, np.float32)
    raise KeyError(kind)


TARGET = -18.0


@functools.lru_cache(maxsize=None)
def reference(kind, rate, seeded=False):
    """computed once, shared, left unchanged"""
    return Run(signal(kind, rate), rate, TARGET, seed=-25.0 if seeded else None)


def cuts(n, hop, seed=0):
    """name -> the lengths of the pushes that cut n samples; the last push of each carries the flush"""
    rng = np.random.default_rng(seed)
    out = {"one": [n]}
    for name, step in (("hop-1", hop - 1), ("hop", hop), ("hop+1", hop + 1), ("4hop-1", 4 * hop - 1), ("4hop+1", 4 * hop + 1)):
        out[name] = [step] * (n // step) + ([n % step] if n % step else [])
    out["0,1,.."] = [0, 1, 0, hop - 1, 1, 0, n - hop - 1, 0]
    parts, left = [], n
    while left:
        m = min(left, int(rng.integers(0, 2 * hop + 2)))
        parts.append(m)
        left -= m
    out["random"] = parts
    assert all(sum(v) == n for v in out.values())
    return out
