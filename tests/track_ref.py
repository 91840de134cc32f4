"""The real-time track output restated in numpy (TEST INFRASTRUCTURE): the one-shot definition of DESIGN 4.19 with fp64
sums over the table of tests/sv_ref.resample_kernel (cast to fp32, as the definition has it), the quantiser, the packets; the streaming rule that says which
outputs exist after N samples; and the shared cases of the CPU and GPU tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_ref  # noqa: E402

RATE_PAIRS = [(32000, 48000), (32000, 16000), (32000, 8000), (32000, 44100), (32000, 24000), (32000, 32000), (48000, 32000)]
PACKETS = [960, 7, 1]
CHANNELS = [1, 2]
SIGNALS = ["noise", "sine", "zeros", "nonfinite"]


def signal(kind, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":                 # uniform in +-1: it clips, which exercises the clamp
        return rng.uniform(-1.0, 1.0, n).astype(np.float32)
    if kind == "sine":
        return (0.01 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 32000.0)).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    x = (0.3 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    if n:
        x[n // 3] = np.nan
        x[n // 2] = np.inf
        x[(2 * n) // 3] = -np.inf
    return x


def params(in_rate, out_rate):
    """-> o, w, width, L"""
    o, w, _, width = sv_ref.resample_params(in_rate, out_rate)
    return o, w, width, 2 * width + o


def total(n, o, w):
    return n if o == w else -(-w * n // o)


def avail(n, o, w, width):
    """the streaming rule: outputs that exist once n samples have been pushed"""
    if o == w:
        return n
    J = 0 if n < width + o else (n - width - o) // o + 1
    return min(w * J, total(n, o, w))


def quantise(y):
    """flac_enc_quantise(y, 16) on an fp64 array: x 2^15, round half to even, clamp, NaN -> 0"""
    y = np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(y * 32768.0), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0.0, q).astype(np.int16)


def resample64(x, in_rate, out_rate):
    """y[j w + p] = sum_i x[j o - width + i] K[p][i] in fp64, samples outside the stream skipped"""
    o, w, width, L = params(in_rate, out_rate)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[0]
    if o == w:
        return x
    M = total(n, o, w)
    if M == 0:
        return np.zeros(0)
    # the table as the definition has it: evaluated in fp64, cast to fp32 (an entry that underflows to 0 there is 0 here, so
    # an inf in the stream meets the same zeros); the sums in fp64
    K = sv_ref.resample_kernel(in_rate, out_rate)[0].astype(np.float32).astype(np.float64)
    frames = -(-M // w)
    xp = np.concatenate([np.zeros(width), x, np.zeros(frames * o + L)])         # a skipped sample adds nothing: a zero
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[::o][:frames]           # [frames][L]
    with np.errstate(invalid="ignore", over="ignore"):
        y = win @ K.T                                                             # [frames][w], phase-interleaved
    return y.reshape(-1)[:M]


def packets(q, packet, channels, flush=True):
    """int16 samples -> [k, packet * channels], every sample written `channels` times, the last packet zero-filled"""
    q = np.asarray(q, np.int16)
    k = -(-q.shape[0] // packet) if flush else q.shape[0] // packet
    full = np.zeros(k * packet, np.int16)
    m = min(q.shape[0], k * packet)
    full[:m] = q[:m]
    return np.repeat(full, channels).reshape(k, packet * channels)


def one_shot(x, in_rate, out_rate, packet, channels):
    return packets(quantise(resample64(x, in_rate, out_rate)), packet, channels)


class Rule:
    """what every push's rec must be, from the streaming rule alone"""

    def __init__(self, in_rate, out_rate, packet):
        self.o, self.w, self.width, self.L = params(in_rate, out_rate)
        self.packet = packet
        self.n_in = self.n_out = self.carry = 0

    def push(self, n, flush):
        n_in = self.n_in + n
        n_out = total(n_in, self.o, self.w) if flush else avail(n_in, self.o, self.w, self.width)
        produced = n_out - self.n_out
        have = self.carry + produced
        k = -(-have // self.packet) if flush else have // self.packet
        rec = [k, produced, 0 if flush else have - k * self.packet, k * self.packet - have if flush else 0]
        self.n_in, self.n_out, self.carry = (0, 0, 0) if flush else (n_in, n_out, rec[2])
        return rec


def chunkings(n, o, width, seed=0):
    """name -> list of (chunk length, flush); every list covers n samples and ends with a flush"""
    rng = np.random.default_rng(77 + seed)

    def cut(sizes, tail_flush=True):
        out, at = [], 0
        for s in sizes:
            s = min(int(s), n - at)
            out.append(s)
            at += s
            if at >= n:
                break
        if at < n:
            out.append(n - at)
        plan = [(s, False) for s in out]
        if tail_flush:
            plan[-1] = (plan[-1][0], True)
        else:
            plan.append((0, True))
        return plan

    def forever(f):
        while True:
            yield f()

    import itertools
    short = max(1, width - 1)
    return {
        "whole": [(n, True)],
        "forty singles then the rest": cut([1] * 40 + [n]),
        "all shorter than width": cut(itertools.islice(forever(lambda: rng.integers(1, short + 1)), n)),
        "multiples of o": cut(itertools.islice(forever(lambda: o * int(rng.integers(1, 40))), n)),
        "non-multiples of o": cut(itertools.islice(forever(lambda: o * int(rng.integers(1, 40)) + 1 + int(rng.integers(0, max(1, o - 1)))), n)),
        "random 0..700": cut(itertools.islice(forever(lambda: rng.integers(0, 701)), 10 * n + 10)),
        "flush as its own empty push": cut([n // 3, n], tail_flush=False),
    }
