"""A feed-forward dynamic range compressor on the device (csrc/compressor.h): a hard-knee gain computer behind the
smooth decoupled peak detector of Giannoulis, Massberg and Reiss (JAES 2012), run over one clip or a packed list of them in one
call, from zero state, in fp64, rounded once to fp32:

    c = Compressor(threshold_db=-18.0, ratio=3.5, attack_ms=1.0, release_ms=100.0, makeup_db=0.0)
    c = Compressor.preset("voice")                             # the values of the reference WebUI's enhance_audio
    clips, recs = compress([a, b, c], 32000, "voice")          # or one Compressor / preset name / None per clip
    recs[0].peak_in, recs[0].peak_out, recs[0].min_gain, recs[0].compressed
    out_db = curve(c, [-40.0, -18.0, 0.0])                     # the static curve, output level against input level

With aA = exp(-2 pi 1000 / (rate attack_ms)) and aR likewise (JUCE's meaning of the two times, so attack_ms=1, release_ms=100 are
pedalboard's defaults), T = 10^(threshold_db / 20), s = 1 / ratio - 1 and M = 10^(makeup_db / 20), per sample

    p = max(|x|, aR p + (1 - aR) |x|);  e = aA e + (1 - aA) p;  g = 1 if e <= T else (e / T)^s;  y = fp32(M g x).

On a GPU device a call is `gsv_compressor` (one small upload, at most six launches); on "cpu" the host twin `gsv_compressor_host`
runs the same scalar routines and gives the same bits.  A clip that never passes its threshold, with 0 dB of makeup, comes back bit
for bit.  A clip holding a NaN or an infinity comes back bit for bit, flagged `nonfinite`.  A ratio of 1 with 0 dB of makeup is the
identity and issues no call.

This is not pedalboard / JUCE sample for sample: JUCE's ballistics filter picks the attack or the release coefficient by comparing
the input with its own state, where this detector runs the release first and smooths it with the attack.  The static curve and the
meaning of the two times are the same; while the level moves the gains differ (DESIGN 4.26 has the figures)."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .eq import _check_rate
from .loudness import _as_list, _device_for, _pack

RUN, SPAN, CHUNK = N.CMP_RUN, N.CMP_SPAN, N.CMP_CHUNK       # samples of a thread's run, of a block's span, of a chunk
MIN_THRESHOLD_DB, MAX_THRESHOLD_DB = -80.0, 0.0
MIN_MS, MAX_MS = 0.01, 10000.0
MAX_MAKEUP_DB = 40.0
PRESETS = ("voice",)


class Compressor:
    """threshold_db (-80 .. 0), ratio (1 .. inf; inf: a limiter's curve), attack_ms and release_ms (0.01 .. 10000: with the rates
    `compress` takes, 4 kHz .. 768 kHz, both one-pole coefficients stay inside (0, 1)), makeup_db (-40 .. 40)"""

    __slots__ = ("threshold_db", "ratio", "attack_ms", "release_ms", "makeup_db")

    def __init__(self, threshold_db=-18.0, ratio=3.5, attack_ms=1.0, release_ms=100.0, makeup_db=0.0):
        try:
            vals = [float(v) for v in (threshold_db, ratio, attack_ms, release_ms, makeup_db)]
        except (TypeError, ValueError):
            raise ValueError("compressor: numbers, not %r" % ((threshold_db, ratio, attack_ms, release_ms, makeup_db),))
        self.threshold_db, self.ratio, self.attack_ms, self.release_ms, self.makeup_db = vals
        if not MIN_THRESHOLD_DB <= self.threshold_db <= MAX_THRESHOLD_DB:
            raise ValueError("compressor: a threshold of %r dB (%g .. %g)" % (threshold_db, MIN_THRESHOLD_DB, MAX_THRESHOLD_DB))
        if not self.ratio >= 1.0:
            raise ValueError("compressor: a ratio of %r (1 .. inf)" % (ratio,))
        for name, v in (("attack", self.attack_ms), ("release", self.release_ms)):
            if not MIN_MS <= v <= MAX_MS:
                raise ValueError("compressor: %s of %r ms (%g .. %g)" % (name, v, MIN_MS, MAX_MS))
        if not abs(self.makeup_db) <= MAX_MAKEUP_DB:
            raise ValueError("compressor: a makeup of %r dB (-%g .. %g)" % (makeup_db, MAX_MAKEUP_DB, MAX_MAKEUP_DB))

    @staticmethod
    def preset(name) -> "Compressor":
        """"voice": the compressor of the reference WebUI's enhance_audio -- -18 dB, 3.5 : 1, pedalboard's default times 1 ms and
        100 ms.  The chain's fixed +2 dB behind it is makeup_db=2.0; the preset leaves it out, since loudness= makes it moot."""
        if name != "voice":
            raise ValueError("compressor preset %r (one of %s)" % (name, ", ".join(PRESETS)))
        return Compressor(-18.0, 3.5, 1.0, 100.0, 0.0)

    @property
    def is_identity(self) -> bool:
        return self.ratio == 1.0 and self.makeup_db == 0.0

    def coefficients(self, rate) -> np.ndarray:
        """fp64 [5] at `rate`: aA, aR, T, s, M as the call takes them"""
        rate = _check_rate(rate)
        a_a = math.exp(-2.0 * math.pi * 1000.0 / (rate * self.attack_ms))
        a_r = math.exp(-2.0 * math.pi * 1000.0 / (rate * self.release_ms))
        return np.array([a_a, a_r, 10.0 ** (self.threshold_db / 20.0), 1.0 / self.ratio - 1.0, 10.0 ** (self.makeup_db / 20.0)], np.float64)

    def __repr__(self):
        return "Compressor(threshold_db=%r, ratio=%r, attack_ms=%r, release_ms=%r, makeup_db=%r)" % (
            self.threshold_db, self.ratio, self.attack_ms, self.release_ms, self.makeup_db)


def resolve(value):
    """what the compress= keywords take -- None, a preset name or a Compressor -> None (nothing to do: None, or the identity) or
    the Compressor; anything else is a ValueError"""
    if value is None:
        return None
    if isinstance(value, str):
        value = Compressor.preset(value)
    if not isinstance(value, Compressor):
        raise ValueError("compress: None, a preset name (%s) or a compressor.Compressor, not %r" % (", ".join(PRESETS), type(value).__name__))
    return None if value.is_identity else value


def curve(c, levels_db) -> np.ndarray:
    """the static curve of `c` (a Compressor or a preset name): the output level in dB of a steady input at `levels_db`, makeup
    included -> fp64, shaped like levels_db.  Below the threshold the diagonal (plus the makeup), above it a slope of 1 / ratio."""
    c = Compressor.preset(c) if isinstance(c, str) else c
    if not isinstance(c, Compressor):
        raise ValueError("curve: a preset name (%s) or a compressor.Compressor, not %r" % (", ".join(PRESETS), type(c).__name__))
    lv = np.asarray(levels_db, np.float64)
    over = np.maximum(lv - c.threshold_db, 0.0)
    return lv + (1.0 / c.ratio - 1.0) * over + c.makeup_db


class CmpRecord:
    """peak_in / peak_out: max |x| and max |y| (np.float32); min_gain: the smallest gain among the clip's samples, makeup excluded
    (np.float32; 1 for a clip that was copied); compressed: it is below 1; nonfinite: the clip holds a NaN or an infinity and came
    back as it was"""

    __slots__ = ("peak_in", "peak_out", "min_gain", "compressed", "nonfinite")

    def __init__(self, peak_in, peak_out, min_gain, flags):
        self.peak_in, self.peak_out, self.min_gain = np.float32(peak_in), np.float32(peak_out), np.float32(min_gain)
        self.compressed = bool(flags & N.CMP_COMPRESSED)
        self.nonfinite = bool(flags & N.CMP_NONFINITE)

    def __repr__(self):
        return "CmpRecord(peak_in=%r, peak_out=%r, min_gain=%r, compressed=%r, nonfinite=%r)" % (
            float(self.peak_in), float(self.peak_out), float(self.min_gain), self.compressed, self.nonfinite)


_REC = np.dtype([("peak_in", "<f4"), ("peak_out", "<f4"), ("min_gain", "<f4"), ("flags", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.CompressorRecord)
RECORD_BYTES = _REC.itemsize


def _tables(offsets, lengths, index, params):
    n = len(lengths)
    clips = (N.CompressorClip * n)(*[N.CompressorClip(int(o), int(l), int(d)) for o, l, d in zip(offsets, lengths, index)])
    tab = (N.CompressorParams * max(1, len(params)))()
    for k, co in enumerate(params):
        co = np.asarray(co, np.float64)
        if co.shape != (5,):
            raise ValueError("compressor: a parameter set is 5 doubles (aA, aR, T, s, M), not %r" % (co.shape,))
        tab[k] = N.CompressorParams(*[float(v) for v in co])
    return clips, tab


def run_packed(x: torch.Tensor, offsets, lengths, index, params, out, rec=None, work=None):
    """The raw call over one packed fp32 tensor on its device: clip c is x[offsets[c] : offsets[c] + lengths[c]] and runs through
    params[index[c]] (five doubles as `Compressor.coefficients` gives them), or is measured and copied for index[c] == -1.  out: x
    itself (in place) or a tensor like x.  -> the records as a uint8 tensor [n_clips * 16] on x's device, not read back:
    `records(t)` turns it into CmpRecords.  rec: where to write them instead (a uint8 tensor of that size on x's device, 4-byte
    aligned), e.g. behind the samples so that one copy carries both.  work: a uint8 tensor to use as the workspace."""
    n = len(lengths)
    clips, tab = _tables(offsets, lengths, index, params)
    L = N.lib()
    need = L.gsv_compressor_work_bytes(clips, n, tab, len(params))
    if need == 0:
        raise ValueError("compressor: %d clips (1..65535) over %d parameter sets, or an index outside them" % (n, len(params)))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    if rec is None:
        rec = torch.empty(n * _REC.itemsize, dtype=torch.uint8, device=x.device)
    elif rec.numel() != n * _REC.itemsize or rec.dtype != torch.uint8 or rec.device != x.device or rec.data_ptr() % 4:
        raise ValueError("compressor: records need %d uint8 on %s, 4-byte aligned" % (n * _REC.itemsize, x.device))
    args = (x.data_ptr() or None, int(x.numel()), clips, n, tab, len(params), out.data_ptr() or None, rec.data_ptr(), work.data_ptr(),
            int(work.numel()))
    if x.device.type == "cuda":
        with torch.cuda.device(x.device):
            N.check(L.gsv_compressor(*args, N.current_stream_ptr(x.device)))
    else:
        N.check(L.gsv_compressor_host(*args))
    return rec


def records(rec):
    """the record bytes of run_packed (a tensor on any device, or the bytes themselves in a numpy array) -> [CmpRecord]"""
    raw = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.frombuffer(raw.tobytes(), dtype=_REC)
    return [CmpRecord(*r.tolist()) for r in a]


def _copied(c):
    """the record and the copy of a clip no call is issued for"""
    if isinstance(c, torch.Tensor):
        y = c.detach().to(torch.float32).clone()
        bits = y.reshape(-1).cpu().numpy().view(np.uint32)
    else:
        y = np.array(c, dtype=np.float32)
        bits = y.reshape(-1).view(np.uint32)
    top = np.uint32((bits & np.uint32(0x7FFFFFFF)).max()) if bits.size else np.uint32(0)
    peak = top.view(np.float32)
    return y, CmpRecord(peak, peak, 1.0, N.CMP_NONFINITE if top >= 0x7F800000 else 0)


def compress(clips, rate, c, device=None):
    """Every clip through its compressor -- `c` is None, a preset name or a Compressor for all of them, or a list with one of those
    per clip.  -> (clips, records): each clip comes back as what it came as (a numpy array, or a tensor on the device of the call),
    fp32, a new object; a list is ONE packed call with the distinct parameter sets passed once.  Clips whose compressor is None or
    the identity are measured and copied by that call; when that is all of them, no call is issued."""
    items, single = _as_list(clips)
    if not items:
        return [], []
    rate = _check_rate(rate)
    if isinstance(c, (list, tuple)):
        cs = list(c)
        if len(cs) != len(items):
            raise ValueError("compress: %d compressors for %d clips" % (len(cs), len(items)))
    else:
        cs = [c] * len(items)
    params, index, seen = [], [], {}
    for v in cs:
        v = resolve(v)
        if v is None:
            index.append(-1)
            continue
        co = v.coefficients(rate)
        index.append(seen.setdefault(co.tobytes(), len(params)))
        if index[-1] == len(params):
            params.append(co)
    if not params:
        res, recs = zip(*[_copied(v) for v in items])
        return (res[0], recs[0]) if single else (list(res), list(recs))
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    out = torch.empty_like(x)
    recs = records(run_packed(x, offsets, lengths, index, params, out))
    res = []
    host = None
    for v, o, n in zip(items, offsets, lengths):
        if isinstance(v, torch.Tensor):
            res.append(out[o:o + n].reshape(v.shape))
        else:
            host = out.cpu().numpy() if host is None else host
            res.append(host[o:o + n].reshape(np.shape(v)).copy())
    return (res[0], recs[0]) if single else (res, recs)


def routine(which, values) -> np.ndarray:
    """the call's own log2 (which "log2": positive normal arguments) or exp2 ("exp2": clamped to [-1000, 1000]) of fp64 `values`,
    evaluated on the host by the routine the kernels share -- for measuring it against a library's"""
    v = np.ascontiguousarray(values, np.float64)
    out = np.empty_like(v)
    N.check(N.lib().gsv_compressor_math_host({"log2": 0, "exp2": 1}[which], v.ctypes.data, out.ctypes.data, v.size))
    return out
