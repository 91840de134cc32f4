"""Ambience on the device (csrc/reverb.h): Freeverb -- eight parallel damped comb filters, their sum through four
all-pass filters in series -- run over one clip or a packed list of them in one call, from zero state, in fp64, rounded once to
fp32.  The output has the input's length; the tail behind the clip is cut:

    r = Reverb(room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0)     # pedalboard's names and defaults
    r = Reverb.preset("voice")                                 # the values of the reference WebUI's enhance_audio
    clips, recs = reverberate([a, b, c], 32000, "voice")       # or one Reverb / preset name / None per clip
    recs[0].peak_in, recs[0].peak_out, recs[0].reverbed
    h = impulse_response("voice", 32000, 4000)                 # what a unit impulse turns into

At a rate r the comb delays are r t // 44100 for t in COMB_TUNING and the all-pass delays r t // 44100 for t in ALLPASS_TUNING;
d = 0.4 damping, fb = 0.28 room_size + 0.7, gin = 0.015, gw = 1.5 wet_level (1 + width) (the mono wet gain), gd = 2 dry_level.
Per sample, v = x[n]:

    u = gin v;   comb k: o_k = b_k[n - Dk];  l_k = (1 - d) o_k + d l_k;  b_k[n] = u + fb l_k;   s = o_0 + ... + o_7 in order
    all-pass j in order: t = a_j[n - Ej];  a_j[n] = s + 0.5 t;  s = t - s;                      y = fp32(gw s + gd v)

On a GPU device a call is `gsv_reverb` (one small upload, seven launches); on "cpu" the host twin `gsv_reverb_host` runs the same
scalar routines and gives the same bits.  Nothing clamps the level: the "voice" preset's dry gain is 1.94, so its clips come out
about 5.8 dB louder, and `loudness=` and `true_peak=` behind it set the level.  A clip holding a NaN or an infinity comes back bit
for bit, flagged `nonfinite`.  wet_level 0 with dry_level 0.5 is the identity and issues no call.

These are Freeverb's constants as JUCE (and so pedalboard) uses them, but not pedalboard sample for sample: JUCE computes in fp32
with a +0.1f -0.1f denormal guard and smooths parameter changes over 10 ms; its freeze mode and its stereo form (a second bank
of lines 23 samples longer) are not here."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as N
from .eq import _check_rate
from .loudness import _as_list, _device_for, _pack

COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)     # Freeverb's line lengths at 44.1 kHz
ALLPASS_TUNING = (556, 441, 341, 225)
MAX_DELAY = N.RVB_MAX_DELAY
PRESETS = ("voice",)


class Reverb:
    """room_size, damping, wet_level, dry_level, width: each 0 .. 1, pedalboard's names and defaults"""

    __slots__ = ("room_size", "damping", "wet_level", "dry_level", "width")

    def __init__(self, room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0):
        names = ("room_size", "damping", "wet_level", "dry_level", "width")
        given = (room_size, damping, wet_level, dry_level, width)
        try:
            vals = [float(v) for v in given]
        except (TypeError, ValueError):
            raise ValueError("reverb: numbers, not %r" % (given,))
        for name, v, g in zip(names, vals, given):
            if not 0.0 <= v <= 1.0:
                raise ValueError("reverb: a %s of %r (0 .. 1)" % (name, g))
        self.room_size, self.damping, self.wet_level, self.dry_level, self.width = vals

    @staticmethod
    def preset(name) -> "Reverb":
        """"voice": the reverb of the reference WebUI's enhance_audio -- a small room, 3 % wet against 97 % dry"""
        if name != "voice":
            raise ValueError("reverb preset %r (one of %s)" % (name, ", ".join(PRESETS)))
        return Reverb(room_size=0.1, damping=0.5, wet_level=0.03, dry_level=0.97)

    @property
    def is_identity(self) -> bool:
        return self.wet_level == 0.0 and self.dry_level == 0.5

    def parameters(self, rate):
        """(delays int32 [12]: eight combs then four all-passes, gains fp64 [5]: d, fb, gin, gw, gd) at `rate`, as the call takes
        them"""
        rate = _check_rate(rate)
        delays = np.array([rate * t // 44100 for t in COMB_TUNING + ALLPASS_TUNING], np.int32)
        gains = np.array([0.4 * self.damping, 0.28 * self.room_size + 0.7, 0.015, 1.5 * self.wet_level * (1.0 + self.width),
                          2.0 * self.dry_level], np.float64)
        return delays, gains

    def __repr__(self):
        return "Reverb(room_size=%r, damping=%r, wet_level=%r, dry_level=%r, width=%r)" % (
            self.room_size, self.damping, self.wet_level, self.dry_level, self.width)


def resolve(value):
    """what the ambience= keywords take -- None, a preset name or a Reverb -> None (nothing to do: None, or the identity) or the
    Reverb; anything else is a ValueError"""
    if value is None:
        return None
    if isinstance(value, str):
        value = Reverb.preset(value)
    if not isinstance(value, Reverb):
        raise ValueError("ambience: None, a preset name (%s) or a reverb.Reverb, not %r" % (", ".join(PRESETS), type(value).__name__))
    return None if value.is_identity else value


class RvbRecord:
    """peak_in / peak_out: max |x| and max |y| (np.float32); reverbed: the clip went through the network; nonfinite: the clip holds
    a NaN or an infinity and came back as it was"""

    __slots__ = ("peak_in", "peak_out", "reverbed", "nonfinite")

    def __init__(self, peak_in, peak_out, flags, pad=0):
        self.peak_in, self.peak_out = np.float32(peak_in), np.float32(peak_out)
        self.reverbed = bool(flags & N.RVB_REVERBED)
        self.nonfinite = bool(flags & N.RVB_NONFINITE)

    def __repr__(self):
        return "RvbRecord(peak_in=%r, peak_out=%r, reverbed=%r, nonfinite=%r)" % (
            float(self.peak_in), float(self.peak_out), self.reverbed, self.nonfinite)


_REC = np.dtype([("peak_in", "<f4"), ("peak_out", "<f4"), ("flags", "<i4"), ("pad", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.ReverbRecord)
RECORD_BYTES = _REC.itemsize


def _tables(offsets, lengths, index, params):
    n = len(lengths)
    clips = (N.ReverbClip * n)(*[N.ReverbClip(int(o), int(l), int(d)) for o, l, d in zip(offsets, lengths, index)])
    tab = (N.ReverbParams * max(1, len(params)))()
    for k, (delays, gains) in enumerate(params):
        delays, gains = np.asarray(delays), np.asarray(gains, np.float64)
        if delays.shape != (12,) or gains.shape != (5,) or delays.dtype.kind not in "iu":
            raise ValueError("reverb: a parameter set is 12 integer delays and 5 doubles (d, fb, gin, gw, gd), not %r and %r"
                             % (delays.shape, gains.shape))
        if delays.min() < -2 ** 31 or delays.max() >= 2 ** 31:
            raise ValueError("reverb: a delay outside 1..%d samples" % MAX_DELAY)
        tab[k] = N.ReverbParams((ctypes.c_int32 * 8)(*[int(v) for v in delays[:8]]), (ctypes.c_int32 * 4)(*[int(v) for v in delays[8:]]),
                                *[float(v) for v in gains])
    return clips, tab


def run_packed(x: torch.Tensor, offsets, lengths, index, params, out, rec=None, work=None):
    """The raw call over one packed fp32 tensor on its device: clip c is x[offsets[c] : offsets[c] + lengths[c]] and runs through
    params[index[c]] (a pair as `Reverb.parameters` gives it), or is measured and copied for index[c] == -1.  out: x itself (in
    place) or a tensor like x.  -> the records as a uint8 tensor [n_clips * 16] on x's device, not read back: `records(t)` turns it
    into RvbRecords.  rec: where to write them instead (a uint8 tensor of that size on x's device, 4-byte aligned), e.g. behind the
    samples so that one copy carries both.  work: a uint8 tensor to use as the workspace."""
    n = len(lengths)
    clips, tab = _tables(offsets, lengths, index, params)
    L = N.lib()
    need = L.gsv_reverb_work_bytes(clips, n, tab, len(params))
    if need == 0:
        raise ValueError("reverb: %d clips (1..65535) over %d parameter sets, or an index outside them" % (n, len(params)))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    if rec is None:
        rec = torch.empty(n * _REC.itemsize, dtype=torch.uint8, device=x.device)
    elif rec.numel() != n * _REC.itemsize or rec.dtype != torch.uint8 or rec.device != x.device or rec.data_ptr() % 4:
        raise ValueError("reverb: records need %d uint8 on %s, 4-byte aligned" % (n * _REC.itemsize, x.device))
    args = (x.data_ptr() or None, int(x.numel()), clips, n, tab, len(params), out.data_ptr() or None, rec.data_ptr(), work.data_ptr(),
            int(work.numel()))
    if x.device.type == "cuda":
        with torch.cuda.device(x.device):
            N.check(L.gsv_reverb(*args, N.current_stream_ptr(x.device)))
    else:
        N.check(L.gsv_reverb_host(*args))
    return rec


def records(rec):
    """the record bytes of run_packed (a tensor on any device, or the bytes themselves in a numpy array) -> [RvbRecord]"""
    raw = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.frombuffer(raw.tobytes(), dtype=_REC)
    return [RvbRecord(*r.tolist()) for r in a]


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
    return y, RvbRecord(peak, peak, N.RVB_NONFINITE if top >= 0x7F800000 else 0)


def plan(values, rate):
    """one of None / preset name / Reverb per clip -> (index per clip, the distinct parameter sets), as run_packed takes them"""
    params, index, seen = [], [], {}
    for v in values:
        v = resolve(v)
        if v is None:
            index.append(-1)
            continue
        delays, gains = v.parameters(rate)
        index.append(seen.setdefault(delays.tobytes() + gains.tobytes(), len(params)))
        if index[-1] == len(params):
            params.append((delays, gains))
    return index, params


def reverberate(clips, rate, r, device=None):
    """Every clip through its reverb -- `r` is None, a preset name or a Reverb for all of them, or a list with one of those per
    clip.  -> (clips, records): each clip comes back as what it came as (a numpy array, or a tensor on the device of the call),
    fp32, a new object; a list is ONE packed call with the distinct parameter sets passed once.  Clips whose reverb is None or the
    identity are measured and copied by that call; when that is all of them, no call is issued."""
    items, single = _as_list(clips)
    if not items:
        return [], []
    rate = _check_rate(rate)
    if isinstance(r, (list, tuple)):
        rs = list(r)
        if len(rs) != len(items):
            raise ValueError("reverberate: %d reverbs for %d clips" % (len(rs), len(items)))
    else:
        rs = [r] * len(items)
    index, params = plan(rs, rate)
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


def impulse_response(r, rate, n) -> np.ndarray:
    """the first n samples of what `r` (a preset name or a Reverb) makes of a unit impulse at `rate`, by the host twin -> fp32 [n]"""
    r = Reverb.preset(r) if isinstance(r, str) else r
    if not isinstance(r, Reverb):
        raise ValueError("impulse_response: a preset name (%s) or a reverb.Reverb, not %r" % (", ".join(PRESETS), type(r).__name__))
    n = int(n)
    if n < 0:
        raise ValueError("impulse_response: %d samples" % n)
    x = torch.zeros(n, dtype=torch.float32)
    if n:
        x[0] = 1.0
    if n == 0 or r.is_identity:
        return x.numpy().copy()
    out = torch.empty_like(x)
    run_packed(x, [0], [n], [0], [r.parameters(rate)], out)
    return out.numpy()
