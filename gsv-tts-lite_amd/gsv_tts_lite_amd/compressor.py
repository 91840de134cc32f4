"""A feed-forward dynamic range compressor on the device (csrc/compressor.h): a hard-knee gain computer behind the
smooth decoupled peak detector of Giannoulis, Massberg and Reiss (JAES 2012), run over one clip or a packed list of them in one
call, from zero state, in fp64, rounded once to fp32:

    c = Compressor(threshold_db=-18.0, ratio=3.5, attack_ms=1.0, release_ms=100.0, makeup_db=0.0)
    c = Compressor.preset("voice")                             # the values of the reference WebUI's enhance_audio
    clips, recs = compress([a, b, c], 32000, "voice")          # or one Compressor / preset name / None per clip
    recs[0].peak_in, recs[0].peak_out, recs[0].min_gain, recs[0].compressed
    out_db = curve(c, [-40.0, -18.0, 0.0])                     # the static curve, output level against input level
    s = StreamCompressor("voice", 32000, "cuda"); y = s.push(chunk)    # a stream in pushes: the same bytes however it is cut

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


# ----------------------------------------------------------------------------------------------------------------------
# streams (csrc/cmpstream.h)
# ----------------------------------------------------------------------------------------------------------------------
_SREC = np.dtype([("emitted", "<i4"), ("flags", "<i4"), ("peak_in", "<f4"), ("peak_out", "<f4"), ("min_gain", "<f4"),
                  ("peak_in_run", "<f4"), ("peak_out_run", "<f4"), ("min_gain_run", "<f4"), ("total", "<i8")])
assert _SREC.itemsize == ctypes.sizeof(N.CmpstreamRecord)
STREAM_RECORD_BYTES = _SREC.itemsize


class CmpStreamRecord:
    """emitted: samples the push handed out (as many as it took); total: samples of the stream so far; peak_in / peak_out: max |x|
    and max |y| over the push's finite samples (np.float32, 0 for none), min_gain: the smallest gain among them, makeup excluded
    (np.float32, 1 for none); peak_in_run / peak_out_run / min_gain_run: over the stream's so far; live: the record of a state
    init made; compressed: min_gain is below 1; nonfinite: a NaN or an infinity among this push's samples (it ran through the
    detector as 0.0 and was copied to the output), nonfinite_ever: among the stream's so far"""

    __slots__ = ("emitted", "total", "peak_in", "peak_out", "min_gain", "peak_in_run", "peak_out_run", "min_gain_run", "live",
                 "compressed", "nonfinite", "nonfinite_ever")

    def __init__(self, emitted, flags, peak_in, peak_out, min_gain, peak_in_run, peak_out_run, min_gain_run, total):
        self.emitted, self.total = int(emitted), int(total)
        self.peak_in, self.peak_out, self.min_gain = np.float32(peak_in), np.float32(peak_out), np.float32(min_gain)
        self.peak_in_run, self.peak_out_run = np.float32(peak_in_run), np.float32(peak_out_run)
        self.min_gain_run = np.float32(min_gain_run)
        self.live = flags >= 0 and bool(flags & N.CMS_STREAM)
        self.compressed = flags >= 0 and bool(flags & N.CMS_COMPRESSED)
        self.nonfinite = flags >= 0 and bool(flags & N.CMS_NONFINITE)
        self.nonfinite_ever = flags >= 0 and bool(flags & N.CMS_NONFINITE_EVER)

    def __repr__(self):
        return ("CmpStreamRecord(emitted=%d, total=%d, peak_in=%r, peak_out=%r, min_gain=%r, peak_in_run=%r, peak_out_run=%r, "
                "min_gain_run=%r, compressed=%r, nonfinite=%r, nonfinite_ever=%r)" % (
                    self.emitted, self.total, float(self.peak_in), float(self.peak_out), float(self.min_gain), float(self.peak_in_run),
                    float(self.peak_out_run), float(self.min_gain_run), self.compressed, self.nonfinite, self.nonfinite_ever))


def stream_record(raw):
    """the 40 record bytes (a tensor on any device, or a numpy array of them) -> CmpStreamRecord"""
    raw = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    return CmpStreamRecord(*np.frombuffer(raw.tobytes()[:STREAM_RECORD_BYTES], dtype=_SREC)[0].tolist())


class StreamCompressor:
    """One stream through the compressor `c` -- a preset name or a Compressor -- at `rate`.  push(x, flush) -> float32
    numpy, as many samples as went in: the compressor is causal, so there is no delay, and a flush hands out nothing extra; it ends
    the stream, and the next push starts a fresh one with the same parameters.  The samples never depend on how the stream was cut
    into pushes: concatenated they are `compress` of the concatenated input, bit for bit.  A NaN or an infinity runs through the
    detector as 0.0 and is copied to the output.  On a GPU device a push is the six launches of `gsv_cmpstream_push`; on "cpu" the
    host twin runs the same scalar routines and gives the same bytes."""

    def __init__(self, c, rate: int, device="cpu"):
        self.rate = _check_rate(rate)
        self.compressor = resolve(c)
        if self.compressor is None:
            raise ValueError("a stream compressor needs a compressor that is not the identity")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _, tab = _tables([], [], [], [self.compressor.coefficients(self.rate)])
        L = N.lib()
        nbytes = L.gsv_cmpstream_state_bytes()
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.on_device:
            with torch.cuda.device(self.device):
                N.check(L.gsv_cmpstream_init(self.state.data_ptr(), nbytes, tab, N.current_stream_ptr(self.device)))
        else:
            N.check(L.gsv_cmpstream_init_host(self.state.data_ptr(), nbytes, tab))
        self._rec = None        # the last push's record

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def enqueue(self, chunk_ptr: int, n_cap: int, n_dev_ptr, flush: bool, out_ptr: int, rec_ptr: int):
        """the raw device call on the current stream: nothing is read back (ChunkEmitter's use); out_ptr may be chunk_ptr"""
        N.check(N.lib().gsv_cmpstream_push(self.state.data_ptr(), chunk_ptr or None, int(n_cap), n_dev_ptr, int(bool(flush)),
                                           out_ptr or None, rec_ptr, N.current_stream_ptr(self.device)))

    def _push_once(self, x: torch.Tensor, flush: bool):
        n = int(x.numel())
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        rec = torch.empty(STREAM_RECORD_BYTES // 8, dtype=torch.int64, device=self.device)      # 8-byte aligned
        if self.on_device:
            with torch.cuda.device(self.device):
                self.enqueue(x.data_ptr(), n, None, flush, out.data_ptr(), rec.data_ptr())
        else:
            N.check(N.lib().gsv_cmpstream_push_host(self.state.data_ptr(), x.data_ptr() or None, n, None, int(bool(flush)),
                                                    out.data_ptr() or None, rec.data_ptr()))
        return out, rec

    def push_tensor(self, x: torch.Tensor, flush: bool = False) -> torch.Tensor:
        """x on the compressor's device -> the compressed samples, a new fp32 tensor there of x's length.  The record is read, so
        the call waits for the push.  Input longer than one push may be (2^20 samples) goes in as several, which changes no byte;
        `rec` is then the last one's."""
        x = x.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        parts = []
        cuts = list(range(0, int(x.numel()), N.CMS_MAX_CHUNK)) or [0]
        for k, at in enumerate(cuts):
            out, rec = self._push_once(x[at: at + N.CMS_MAX_CHUNK], flush and k + 1 == len(cuts))
            self._rec = stream_record(rec.view(torch.uint8))
            parts.append(out[: self._rec.emitted])
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def push(self, x, flush: bool = False) -> np.ndarray:
        return self.push_tensor(torch.as_tensor(x), flush).cpu().numpy()

    @property
    def rec(self):
        """the last push's CmpStreamRecord (None before the first push)"""
        return self._rec


def compress_stream(x, rate, c, cuts=None, device=None):
    """the whole signal compressed as one stream on the CPU's host twin (the GPU gives the same bytes: name a device to run there)
    -> (float32 numpy, the last push's CmpStreamRecord).  cuts: the lengths of the pushes to cut it into (they must add up to the
    signal's; an empty push is legal), default one push; the last one flushes.  However it is cut, the samples are
    `compress(x, rate, c)`'s."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(-1)
    cuts = [len(x)] if cuts is None else [int(v) for v in cuts]
    if any(v < 0 for v in cuts) or sum(cuts) != len(x) or not cuts:
        raise ValueError("compress: cuts of %r for %d samples" % (cuts, len(x)))
    st = StreamCompressor(c, rate, torch.device("cpu") if device is None else device)
    parts, at = [], 0
    for k, v in enumerate(cuts):
        parts.append(st.push(x[at: at + v], flush=k + 1 == len(cuts)))
        at += v
    return np.concatenate(parts), st.rec
