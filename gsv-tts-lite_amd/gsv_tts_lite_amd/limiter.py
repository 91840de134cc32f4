"""True peak and a look-ahead limiter that holds a clip under a true-peak ceiling, on the device (csrc/limiter.h): the
clip oversampled 4x by a 49-tap windowed sinc, the gain every sample needs, held over the look-ahead, released at 1/release per
sample, smoothed over the look-ahead, applied, and one trim for what the smoothing moved -- for one clip or a packed list of them in
one call:

    dbtp = true_peak(x, 32000)                                 # float; -inf for silence
    clips, recs = limit([a, b, c], 32000, ceiling_db=-1.0)     # every clip at or under -1 dBTP
    recs[0].true_peak_in, recs[0].true_peak_out, recs[0].min_gain, recs[0].trim, recs[0].limited

On a GPU device a call is `gsv_limiter` (one small upload, at most six launches); on "cpu" the host twin `gsv_limiter_host` runs the
same scalar routines and gives the same bits.  A clip already under its ceiling comes back bit for bit; so does one holding a NaN or
an infinity, flagged `nonfinite`.

Streams (csrc/limstream.h): the same stages 1 - 6 without the trim, as a state that emits every sample once the
look-ahead behind it has arrived, independent of how the stream was cut into pushes:

    lm = StreamLimiter(-1.0, 32000, device="cuda:0")
    for chunk, last in chunks:
        out = lm.push(chunk, flush=last)           # float32 numpy; lm.delay samples behind the input until the flush
    lm.rec.limited_ever, lm.rec.dbtp_in, lm.rec.min_gain
    y, rec = limit_stream(x, 32000, ceiling_db=-1.0)           # one push with flush"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .loudness import _as_list, _device_for, _pack

TILE = N.LIM_TILE       # samples of a tile of the release scan


def dbtp(v) -> float:
    """a linear peak as dBTP; -inf for 0"""
    v = float(v)
    return 20.0 * math.log10(v) if v > 0 else (-math.inf if v == 0 else math.nan)


class LimiterRecord:
    """true_peak_in / true_peak_out: the linear true peak before and after (np.float32; true_peak_out is trim times the true peak
    behind the gain); min_gain: the smallest gain of the limiter; trim: the factor applied behind it; limited: the true peak was
    above the ceiling; nonfinite: the clip holds a NaN or an infinity; lookahead / release: samples"""

    __slots__ = ("true_peak_in", "true_peak_out", "min_gain", "trim", "limited", "nonfinite", "lookahead", "release")

    def __init__(self, true_peak_in, true_peak_out, min_gain, trim, flags, lookahead, release, reserved=0):
        self.true_peak_in, self.true_peak_out = np.float32(true_peak_in), np.float32(true_peak_out)
        self.min_gain, self.trim = np.float32(min_gain), np.float32(trim)
        self.limited = bool(flags & N.LIM_LIMITED)
        self.nonfinite = bool(flags & N.LIM_NONFINITE)
        self.lookahead, self.release = int(lookahead), int(release)

    @property
    def dbtp_in(self) -> float:
        return dbtp(self.true_peak_in)

    @property
    def dbtp_out(self) -> float:
        return dbtp(self.true_peak_out)

    def __repr__(self):
        return "LimiterRecord(true_peak_in=%r, true_peak_out=%r, min_gain=%r, trim=%r, limited=%r, nonfinite=%r)" % (
            float(self.true_peak_in), float(self.true_peak_out), float(self.min_gain), float(self.trim), self.limited, self.nonfinite)


_REC = np.dtype([("true_peak_in", "<f4"), ("true_peak_out", "<f4"), ("min_gain", "<f4"), ("trim", "<f4"), ("flags", "<i4"),
                 ("lookahead", "<i4"), ("release", "<i4"), ("reserved", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.LimiterRecord)
RECORD_BYTES = _REC.itemsize


def check_ceiling(v):
    """a ceiling in dBTP: None, or a finite number <= 0 -> None or a float"""
    if v is None:
        return None
    v = float(v)
    if not math.isfinite(v) or v > 0 or v < -200:
        raise ValueError("true-peak ceiling %r dBTP (-200..0)" % (v,))
    return v


def times(rate: int, lookahead_ms: float = 1.5, release_ms: float = 50.0):
    """-> (lookahead, release) in samples: max(1, round(ms * rate / 1000))"""
    if not (int(rate) > 0 and math.isfinite(lookahead_ms) and math.isfinite(release_ms) and lookahead_ms >= 0 and release_ms >= 0):
        raise ValueError("limiter: rate %r, look-ahead %r ms, release %r ms" % (rate, lookahead_ms, release_ms))
    L = max(1, int(round(lookahead_ms * int(rate) / 1000.0)))
    R = max(1, int(round(release_ms * int(rate) / 1000.0)))
    if L > N.LIM_MAX_LOOKAHEAD or R > N.LIM_MAX_RELEASE:
        raise ValueError("limiter: a look-ahead of %d samples (1..%d) or a release of %d (1..%d)" % (L, N.LIM_MAX_LOOKAHEAD, R,
                                                                                                     N.LIM_MAX_RELEASE))
    return L, R


def _clip_table(offsets, lengths, ceilings):
    n = len(lengths)
    return (N.LimiterClip * n)(*[N.LimiterClip(int(o), int(l), float("nan") if c is None else float(c))
                                 for o, l, c in zip(offsets, lengths, ceilings)])


def run_packed(x: torch.Tensor, offsets, lengths, ceilings, lookahead: int, release: int, out=None, rec=None, work=None):
    """The raw call over one packed fp32 tensor on its device: clip c is x[offsets[c] : offsets[c] + lengths[c]], ceilings[c] its
    ceiling in dBTP or None; lookahead and release in samples.  out: None (measure only), x itself (in place) or a tensor like x.
    -> the records as a uint8 tensor [n_clips * 32] on x's device, not read back: `records(t)` turns it into LimiterRecords.  rec:
    where to write them instead (a uint8 tensor of that size on x's device, 4-byte aligned).  work: a uint8 tensor to use as the
    workspace (at least `work_bytes(lengths)`, 16-byte aligned); its stage arrays are read by `stages`."""
    n = len(lengths)
    arr = _clip_table(offsets, lengths, ceilings)
    L = N.lib()
    need = L.gsv_limiter_work_bytes(arr, n)
    if need == 0:
        raise ValueError("limiter: %d clips (1..65535), or a ceiling outside -200..0 dBTP" % n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    if rec is None:
        rec = torch.empty(n * _REC.itemsize, dtype=torch.uint8, device=x.device)
    elif rec.numel() != n * _REC.itemsize or rec.dtype != torch.uint8 or rec.device != x.device or rec.data_ptr() % 4:
        raise ValueError("limiter: records need %d uint8 on %s, 4-byte aligned" % (n * _REC.itemsize, x.device))
    args = (x.data_ptr() or None, int(x.numel()), arr, n, int(lookahead), int(release), None if out is None else out.data_ptr() or None,
            rec.data_ptr(), work.data_ptr(), int(work.numel()))
    if x.device.type == "cuda":
        with torch.cuda.device(x.device):
            N.check(L.gsv_limiter(*args, N.current_stream_ptr(x.device)))
    else:
        N.check(L.gsv_limiter_host(*args))
    return rec


def work_bytes(lengths) -> int:
    return int(N.lib().gsv_limiter_work_bytes(_clip_table([0] * len(lengths), lengths, [None] * len(lengths)), len(lengths)))


def stages(work, lengths):
    """the stage arrays a call with `out` left in its workspace (csrc/limiter.h states the layout) -> per clip a dict of fp32 numpy
    arrays: c (the gain each sample needs), h (held), r (released), g (the gain applied; 1 for a clip that was not limited)"""
    raw = work.cpu().numpy() if isinstance(work, torch.Tensor) else np.asarray(work)
    a16 = lambda v: (v + 15) & ~15
    total = sum(lengths)
    at = a16(40 * len(lengths)) + a16(16 * len(lengths))       # behind the rows and the statistics
    arrays = {}
    for name in ("c", "h", "v", "r", "g"):
        arrays[name] = raw[at: at + 4 * total].view(np.float32)
        at += a16(4 * total)
    res, o = [], 0
    for n in lengths:
        res.append({k: arrays[k][o: o + n].copy() for k in ("c", "h", "r", "g")})
        o += n
    return res


def records(rec):
    """the record bytes of run_packed (a tensor on any device, or the bytes themselves in a numpy array) -> [LimiterRecord]"""
    raw = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.frombuffer(raw.tobytes(), dtype=_REC)
    return [LimiterRecord(*r.tolist()) for r in a]


def measure(clips, rate: int, device=None):
    """clips: an array, a tensor or a list of them (a list is ONE packed call) -> a LimiterRecord, or a list of them"""
    items, single = _as_list(clips)
    if not items:
        return []
    L, R = times(rate)
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    recs = records(run_packed(x, offsets, lengths, [None] * len(items), L, R))
    return recs[0] if single else recs


def true_peak(clips, rate: int, device=None):
    """the true peak in dBTP of one mono signal (-inf for silence), or a list of them for a list (ONE packed call)"""
    recs = measure(clips, rate, device)
    return [r.dbtp_in for r in recs] if isinstance(recs, list) else recs.dbtp_in


def limit(clips, rate: int, ceiling_db=-1.0, lookahead_ms: float = 1.5, release_ms: float = 50.0, device=None):
    """Every clip held at or under `ceiling_db` dBTP -- a number, or one per clip with None for a clip that is only measured.
    -> (clips, records): each clip comes back as what it came as (a numpy array, or a tensor on the device of the call), fp32, a new
    object; a list is ONE packed call."""
    items, single = _as_list(clips)
    if not items:
        return [], []
    if isinstance(ceiling_db, (list, tuple)):
        ceilings = list(ceiling_db)
        if len(ceilings) != len(items):
            raise ValueError("limiter: %d ceilings for %d clips" % (len(ceilings), len(items)))
    else:
        ceilings = [ceiling_db] * len(items)
    ceilings = [check_ceiling(c) for c in ceilings]
    L, R = times(rate, lookahead_ms, release_ms)
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    out = torch.empty_like(x)
    recs = records(run_packed(x, offsets, lengths, ceilings, L, R, out))
    res = []
    host = None
    for c, o, n in zip(items, offsets, lengths):
        if isinstance(c, torch.Tensor):
            res.append(out[o:o + n].reshape(c.shape))
        else:
            host = out.cpu().numpy() if host is None else host
            res.append(host[o:o + n].reshape(np.shape(c)).copy())
    return (res[0], recs[0]) if single else (res, recs)


# ----------------------------------------------------------------------------------------------------------------------
# streams (csrc/limstream.h)
# ----------------------------------------------------------------------------------------------------------------------
_SREC = np.dtype([("emitted", "<i4"), ("flags", "<i2"), ("lookahead", "<i2"), ("peak_in", "<f4"), ("peak_run", "<f4"),
                  ("min_gain", "<f4"), ("release", "<i4"), ("total", "<i8")])
assert _SREC.itemsize == ctypes.sizeof(N.LimstreamRecord)
STREAM_RECORD_BYTES = _SREC.itemsize


class StreamLimiterRecord:
    """emitted: samples the push handed out; total: samples the stream has handed out; peak_in: the largest finite true-peak
    envelope among the push's samples as they came (np.float32, 0 for none), peak_run: among the stream's so far; min_gain: the
    smallest gain among the push's samples (1 for none); limited: a gain below 1 in this push, limited_ever: in the stream so far;
    nonfinite: a sample of this push whose envelope is a NaN or an infinity (copied); lookahead / release: samples"""

    __slots__ = ("emitted", "total", "peak_in", "peak_run", "min_gain", "limited", "limited_ever", "nonfinite", "lookahead", "release")

    def __init__(self, emitted, flags, lookahead, peak_in, peak_run, min_gain, release, total):
        self.emitted, self.total = int(emitted), int(total)
        self.peak_in, self.peak_run, self.min_gain = np.float32(peak_in), np.float32(peak_run), np.float32(min_gain)
        self.limited = bool(flags & N.LIMS_LIMITED)
        self.limited_ever = bool(flags & N.LIMS_LIMITED_EVER)
        self.nonfinite = bool(flags & N.LIMS_NONFINITE)
        self.lookahead, self.release = int(lookahead), int(release)

    @property
    def dbtp_in(self) -> float:
        """the highest true peak of the unlimited stream so far, dBTP"""
        return dbtp(self.peak_run)

    def __repr__(self):
        return "StreamLimiterRecord(emitted=%d, total=%d, peak_in=%r, peak_run=%r, min_gain=%r, limited=%r, limited_ever=%r, nonfinite=%r)" % (
            self.emitted, self.total, float(self.peak_in), float(self.peak_run), float(self.min_gain), self.limited, self.limited_ever,
            self.nonfinite)


def stream_record(raw):
    """the 32 record bytes (a tensor on any device, or a numpy array of them) -> StreamLimiterRecord"""
    raw = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    return StreamLimiterRecord(*np.frombuffer(raw.tobytes()[:STREAM_RECORD_BYTES], dtype=_SREC)[0].tolist())


class StreamLimiter:
    """One stream held under `ceiling_db` dBTP: the clip limiter's stages 1 - 6 over the whole stream, without the
    trim.  push(x, flush) -> float32 numpy: after N samples in all, max(0, N - delay) have come out, so a push may return nothing; a
    flush returns the rest and the next push starts a fresh stream with the same constants.  The samples never depend on how the
    stream was cut into pushes.  delay = lookahead + 5 samples.  On a GPU device a push is three launches of `gsv_limstream_push`;
    on "cpu" the host twin runs the same scalar routines and gives the same bytes."""

    def __init__(self, ceiling_db, rate: int, device="cpu", lookahead_ms: float = 1.5, release_ms: float = 50.0):
        self.ceiling_db = check_ceiling(ceiling_db)
        if self.ceiling_db is None:
            raise ValueError("a stream limiter needs a ceiling")
        self.rate, self.device = int(rate), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lookahead, self.release = times(rate, lookahead_ms, release_ms)
        self.delay = self.lookahead + 5
        L = N.lib()
        nbytes = L.gsv_limstream_state_bytes(self.lookahead, self.release)
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.on_device:
            with torch.cuda.device(self.device):
                N.check(L.gsv_limstream_init(self.state.data_ptr(), nbytes, self.ceiling_db, self.lookahead, self.release,
                                             N.current_stream_ptr(self.device)))
        else:
            N.check(L.gsv_limstream_init_host(self.state.data_ptr(), nbytes, self.ceiling_db, self.lookahead, self.release))
        self._rec = None        # the last push's record bytes, on the device of the call

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def capacity(self, n_cap: int) -> int:
        """the floats `out` must hold for a push of at most n_cap samples"""
        return int(n_cap) + self.delay

    def enqueue(self, chunk_ptr: int, n_cap: int, n_dev_ptr, flush: bool, out_ptr: int, rec_ptr: int):
        """the raw device call on the current stream: nothing is read back (ChunkEmitter's use)"""
        N.check(N.lib().gsv_limstream_push(self.state.data_ptr(), chunk_ptr or None, int(n_cap), n_dev_ptr, int(bool(flush)),
                                           out_ptr or None, rec_ptr, N.current_stream_ptr(self.device)))

    def _push_once(self, x: torch.Tensor, flush: bool):
        n = int(x.numel())
        out = torch.empty(self.capacity(n), dtype=torch.float32, device=self.device)
        rec = torch.empty(STREAM_RECORD_BYTES // 8, dtype=torch.int64, device=self.device)      # 8-byte aligned
        if self.on_device:
            with torch.cuda.device(self.device):
                self.enqueue(x.data_ptr(), n, None, flush, out.data_ptr(), rec.data_ptr())
        else:
            N.check(N.lib().gsv_limstream_push_host(self.state.data_ptr(), x.data_ptr() or None, n, None, int(bool(flush)),
                                                    out.data_ptr(), rec.data_ptr()))
        return out, rec

    def push_tensor(self, x: torch.Tensor, flush: bool = False) -> torch.Tensor:
        """x on the limiter's device -> the samples this push emits, a new fp32 tensor there.  Its length is read from the record, so
        the call waits for the push.  Input longer than one push may be (2^20 samples) goes in as several, which changes no byte;
        `rec` is then the last one's."""
        x = x.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        parts = []
        cuts = list(range(0, int(x.numel()), N.LIMS_MAX_CHUNK)) or [0]
        for k, at in enumerate(cuts):
            out, rec = self._push_once(x[at: at + N.LIMS_MAX_CHUNK], flush and k + 1 == len(cuts))
            self._rec = stream_record(rec.view(torch.uint8))
            parts.append(out[: self._rec.emitted])
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def push(self, x, flush: bool = False) -> np.ndarray:
        return self.push_tensor(torch.as_tensor(x), flush).cpu().numpy()

    @property
    def rec(self):
        """the last push's StreamLimiterRecord (None before the first push)"""
        return self._rec


def limit_stream(x, rate: int, ceiling_db=-1.0, lookahead_ms: float = 1.5, release_ms: float = 50.0, device=None):
    """the whole signal limited as one stream: one push with flush -> (float32 numpy, StreamLimiterRecord).  device: where the
    samples are, else the GPU when there is one, else the CPU -- the bytes are the same."""
    if device is None:
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            device = x.device
        else:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    lm = StreamLimiter(ceiling_db, rate, device, lookahead_ms, release_ms)
    out = lm.push(x, flush=True)
    return out, lm.rec
