"""A parametric equaliser on the device (csrc/eq.h): an ordered list of 1 to 6 second-order sections -- high pass, low
pass, peak, low shelf, high shelf --, designed here in fp64 by the RBJ Audio-EQ-Cookbook formulas and run over one clip or a packed
list of them in one call, from zero state, in fp64, rounded once to fp32:

    e = EQ([Band("highpass", 80.0), Band("peak", 300.0, q=1.0, gain_db=2.5)])
    e = EQ.preset("voice", 32000)                              # the three filters of the reference WebUI's enhance_audio
    clips, recs = equalise([a, b, c], 32000, e)                # or one EQ / preset name / None per clip
    recs[0].peak_in, recs[0].peak_out, recs[0].sections
    h = response(e, 32000, [100.0, 1000.0])                    # complex fp64, from the coefficients
    s = StreamEQ("voice", 32000, "cuda"); y = s.push(chunk)    # a stream in pushes: the same bytes however it is cut

On a GPU device a call is `gsv_eq` (one small upload, at most four launches); on "cpu" the host twin `gsv_eq_host` runs the same
scalar routines and gives the same bits.  Nothing clamps the output: boosts may lift the peak above 1.0 and the record says so;
`true_peak=` / limiter.py is what holds a ceiling.  A clip holding a NaN or an infinity comes back bit for bit, flagged
`nonfinite`.  An EQ without bands is the identity and issues no call; peak and shelf bands of 0 dB are dropped at design time
(their section is the identity in exact arithmetic, not in bits).

The "voice" preset is the cookbook's second-order high pass (80 Hz, Q 1/sqrt 2) and two peaks (300 Hz +2.5 dB Q 1, 7 kHz -3 dB
Q 2) in fp64.  It is not pedalboard / JUCE bit for bit, and not the same curve at the bottom either: those filters run in fp32
and pedalboard's HighpassFilter is first-order."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N
from .loudness import _as_list, _device_for, _pack

KINDS = ("highpass", "lowpass", "peak", "lowshelf", "highshelf")
MIN_RATE, MAX_RATE = 4000, 768000
MAX_SECTIONS = N.EQ_MAX_SECTIONS
RUN, SPAN, CHUNK = N.EQ_RUN, N.EQ_SPAN, N.EQ_CHUNK      # samples of a thread's run, of a block's span, of a chunk


class Band:
    """One second-order section: kind (one of KINDS), f0_hz (10 Hz .. 0.45 rate), q (0.1 .. 40), gain_db (-40 .. 40; ignored by
    highpass and lowpass).  The shelves use the cookbook's Q form, alpha = sin w0 / (2 Q)."""

    __slots__ = ("kind", "f0_hz", "q", "gain_db")

    def __init__(self, kind, f0_hz, q=1.0 / math.sqrt(2.0), gain_db=0.0):
        if kind not in KINDS:
            raise ValueError("eq band kind %r (one of %s)" % (kind, ", ".join(KINDS)))
        self.kind, self.f0_hz, self.q, self.gain_db = kind, float(f0_hz), float(q), float(gain_db)
        if not (math.isfinite(self.f0_hz) and self.f0_hz >= 10.0):
            raise ValueError("eq band at %r Hz (10 Hz .. 0.45 of the rate)" % (f0_hz,))
        if not 0.1 <= self.q <= 40.0:
            raise ValueError("eq band with Q %r (0.1 .. 40)" % (q,))
        if not abs(self.gain_db) <= 40.0:
            raise ValueError("eq band with a gain of %r dB (-40 .. 40)" % (gain_db,))

    @property
    def is_identity(self) -> bool:
        return self.kind in ("peak", "lowshelf", "highshelf") and self.gain_db == 0.0

    def coefficients(self, rate):
        """(b0, b1, b2, a1, a2) at `rate`, normalised by a0, fp64"""
        rate = _check_rate(rate)
        if self.f0_hz > 0.45 * rate:
            raise ValueError("eq band at %r Hz for a rate of %d Hz (10 Hz .. %g Hz)" % (self.f0_hz, rate, 0.45 * rate))
        w0 = 2.0 * math.pi * self.f0_hz / rate
        al, c = math.sin(w0) / (2.0 * self.q), math.cos(w0)
        A = 10.0 ** (self.gain_db / 40.0)
        if self.kind == "highpass":
            b, a = ((1 + c) / 2, -(1 + c), (1 + c) / 2), (1 + al, -2 * c, 1 - al)
        elif self.kind == "lowpass":
            b, a = ((1 - c) / 2, 1 - c, (1 - c) / 2), (1 + al, -2 * c, 1 - al)
        elif self.kind == "peak":
            b, a = (1 + al * A, -2 * c, 1 - al * A), (1 + al / A, -2 * c, 1 - al / A)
        else:
            r = 2 * math.sqrt(A) * al
            if self.kind == "lowshelf":
                b = (A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r))
                a = ((A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r)
            else:
                b = (A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r))
                a = ((A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r)
        return (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])

    def __repr__(self):
        return "Band(%r, %r, q=%r, gain_db=%r)" % (self.kind, self.f0_hz, self.q, self.gain_db)


def _check_rate(rate):
    if isinstance(rate, bool) or int(rate) != rate or not MIN_RATE <= int(rate) <= MAX_RATE:
        raise ValueError("eq: a rate of %r Hz (%d..%d)" % (rate, MIN_RATE, MAX_RATE))
    return int(rate)


PRESETS = ("voice",)


class EQ:
    """An ordered list of at most 6 Bands; none: the identity"""

    __slots__ = ("bands",)

    def __init__(self, bands=()):
        bands = tuple(bands)
        if not all(isinstance(b, Band) for b in bands):
            raise ValueError("an EQ is made of eq.Band objects")
        if len(bands) > MAX_SECTIONS:
            raise ValueError("an EQ of %d bands (at most %d)" % (len(bands), MAX_SECTIONS))
        self.bands = bands

    @staticmethod
    def preset(name, rate) -> "EQ":
        """"voice": the three filters of the reference WebUI's enhance_audio as cookbook designs -- high pass 80 Hz (Q 1/sqrt 2),
        peak 300 Hz +2.5 dB (Q 1), peak 7 kHz -3 dB (Q 2; at 0.45 rate where that is lower)"""
        rate = _check_rate(rate)
        if name != "voice":
            raise ValueError("eq preset %r (one of %s)" % (name, ", ".join(PRESETS)))
        return EQ([Band("highpass", 80.0, q=1.0 / math.sqrt(2.0)), Band("peak", 300.0, q=1.0, gain_db=2.5),
                   Band("peak", min(7000.0, 0.45 * rate), q=2.0, gain_db=-3.0)])

    def __repr__(self):
        return "EQ([%s])" % ", ".join(repr(b) for b in self.bands)


def resolve(value, rate):
    """what the eq= keywords take -- None, a preset name or an EQ -> None (nothing to do: None, or an EQ whose design is the
    identity) or the EQ; a bare list of Bands and anything else is a ValueError"""
    if value is None:
        return None
    if isinstance(value, str):
        value = EQ.preset(value, rate)
    if not isinstance(value, EQ):
        raise ValueError("eq: None, a preset name (%s) or an eq.EQ, not %r" % (", ".join(PRESETS), type(value).__name__))
    return value if len(design(value, rate)) else None


def design(eq: EQ, rate) -> np.ndarray:
    """-> fp64 [sections, 5]: b0 b1 b2 a1 a2 per section, normalised by a0, in list order; bands of 0 dB dropped"""
    rate = _check_rate(rate)
    rows = [b.coefficients(rate) for b in eq.bands if not b.is_identity]
    return np.asarray(rows, np.float64).reshape(len(rows), 5)


def response(eq: EQ, rate, freqs) -> np.ndarray:
    """the cascade's frequency response at `freqs` (Hz) from its coefficients -> complex fp64, shaped like freqs"""
    z = np.exp(-2j * np.pi * np.asarray(freqs, np.float64) / _check_rate(rate))
    h = np.ones(z.shape, np.complex128)
    for b0, b1, b2, a1, a2 in design(eq, rate):
        h = h * ((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z))
    return h


class EqRecord:
    """peak_in / peak_out: max |x| and max |y| (np.float32); sections: the sections run over the clip (0 for a clip that was
    copied); equalised: they were run; nonfinite: the clip holds a NaN or an infinity and came back as it was"""

    __slots__ = ("peak_in", "peak_out", "sections", "equalised", "nonfinite")

    def __init__(self, peak_in, peak_out, sections, flags):
        self.peak_in, self.peak_out, self.sections = np.float32(peak_in), np.float32(peak_out), int(sections)
        self.equalised = bool(flags & N.EQ_EQUALISED)
        self.nonfinite = bool(flags & N.EQ_NONFINITE)

    def __repr__(self):
        return "EqRecord(peak_in=%r, peak_out=%r, sections=%d, equalised=%r, nonfinite=%r)" % (
            float(self.peak_in), float(self.peak_out), self.sections, self.equalised, self.nonfinite)


_REC = np.dtype([("peak_in", "<f4"), ("peak_out", "<f4"), ("sections", "<i4"), ("flags", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.EqRecord)
RECORD_BYTES = _REC.itemsize


def _tables(offsets, lengths, index, designs):
    n = len(lengths)
    clips = (N.EqClip * n)(*[N.EqClip(int(o), int(l), int(d)) for o, l, d in zip(offsets, lengths, index)])
    des = (N.EqDesign * max(1, len(designs)))()
    for k, co in enumerate(designs):
        co = np.asarray(co, np.float64)
        if co.ndim != 2 or co.shape[1] != 5 or not 1 <= co.shape[0] <= MAX_SECTIONS:
            raise ValueError("eq: a design is [1..%d sections, 5 coefficients], not %r" % (MAX_SECTIONS, co.shape))
        des[k].n_sections = co.shape[0]
        for s in range(co.shape[0]):
            for j in range(5):
                des[k].coef[s][j] = float(co[s, j])
    return clips, des


def work_bytes(lengths, n_designs: int) -> int:
    clips, des = _tables([0] * len(lengths), lengths, [-1] * len(lengths), [])
    return int(N.lib().gsv_eq_work_bytes(clips, len(lengths), des, int(n_designs)))


def run_packed(x: torch.Tensor, offsets, lengths, index, designs, out, rec=None, work=None):
    """The raw call over one packed fp32 tensor on its device: clip c is x[offsets[c] : offsets[c] + lengths[c]] and runs through
    designs[index[c]] (an array [sections, 5] as `design` gives it), or is measured and copied for index[c] == -1.  out: x itself
    (in place) or a tensor like x.  -> the records as a uint8 tensor [n_clips * 16] on x's device, not read back: `records(t)`
    turns it into EqRecords.  rec: where to write them instead (a uint8 tensor of that size on x's device, 4-byte aligned), e.g.
    behind the samples so that one copy carries both.  work: a uint8 tensor to use as the workspace."""
    n = len(lengths)
    clips, des = _tables(offsets, lengths, index, designs)
    L = N.lib()
    need = L.gsv_eq_work_bytes(clips, n, des, len(designs))
    if need == 0:
        raise ValueError("eq: %d clips (1..65535) over %d designs, or a design index outside them" % (n, len(designs)))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=x.device)
    if rec is None:
        rec = torch.empty(n * _REC.itemsize, dtype=torch.uint8, device=x.device)
    elif rec.numel() != n * _REC.itemsize or rec.dtype != torch.uint8 or rec.device != x.device or rec.data_ptr() % 4:
        raise ValueError("eq: records need %d uint8 on %s, 4-byte aligned" % (n * _REC.itemsize, x.device))
    args = (x.data_ptr() or None, int(x.numel()), clips, n, des, len(designs), out.data_ptr() or None, rec.data_ptr(), work.data_ptr(),
            int(work.numel()))
    if x.device.type == "cuda":
        with torch.cuda.device(x.device):
            N.check(L.gsv_eq(*args, N.current_stream_ptr(x.device)))
    else:
        N.check(L.gsv_eq_host(*args))
    return rec


def records(rec):
    """the record bytes of run_packed (a tensor on any device, or the bytes themselves in a numpy array) -> [EqRecord]"""
    raw = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.frombuffer(raw.tobytes(), dtype=_REC)
    return [EqRecord(*r.tolist()) for r in a]


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
    return y, EqRecord(peak, peak, 0, N.EQ_NONFINITE if top >= 0x7F800000 else 0)


def equalise(clips, rate, eq, device=None):
    """Every clip through its equaliser -- `eq` is None, a preset name or an EQ for all of them, or a list with one of those per
    clip.  -> (clips, records): each clip comes back as what it came as (a numpy array, or a tensor on the device of the call),
    fp32, a new object; a list is ONE packed call with the distinct designs passed once.  Clips whose EQ is None or the identity
    are measured and copied by that call; when that is all of them, no call is issued."""
    items, single = _as_list(clips)
    if not items:
        return [], []
    rate = _check_rate(rate)
    if isinstance(eq, (list, tuple)):
        eqs = list(eq)
        if len(eqs) != len(items):
            raise ValueError("eq: %d equalisers for %d clips" % (len(eqs), len(items)))
    else:
        eqs = [eq] * len(items)
    designs, index, seen = [], [], {}
    for e in eqs:
        e = resolve(e, rate)
        if e is None:
            index.append(-1)
            continue
        co = design(e, rate)
        index.append(seen.setdefault(co.tobytes(), len(designs)))
        if index[-1] == len(designs):
            designs.append(co)
    if not designs:
        res, recs = zip(*[_copied(c) for c in items])
        return (res[0], recs[0]) if single else (list(res), list(recs))
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    out = torch.empty_like(x)
    recs = records(run_packed(x, offsets, lengths, index, designs, out))
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
# streams (csrc/eqstream.h)
# ----------------------------------------------------------------------------------------------------------------------
_SREC = np.dtype([("emitted", "<i4"), ("flags", "<i4"), ("peak_in", "<f4"), ("peak_out", "<f4"), ("peak_in_run", "<f4"),
                  ("peak_out_run", "<f4"), ("total", "<i8")])
assert _SREC.itemsize == ctypes.sizeof(N.EqstreamRecord)
STREAM_RECORD_BYTES = _SREC.itemsize


class EqStreamRecord:
    """emitted: samples the push handed out (as many as it took); total: samples of the stream so far; peak_in / peak_out: max |x|
    and max |y| over the push's finite samples (np.float32, 0 for none), peak_in_run / peak_out_run: over the stream's so far
    (nothing clamps them: boosts may lift peak_out_run above 1.0); equalised: the record of a live state; nonfinite: a NaN or an
    infinity among this push's samples (it ran through the filter as 0.0 and was copied to the output), nonfinite_ever: among the
    stream's so far"""

    __slots__ = ("emitted", "total", "peak_in", "peak_out", "peak_in_run", "peak_out_run", "equalised", "nonfinite", "nonfinite_ever")

    def __init__(self, emitted, flags, peak_in, peak_out, peak_in_run, peak_out_run, total):
        self.emitted, self.total = int(emitted), int(total)
        self.peak_in, self.peak_out = np.float32(peak_in), np.float32(peak_out)
        self.peak_in_run, self.peak_out_run = np.float32(peak_in_run), np.float32(peak_out_run)
        self.equalised = bool(flags & N.EQS_EQUALISED)
        self.nonfinite = bool(flags & N.EQS_NONFINITE)
        self.nonfinite_ever = bool(flags & N.EQS_NONFINITE_EVER)

    def __repr__(self):
        return "EqStreamRecord(emitted=%d, total=%d, peak_in=%r, peak_out=%r, peak_in_run=%r, peak_out_run=%r, nonfinite=%r, nonfinite_ever=%r)" % (
            self.emitted, self.total, float(self.peak_in), float(self.peak_out), float(self.peak_in_run), float(self.peak_out_run),
            self.nonfinite, self.nonfinite_ever)


def stream_record(raw):
    """the 32 record bytes (a tensor on any device, or a numpy array of them) -> EqStreamRecord"""
    raw = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    return EqStreamRecord(*np.frombuffer(raw.tobytes()[:STREAM_RECORD_BYTES], dtype=_SREC)[0].tolist())


class StreamEQ:
    """One stream through the equaliser `eq` -- a preset name or an EQ -- at `rate`.  push(x, flush) -> float32 numpy,
    as many samples as went in: an equaliser is causal, so there is no delay, and a flush hands out nothing extra; it ends the
    stream, and the next push starts a fresh one with the same design.  The samples never depend on how the stream was cut into
    pushes: concatenated they are `equalise` of the concatenated input, bit for bit.  A NaN or an infinity runs through the filter
    as 0.0 and is copied to the output.  On a GPU device a push is the four launches of `gsv_eqstream_push`; on "cpu" the host
    twin runs the same scalar routines and gives the same bytes."""

    def __init__(self, eq, rate: int, device="cpu"):
        self.rate = _check_rate(rate)
        self.eq = resolve(eq, self.rate)
        if self.eq is None:
            raise ValueError("a stream equaliser needs an equaliser that is not the identity")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _, des = _tables([], [], [], [design(self.eq, self.rate)])
        L = N.lib()
        nbytes = L.gsv_eqstream_state_bytes()
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.on_device:
            with torch.cuda.device(self.device):
                N.check(L.gsv_eqstream_init(self.state.data_ptr(), nbytes, des, N.current_stream_ptr(self.device)))
        else:
            N.check(L.gsv_eqstream_init_host(self.state.data_ptr(), nbytes, des))
        self._rec = None        # the last push's record

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def enqueue(self, chunk_ptr: int, n_cap: int, n_dev_ptr, flush: bool, out_ptr: int, rec_ptr: int):
        """the raw device call on the current stream: nothing is read back (ChunkEmitter's use); out_ptr may be chunk_ptr"""
        N.check(N.lib().gsv_eqstream_push(self.state.data_ptr(), chunk_ptr or None, int(n_cap), n_dev_ptr, int(bool(flush)),
                                          out_ptr or None, rec_ptr, N.current_stream_ptr(self.device)))

    def _push_once(self, x: torch.Tensor, flush: bool):
        n = int(x.numel())
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        rec = torch.empty(STREAM_RECORD_BYTES // 8, dtype=torch.int64, device=self.device)      # 8-byte aligned
        if self.on_device:
            with torch.cuda.device(self.device):
                self.enqueue(x.data_ptr(), n, None, flush, out.data_ptr(), rec.data_ptr())
        else:
            N.check(N.lib().gsv_eqstream_push_host(self.state.data_ptr(), x.data_ptr() or None, n, None, int(bool(flush)),
                                                   out.data_ptr() or None, rec.data_ptr()))
        return out, rec

    def push_tensor(self, x: torch.Tensor, flush: bool = False) -> torch.Tensor:
        """x on the equaliser's device -> the equalised samples, a new fp32 tensor there of x's length.  The record is read, so the
        call waits for the push.  Input longer than one push may be (2^20 samples) goes in as several, which changes no byte; `rec`
        is then the last one's."""
        x = x.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        parts = []
        cuts = list(range(0, int(x.numel()), N.EQS_MAX_CHUNK)) or [0]
        for k, at in enumerate(cuts):
            out, rec = self._push_once(x[at: at + N.EQS_MAX_CHUNK], flush and k + 1 == len(cuts))
            self._rec = stream_record(rec.view(torch.uint8))
            parts.append(out[: self._rec.emitted])
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def push(self, x, flush: bool = False) -> np.ndarray:
        return self.push_tensor(torch.as_tensor(x), flush).cpu().numpy()

    @property
    def rec(self):
        """the last push's EqStreamRecord (None before the first push)"""
        return self._rec


def equalise_stream(x, rate, eq, cuts=None, device=None):
    """the whole signal equalised as one stream on the CPU's host twin (the GPU gives the same bytes: name a device to run there)
    -> (float32 numpy, the last push's EqStreamRecord).  cuts: the lengths of the pushes to cut it into (they must add up to the
    signal's; an empty push is legal), default one push; the last one flushes.  However it is cut, the samples are
    `equalise(x, rate, eq)`'s."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(-1)
    cuts = [len(x)] if cuts is None else [int(c) for c in cuts]
    if any(c < 0 for c in cuts) or sum(cuts) != len(x) or not cuts:
        raise ValueError("eq: cuts of %r for %d samples" % (cuts, len(x)))
    st = StreamEQ(eq, rate, torch.device("cpu") if device is None else device)
    parts, at = [], 0
    for k, c in enumerate(cuts):
        parts.append(st.push(x[at: at + c], flush=k + 1 == len(cuts)))
        at += c
    return np.concatenate(parts), st.rec
