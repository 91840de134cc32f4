"""Integrated loudness (ITU-R BS.1770: K-weighting, gated 400 ms blocks) and normalisation to a target level, on the device
(csrc/loudness.h).  What `pyloudnorm.Meter(rate).integrated_loudness(x)` followed by
`pyloudnorm.normalize.loudness(x, measured, target)` computes -- the last step of the reference WebUI's enhance_audio -- for one
clip or a packed list of them in one call:

    lufs = integrated_loudness(x, 32000)                        # float; -inf when there is nothing to measure
    clips, recs = normalise([a, b, c], 32000, target=-18.0)     # every clip at -18 LUFS, unless its peak would pass 1.0
    recs[0].lufs, recs[0].gain, recs[0].limited

On a GPU device a call is `gsv_loudness` (one small upload, at most seven launches); on "cpu" the host twin `gsv_loudness_host` runs the
same scalar routines and gives the same bits.  A clip shorter than 400 ms, a silent one, one whose blocks all fall under the
gates and one holding a NaN or an infinity has no measurement: lufs -inf, gain 1, samples unchanged."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N


class LoudnessRecord:
    """lufs: the integrated loudness before the gain (-inf: no measurement); gain: the factor applied; peak: max|x| before it;
    limited: the peak limit, not the target, set the gain; blocks / above_abs / kept: 400 ms blocks in all, at or above the
    absolute gate, past both gates; zbar: the mean square behind lufs; nonfinite: the clip holds a NaN or an infinity"""

    __slots__ = ("zbar", "lufs", "gain", "peak", "blocks", "above_abs", "kept", "limited", "measured", "nonfinite")

    def __init__(self, zbar, gain, peak, blocks, above_abs, kept, flags):
        self.zbar, self.gain, self.peak = float(zbar), np.float32(gain), np.float32(peak)
        self.blocks, self.above_abs, self.kept = int(blocks), int(above_abs), int(kept)
        self.limited = bool(flags & N.LOUD_LIMITED)
        self.measured = bool(flags & N.LOUD_MEASURED)
        self.nonfinite = bool(flags & N.LOUD_NONFINITE)
        self.lufs = -0.691 + 10.0 * math.log10(self.zbar) if self.measured else -math.inf

    def __repr__(self):
        return "LoudnessRecord(lufs=%.4f, gain=%r, peak=%r, blocks=%d, above_abs=%d, kept=%d, limited=%r)" % (
            self.lufs, float(self.gain), float(self.peak), self.blocks, self.above_abs, self.kept, self.limited)


_REC = np.dtype([("zbar", "<f8"), ("gain", "<f4"), ("peak", "<f4"), ("blocks", "<i4"), ("above_abs", "<i4"), ("kept", "<i4"),
                 ("flags", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.LoudnessRecord)


def _device_for(clips, device):
    if device is not None:
        device = torch.device(device)
    else:
        first = next((c for c in clips if isinstance(c, torch.Tensor) and c.device.type == "cuda"), None)
        if first is not None:
            device = first.device
        else:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


RECORD_BYTES = _REC.itemsize


def run_packed(x: torch.Tensor, offsets, lengths, targets, rate: int, peak_limit: float = 1.0, out=None, rec=None):
    """The raw call over one packed fp32 tensor on its device: clip c is x[offsets[c] : offsets[c] + lengths[c]], targets[c] its
    LUFS target or None.  out: None (measure only), x itself (in place) or a tensor like x.  -> the records as a uint8 tensor
    [n_clips * 32] on x's device, not read back: `records(t)` turns it into LoudnessRecords.  rec: where to write them instead (a
    uint8 tensor of that size on x's device, 8-byte aligned), e.g. behind the samples so that one copy carries both."""
    n = len(lengths)
    arr = (N.LoudnessClip * n)(*[N.LoudnessClip(int(o), int(l), float("nan") if t is None else float(t))
                                 for o, l, t in zip(offsets, lengths, targets)])
    L = N.lib()
    need = L.gsv_loudness_work_bytes(arr, n, int(rate))
    if need == 0:
        raise ValueError("loudness: %d clips at %r Hz (1..65535 clips, 4000..768000 Hz)" % (n, rate))
    work = torch.empty(need, dtype=torch.uint8, device=x.device)
    if rec is None:
        rec = torch.empty(n * _REC.itemsize, dtype=torch.uint8, device=x.device)
    elif rec.numel() != n * _REC.itemsize or rec.dtype != torch.uint8 or rec.device != x.device or rec.data_ptr() % 8:
        raise ValueError("loudness: records need %d uint8 on %s, 8-byte aligned" % (n * _REC.itemsize, x.device))
    args = (x.data_ptr() or None, int(x.numel()), arr, n, int(rate), float(peak_limit), None if out is None else out.data_ptr() or None,
            rec.data_ptr(), work.data_ptr(), need)
    if x.device.type == "cuda":
        with torch.cuda.device(x.device):
            N.check(L.gsv_loudness(*args, N.current_stream_ptr(x.device)))
    else:
        N.check(L.gsv_loudness_host(*args))
    return rec


def records(rec):
    """the record bytes of run_packed (a tensor on any device, or the bytes themselves in a numpy array) -> [LoudnessRecord]"""
    raw = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.frombuffer(raw.tobytes(), dtype=_REC)
    return [LoudnessRecord(*r.tolist()) for r in a]


def _pack(clips, device):
    """-> (one fp32 tensor on `device` holding every clip, offsets, lengths)"""
    flat = [torch.as_tensor(c).detach().to(dtype=torch.float32).reshape(-1) for c in clips]
    lengths = [int(f.numel()) for f in flat]
    offsets = [0] * len(flat)
    for i in range(1, len(flat)):
        offsets[i] = offsets[i - 1] + lengths[i - 1]
    if len(flat) == 1:
        x = flat[0].to(device).contiguous()
    else:
        x = torch.cat([f.to(device) for f in flat]) if flat else torch.empty(0, device=device)
    return x, offsets, lengths


def _as_list(clips):
    single = not isinstance(clips, (list, tuple))
    return ([clips] if single else list(clips)), single


def measure(clips, rate: int, device=None):
    """clips: an array, a tensor or a list of them (a list is ONE packed call) -> a LoudnessRecord, or a list of them"""
    items, single = _as_list(clips)
    if not items:
        return []
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    recs = records(run_packed(x, offsets, lengths, [None] * len(items), rate))
    return recs[0] if single else recs


def integrated_loudness(x, rate: int, device=None) -> float:
    """LUFS of one mono signal; -inf when there is no measurement"""
    return measure(x, rate, device).lufs


def normalise(clips, rate: int, target=-18.0, peak_limit: float = 1.0, device=None):
    """Every clip scaled to `target` LUFS -- a number, or one per clip with None for a clip that is only measured --, never so far
    that its peak passes peak_limit.  -> (clips, records): each clip comes back as what it came as (a numpy array, or a tensor on
    the device of the call), fp32, a new object; a list is ONE packed call."""
    items, single = _as_list(clips)
    if not items:
        return [], []
    if isinstance(target, (list, tuple)):
        targets = list(target)
        if len(targets) != len(items):
            raise ValueError("loudness: %d targets for %d clips" % (len(targets), len(items)))
    else:
        targets = [target] * len(items)
    for t in targets:
        if t is not None and not math.isfinite(float(t)):
            raise ValueError("loudness target %r" % (t,))
    if not float(peak_limit) > 0:
        raise ValueError("peak_limit %r" % (peak_limit,))
    device = _device_for(items, device)
    x, offsets, lengths = _pack(items, device)
    out = torch.empty_like(x)
    recs = records(run_packed(x, offsets, lengths, targets, rate, peak_limit, out))
    res = []
    host = None
    for c, o, n in zip(items, offsets, lengths):
        if isinstance(c, torch.Tensor):
            res.append(out[o:o + n].reshape(c.shape))
        else:
            host = out.cpu().numpy() if host is None else host
            res.append(host[o:o + n].reshape(np.shape(c)).copy())
    return (res[0], recs[0]) if single else (res, recs)
