"""A running BS.1770 gain for streams (csrc/level.h): what `loudness=` is to a clip, for audio that is handed out
before the programme is complete.  The K-weighting, the 400 ms blocks and both gates of loudness.py are measured over the stream
so far, and a gain moves towards the target at a bounded rate, decided at every tenth of a second from the audio that came before
it -- so the leveller adds no delay, and its output does not depend on how the stream was cut into pushes:

    lv = StreamLeveller(target=-18.0, rate=32000, device="cuda:0", seed=last_lufs_of_this_voice)
    for chunk, last in chunks:
        out = lv.push(chunk, flush=last)           # float32 numpy, as many samples as came in
    lv.lufs, lv.rec.gain_last, lv.rec.limited

On a GPU device a push is two launches of `gsv_level_push`; on "cpu" the host twin `gsv_level_push_host` runs the same scalar
routines and gives the same bits.  `level` is one push with flush.  `stream.ChunkEmitter(level=...)` enqueues the push behind
`gsv_stream_emit`, in place on the emitted samples with their number read from device memory, which is how
TTS.infer_stream_batched(loudness=...) serves it."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N

_REC = np.dtype([("zbar", "<f8"), ("gain_first", "<f4"), ("gain_last", "<f4"), ("clamped", "<i8"), ("blocks", "<i4"),
                 ("above_abs", "<i4"), ("kept", "<i4"), ("flags", "<i4")])
assert _REC.itemsize == ctypes.sizeof(N.LevelRecord)
RECORD_BYTES = _REC.itemsize
_HEADER = 2864         # sizeof(LevelHeader): the knots lie behind it (csrc/level.h asserts both offsets)


class LevelRecord:
    """lufs: the running loudness of the UNLEVELLED stream behind the push (-inf: no measurement yet); zbar: the mean square behind
    it; gain_first / gain_last: the gain of the push's first and last sample; clamped: samples set to +-peak_limit so far, limited:
    any; blocks / above_abs / kept: 400 ms blocks measured, at or above the absolute gate, past both gates; nonfinite / full: the
    measure is frozen by a NaN or an infinity / by a full block history"""

    __slots__ = ("zbar", "lufs", "gain_first", "gain_last", "clamped", "limited", "blocks", "above_abs", "kept", "measured",
                 "nonfinite", "full")

    def __init__(self, zbar, gain_first, gain_last, clamped, blocks, above_abs, kept, flags):
        self.zbar, self.gain_first, self.gain_last = float(zbar), np.float32(gain_first), np.float32(gain_last)
        self.clamped, self.blocks, self.above_abs, self.kept = int(clamped), int(blocks), int(above_abs), int(kept)
        self.limited = self.clamped > 0
        self.measured = bool(flags & N.LEVEL_MEASURED)
        self.nonfinite = bool(flags & N.LEVEL_NONFINITE)
        self.full = bool(flags & N.LEVEL_FULL)
        self.lufs = -0.691 + 10.0 * math.log10(self.zbar) if self.measured else -math.inf

    def __repr__(self):
        return "LevelRecord(lufs=%.4f, gain_first=%r, gain_last=%r, clamped=%d, blocks=%d, kept=%d)" % (
            self.lufs, float(self.gain_first), float(self.gain_last), self.clamped, self.blocks, self.kept)


def record(raw):
    """the 40 record bytes (a tensor on any device, or a numpy array of them) -> LevelRecord"""
    raw = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    return LevelRecord(*np.frombuffer(raw.tobytes()[:RECORD_BYTES], dtype=_REC)[0].tolist())


class StreamLeveller:
    """One stream.  push(x, flush) -> float32 numpy of x's length; a flush ends the stream (its incomplete last tenth of a second
    has been output and is never measured) and the next push starts a fresh one with the same constants.

    target: LUFS.  seed: the loudness in LUFS this voice is expected to have -- the last `lufs` of the same voice --, counted as
    seed_blocks measured blocks, so the stream starts at the right gain instead of converging to it; None: start at gain 1.
    slew_db_s: how fast the gain may move; max_gain_db: how far from 1 it may go; peak_limit: no gain lifts the peak seen so far
    above it, and a sample that would pass it is set to it; max_seconds: the block history, after which the gain holds."""

    def __init__(self, target, rate: int, device="cpu", seed=None, seed_blocks=10, slew_db_s: float = 10.0, max_gain_db: float = 20.0,
                 peak_limit: float = 1.0, max_seconds: int = 600):
        self.target, self.rate, self.device = float(target), int(rate), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = N.lib()
        self._args = (self.rate, self.target, float("nan") if seed is None else float(seed), float(seed_blocks), float(slew_db_s),
                      float(max_gain_db), float(peak_limit), int(max_seconds))
        nbytes = L.gsv_level_state_bytes(self.rate, int(max_seconds))
        if nbytes == 0:
            raise ValueError("no leveller at %r Hz with a history of %r s (4000..192000 Hz, 1..3600 s)" % (rate, max_seconds))
        # built in place, stream by stream: the constants hold the seed, which differs from call to call, so a cache keyed by them
        # would only grow; the init is a few pow calls, one memset and an upload of the header
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.on_device:
            with torch.cuda.device(self.device):
                N.check(L.gsv_level_init(self.state.data_ptr(), nbytes, *self._args, N.current_stream_ptr(self.device)))
        else:
            N.check(L.gsv_level_init_host(self.state.data_ptr(), nbytes, *self._args))
        self._rec = None        # the last push's record bytes, on the device of the call

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def enqueue(self, chunk_ptr: int, n_cap: int, n_dev_ptr, flush: bool, out_ptr: int, rec_ptr: int):
        """the raw device call on the current stream: nothing is read back (ChunkEmitter's use)"""
        N.check(N.lib().gsv_level_push(self.state.data_ptr(), chunk_ptr or None, int(n_cap), n_dev_ptr, int(bool(flush)),
                                       out_ptr or None, rec_ptr, N.current_stream_ptr(self.device)))

    def push_tensor(self, x: torch.Tensor, flush: bool = False) -> torch.Tensor:
        """x on the leveller's device -> the levelled samples, a new fp32 tensor there; the record stays there until `rec` is read"""
        x = x.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        n = int(x.numel())
        out = torch.empty_like(x)
        rec = torch.empty(RECORD_BYTES // 8, dtype=torch.int64, device=self.device)        # 8-byte aligned
        if self.on_device:
            with torch.cuda.device(self.device):
                self.enqueue(x.data_ptr(), n, None, flush, out.data_ptr(), rec.data_ptr())
        else:
            N.check(N.lib().gsv_level_push_host(self.state.data_ptr(), x.data_ptr() or None, n, None, int(bool(flush)),
                                                out.data_ptr() or None, rec.data_ptr()))
        self._rec = rec.view(torch.uint8)
        return out

    def push(self, x, flush: bool = False) -> np.ndarray:
        return self.push_tensor(torch.as_tensor(x), flush).cpu().numpy()

    def knot_gains(self) -> np.ndarray:
        """the knots decided so far, A_0 .. A_K in fp64, read from the state (diagnostics, tests)"""
        raw = self.state.cpu().numpy()
        K = int(raw[52:56].view("<i4")[0])
        return raw[_HEADER: _HEADER + 8 * (K + 1)].view("<f8").copy()

    @property
    def rec(self):
        """the last push's LevelRecord (None before the first push)"""
        if isinstance(self._rec, torch.Tensor):
            self._rec = record(self._rec)
        return self._rec

    @property
    def lufs(self) -> float:
        r = self.rec
        return -math.inf if r is None else r.lufs


def level(x, rate: int, target=-18.0, device=None, **kw):
    """the whole signal levelled as one stream: one push with flush -> (float32 numpy, LevelRecord).  device: where the samples
    are, else the GPU when there is one, else the CPU -- the bits are the same.  kw: StreamLeveller's constants."""
    if device is None:
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            device = x.device
        else:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    lv = StreamLeveller(target, rate, device, **kw)
    out = lv.push(x, flush=True)
    return out, lv.rec
