"""Real-time track output: a stream of fp32 samples -> fixed s16 packets at the track's rate (csrc/track.h).

What a WebRTC / RTP track, a telephony leg or a sound card wants is not the vocoder's 32 kHz fp32 but s16 at 8, 16, 44.1 or 48 kHz in
packets of a fixed duration.  `TrackResampler` is the stateful link: torchaudio's sinc resampler with a history that spans chunk
boundaries, the FLAC writer's quantiser and a packetiser with a carry, so the packets do not depend on how the stream was cut:

    fmt = TrackFormat(rate=48000, channels=1, packet_ms=20)        # packets of 960 samples
    rs = TrackResampler(fmt, in_rate=32000, device="cuda:0")
    for chunk, last in chunks:
        for packet in rs.push(chunk, flush=last):                 # int16 [k, 960]; k may be 0
            track.send(packet.tobytes())

On a GPU device a push is two launches of `gsv_track_push`; on "cpu" the host twin `gsv_track_push_host` runs the same scalar
routines and gives the same bytes.  `pcm16` is one push with flush.  `stream.ChunkEmitter(track=...)` enqueues the push behind
`gsv_stream_emit` with the chunk's length read from device memory, which is how TTS.infer_stream_batched(track=...) serves it."""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N


class TrackFormat:
    """rate in Hz, channels 1 or 2 (a mono source written twice, interleaved), packets of packet_ms milliseconds -- or of
    packet_samples samples per channel when that is given"""

    def __init__(self, rate: int = 48000, channels: int = 1, packet_ms=20, packet_samples=None):
        self.rate, self.channels = int(rate), int(channels)
        if self.rate < 1:
            raise ValueError("track rate %r" % (rate,))
        if self.channels not in (1, 2):
            raise ValueError("a track has 1 or 2 channels, got %r" % (channels,))
        if packet_samples is not None:
            self.packet = int(packet_samples)
        else:
            from fractions import Fraction
            samples = Fraction(str(packet_ms)) * self.rate / 1000
            if samples.denominator != 1:
                raise ValueError("packets of %r ms at %d Hz are not a whole number of samples" % (packet_ms, self.rate))
            self.packet = int(samples)
        if not 1 <= self.packet <= 4096:
            raise ValueError("packets of %d samples (1..4096)" % self.packet)

    def __repr__(self):
        return "TrackFormat(rate=%d, channels=%d, packet_samples=%d)" % (self.rate, self.channels, self.packet)


class TrackResampler:
    """One stream.  push(x, flush) -> int16 numpy [k, packet * channels]: the whole packets the stream has completed; a flush
    makes the outputs still waiting for their last taps, fills the last packet with zeros and leaves the state fresh for the next
    stream.  `rec` holds the last push's record {packets, outputs produced, samples left in the carry, zeros padded}."""

    _fresh = {}         # (in_rate, out_rate, packet, channels, device) -> a state as gsv_track_init leaves it

    def __init__(self, fmt: TrackFormat, in_rate: int, device="cpu"):
        self.fmt, self.in_rate, self.device = fmt, int(in_rate), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L = N.lib()
        self._args = (self.in_rate, fmt.rate, fmt.packet, fmt.channels)
        nbytes = L.gsv_track_state_bytes(*self._args)
        if nbytes == 0:
            raise ValueError("no track from %d Hz to %r" % (self.in_rate, fmt))
        # a fresh state per (rates, packet, channels, device) is built once -- the 32 -> 44.1 kHz table is 147 294 sin / cos pairs on
        # the host -- and every stream starts from a copy of it: 32 texts do not build 32 tables in front of their first clip
        key = self._args + (str(self.device),)
        if key not in self._fresh:
            fresh = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if self.on_device:
                N.check(L.gsv_track_init(fresh.data_ptr(), nbytes, *self._args, N.current_stream_ptr(self.device)))
                torch.cuda.current_stream(self.device).synchronize()       # once: a copy made on another stream finds it complete
            else:
                N.check(L.gsv_track_init_host(fresh.data_ptr(), nbytes, *self._args))
            self._fresh[key] = fresh
        self.state = self._fresh[key].clone()
        self.rec = [0, 0, 0, 0]

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def capacity(self, n_cap: int) -> int:
        """int16 elements a push of at most n_cap samples can write"""
        return int(N.lib().gsv_track_out_capacity(int(n_cap), *self._args))

    def enqueue(self, chunk_ptr: int, n_cap: int, n_dev_ptr, flush: bool, out_ptr: int, rec_ptr: int):
        """the raw device call on the current stream: nothing is read back (ChunkEmitter's use)"""
        N.check(N.lib().gsv_track_push(self.state.data_ptr(), chunk_ptr or None, int(n_cap), n_dev_ptr, int(bool(flush)), out_ptr,
                                       rec_ptr, N.current_stream_ptr(self.device)))

    def push(self, x, flush: bool = False) -> np.ndarray:
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        n = int(x.numel())
        out = torch.empty(self.capacity(n), dtype=torch.int16, device=self.device)
        rec = torch.empty(4, dtype=torch.int32, device=self.device)
        if self.on_device:
            self.enqueue(x.data_ptr(), n, None, flush, out.data_ptr(), rec.data_ptr())
        else:
            N.check(N.lib().gsv_track_push_host(self.state.data_ptr(), x.data_ptr() or None, n, None, int(bool(flush)),
                                                out.data_ptr(), rec.data_ptr()))
        self.rec = rec.tolist()
        width = self.fmt.packet * self.fmt.channels
        return out[: self.rec[0] * width].cpu().numpy().reshape(self.rec[0], width)


def pcm16(x, in_rate: int, fmt: TrackFormat, device=None) -> np.ndarray:
    """the whole signal as packets, int16 [k, packet * channels]: one push with flush.  device: where the samples are, else the
    GPU when there is one, else the CPU -- the bytes are the same."""
    if device is None:
        if isinstance(x, torch.Tensor) and x.device.type == "cuda":
            device = x.device
        else:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    return TrackResampler(fmt, in_rate, device).push(x, flush=True)
