"""Streaming splice on the device: what TTS.infer_stream does between the vocoder and the hand-out of a chunk.

The reference (gsv_tts/TTS.py:429-436) aligns each new chunk to the previous chunk's tail with `_sola_algorithm` (TTS.py:1612-1627:
normalised cross-correlation over 320 candidate offsets + a linear cross-fade, three torch ops and an `.item()`), keeps the last
`overlap` samples back, and hands out the rest.  Here that is one library call per chunk (`gsv_sola`, csrc/sola.h: a score launch
with one block per offset and a splice launch) driven by `ChunkSplicer`, which owns the tail between chunks.  There is no torch
compute on this path and no CPU fallback.

`ChunkEmitter` is the same splice for a loop that serves many streams (TTS.infer_stream_batched) and may not wait for the device:
`gsv_stream_emit` also trims the head of a segment's first chunk and appends the mute behind its last, decides the chunk's length on
the device, and the samples reach the host by one asynchronous copy behind a handle.  With a `track` (track.TrackResampler) the s16
packets of a real-time track are made behind it by `gsv_track_push`, which reads the chunk's length from the emit record on the
device, and travel in the same copy.  With a `level` (level.StreamLeveller) the emitted samples are levelled in place by
`gsv_level_push` between the two, the same way: a track then carries levelled audio.  With an `eq` (eq.StreamEQ) they are equalised
in place by `gsv_eqstream_push` first of all, so the leveller measures equalised audio as `loudness=` does on clips.  With a
`compress` (compressor.StreamCompressor) they are compressed in place by `gsv_cmpstream_push` behind the equaliser and in front of
the leveller: the clip path's order."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native as N
from .finish import STREAM_STAGES


def sola(prev_tail: torch.Tensor, chunk: torch.Tensor, search_len: int = 320) -> Tuple[torch.Tensor, int]:
    """prev_tail fp32 [overlap], chunk fp32 [n] (device) -> (spliced chunk fp32 [n - offset], offset)"""
    if not chunk.is_cuda:
        raise RuntimeError("the streaming splice runs on the HIP device only (no CPU fallback)")
    L = N.lib()
    tail = prev_tail.to(device=chunk.device, dtype=torch.float32).reshape(-1).contiguous()
    x = chunk.to(torch.float32).reshape(-1).contiguous()
    n, ov = int(x.numel()), int(tail.numel())
    ws = torch.empty(L.gsv_sola_workspace(int(search_len)), dtype=torch.uint8, device=x.device)
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    off = torch.empty(1, dtype=torch.int32, device=x.device)
    N.check(L.gsv_sola(tail.data_ptr(), x.data_ptr(), n, ov, int(search_len), out.data_ptr(), off.data_ptr(), ws.data_ptr(), ws.numel(),
                       N.current_stream_ptr(x.device)))
    k = int(off.item())          # the chunk's length depends on it; the samples go to the host right after anyway
    return out[:n - k], k


class ChunkSplicer:
    """One streamed utterance: push() every vocoded chunk (which starts `overlap` samples before the previous one ended), get back
    the samples to hand out.  All but the final chunk keep their last `overlap` samples back as the next splice's tail."""

    def __init__(self, overlap_samples: int, search_len: int = 320):
        self.overlap, self.search_len = int(overlap_samples), int(search_len)
        self.tail: Optional[torch.Tensor] = None
        self.offsets = []          # the offset chosen for every spliced chunk (diagnostics, tests)

    def push(self, chunk: torch.Tensor, is_final: bool) -> torch.Tensor:
        x = chunk.reshape(-1)
        if self.tail is not None:
            x, k = sola(self.tail, x, self.search_len)
            self.offsets.append(k)
        self.tail = x[-self.overlap:].clone()
        return x if is_final else x[:-self.overlap]


class _Emitted:
    """a chunk on its way to the host: ready() asks the copy's event, result() waits for it.  `eq`, `comp`, `level`, `limit`: the
    record of that stage's push (eq.EqStreamRecord, compressor.CmpStreamRecord, level.LevelRecord, limiter.StreamLimiterRecord)
    once result() has been called, None without the stage."""

    def __init__(self, emitter, bufs, event, at):
        self._emitter, self._bufs, self._event, self._value = emitter, bufs, event, None
        # _eq_at, _comp_at, _level_at, _limit_at, _pcm_at: where that stage's record -- the track's for pcm -- starts in the buffer
        # (fp32 elements), None without it; a limiter's samples lie behind its record
        self._pcm_at = at.get("pcm")
        for st in STREAM_STAGES:
            setattr(self, "_%s_at" % st.handle, at.get(st.handle))
            setattr(self, st.handle, None)

    def ready(self) -> bool:
        return self._value is not None or self._event.query()

    def result(self):
        """-> (samples float32 numpy [rec[0]], SOLA offset, head offset); with a track also its packets, int16 numpy
        [packets, packet * channels].  With a limiter the samples are the ones it emitted with this push: as many as its record
        says, which may be none."""
        if self._value is None:
            self._event.synchronize()
            host = self._bufs[1]
            n_out, k, h, _ = host[:4].view(torch.int32).tolist()
            self._value = (host[4: 4 + n_out].numpy().copy(), k, h)
            for st in STREAM_STAGES:
                at = getattr(self, "_%s_at" % st.handle)
                if at is None:
                    continue
                rec = st.record(host[at: at + st.words].numpy().view("uint8"))
                setattr(self, st.handle, rec)
                if not st.in_place:
                    self._value = (host[at + st.words: at + st.words + rec.emitted].numpy().copy(), k, h)
            if self._pcm_at is not None:
                at, fmt = self._pcm_at, self._emitter.track.fmt
                packets = int(host[at: at + 4].view(torch.int32)[0])
                pcm = host[at + 4:].view(torch.int16)[: packets * fmt.packet * fmt.channels]
                self._value += (pcm.numpy().copy().reshape(packets, fmt.packet * fmt.channels),)
            self._emitter._free.append(self._bufs)
            self._bufs = None
        return self._value


class ChunkEmitter:
    """ChunkSplicer plus the host rules of TTS.infer_stream behind it (head trim on a segment's first chunk, the mute behind its
    last), for a loop that serves many streams and may not wait: push() enqueues one library call (`gsv_stream_emit`: the device
    decides offset, head trim and length) and ONE asynchronous copy of the samples with their record into pinned memory, and
    returns a handle.  Owns two tails used in turn (the call reads one and writes the other) and a pinned buffer per chunk in
    flight, reused once its handle has been read.  `new_segment()` forgets the tail.

    track: a track.TrackResampler on the chunks' device, or None.  With one, push() also enqueues `gsv_track_push` over the samples
    `gsv_stream_emit` wrote, their number read from its record on the device, and the packets with their record ride behind the
    samples in the same buffer and the same copy; `flush` ends the track's stream (the last chunk of a text).  The track's state
    outlives `new_segment()`: one stream spans a text's segments and the mutes between them.

    level: a level.StreamLeveller on the chunks' device, or None.  With one, push() enqueues `gsv_level_push` directly behind
    `gsv_stream_emit`, in place on the samples it wrote, their number read from its record on the device; the samples handed out
    -- and the track's packets -- are the levelled ones, and the handle carries the push's record in `level`.  Its state spans the
    text like the track's, and `flush` ends its stream too.

    limit: a limiter.StreamLimiter on the chunks' device, or None.  With one, push() enqueues `gsv_limstream_push` behind the
    leveller (emit -> level -> limit -> track), out of place into its own region of the buffer, the chunk's length read from
    `gsv_stream_emit`'s record on the device; the samples handed out are the ones the limiter emitted with this push -- `delay`
    samples behind the chunk, so the first chunk of a text is that much shorter and the flushing one that much longer --, the
    track reads them with their number from the limiter's record, and the handle carries that record in `limit`.

    eq: an eq.StreamEQ on the chunks' device, or None.  With one, push() enqueues `gsv_eqstream_push` directly behind
    `gsv_stream_emit` and in front of the leveller (emit -> eq -> level -> limit -> track), in place on the samples it wrote, their
    number read from its record on the device; the stages behind read their length from the equaliser's record, which rides
    8-byte aligned behind the samples in the same buffer and the same copy, and the handle carries it in `eq`.  Its state spans
    the text like the others', and `flush` ends its stream too.  Without one the buffer's layout and every byte are what they
    were.

    compress: a compressor.StreamCompressor on the chunks' device, or None.  With one, push() enqueues `gsv_cmpstream_push` behind
    the equaliser and in front of the leveller (emit -> eq -> compress -> level -> limit -> track, the clip path's order), in place
    on the same samples, their number read on the device from the record of the stage in front; the stages behind read their
    length from the compressor's record, which rides 8-byte aligned in the same buffer and the same copy, and the handle carries
    it in `comp`.  Its state spans the text like the others', and `flush` ends its stream too.  Without one the buffer's layout
    and every byte are what they were.

    Which stages there are, their order, their records' sizes and who reads whose length is finish.STREAM_STAGES:
    push() and the handle's result() walk that table."""

    def __init__(self, overlap_samples: int, search_len: int = 320, track=None, level=None, limit=None, eq=None, compress=None):
        self.overlap, self.search_len, self.track, self.level, self.limit = int(overlap_samples), int(search_len), track, level, limit
        self.eq, self.compress = eq, compress
        self._tails, self._cur, self._ws = None, None, None      # _cur: index of the tail the next splice reads, None: no tail yet
        self._free = []             # (device fp32 [4 + capacity]: rec, out; its pinned twin), not in flight

    def new_segment(self):
        self._cur = None

    def _buffers(self, need, device):
        for j, b in enumerate(self._free):
            if b[0].numel() >= need:
                return self._free.pop(j)
        cap = max(need, 1 << 14)
        return (torch.empty(cap, dtype=torch.float32, device=device), torch.empty(cap, dtype=torch.float32).pin_memory())

    def push(self, chunk: torch.Tensor, is_final: bool, trim_head: bool = False, mute_samples: int = 0, flush: bool = False) -> _Emitted:
        if not chunk.is_cuda:
            raise RuntimeError("the streaming splice runs on the HIP device only (no CPU fallback)")
        L = N.lib()
        x = chunk.to(torch.float32).reshape(-1).contiguous()
        n, dev = int(x.numel()), x.device
        if self._tails is None:
            self._tails = torch.zeros(2, max(1, self.overlap), dtype=torch.float32, device=dev)
            self._ws = torch.empty(L.gsv_stream_emit_workspace(self.search_len, n), dtype=torch.uint8, device=dev)   # the scores: any n
        prev = None if self._cur is None else self._tails[self._cur]
        nxt = 0 if self._cur is None else self._cur ^ 1
        used = 4 + n + int(mute_samples)
        # [rec 4 | samples | a stage's record, 8-byte aligned (| its samples, when it does not run in place) | ... | track rec 4 |
        # packets], all in fp32 elements, in the chain's order (finish.STREAM_STAGES)
        layout, cap = [], used - 4          # cap: the most samples the next stage reads
        for st in STREAM_STAGES:
            stage = getattr(self, st.emitter)
            if stage is not None:
                used += used & 1
                layout.append((st, stage, used, cap))
                cap = cap if st.in_place else stage.capacity(cap)
                used += st.words + (0 if st.in_place else cap)
        pcm_cap = 0 if self.track is None else (self.track.capacity(cap) + 1) // 2      # int16 pairs as fp32 elements
        dbuf, hbuf = bufs = self._buffers(used + (0 if self.track is None else 4 + pcm_cap), dev)
        base = dbuf.data_ptr()
        N.check(L.gsv_stream_emit(None if prev is None else prev.data_ptr(), x.data_ptr(), n, self.overlap, self.search_len,
                                  int(bool(is_final)), int(bool(trim_head)), int(mute_samples), base + 16,
                                  self._tails[nxt].data_ptr(), base, self._ws.data_ptr(), self._ws.numel(),
                                  N.current_stream_ptr(dev)))
        self._cur = nxt
        at, src, src_len = {}, base + 16, base          # what the next stage reads: the samples, and their number on the device
        for st, stage, rec_at, src_cap in layout:
            at[st.handle] = rec_at
            out = src if st.in_place else base + 4 * (rec_at + st.words)
            stage.enqueue(src, src_cap, src_len, flush, out, base + 4 * rec_at)
            src = out
            if st.gives_length:
                src_len = base + 4 * rec_at
        if self.track is not None:
            at["pcm"] = used
            self.track.enqueue(src, cap, src_len, flush, base + 4 * (used + 4), base + 4 * used)
            used += 4 + pcm_cap
        hbuf[:used].copy_(dbuf[:used], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return _Emitted(self, bufs, ev, at)
