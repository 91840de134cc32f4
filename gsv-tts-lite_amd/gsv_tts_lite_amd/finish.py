"""The finishing chain behind the facade's keywords: the one place that knows which stages exist, in which order they
run -- equaliser, compressor, reverb, loudness gain, limiter, then a stream's track --, how a keyword's value is checked, where a
stage's record lies in a buffer it shares with the samples, and which AudioClip fields that record fills.  tts.py and stream.py
loop over `STAGES`; the stage modules (eq.py, compressor.py, reverb.py, loudness.py and level.py, limiter.py) do the work.

    chain = resolve(rate, eq="voice", loudness=-18.0)          # one clip: keyword -> checked value or None
    samples, records = finish_clip(audio, chain, rate)         # TTS.infer / infer_vc: peak rule, 0.2 s of zeros, every stage, one download
    with_records(clip, records)
    chains = resolve(rate, n, eq=[...], true_peak=-1.0)        # n texts: keyword -> list of n or None
    finish_clips(clips, chains, rate, device)                  # TTS.infer_batched: per stage one packed call over the texts that asked
    s = StreamChain(chain_of(chains, t), rate, device, track)  # TTS.infer_stream / infer_stream_batched: a text's stage objects
    audio = s.push_tensor(audio, flush); s.attach(clip)

The table is plain data: nothing registers a stage and nothing reorders them."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import compressor, eq, level, limiter, loudness, reverb, slot_sampling
from .track import TrackResampler


# ----------------------------------------------------------------------------------------------------------------------
# checks: None passes through; an equaliser, compressor or reverb that is the identity is as None
# ----------------------------------------------------------------------------------------------------------------------
def _check_loudness(v, rate=None):
    if v is not None and not np.isfinite(float(v)):
        raise ValueError("loudness target %r" % (v,))
    return None if v is None else float(v)


def _check_loudness_seed(v, rate=None):
    """a stream's loudness_seed: None, or the last `lufs` of the same voice -- which is -inf when nothing was measured, and then
    there is no seed either"""
    if v is None or float(v) == -np.inf:
        return None
    if not np.isfinite(float(v)):
        raise ValueError("loudness seed %r" % (v,))
    return float(v)


def _check_true_peak(v, rate=None):
    return limiter.check_ceiling(v)


def _listed(name, v, n):
    """a per-text value of the kind a list or a tuple names (an EQ, a Compressor, a Reverb, a preset name) -> n values"""
    if not isinstance(v, (list, tuple)):
        return [v] * n
    if len(v) != n:
        raise ValueError("%s has %d entries for %d requests" % (name, len(v), n))
    return list(v)


def _peak_limit(chain) -> float:
    """the loudness gain's own peak limit: off where a limiter follows and holds the ceiling"""
    return math.inf if chain.get("true_peak") is not None else 1.0


# ----------------------------------------------------------------------------------------------------------------------
# what a stage's record writes onto a clip
# ----------------------------------------------------------------------------------------------------------------------
def _sets(field):
    return lambda clip, rec: setattr(clip, field, rec)


def _with_loudness(clip, rec):
    clip.lufs, clip.gain, clip.limited = rec.lufs, rec.gain, rec.limited


def _with_true_peak(clip, rec):
    clip.dbtp, clip.limited = rec.dbtp_out, rec.limited


def _with_level(clip, rec):
    """a clip of a levelled stream: the running measure of the UNLEVELLED stream at its end, the gain of its last sample, and
    whether any sample of the stream so far was set to the peak limit"""
    clip.lufs, clip.gain, clip.limited = rec.lufs, rec.gain_last, rec.limited


def _with_stream_limit(clip, rec):
    """a clip of a stream held under a ceiling (limiter.StreamLimiterRecord): whether the limiter has acted on the stream so far, the
    highest true peak of the unlimited stream so far, the smallest gain among the clip's samples.  No `dbtp`: the output's true
    peak is not measured"""
    clip.limited, clip.dbtp_in, clip.gain_min = rec.limited_ever, rec.dbtp_in, rec.min_gain


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
def _normalise(clips, rate, targets, device, chains):
    """the loudness stage's packed call is two: peak limit 1.0 over the texts with no ceiling, infinity over those whose limiter
    follows"""
    out, recs = [None] * len(clips), [None] * len(clips)
    for limit in (1.0, math.inf):
        pick = [i for i, c in enumerate(chains) if _peak_limit(c) == limit]
        if pick:
            scaled, rs = loudness.normalise([clips[i] for i in pick], rate, [targets[i] for i in pick], limit, device=device)
            for i, a, r in zip(pick, scaled, rs):
                out[i], recs[i] = a, r
    return out, recs


# key: the keyword.  check(v, rate) -> the checked value or None.  per_text(key, v, n) -> v as n values (the first three take a
# list or a tuple as one value per text, the other two whatever slot_sampling.is_sequence does).  module: RECORD_BYTES and
# records() of the clip call.  run(x, v, rate, rec, chain): that call over the one clip x in place, its record into rec.
# many(clips, rate, values, device, chains) -> (clips, records): the packed call over the texts that asked.  write(clip, rec): the
# record onto a clip.  stream: the same stage on a stream, or None.
Stage = namedtuple("Stage", "key check per_text module run many write stream")

# make(v, rate, device, chain) -> the stage object (enqueue, push_tensor, rec).  words / record: its record's fp32 elements and
# their decoder.  in_place: it writes over its input; otherwise its samples lie behind its record.  gives_length: the stages
# behind read their length from its record on the device.  emitter / handle: the names of ChunkEmitter's keyword and of the
# handle's record.  write(clip, rec): the record onto a clip of the stream.
Stream = namedtuple("Stream", "make words record in_place gives_length emitter handle write")

STAGES = (
    Stage(key="eq", check=eq.resolve, per_text=_listed, module=eq,
          run=lambda x, v, rate, rec, chain: eq.run_packed(x, [0], [x.numel()], [0], [eq.design(v, rate)], x, rec),
          many=lambda clips, rate, vs, device, chains: eq.equalise(clips, rate, vs, device=device),
          write=_sets("eq"),
          stream=Stream(make=lambda v, rate, device, chain: eq.StreamEQ(v, rate, device),
                        words=eq.STREAM_RECORD_BYTES // 4, record=eq.stream_record, in_place=True, gives_length=True,
                        emitter="eq", handle="eq", write=_sets("eq"))),
    Stage(key="compress", check=lambda v, rate: compressor.resolve(v), per_text=_listed, module=compressor,
          run=lambda x, v, rate, rec, chain: compressor.run_packed(x, [0], [x.numel()], [0], [v.coefficients(rate)], x, rec),
          many=lambda clips, rate, vs, device, chains: compressor.compress(clips, rate, vs, device=device),
          write=_sets("comp"),
          stream=Stream(make=lambda v, rate, device, chain: compressor.StreamCompressor(v, rate, device),
                        words=compressor.STREAM_RECORD_BYTES // 4, record=compressor.stream_record, in_place=True, gives_length=True,
                        emitter="compress", handle="comp", write=_sets("comp"))),
    Stage(key="ambience", check=lambda v, rate: reverb.resolve(v), per_text=_listed, module=reverb,
          run=lambda x, v, rate, rec, chain: reverb.run_packed(x, [0], [x.numel()], [0], [v.parameters(rate)], x, rec),
          many=lambda clips, rate, vs, device, chains: reverb.reverberate(clips, rate, vs, device=device),
          write=_sets("ambience"),
          stream=None),
    Stage(key="loudness", check=_check_loudness, per_text=slot_sampling.per_request, module=loudness,
          run=lambda x, v, rate, rec, chain: loudness.run_packed(x, [0], [x.numel()], [v], rate, _peak_limit(chain), x, rec),
          many=_normalise,
          write=_with_loudness,
          stream=Stream(make=lambda v, rate, device, chain: level.StreamLeveller(v, rate, device, seed=chain.get("loudness_seed"),
                                                                                 peak_limit=_peak_limit(chain)),
                        words=level.RECORD_BYTES // 4, record=level.record, in_place=True, gives_length=False,
                        emitter="level", handle="level", write=_with_level)),
    Stage(key="true_peak", check=_check_true_peak, per_text=slot_sampling.per_request, module=limiter,
          run=lambda x, v, rate, rec, chain: limiter.run_packed(x, [0], [x.numel()], [v], *limiter.times(rate), x, rec),
          many=lambda clips, rate, vs, device, chains: limiter.limit(clips, rate, vs, device=device),
          write=_with_true_peak,
          stream=Stream(make=lambda v, rate, device, chain: limiter.StreamLimiter(v, rate, device),
                        words=limiter.STREAM_RECORD_BYTES // 4, record=limiter.stream_record, in_place=False, gives_length=True,
                        emitter="limit", handle="limit", write=_with_stream_limit)),
)
STREAM_STAGES = tuple(s.stream for s in STAGES if s.stream is not None)

# the keywords `resolve` takes: the stages', and the stream leveller's seed, which is no stage of its own
_KEYWORDS = {s.key: (s.check, s.per_text) for s in STAGES}
_KEYWORDS["loudness_seed"] = (_check_loudness_seed, slot_sampling.per_request)

# every record starts 8-byte aligned in a shared buffer (the loudness call and the stream stages ask for it); a clip's records lie
# one behind the other, which keeps that alignment because each is a whole number of 8 bytes
ALIGN_WORDS = 2
assert all(s.module.RECORD_BYTES % (4 * ALIGN_WORDS) == 0 for s in STAGES)


# ----------------------------------------------------------------------------------------------------------------------
# keywords -> chain
# ----------------------------------------------------------------------------------------------------------------------
def resolve(rate, n=None, **keywords):
    """The keywords of a facade call, checked -> {keyword: value}.  n None: one clip, each value checked (None, or what the stage
    takes; an equaliser, compressor or reverb that is the identity is as None).  n texts: each keyword one value for all or one
    per text (a wrong length raises ValueError) -> a list of n checked values, or None when no text asked."""
    chain = {}
    for key, v in keywords.items():
        check, per_text = _KEYWORDS[key]
        if n is None:
            chain[key] = check(v, rate)
        else:
            vals = [check(x, rate) for x in per_text(key, v, n)]
            chain[key] = None if all(x is None for x in vals) else vals
    return chain


def chain_of(chains, t):
    """text t's own chain out of resolve(rate, n, ...)"""
    return {key: None if vals is None else vals[t] for key, vals in chains.items()}


def asked(chain) -> bool:
    """does any stage have work? (one clip's chain, or the chains of n texts)"""
    return any(chain.get(s.key) is not None for s in STAGES)


def with_records(clip, records):
    """{keyword: the stage's clip record} onto the clip, in the chain's order -> the clip"""
    for s in STAGES:
        if s.key in records:
            s.write(clip, records[s.key])
    return clip


# ----------------------------------------------------------------------------------------------------------------------
# clips
# ----------------------------------------------------------------------------------------------------------------------
def finish_clip(audio, chain, rate):
    """The tail of TTS.infer / infer_vc with any keyword: the peak rule (an IEEE division by max(peak, 1): dividing by 1 is exact,
    so the same bits as the host's `if peak > 1` without reading the peak back), the 0.2 s of zeros, then every stage the chain
    names over the finished clip in place, one call each in the reference's order, their records written behind the samples: ONE
    download carries all -> (numpy samples, {keyword: record}).  Ahead of a limiter the gain to the loudness target is applied
    with no peak limit: the limiter holds the ceiling."""
    if audio.numel():
        audio = audio / audio.abs().max().clamp(min=1)
    n = audio.numel() + int(0.2 * rate)
    todo = [s for s in STAGES if chain.get(s.key) is not None]
    at, end = {}, -(-n // ALIGN_WORDS) * ALIGN_WORDS
    for s in todo:
        at[s.key] = slice(end, end + s.module.RECORD_BYTES // 4)
        end = at[s.key].stop
    buf = torch.cat([audio, torch.zeros(end - audio.numel(), dtype=audio.dtype, device=audio.device)])    # zeros to n, the pad, the records
    for s in todo:
        s.run(buf[:n], chain[s.key], rate, buf[at[s.key]].view(torch.uint8), chain)
    host = buf.cpu().numpy()
    return host[:n], {s.key: s.module.records(host[at[s.key]].view(np.uint8))[0] for s in todo}


def finish_clips(clips, chains, rate, device):
    """The tail of TTS.infer_batched: per stage ONE packed call over the clips of the texts that asked (the loudness stage: one per
    peak limit), the samples and the record written back onto those AudioClips.  A text that asked for nothing is not touched."""
    for s in STAGES:
        vals = chains.get(s.key)
        if vals is None:
            continue
        pick = [i for i, v in enumerate(vals) if v is not None]
        done, recs = s.many([clips[i].audio_data for i in pick], rate, [vals[i] for i in pick], device, [chain_of(chains, i) for i in pick])
        for i, a, rec in zip(pick, done, recs):
            clips[i].audio_data = a
            s.write(clips[i], rec)


# ----------------------------------------------------------------------------------------------------------------------
# streams
# ----------------------------------------------------------------------------------------------------------------------
class StreamChain:
    """One text's stream: the stage objects its chain names, in order, and the track's resampler behind them (track: a
    track.TrackFormat or None).  Their states span the text -- its segments and the mutes between them -- and a flush ends them all."""

    def __init__(self, chain, rate, device, track=None):
        self.track = None if track is None else TrackResampler(track, rate, device)
        self.stages = [(s.stream, s.stream.make(chain[s.key], rate, device, chain))
                       for s in STAGES if s.stream is not None and chain.get(s.key) is not None]
        self.pcm = None             # with a track: the packets the last push_tensor completed

    def emitter_keywords(self):
        """what stream.ChunkEmitter takes to enqueue the same stages behind its epilogue"""
        return dict([("track", self.track)] + [(st.emitter, obj) for st, obj in self.stages])

    def push_tensor(self, audio, flush):
        """a chunk on the stages' device through every stage (each waits for its record) -> the samples to hand out"""
        for _, obj in self.stages:
            audio = obj.push_tensor(audio, flush=flush)
        if self.track is not None:
            self.pcm = self.track.push(audio, flush=flush)
        return audio

    def attach(self, clip, handle=None):
        """the records of the last push_tensor -- or of a ChunkEmitter handle whose result() has been read -- onto the chunk's
        clip, and with a track its packets -> the clip"""
        for st, obj in self.stages:
            st.write(clip, obj.rec if handle is None else getattr(handle, st.handle))
        if self.track is not None:
            clip.pcm, clip.pcm_rate = self.pcm if handle is None else handle.result()[3], self.track.fmt.rate
        return clip
