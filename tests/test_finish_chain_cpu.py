"""CPU checks of the finishing chain (gsv_tts_lite_amd/finish.py): the one loop over the stage table against the
composition of the public single-stage functions -- AudioClip.equalised, .compressed, .ambient, .normalised and .limited_to for
clips, eq.StreamEQ, compressor.StreamCompressor, level.StreamLeveller and limiter.StreamLimiter for streams --, which that loop
does not go through.  No GPU: every stage has a host twin that the device is pinned to elsewhere, so no tolerance appears here;
samples are compared byte for byte and records field by field.

Clips: every non-empty subset of the five keywords over one clip whose peak is above 1, so the peak rule binds.  Batched clips:
three texts with a per-text mix, None entries included.  Streams: every non-empty subset of the four stream keywords over pushes
of 3001, 0, 2400 and 1777 samples, the last one flushing.  The stage settings are those of tests/test_hip_tts_reverb.py."""
import itertools
import math

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import compressor as CM
from gsv_tts_lite_amd import eq as EQM
from gsv_tts_lite_amd import finish
from gsv_tts_lite_amd import level as LV
from gsv_tts_lite_amd import limiter as LM
from gsv_tts_lite_amd import loudness as LD
from gsv_tts_lite_amd import reverb as RV
from gsv_tts_lite_amd.compressor import Compressor
from gsv_tts_lite_amd.eq import EQ, Band
from gsv_tts_lite_amd.reverb import Reverb
from gsv_tts_lite_amd.tts import AudioClip

RATE = 32000
OTHER = Reverb(room_size=0.8, damping=0.2, wet_level=0.5, dry_level=0.3, width=0.5)
LOW = Compressor(-40.0, 3.5, 1.0, 100.0, 0.0)
AN_EQ = EQ([Band("lowshelf", 150.0, gain_db=4.0), Band("peak", 2500.0, q=3.0, gain_db=-6.0)])
TARGET, CEILING = -16.0, -3.0
SETTINGS = {"eq": AN_EQ, "compress": LOW, "ambience": OTHER, "loudness": TARGET, "true_peak": CEILING}
CLIP_FIELDS = ("lufs", "gain", "limited", "dbtp", "dbtp_in", "gain_min", "pcm", "pcm_rate")
RECORDS = {"eq": EQM.EqRecord, "comp": CM.CmpRecord, "ambience": RV.RvbRecord}


def _noise(n, seed):
    """a modulated noise around 0.2: loud enough for the compressor, the leveller and the limiter to act"""
    t = np.arange(n) / RATE
    return (0.2 * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _subsets(keys):
    return [c for r in range(1, len(keys) + 1) for c in itertools.combinations(keys, r)]


def _clip(audio):
    return AudioClip(None, audio, RATE, len(audio) / RATE, [], "a text.")


def _composed(clip, chain):
    """the public single-stage methods in the chain's order, each only where the chain names its keyword"""
    if chain.get("eq") is not None:
        clip = clip.equalised(chain["eq"])
    if chain.get("compress") is not None:
        clip = clip.compressed(chain["compress"])
    if chain.get("ambience") is not None:
        clip = clip.ambient(chain["ambience"])
    if chain.get("loudness") is not None:
        clip = clip.normalised(chain["loudness"], peak_limit=math.inf if chain.get("true_peak") is not None else 1.0)
    if chain.get("true_peak") is not None:
        clip = clip.limited_to(chain["true_peak"])
    return clip


def _same_record(a, b, cls):
    return type(a) is cls and type(b) is cls and all(getattr(a, f) == getattr(b, f) for f in cls.__slots__)


def _assert_same_clip(got, want, what):
    assert got.audio_data.dtype == np.float32 and got.audio_data.tobytes() == want.audio_data.tobytes(), what
    for f in CLIP_FIELDS:
        assert getattr(got, f) == getattr(want, f), (what, f)
    for f, cls in RECORDS.items():
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None and b is None) or _same_record(a, b, cls), (what, f, a, b)


@pytest.fixture(scope="module")
def loud_clip():
    x = _noise(9001, 7)
    x[4321] = 1.7               # the peak rule binds
    return x


def test_finish_clip_is_the_composition_of_the_public_stages(loud_clip):
    peak = np.abs(loud_clip).max()
    assert peak > 1
    base = _clip(np.concatenate([loud_clip / peak, np.zeros(int(0.2 * RATE), np.float32)]))
    subsets = _subsets(tuple(SETTINGS))
    assert len(subsets) == 31
    for keys in subsets:
        chain = finish.resolve(RATE, **{k: SETTINGS[k] for k in keys})
        assert finish.asked(chain)
        samples, recs = finish.finish_clip(torch.from_numpy(loud_clip), chain, RATE)
        assert sorted(recs) == sorted(keys)
        got = finish.with_records(_clip(samples), recs)
        want = _composed(base, chain)
        _assert_same_clip(got, want, keys)
        assert all((getattr(got, f) is None) == (k not in keys) for k, f in (("eq", "eq"), ("compress", "comp"), ("ambience", "ambience"),
                                                                                ("loudness", "lufs"), ("true_peak", "dbtp")))
    assert not finish.asked(finish.resolve(RATE, eq=None, compress=None, ambience=None, loudness=None, true_peak=None))


def _count_stage_calls(monkeypatch):
    calls = {}
    for name, mod in (("eq", EQM), ("compress", CM), ("ambience", RV), ("loudness", LD), ("true_peak", LM)):
        def counting(*a, _inner=mod.run_packed, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _inner(*a, **k)
        monkeypatch.setattr(mod, "run_packed", counting)
    return calls


def test_finish_clips_is_one_packed_call_per_stage(monkeypatch):
    audios = [_noise(n, seed) for n, seed in ((7001, 1), (4000, 2), (5555, 3))]
    mix = dict(eq=[AN_EQ, "voice", None], compress=[LOW, None, LOW], ambience=[OTHER, "voice", None],
               loudness=[TARGET, None, TARGET], true_peak=[CEILING, CEILING, None])
    chains = finish.resolve(RATE, 3, **mix)
    want = [_composed(_clip(a), {k: v[i] for k, v in mix.items()}) for i, a in enumerate(audios)]
    assert want[0].dbtp is not None and want[1].lufs is None and want[2].dbtp is None and want[2].limited is not None
    calls = _count_stage_calls(monkeypatch)
    clips = [_clip(a) for a in audios]
    finish.finish_clips(clips, chains, RATE, "cpu")
    assert calls == {"eq": 1, "compress": 1, "ambience": 1, "loudness": 2, "true_peak": 1}      # loudness: one per peak limit
    for i, (got, w) in enumerate(zip(clips, want)):
        _assert_same_clip(got, w, i)
    calls.clear()
    asked_by_some = finish.resolve(RATE, 3, eq=[AN_EQ, None, None], compress=[LOW, None, LOW], ambience=None,
                                   loudness=[None, None, TARGET], true_peak=[None, None, None])
    assert asked_by_some["true_peak"] is None and asked_by_some["ambience"] is None
    clips = [_clip(a) for a in audios]
    finish.finish_clips(clips, asked_by_some, RATE, "cpu")
    assert calls == {"eq": 1, "compress": 1, "loudness": 1}
    assert clips[1].audio_data is audios[1] and clips[1].audio_data.tobytes() == _noise(4000, 2).tobytes()     # all None: not touched
    _assert_same_clip(clips[1], _clip(audios[1]), "a text with all None")
    _assert_same_clip(clips[0], _composed(_clip(audios[0]), {"eq": AN_EQ, "compress": LOW}), 0)
    _assert_same_clip(clips[2], _composed(_clip(audios[2]), {"compress": LOW, "loudness": TARGET}), 2)


def test_stream_chain_is_the_composition_of_the_stream_stages():
    pushes = (3001, 0, 2400, 1777)
    x = _noise(sum(pushes), 11)
    x[100], x[5000] = 0.99, -0.97           # above the ceiling: the limiter acts
    settings = {"eq": AN_EQ, "compress": LOW, "loudness": TARGET, "true_peak": CEILING}
    classes = {"eq": EQM.EqStreamRecord, "compress": CM.CmpStreamRecord, "loudness": LV.LevelRecord, "true_peak": LM.StreamLimiterRecord}
    subsets = _subsets(tuple(settings))
    assert len(subsets) == 15
    for keys in subsets:
        chain = finish.resolve(RATE, loudness_seed=-23.0, **{k: settings[k] for k in keys})
        stream = finish.StreamChain(chain, RATE, "cpu")
        hand = {}
        if "eq" in keys:
            hand["eq"] = EQM.StreamEQ(AN_EQ, RATE, "cpu")
        if "compress" in keys:
            hand["compress"] = CM.StreamCompressor(LOW, RATE, "cpu")
        if "loudness" in keys:
            hand["loudness"] = LV.StreamLeveller(TARGET, RATE, "cpu", seed=-23.0, peak_limit=math.inf if "true_peak" in keys else 1.0)
        if "true_peak" in keys:
            hand["true_peak"] = LM.StreamLimiter(CEILING, RATE, "cpu")
        assert [st.emitter for st, _ in stream.stages] == [{"eq": "eq", "compress": "compress", "loudness": "level", "true_peak": "limit"}[k]
                                                           for k in keys]
        at, total = 0, 0
        for j, n in enumerate(pushes):
            flush = j == len(pushes) - 1
            got = stream.push_tensor(torch.from_numpy(x[at: at + n]), flush)
            want = x[at: at + n]
            for stage in hand.values():
                want = stage.push(want, flush)
            at += n
            total += len(want)
            assert got.dtype == torch.float32 and got.numpy().tobytes() == want.tobytes(), (keys, j)
            for (_, obj), (k, stage) in zip(stream.stages, hand.items()):
                assert _same_record(obj.rec, stage.rec, classes[k]), (keys, j, k, obj.rec, stage.rec)
            clip = stream.attach(_clip(got.numpy()))
            assert (clip.eq is hand_rec(stream, "eq")) and (clip.comp is hand_rec(stream, "compress"))
            if "true_peak" in keys:
                r = hand["true_peak"].rec
                assert (clip.limited, clip.dbtp_in, clip.gain_min) == (r.limited_ever, r.dbtp_in, r.min_gain) and clip.dbtp is None
            if "loudness" in keys:
                r = hand["loudness"].rec
                assert (clip.lufs, clip.gain) == (r.lufs, r.gain_last) and ("true_peak" in keys or clip.limited == r.limited)
            assert clip.pcm is None and clip.pcm_rate is None
        assert total == len(x)              # the flush hands out what the limiter held back


def hand_rec(stream, emitter):
    """the record of the chain's own stage object behind ChunkEmitter's keyword `emitter`, None without the stage"""
    return next((obj.rec for st, obj in stream.stages if st.emitter == emitter), None)


def test_stream_chain_with_a_track():
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    fmt = TrackFormat(48000, 1, 20)
    x = _noise(5000, 5)
    stream = finish.StreamChain(finish.resolve(RATE, eq="voice"), RATE, "cpu", fmt)
    h_eq, h_track = EQM.StreamEQ("voice", RATE, "cpu"), TrackResampler(fmt, RATE, "cpu")
    assert stream.emitter_keywords() == {"track": stream.track, "eq": stream.stages[0][1]}
    for lo, hi, flush in ((0, 3001, False), (3001, 5000, True)):
        got = stream.push_tensor(torch.from_numpy(x[lo:hi]), flush)
        want = h_eq.push(x[lo:hi], flush)
        clip = stream.attach(_clip(got.numpy()))
        assert got.numpy().tobytes() == want.tobytes() and clip.pcm_rate == 48000
        assert np.array_equal(clip.pcm, h_track.push(torch.from_numpy(want), flush=flush))


def test_resolve_checks_as_the_facade_did():
    for kw, n, message in ((dict(eq=[AN_EQ, None]), 3, "eq has 2 entries for 3 requests"),
                           (dict(loudness=[-16.0, -18.0]), 3, "loudness has 2 entries for 3 requests"),
                           (dict(true_peak=np.array([-1.0])), 2, "true_peak has 1 entries for 2 requests"),
                           (dict(eq="radio"), None, r"eq preset 'radio' \(one of voice\)"),
                           (dict(compress="radio"), 2, r"compressor preset 'radio' \(one of voice\)"),
                           (dict(ambience=["radio", None]), 2, r"reverb preset 'radio' \(one of voice\)"),
                           (dict(eq=[Band("peak", 300.0, gain_db=2.0)]), None, r"eq: None, a preset name \(voice\) or an eq.EQ, not 'list'"),
                           (dict(eq=[Band("peak", 300.0, gain_db=2.0)]), 1, r"eq: None, a preset name \(voice\) or an eq.EQ, not 'Band'"),
                           (dict(loudness=math.inf), None, "loudness target inf"),
                           (dict(loudness=[-16.0, math.nan]), 2, "loudness target nan"),
                           (dict(loudness_seed=math.nan), None, "loudness seed nan"),
                           (dict(true_peak=1.0), None, r"true-peak ceiling 1.0 dBTP \(-200..0\)"),
                           (dict(true_peak=[-1.0, 0.5]), 2, r"true-peak ceiling 0.5 dBTP \(-200..0\)")):
        with pytest.raises(ValueError, match=message):
            finish.resolve(RATE, n, **kw)
    identities = dict(eq=EQ([Band("peak", 300.0, gain_db=0.0)]), compress=Compressor(ratio=1.0), ambience=Reverb(wet_level=0.0, dry_level=0.5))
    assert finish.resolve(RATE, **identities) == {"eq": None, "compress": None, "ambience": None}
    assert finish.resolve(RATE, 2, **identities) == {"eq": None, "compress": None, "ambience": None}
    assert finish.resolve(RATE, 2, eq=[None, None], loudness=[None, None], true_peak=None, loudness_seed=-math.inf) == {
        "eq": None, "loudness": None, "true_peak": None, "loudness_seed": None}
    got = finish.resolve(RATE, 3, loudness=np.array([-16.0, -18.5, -23.0]), true_peak=-1, eq=(AN_EQ, None, "voice"))
    assert got["loudness"] == [-16.0, -18.5, -23.0] and all(type(v) is float for v in got["loudness"])
    assert got["true_peak"] == [-1.0, -1.0, -1.0] and got["eq"][0] is AN_EQ and got["eq"][1] is None and isinstance(got["eq"][2], EQ)
    assert finish.chain_of(got, 1) == {"loudness": -18.5, "true_peak": -1.0, "eq": None}
    one = finish.resolve(RATE, eq="voice", loudness=-18, true_peak=None, loudness_seed=-20)
    assert isinstance(one["eq"], EQ) and one["loudness"] == -18.0 and one["true_peak"] is None and one["loudness_seed"] == -20.0
