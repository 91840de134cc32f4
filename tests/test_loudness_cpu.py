"""CPU checks of the loudness meter (csrc/loudness.h behind gsv_loudness_host, loudness.py): the host twin against the fp64
restatement tests/loudness_ref.py over rates, lengths and signals, the gates, the gain and its limit, the clips without a
measurement, packed lists and the round trip.  No GPU: the host twin is built from the scalar routines the device kernels
share, and tests/test_hip_loudness.py pins the device to it bit for bit.

Tolerance.  The twin filters in fp64 like the oracle, in another order (a scan over 512 runs of 16 samples, chunks of 16 384
samples chained), and stores the filtered signal as fp32 before the block sums: a relative 2^-24 per sample, about 1e-9 of a
block's mean square.  Measured over the whole grid of this file (every length of loudness_ref.LENGTHS with every signal of KINDS,
the gating signals, the worked values) the twin's L differs from the oracle's by at most 1.35e-8 LU (the 60 Hz sine of 22 400
samples at 32 kHz); DESIGN 4.20 asks that worst difference to stay under 0.01 LU.  TOL is four times it.  The gain is held to the
same relative tolerance -- 1 LU is a factor of 10^(1/20) -- plus the fp32 rounding of the gain itself.  The round trip reads the
target within TOL plus one ulp of the gain's effect, 20 log10(1 + 2^-23) = 1.04e-6 LU."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import loudness as LD  # noqa: E402

WORST_MEASURED = 1.35e-8
TOL = 4 * WORST_MEASURED                                   # LU
GAIN_RTOL = 10 ** (TOL / 20) - 1 + 2.0 ** -24
ROUND_TRIP_TOL = TOL + 20 * math.log10(1 + 2.0 ** -23)       # + one ulp of the gain's effect: half an ulp from the gain, half from the products

SPAN, LENGTHS, KINDS, _signal = R.SPAN, R.LENGTHS, R.KINDS, R.grid_signal
BLOCKS_32K = {12799: None, 12800: 1, 14400: 1, 17600: 3, 20800: 3, 22400: 4}


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, rate):
    return R.Measurement(_signal(kind, n, rate), rate)


def _compare(rec, ref, what):
    assert rec.blocks == ref.blocks, what
    assert rec.above_abs == ref.above_abs and rec.kept == ref.kept, (what, rec, ref.above_abs, ref.kept)
    if ref.kept == 0:
        assert rec.lufs == -math.inf and rec.zbar == 0.0 and rec.gain == 1 and not rec.measured, (what, rec)
        return 0.0
    d = abs(rec.lufs - ref.lufs)
    assert d <= TOL, (what, rec.lufs, ref.lufs, d)
    return d


def test_worked_values_of_the_definition():
    """the oracle reproduces DESIGN 4.20's worked values to 1e-3 LU, and the twin the oracle"""
    for rate, want in [(32000, -9.0772), (48000, -9.0723), (8000, -9.2128)]:
        x = R.sine(997.0, 2.3, rate)
        ref = R.Measurement(x, rate)
        assert abs(ref.lufs - want) < 1e-3, (rate, ref.lufs)
        assert abs(LD.integrated_loudness(x, rate, device="cpu") - ref.lufs) <= TOL
    for n, nb in BLOCKS_32K.items():
        assert R.block_count(n, 32000) == nb
    assert R.block_count(17600, 32000) == 3
    z = R.block_values(np.ones(17600, np.float32), 32000)
    assert len(z) == 3 and int(0.4 * (2 * 0.25) * 32000) == 6400          # the third block covers 11 200 samples


@pytest.mark.parametrize("rate", sorted(LENGTHS))
def test_twin_against_the_oracle_over_lengths_and_signals(rate):
    worst = 0.0
    for n in LENGTHS[rate]:
        kinds = list(KINDS)
        xs = [_signal(k, n, rate) for k in kinds]
        recs = LD.measure(xs, rate, device="cpu")
        for k, x, rec in zip(kinds, xs, recs):
            ref = _oracle(k, n, rate)
            worst = max(worst, _compare(rec, ref, (rate, n, k)))
            assert rec.peak == (np.abs(x).max() if n else 0)
            if rate == 32000 and n in BLOCKS_32K:
                assert rec.blocks == (BLOCKS_32K[n] or 0)
            if k == "zeros":
                assert rec.lufs == -math.inf and rec.above_abs == 0
    print("rate %d: worst |L_twin - L_oracle| = %.3e LU" % (rate, worst))


@pytest.mark.parametrize("rate", [8000, 32000, 44100])
def test_gates(rate):
    x = _signal("gating", 0, rate)
    ref = _oracle("gating", 0, rate)
    assert ref.margin() >= 1.0, ref.margin()            # no rounding difference can flip a gate
    assert ref.blocks - ref.above_abs >= 3 and ref.above_abs - ref.kept >= 5
    assert ref.ungated < ref.lufs - 2.0                 # a missing gate shows as more than 2 LU
    if rate == 32000:
        assert len(x) == 96960 and ref.blocks == 27 and ref.above_abs == 23 and ref.kept == 14
        assert abs(ref.lufs + 13.31) < 0.005 and abs(ref.ungated + 16.16) < 0.005
    rec = LD.measure(x, rate, device="cpu")
    d = _compare(rec, ref, rate)
    print("gating signal at %d Hz: L %.4f, twin - oracle %.3e LU, margin %.2f LU" % (rate, ref.lufs, d, ref.margin()))
    for target in (-18.0, -30.0):
        y, r = LD.normalise(x, rate, target, device="cpu")
        want = ref.gain(target)
        assert not r.limited and abs(float(r.gain) / want - 1) <= GAIN_RTOL, (target, r.gain, want)
        assert y.dtype == np.float32 and np.array_equal(y, x * r.gain)
        assert r.lufs == rec.lufs


def test_limiter():
    x = _signal("gating", 0, 32000)
    ref = _oracle("gating", 0, 32000)
    peak = np.abs(x).max()
    assert ref.gain(0.0) * peak > 1.0
    y, r = LD.normalise(x, 32000, 0.0, device="cpu")
    assert r.limited and r.gain == np.float32(1.0 / np.float64(peak))
    assert np.abs(y).max() <= 1.0 and np.array_equal(y, x * r.gain)
    y, r = LD.normalise(x, 32000, 0.0, peak_limit=0.5, device="cpu")
    assert r.limited and np.abs(y).max() <= 0.5 and abs(float(r.gain) - 0.5 / float(peak)) <= 2.0 ** -23 * 0.5 / float(peak)
    y, r = LD.normalise(x, 32000, 0.0, peak_limit=math.inf, device="cpu")
    assert not r.limited and abs(float(r.gain) / ref.gain(0.0) - 1) <= GAIN_RTOL


def test_clips_without_a_measurement_come_back_bit_identical():
    rate = 32000
    nan = _signal("noise", 20000, rate).copy()
    nan[7] = np.nan
    inf = _signal("noise", 20000, rate).copy()
    inf[19999] = -np.inf
    quiet = (_signal("noise", 20000, rate) * np.float32(1e-5)).astype(np.float32)      # every block under the absolute gate
    cases = {"empty": np.zeros(0, np.float32), "one": np.ones(1, np.float32), "short": _signal("noise", 12799, rate),
             "zeros": np.zeros(20000, np.float32), "quiet": quiet, "nan": nan, "inf": inf}
    ys, recs = LD.normalise(list(cases.values()), rate, -18.0, device="cpu")
    for (name, x), y, r in zip(cases.items(), ys, recs):
        assert r.lufs == -math.inf and r.gain == 1 and not r.measured and not r.limited and r.kept == 0, (name, r)
        assert y.tobytes() == x.tobytes(), name
        assert r.nonfinite == (name in ("nan", "inf")), name
    assert recs[4].blocks == 3 and recs[4].above_abs == 0
    assert np.isnan(recs[5].peak) and np.isinf(recs[6].peak) and recs[5].blocks == 3
    # a non-finite clip does not disturb its neighbours in the pack
    good = _signal("gating", 0, rate)
    (_, _, y), (_, _, r) = LD.normalise([nan, inf, good], rate, -18.0, device="cpu")
    y1, r1 = LD.normalise(good, rate, -18.0, device="cpu")
    assert y.tobytes() == y1.tobytes() and r.zbar == r1.zbar and r.gain == r1.gain


def test_samples_near_the_end_of_the_fp32_range_keep_the_measurement_finite():
    """the shelf lifts |x| = 3e38 past FLT_MAX; the filtered signal is stored saturating, so zbar and the gain stay finite"""
    x = (R.grid_signal("sine997", 22400, 32000) * np.float32(2.0) * np.float32(3e38)).astype(np.float32)
    assert np.all(np.isfinite(x)) and np.abs(x).max() > 2.9e38
    y, r = LD.normalise(x, 32000, -18.0, device="cpu")
    assert r.measured and not r.nonfinite and math.isfinite(r.zbar) and r.zbar > 1e75 and r.kept == 4
    assert r.gain > 0 and np.all(np.isfinite(y)) and np.array_equal(y, x * r.gain)


def test_packed_clips_at_odd_offsets_equal_single_calls():
    rate = 8000
    clips = [_signal("noise", 5201, rate), np.zeros(0, np.float32), _signal("sine60", 2 * SPAN + 77, rate), _signal("noise", 3199, rate),
             _signal("gating", 0, rate), _signal("noise", 3601, rate)]
    targets = [-18.0, -18.0, None, -23.0, -16.0, 0.0]
    ys, recs = LD.normalise(clips, rate, targets, device="cpu")
    for x, t, y, r in zip(clips, targets, ys, recs):
        y1, r1 = LD.normalise(x, rate, t, device="cpu")
        assert y.tobytes() == y1.tobytes()
        assert (r.zbar, r.gain, r.peak, r.blocks, r.above_abs, r.kept, r.limited) == (r1.zbar, r1.gain, r1.peak, r1.blocks,
                                                                                        r1.above_abs, r1.kept, r1.limited)
    assert recs[2].gain == 1 and ys[2].tobytes() == clips[2].tobytes() and recs[2].measured       # measured, not scaled
    assert recs[5].limited
    # tensors come back as tensors, arrays as arrays, shapes kept
    t, r = LD.normalise(torch.from_numpy(clips[0]).reshape(1, -1), rate, -18.0, device="cpu")
    assert isinstance(t, torch.Tensor) and t.shape == (1, 5201) and np.array_equal(t.numpy()[0], ys[0])


def test_round_trip():
    for rate, kind, n in [(32000, "gating", 0), (8000, "noise", 5600), (44100, "sine60", 30000), (32000, "sine997", 22400)]:
        x = _signal(kind, n, rate)
        y, r = LD.normalise(x, rate, -18.0, device="cpu")
        assert not r.limited
        back = LD.integrated_loudness(y, rate, device="cpu")
        assert abs(back + 18.0) <= ROUND_TRIP_TOL, (rate, kind, back)


def test_argument_checks():
    L = N.lib()
    clip = (N.LoudnessClip * 1)(N.LoudnessClip(0, 100, float("nan")))
    assert L.gsv_loudness_work_bytes(clip, 1, 32000) > 0
    assert L.gsv_loudness_work_bytes(clip, 1, 3999) == 0 and L.gsv_loudness_work_bytes(clip, 0, 32000) == 0
    assert L.gsv_loudness_work_bytes(None, 1, 32000) == 0
    assert L.gsv_loudness_work_bytes((N.LoudnessClip * 1)(N.LoudnessClip(0, -1, 0.0)), 1, 32000) == 0
    need = L.gsv_loudness_work_bytes(clip, 1, 32000)
    x = torch.zeros(100)
    work = torch.zeros(need, dtype=torch.uint8)
    rec = torch.zeros(32, dtype=torch.uint8)
    ok = (x.data_ptr(), 100, clip, 1, 32000, 1.0, None, rec.data_ptr(), work.data_ptr(), need)
    assert L.gsv_loudness_host(*ok) == 0
    for i, bad in [(1, 99), (3, 0), (4, 100), (5, 0.0), (5, float("nan")), (7, None), (8, None), (9, need - 1), (2, None)]:
        args = list(ok)
        args[i] = bad
        assert L.gsv_loudness_host(*args) == 1, (i, bad)
    with pytest.raises(ValueError):
        LD.normalise(np.zeros(10, np.float32), 32000, float("nan"), device="cpu")
    with pytest.raises(ValueError):
        LD.normalise([np.zeros(10, np.float32)], 32000, [-18.0, -18.0], device="cpu")
    with pytest.raises(ValueError):
        LD.measure(np.zeros(10, np.float32), 100, device="cpu")
    assert LD.measure([], 32000) == []


def test_audioclip_loudness_and_normalised(monkeypatch):
    from gsv_tts_lite_amd.tts import AudioClip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # the CPU path wherever this runs
    x = _signal("gating", 0, 32000)
    clip = AudioClip(None, x, 32000, len(x) / 32000, [{"text": "a", "start_s": 0.0, "end_s": 1.0}], "text")
    assert clip.lufs is None and clip.gain is None
    assert abs(clip.loudness() - _oracle("gating", 0, 32000).lufs) <= TOL
    out = clip.normalised(-23.0)
    assert out is not clip and out.subtitles == clip.subtitles and out.orig_text == "text" and out.samplerate == 32000
    assert out.lufs == clip.loudness() and np.array_equal(out.audio_data, x * out.gain) and not out.limited
    assert abs(out.loudness() + 23.0) <= ROUND_TRIP_TOL
    assert np.array_equal(clip.audio_data, x)
