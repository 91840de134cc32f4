"""CPU checks of the true-peak limiter (csrc/limiter.h behind gsv_limiter_host, limiter.py): the host twin against the fp64
restatement tests/limiter_ref.py over lengths and signals, the exact properties of its stages, the ceiling, packed lists, AudioClip
and the TTS keyword.  No GPU: the host twin is built from the scalar routines the device kernels share, and
tests/test_hip_limiter.py pins the device to it bit for bit.

Bounds, with eps = 2^-24 (half an ulp of a value below 1; every stage value here is below 2, which doubles nothing that matters
because the bound counts whole roundings of values below 1 or products with |x|), S the largest per-phase sum of |tap|,
X = max |x|, T the ceiling:

  meter   |tp_twin - tp_ref| <= 14 eps S X: 12 products and 12 additions fused into 12 roundings, the cast of each tap, one to spare
          -- the issue's (12 + 2) 2^-24 S max|x|.
  c       min(1, T / e) has slope at most 1 / T in e:                     dc  = 14 eps S X / T + 2 eps   (the cast of T, the division)
  h       a minimum moves by no more than its arguments:                  dh  = dc
  r       the tile scan adds LOG_TILE times, the chain once per tile over ceil(R / TILE) + 1 tiles, the closing fmaf once, and
          s = fl(1 / R) is off by eps over a distance that adds at most 1: dr  = dh + (LOG_TILE + ceil(R / TILE) + 3) eps
  g       L additions of values up to 1 (relative (L - 1) eps of a sum of at most L, then times 1 / L), the cast of 1 / L, the
          product:                                                        dg  = dr + (L + 1) eps
  y1      one product:                                                    dy1 = (dg + eps) X
  t       the meter on y1 (its own roundings plus S times what y1 is off), slope 1 / T, the division and the cast of T:
                                                                          dt  = (S dy1 + 14 eps S X) / T + 2 eps
  y       one product:                                                    dy  = dt X + dy1 + eps X

For X = 1.5, T = 0.891, L = 48, R = 1600 that is dy = 714 eps = 4.3e-5.  Measured over the whole grid of this file (every length of
limiter_ref.LENGTHS with every signal of KINDS at 32 kHz, three lengths at 8 and 44.1 kHz): the worst |y_twin - y_ref| is 1.15e-6
(the 1.2 sine of 2095 samples at 44.1 kHz; 6.8e-7 at 32 kHz), the worst |tp_twin - tp_ref| 2.4e-7 = 4.0 eps (44.1 kHz; 2.6 eps
at 32 kHz)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as R  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402

EPS = 2.0 ** -24
S = R.phase_sum()
TILE = LM.TILE
LOG_TILE = 10
CEILING = -1.0
T32 = np.float32(10.0 ** (CEILING / 20.0))
RATES = {32000: R.LENGTHS, 8000: [49, TILE + 1, 2 * TILE + 47], 44100: [49, TILE + 1, 2 * TILE + 47]}
cpu = torch.device("cpu")


def meter_bound(X):
    return 14 * EPS * S * X


def output_bound(X, T, L, Rel):
    dc = 14 * EPS * S * X / T + 2 * EPS
    dr = dc + (LOG_TILE + math.ceil(Rel / TILE) + 3) * EPS
    dg = dr + (L + 1) * EPS
    dy1 = (dg + EPS) * X
    dt = (S * dy1 + 14 * EPS * S * X) / T + 2 * EPS
    return dt * X + dy1 + EPS * X


def _peak(x):
    return float(np.abs(x[np.isfinite(x)]).max()) if np.isfinite(x).any() else 0.0


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, rate):
    return R.Limited(R.grid_signal(kind, n, rate), CEILING, *R.times(rate))


@functools.lru_cache(maxsize=None)
def _twin(n, rate):
    """every signal of the grid at one length as ONE packed call of the twin -> ({kind: (y, record, stages)})"""
    xs = [R.grid_signal(k, n, rate) for k in R.KINDS]
    L, Rel = LM.times(rate)
    x = torch.from_numpy(np.concatenate(xs)) if n else torch.zeros(0)
    lengths = [n] * len(xs)
    offsets = [i * n for i in range(len(xs))]
    out = torch.full_like(x, 9.0)
    work = torch.zeros(LM.work_bytes(lengths), dtype=torch.uint8)
    recs = LM.records(LM.run_packed(x, offsets, lengths, [CEILING] * len(xs), L, Rel, out, work=work))
    st = LM.stages(work, lengths)
    return {k: (out.numpy()[o: o + n], r, s) for k, o, r, s in zip(R.KINDS, offsets, recs, st)}


@pytest.mark.parametrize("rate", sorted(RATES))
def test_meter_against_upfirdn(rate):
    assert abs(S - 1.763) < 1e-3
    worst = 0.0
    for n in RATES[rate]:
        kinds = [k for k in R.KINDS if k != "nan"]
        xs = [R.grid_signal(k, n, rate) for k in kinds]
        recs = LM.measure(xs, rate, device="cpu")
        dbs = LM.true_peak(xs, rate, device="cpu")
        for k, x, rec, db in zip(kinds, xs, recs, dbs):
            ref = R.true_peak(x)
            d = abs(float(rec.true_peak_in) - ref)
            worst = max(worst, d)
            assert d <= meter_bound(_peak(x)), (rate, n, k, float(rec.true_peak_in), ref)
            assert rec.true_peak_in >= np.float32(_peak(x)) and not rec.limited and rec.min_gain == 1 and rec.trim == 1
            assert db == LM.dbtp(rec.true_peak_in) and (db == -math.inf) == (_peak(x) == 0)
            if k == "quarter" and n >= 49:      # every sample is +-0.7071; the peaks lie between them
                assert abs(_peak(x) - math.sqrt(0.5)) < 1e-6 and rec.true_peak_in > 1.0
    print("rate %d: worst |tp_twin - tp_ref| = %.3e = %.2f eps" % (rate, worst, worst / EPS))
    # away from the clip's edges the fs / 4 sine reads its amplitude, 1.0 against samples of 0.7071 (the table makes 0.99996 of it);
    # the clip's abrupt start and end, zeros outside, overshoot to 1.057, which is the clip's true peak
    x = R.grid_signal("quarter", 2 * TILE + 47, rate)
    assert abs(R.envelope(x)[100:-100].max() - 1.0) < 1e-3 and abs(R.true_peak(x) - 1.057) < 1e-3


def test_exact_properties_of_the_stages():
    rate = 32000
    L, Rel = LM.times(rate)
    assert (L, Rel) == (48, 1600) and R.times(rate) == (L, Rel)
    for n in R.LENGTHS:
        for k, (y, rec, st) in _twin(n, rate).items():
            x = R.grid_signal(k, n, rate)
            what = (n, k, rec)
            assert rec.lookahead == L and rec.release == Rel
            if k == "nan" and n:
                assert rec.nonfinite and not rec.limited and y.tobytes() == x.tobytes(), what
                assert np.isnan(rec.true_peak_in) and np.isnan(rec.true_peak_out) and rec.min_gain == 1 and rec.trim == 1
                continue
            assert not rec.nonfinite
            c, h, r, g = st["c"], st["h"], st["r"], st["g"]
            assert np.all(c > 0) and np.all(c <= 1) and np.all(h <= c) and np.all(r <= h) and np.all(r > 0), what
            if n:       # the hold is exact: a minimum rounds nothing
                want_h = np.lib.stride_tricks.sliding_window_view(np.concatenate([c, np.ones(L - 1, np.float32)]), L).min(axis=1)
                assert h.tobytes() == want_h.tobytes(), what
                assert np.all(np.diff(r.astype(np.float64)) <= 1.0 / Rel + 4 * EPS), what      # never rises faster than the release
            assert np.all(g > 0) and np.all(g <= 1) and np.all(g <= c), what
            nz = x != 0
            ratio = y[nz].astype(np.float64) / x[nz].astype(np.float64)
            assert np.all(ratio > 0) and np.all(ratio <= 1) and np.all(y[~nz] == 0), what
            assert rec.limited == bool(rec.true_peak_in > T32) == bool(rec.min_gain < 1), what
            if rec.limited:
                assert rec.min_gain == g.min() and 0 < rec.trim <= 1, what
                assert np.array_equal(y, np.float32(g * x) if rec.trim == 1 else rec.trim * np.float32(g * x)), what
            else:       # under the ceiling: bit for bit
                assert y.tobytes() == x.tobytes() and rec.trim == 1 and rec.true_peak_out == rec.true_peak_in and np.all(g == 1), what
            if k in ("zeros", "quiet") or n == 0:
                assert not rec.limited, what
            elif k.startswith("click") or n >= TILE - 1:        # a short sine or noise may stay under the ceiling
                assert rec.limited, what


@pytest.mark.parametrize("rate", sorted(RATES))
def test_twin_against_the_fp64_restatement(rate):
    L, Rel = LM.times(rate)
    worst, worst_at = 0.0, None
    for n in RATES[rate]:
        for k, (y, rec, st) in _twin(n, rate).items():
            if k == "nan" or n == 0:
                continue
            x = R.grid_signal(k, n, rate)
            ref = _oracle(k, n, rate)
            bound = output_bound(_peak(x), ref.T, L, Rel)
            d = float(np.abs(y - ref.y).max())
            if d > worst:
                worst, worst_at = d, (n, k)
            assert d <= bound, (rate, n, k, d, bound)
            # the stages on the way, each within its line of the bound
            dc = 14 * EPS * S * _peak(x) / ref.T + 2 * EPS
            assert np.abs(st["c"] - ref.c).max() <= dc and np.abs(st["h"] - ref.h).max() <= dc, (rate, n, k)
            dr = dc + (LOG_TILE + math.ceil(Rel / TILE) + 3) * EPS
            assert np.abs(st["r"] - ref.r).max() <= dr, (rate, n, k, np.abs(st["r"] - ref.r).max(), dr)
            if rec.limited:
                assert np.abs(st["g"] - ref.g).max() <= dr + (L + 1) * EPS, (rate, n, k)
                assert abs(float(rec.min_gain) - ref.g.min()) <= dr + (L + 1) * EPS
            assert abs(float(rec.true_peak_in) - ref.true_peak_in) <= meter_bound(_peak(x))
    print("rate %d: worst |y_twin - y_ref| = %.3e at %r" % (rate, worst, worst_at))


@pytest.mark.parametrize("rate", sorted(RATES))
def test_the_output_is_under_the_ceiling(rate):
    T = float(T32)
    for n in RATES[rate]:
        for k, (y, rec, _) in _twin(n, rate).items():
            if k == "nan":
                continue
            tp = R.true_peak(y)
            assert tp <= T + 14 * EPS * S * T, (rate, n, k, tp)
            assert abs(float(rec.true_peak_out) - tp) <= 14 * EPS * S * T + 2 * EPS, (rate, n, k, rec, tp)
            if rec.limited:
                assert rec.dbtp_out <= CEILING + 1e-5


def test_packed_clips_equal_single_calls():
    rate = 32000
    g = lambda k, n: R.grid_signal(k, n, rate)
    clips = [g("click_last", TILE + 1), g("quiet", 97), g("noise", 2 * TILE + 47), np.zeros(0, np.float32), g("nan", 49), g("sine997", TILE - 1),
             g("noise", 13), g("quarter", TILE)]
    ceilings = [-1.0, -1.0, -3.0, -1.0, -1.0, None, -6.0, -0.1]
    ys, recs = LM.limit(clips, rate, ceilings, device="cpu")
    for x, c, y, r in zip(clips, ceilings, ys, recs):
        y1, r1 = LM.limit(x, rate, c, device="cpu")
        assert y.tobytes() == y1.tobytes()
        for f in LM.LimiterRecord.__slots__:
            assert np.array_equal(getattr(r, f), getattr(r1, f), equal_nan=True), (f, r, r1)
    assert recs[0].limited and not recs[1].limited and ys[1].tobytes() == clips[1].tobytes()       # the click does not reach the quiet clip
    assert recs[5].true_peak_in > 1.2 and not recs[5].limited and ys[5].tobytes() == clips[5].tobytes()     # measured, not limited
    assert recs[4].nonfinite and [r.limited for r in recs] == [True, False, True, False, False, False, True, True]
    for r, c in zip(recs, ceilings):
        if r.limited:
            assert r.dbtp_out <= c + 1e-5
    # tensors come back as tensors, arrays as arrays, shapes kept; other times give another gain
    t, r = LM.limit(torch.from_numpy(clips[2]).reshape(1, -1), rate, -3.0, device="cpu")
    assert isinstance(t, torch.Tensor) and t.shape == (1, 2 * TILE + 47) and np.array_equal(t.numpy()[0], ys[2])
    y2, r2 = LM.limit(clips[2], rate, -3.0, lookahead_ms=0.0, release_ms=5.0, device="cpu")
    assert (r2.lookahead, r2.release) == (1, 160) and r2.limited and y2.tobytes() != ys[2].tobytes() and r2.dbtp_out <= -3.0 + 1e-5


def test_argument_checks():
    L = N.lib()
    clip = (N.LimiterClip * 1)(N.LimiterClip(0, 100, -1.0))
    need = L.gsv_limiter_work_bytes(clip, 1)
    assert need > 0 and L.gsv_limiter_work_bytes(clip, 0) == 0 and L.gsv_limiter_work_bytes(None, 1) == 0
    assert L.gsv_limiter_work_bytes((N.LimiterClip * 1)(N.LimiterClip(0, -1, -1.0)), 1) == 0
    assert L.gsv_limiter_work_bytes((N.LimiterClip * 1)(N.LimiterClip(0, 100, 0.5)), 1) == 0
    assert L.gsv_limiter_work_bytes((N.LimiterClip * 1)(N.LimiterClip(0, 100, float("inf"))), 1) == 0
    x = torch.zeros(100)
    work = torch.zeros(need, dtype=torch.uint8)
    rec = torch.zeros(32, dtype=torch.uint8)
    ok = (x.data_ptr(), 100, clip, 1, 48, 1600, None, rec.data_ptr(), work.data_ptr(), need)
    assert L.gsv_limiter_host(*ok) == 0
    for i, bad in [(1, 99), (3, 0), (4, 0), (4, 4097), (5, 0), (7, None), (8, None), (9, need - 1), (2, None)]:
        args = list(ok)
        args[i] = bad
        assert L.gsv_limiter_host(*args) == 1, (i, bad)
    for bad in (0.5, float("nan"), float("inf"), -math.inf):
        with pytest.raises(ValueError):
            LM.limit(np.zeros(10, np.float32), 32000, bad, device="cpu")
    with pytest.raises(ValueError):
        LM.limit([np.zeros(10, np.float32)], 32000, [-1.0, -1.0], device="cpu")
    with pytest.raises(ValueError):
        LM.limit(np.zeros(10, np.float32), 32000, -1.0, lookahead_ms=1000.0, device="cpu")
    assert LM.measure([], 32000) == [] and LM.limit([], 32000) == ([], [])


def test_audioclip_true_peak_and_limited_to(monkeypatch):
    from gsv_tts_lite_amd.tts import AudioClip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # the CPU path wherever this runs
    x = R.grid_signal("sine997", 2 * TILE + 47, 32000)
    clip = AudioClip(None, x, 32000, len(x) / 32000, [{"text": "a", "start_s": 0.0, "end_s": 1.0}], "text")
    assert clip.dbtp is None and clip.limited is None
    ref = _oracle("sine997", 2 * TILE + 47, 32000)
    assert abs(10 ** (clip.true_peak() / 20) - ref.true_peak_in) <= meter_bound(1.2)
    out = clip.limited_to(-1.0)
    assert out is not clip and out.subtitles == clip.subtitles and out.orig_text == "text" and out.samplerate == 32000
    assert out.limited and out.dbtp <= -1.0 + 1e-5 and out.true_peak() <= -1.0 + 1e-5
    assert out.audio_data.tobytes() == _twin(2 * TILE + 47, 32000)["sine997"][0].tobytes()
    assert np.array_equal(clip.audio_data, x)
    quiet = AudioClip(None, R.grid_signal("quiet", 97, 32000), 32000, 97 / 32000, [], "q").limited_to()
    assert not quiet.limited and quiet.audio_data.tobytes() == R.grid_signal("quiet", 97, 32000).tobytes()


def test_tts_keyword_validates(tmp_path):
    from gsv_tts import TTS
    from gsv_tts_lite_amd.tts import _check_true_peak
    assert _check_true_peak(None) is None and _check_true_peak(-1) == -1.0 and _check_true_peak(0) == 0.0
    t = TTS(models_dir=str(tmp_path), device="cpu")
    for bad in (0.5, float("nan"), float("inf"), -math.inf):
        with pytest.raises(ValueError, match="ceiling"):
            t.infer("spk.wav", "prompt.wav", "prompt.", "text.", true_peak=bad)
        with pytest.raises(ValueError, match="ceiling"):
            t.infer_vc("spk.wav", "prompt.wav", "prompt.", true_peak=bad)
        with pytest.raises(ValueError, match="ceiling"):
            t.infer_batched("spk.wav", "prompt.wav", "prompt.", ["one.", "two."], true_peak=[-1.0, bad])
    with pytest.raises(ValueError, match="true_peak has 3 entries for 2 requests"):
        t.infer_batched("spk.wav", "prompt.wav", "prompt.", ["one.", "two."], true_peak=[-1.0, None, -1.0])
