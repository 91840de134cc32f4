"""CPU checks of the stream limiter (csrc/limstream.h behind gsv_limstream_push_host, limiter.StreamLimiter).  No GPU:
the host twin is built from the scalar routines the device kernels share, and tests/test_hip_limstream.py pins the device to it
byte for byte.

What is held: the whole stream in one flushed push equals fl(g x) with g the CLIP twin's stage array, bit for bit (x itself where
the clip was not limited); every cutting of a stream -- one push, single samples, pushes of D - 1, D and D + 1, cuts around a tile
edge, seeded random cuts with empty pushes, a flush by an empty push -- gives the same bytes and the per-push counts of 4.23; the
output against the fp64 restatement tests/limstream_ref.py within the bound test_limiter_cpu.py derives stage by stage (714 2^-24
at the defaults; the stream has no trim, so its error is the dy1 part of that bound and the whole bound holds with room);
|y| <= T (1 + 2^-22); the fp64 meter on the output at most max(T, oracle's true peak of y) + 14 2^-24 S T.

Measured over this file's grid: the worst |y_twin - y_ref| is 1.15e-6 (the 1.2 sine of 2095 samples at 44.1 kHz; 6.7e-7 at 32 kHz),
and the largest overshoot true_peak(y) / T of the oracle is 1.00082 at 32 kHz (0.007 dB), 1.00041 at 44.1 kHz and 1.0057 at 8 kHz
(0.05 dB), each on the noise; the fs / 4 sine gives 1.00007 at 32 kHz, the 997 Hz sine and the clicks nothing."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as R  # noqa: E402
import limstream_ref as SR  # noqa: E402
from test_limiter_cpu import EPS, S, output_bound, _peak  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402

TILE = LM.TILE
CEILING = -1.0
T32 = np.float32(10.0 ** (CEILING / 20.0))
LENGTHS = R.LENGTHS + [4 * TILE + 47]        # the release (R = 1600 > TILE) chained over several tiles
RATES = {32000: LENGTHS, 8000: [49, TILE + 1, 2 * TILE + 47], 44100: [49, TILE + 1, 2 * TILE + 47]}


@functools.lru_cache(maxsize=None)
def _limiter(rate):
    return LM.StreamLimiter(CEILING, rate, "cpu")


def run(lm, x, cuts):
    """the stream cut at `cuts` (the last push flushes) -> (samples, what each push emitted, the records)"""
    parts, recs, at = [], [], 0
    for k, n in enumerate(cuts):
        parts.append(lm.push(x[at: at + n], flush=k + 1 == len(cuts)))
        recs.append(lm.rec)
        at += n
    assert at == len(x)
    return np.concatenate(parts), [len(p) for p in parts], recs


@functools.lru_cache(maxsize=None)
def _whole(kind, n, rate):
    y, counts, recs = run(_limiter(rate), R.grid_signal(kind, n, rate), [n])
    assert counts == [n]
    return y, recs[0]


@functools.lru_cache(maxsize=None)
def _clip(kind, n, rate):
    """the clip twin on the same samples -> (record, g)"""
    x = torch.from_numpy(R.grid_signal(kind, n, rate))
    L, Rel = LM.times(rate)
    work = torch.zeros(LM.work_bytes([n]), dtype=torch.uint8)
    rec = LM.records(LM.run_packed(x, [0], [n], [CEILING], L, Rel, torch.empty_like(x), work=work))[0]
    return rec, LM.stages(work, [n])[0]["g"]


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, rate):
    return SR.StreamLimited(R.grid_signal(kind, n, rate), CEILING, *R.times(rate))


def cuttings(n, D):
    res = [[n]]
    if n <= 97:
        res.append(SR.cut_every(n, 1))
    res += [SR.cut_every(n, s) for s in (D - 1, D, D + 1, TILE - 1, TILE, TILE + 1)]
    res += [SR.cut_random(n, 7 * n + j) for j in range(3)]
    res.append(SR.cut_every(n, 700) + [0])         # a flush carried by an empty push
    return res


def test_the_default_lookaheads_average_ones_to_one():
    for rate in (8000, 16000, 22050, 24000, 32000, 44100, 48000):
        L = np.float32(LM.times(rate)[0])
        assert L * (np.float32(1) / L) == np.float32(1)


@pytest.mark.parametrize("rate", sorted(RATES))
def test_whole_stream_equals_the_clip_twins_gain(rate):
    L, Rel = LM.times(rate)
    assert _limiter(rate).delay == L + 5 == SR.delay(L)
    limited = 0
    for n in RATES[rate]:
        for k in R.KINDS:
            if k == "nan":
                continue
            x = R.grid_signal(k, n, rate)
            y, rec = _whole(k, n, rate)
            crec, g = _clip(k, n, rate)
            what = (rate, n, k, rec, crec)
            assert rec.lookahead == L and rec.release == Rel and rec.total == n and rec.emitted == n and not rec.nonfinite
            assert rec.limited == rec.limited_ever == crec.limited, what
            if crec.limited:
                limited += 1
                assert y.tobytes() == np.float32(g * x).tobytes(), what
                assert rec.min_gain == g.min() and rec.min_gain < 1, what
            else:
                assert y.tobytes() == x.tobytes() and rec.min_gain == 1, what
            assert rec.peak_in == rec.peak_run == crec.true_peak_in, what
    assert limited >= len(RATES[rate])


@pytest.mark.parametrize("rate", sorted(RATES))
def test_chunk_invariance(rate):
    lm = _limiter(rate)
    D = lm.delay
    for n in RATES[rate]:
        for k in R.KINDS:
            x = R.grid_signal(k, n, rate)
            want, wrec = _whole(k, n, rate)
            for cuts in cuttings(n, D):
                y, counts, recs = run(lm, x, cuts)
                what = (rate, n, k, cuts[:8])
                assert counts == SR.counts(cuts, lm.lookahead), what
                assert y.tobytes() == want.tobytes(), what
                assert [r.emitted for r in recs] == counts and [r.total for r in recs] == list(np.cumsum(counts)), what
                assert any(r.nonfinite for r in recs) == (k == "nan" and n > 0) == wrec.nonfinite, what
                assert any(r.limited for r in recs) == wrec.limited == recs[-1].limited_ever, what
                assert max(r.peak_in for r in recs) == wrec.peak_in == recs[-1].peak_run, what
                assert min(r.min_gain for r in recs) == wrec.min_gain, what
                runs = [r.peak_run for r in recs]
                assert runs == sorted(runs) and all(r.peak_run >= r.peak_in for r in recs), what


@pytest.mark.parametrize("rate", sorted(RATES))
def test_twin_against_the_fp64_restatement(rate):
    L, Rel = LM.times(rate)
    worst, worst_at, over = 0.0, None, {}
    for n in RATES[rate]:
        for k in R.KINDS:
            if k == "nan" or n == 0:
                continue
            x = R.grid_signal(k, n, rate)
            y, rec = _whole(k, n, rate)
            ref = _oracle(k, n, rate)
            bound = output_bound(_peak(x), ref.T, L, Rel)
            d = float(np.abs(y - ref.y).max())
            if d > worst:
                worst, worst_at = d, (n, k)
            over[k] = max(over.get(k, 0.0), ref.overshoot)
            assert d <= bound, (rate, n, k, d, bound)
            assert abs(float(rec.peak_in) - ref.true_peak_in) <= 14 * EPS * S * _peak(x)
    print("rate %d: worst |y_twin - y_ref| = %.3e at %r; overshoot true_peak(y) / T per signal: %r" % (rate, worst, worst_at, over))


@pytest.mark.parametrize("rate", sorted(RATES))
def test_the_bounds_on_the_output(rate):
    T = float(T32)
    for n in RATES[rate]:
        for k in R.KINDS:
            y, rec = _whole(k, n, rate)
            x = R.grid_signal(k, n, rate)
            if k == "nan":      # the samples whose envelope the NaN reaches are copied; the rest obey the bound
                ok = np.isfinite(y)
                far = np.ones(n, bool)
                if n:
                    far[max(0, n // 3 - 6): n // 3 + 7] = False
                assert np.array_equal(y[~far], x[~far], equal_nan=True) and np.all(np.abs(y[far & ok]) <= T32 * np.float32(1 + 2.0 ** -22))
                continue
            assert np.all(np.abs(y) <= T32 * np.float32(1 + 2.0 ** -22)), (rate, n, k)
            assert np.all(np.abs(y) <= np.abs(x)), (rate, n, k)
            tp = R.true_peak(y)
            assert tp <= max(T, _oracle(k, n, rate).true_peak_y) + 14 * EPS * S * T, (rate, n, k, tp)


def test_a_flushed_state_is_a_fresh_state():
    rate = 32000
    x = R.grid_signal("noise", 2 * TILE + 47, rate)
    fresh = LM.StreamLimiter(CEILING, rate, "cpu")
    a, ca, ra = run(fresh, x, SR.cut_every(len(x), 333))
    used = LM.StreamLimiter(CEILING, rate, "cpu")
    run(used, R.grid_signal("click_tile", TILE + 1, rate), SR.cut_every(TILE + 1, 100))
    run(used, R.grid_signal("quiet", 97, rate), [97, 0])
    b, cb, rb = run(used, x, SR.cut_every(len(x), 333))
    assert a.tobytes() == b.tobytes() and ca == cb
    for p, q in zip(ra, rb):
        assert all(getattr(p, f) == getattr(q, f) for f in LM.StreamLimiterRecord.__slots__)
    # the quiet stream behind the click came back to its bits: the click's release did not reach over the flush
    y, _, recs = run(used, R.grid_signal("quiet", 97, rate), [50, 47])
    assert y.tobytes() == R.grid_signal("quiet", 97, rate).tobytes() and not recs[-1].limited_ever
    # limit_stream is one flushed push; other times give another gain; long input goes in as several pushes
    y1, r1 = LM.limit_stream(x, rate, CEILING, device="cpu")
    assert y1.tobytes() == a.tobytes() and r1.total == len(x) and r1.limited
    y2, r2 = LM.limit_stream(x, rate, CEILING, lookahead_ms=0.0, release_ms=5.0, device="cpu")
    assert (r2.lookahead, r2.release) == (1, 160) and y2.tobytes() != a.tobytes()
    t = fresh.push_tensor(torch.from_numpy(x), flush=True)
    assert isinstance(t, torch.Tensor) and t.numpy().tobytes() == a.tobytes()


def test_stream_keyword_validates(tmp_path):
    from gsv_tts import TTS
    t = TTS(models_dir=str(tmp_path), device="cpu")
    ref = ("spk.wav", "prompt.wav", "prompt.")
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ceiling"):
            next(t.infer_stream(*ref, "text.", true_peak=bad))
        with pytest.raises(ValueError, match="ceiling"):
            next(t.infer_stream_batched(*ref, ["one.", "two."], true_peak=[-1.0, bad]))
    with pytest.raises(ValueError, match="true_peak has 3 entries for 2 requests"):
        next(t.infer_stream_batched(*ref, ["one.", "two."], true_peak=[-1.0, None, -1.0]))


def test_argument_checks():
    L = N.lib()
    need = L.gsv_limstream_state_bytes(48, 1600)
    assert need > 0 and need % 16 == 0
    for bad in ((0, 1600), (4097, 1600), (48, 0), (48, (1 << 24) + 1)):
        assert L.gsv_limstream_state_bytes(*bad) == 0
    assert L.gsv_limstream_out_capacity(1000, 48) == 1053 and L.gsv_limstream_out_capacity(-1, 48) == 0
    assert L.gsv_limstream_out_capacity(10, 0) == 0
    state = torch.zeros(need + 16, dtype=torch.uint8)
    sp = state.data_ptr()
    assert sp % 16 == 0
    err = lambda: L.gsv_last_error().decode()
    assert L.gsv_limstream_init_host(None, need, -1.0, 48, 1600) == 1 and "null" in err()
    assert L.gsv_limstream_init_host(sp, need - 1, -1.0, 48, 1600) == 1 and "state" in err()
    assert L.gsv_limstream_init_host(sp + 4, need, -1.0, 48, 1600) == 1 and "aligned" in err()
    for c in (0.5, -201.0, float("nan"), float("inf")):
        assert L.gsv_limstream_init_host(sp, need, c, 48, 1600) == 1 and "ceiling" in err()
    assert L.gsv_limstream_init_host(sp, need, -1.0, 0, 1600) == 1 and "look-ahead" in err()
    x, out = torch.zeros(100), torch.zeros(153)
    rec = torch.zeros(4, dtype=torch.int64)
    ok = [sp, x.data_ptr(), 100, None, 0, out.data_ptr(), rec.data_ptr()]
    assert L.gsv_limstream_push_host(*ok) == 1 and "not a state" in err()       # zeros: no state yet
    assert L.gsv_limstream_init_host(sp, need, -1.0, 48, 1600) == 0
    assert L.gsv_limstream_push_host(*ok) == 0
    for i, bad, word in [(0, None, "null"), (1, None, "null"), (5, None, "null"), (6, None, "null"), (2, -1, "chunk of -1"),
                         (2, (1 << 20) + 1, "chunk of"), (5, x.data_ptr(), "out is the chunk"), (0, sp + 4, "aligned"),
                         (6, rec.data_ptr() + 4, "aligned")]:
        args = list(ok)
        args[i] = bad
        assert L.gsv_limstream_push_host(*args) == 1 and word in err(), (i, bad, err())
    n_host = torch.tensor([40], dtype=torch.int32)      # a held length smaller than n_cap is honoured, and clamped
    lm = LM.StreamLimiter(CEILING, 32000, "cpu")
    sig = torch.from_numpy(R.grid_signal("sine997", 100, 32000))
    o = torch.zeros(153)
    for held, n in ((40, 40), (-3, 0), (500, 100)):
        n_host[0] = held
        assert L.gsv_limstream_push_host(lm.state.data_ptr(), sig.data_ptr(), 100, n_host.data_ptr(), 1, o.data_ptr(), rec.data_ptr()) == 0
        r = LM.stream_record(rec.view(torch.uint8))
        assert r.emitted == n and o[:n].numpy().tobytes() == LM.limit_stream(sig[:n], 32000, CEILING, device="cpu")[0].tobytes()
    for bad in (0.5, float("nan"), None):
        with pytest.raises(ValueError):
            LM.StreamLimiter(bad, 32000, "cpu")
    with pytest.raises(ValueError):
        LM.StreamLimiter(-1.0, 32000, "cpu", lookahead_ms=1000.0)
