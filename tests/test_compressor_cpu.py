"""CPU checks of the compressor (csrc/compressor.h behind gsv_compressor_host, compressor.py): the host twin against the serial fp64
definition tests/compressor_ref.py over rates, parameter sets, lengths and signals, the accuracy of the two routines, clips under
the threshold, the fall of the detector through the denormals, packed lists, in place, guards, non-finite and empty clips, the C
entry's checks, the identity, the static curve, AudioClip.  No GPU: the host twin is built from the scalar routines the device
kernels share, and tests/test_hip_compressor.py pins the device to it bit for bit.

Bounds, derived and not measured:

  twin    Every sample of the twin within ONE fp32 ulp of the oracle's fp32 result.  Both evaluate the definition in fp64; the
          twin's scans differ from the serial recurrences by a few 2^-53 relative per combine, which the contractions aR, aA < 1
          damp, and its log2 / exp2 are good to 2^-40 (below), so M g x is off by far less than half an fp32 ulp before the one
          rounding: the two fp32 results differ only where the fp64 value sits next to a rounding boundary, and then by one ulp.
  log2,   Relative error at most 2^-40 against libm in fp64 (numpy's log2 / exp2): a dense sweep of log2 over [1, 2) and over
  exp2    [2^-30, 2^30] by decades, of exp2 over [-64, 0].  2^-40 is far below the 2^-24 of the final rounding.
  settle  A full-scale square wave's p and e settle to the amplitude exactly (|x| is constant), so the gain settles to the static
          curve's: 1e-6 relative, which holds the two routines and the curve's formula against each other."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compressor_ref as R  # noqa: E402
import compressor_cases as C  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import compressor as CM  # noqa: E402
from gsv_tts_lite_amd.compressor import Compressor  # noqa: E402

CPU = torch.device("cpu")
ULPS = 1
ROUTINE_REL = 2.0 ** -40
NAMES = list(R.SETS)


def _params(rate):
    return [np.array(R.coefficients(R.SETS[n], rate), np.float64) for n in NAMES]


# ---------------------------------------------------------------------------------------------------------------- module
def test_constants_and_coefficients_are_the_definition():
    assert (CM.RUN, CM.SPAN, CM.CHUNK) == (R.RUN, R.SPAN, R.CHUNK) and CM.RECORD_BYTES == C.REC
    for rate in R.RATES:
        for name, p in R.SETS.items():
            assert Compressor(*p).coefficients(rate).tolist() == list(R.coefficients(p, rate)), (rate, name)
    v = Compressor.preset("voice")
    assert (v.threshold_db, v.ratio, v.attack_ms, v.release_ms, v.makeup_db) == R.SETS["voice"] and CM.PRESETS == ("voice",)
    assert Compressor(ratio=math.inf).coefficients(32000)[3] == -1.0
    # the extremes of the documented ranges keep both coefficients inside (0, 1)
    for rate in (4000, 768000):
        for ms in (CM.MIN_MS, CM.MAX_MS):
            a_a, a_r = Compressor(attack_ms=ms, release_ms=ms).coefficients(rate)[:2]
            assert 0.0 < a_a < 1.0 and 0.0 < a_r < 1.0


def test_out_of_range_fields_raise():
    x = np.zeros(4, np.float32)
    for bad in (lambda: Compressor(threshold_db=0.5), lambda: Compressor(threshold_db=-80.5), lambda: Compressor(threshold_db=float("nan")),
                lambda: Compressor(ratio=0.99), lambda: Compressor(ratio=float("nan")), lambda: Compressor(attack_ms=0.0),
                lambda: Compressor(attack_ms=0.009), lambda: Compressor(release_ms=10001.0), lambda: Compressor(release_ms=float("inf")),
                lambda: Compressor(makeup_db=40.5), lambda: Compressor(makeup_db=float("nan")), lambda: Compressor(threshold_db="loud"),
                lambda: Compressor.preset("radio"), lambda: CM.resolve(3.0), lambda: CM.resolve([Compressor()]),
                lambda: CM.compress(x, 100, "voice"), lambda: CM.compress(x, 900000, "voice"), lambda: CM.compress([x, x], 32000, ["voice"]),
                lambda: CM.compress(x, 32000, -18.0), lambda: CM.curve(3.0, [0.0]), lambda: Compressor().coefficients(3999)):
        with pytest.raises(ValueError):
            bad()
    assert CM.resolve(None) is None and CM.resolve(Compressor(ratio=1.0)) is None and CM.resolve("voice").ratio == 3.5
    assert CM.resolve(Compressor(ratio=1.0, makeup_db=1.0)) is not None
    Compressor(-80.0, math.inf, 0.01, 10000.0, -40.0), Compressor(0.0, 1.0, 10000.0, 0.01, 40.0)


# ------------------------------------------------------------------------------------------------------------- routines
def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def test_log2_and_exp2_against_libm():
    dense = 1.0 + (np.arange(1, 1 << 20, dtype=np.float64) / (1 << 20))                   # (1, 2): log2(1) = 0 is checked apart
    worst = [("log2 (1, 2)", _rel(CM.routine("log2", dense), np.log2(dense)))]
    near = 1.0 + np.ldexp(1.0, -np.arange(1, 53, dtype=np.int32))                         # next to 1, where the result is tiny
    worst.append(("log2 next to 1", _rel(CM.routine("log2", near), np.log2(near))))
    assert CM.routine("log2", [1.0, 2.0, 0.5, 1024.0, 2.0 ** -30]).tolist() == [0.0, 1.0, -1.0, 10.0, -30.0]
    rng = np.random.default_rng(3)
    for k in range(-30, 30):                                                              # [2^-30, 2^30], decade by decade
        v = np.ldexp(1.0 + rng.uniform(0.0, 1.0, 20000), k)
        v = v[np.abs(np.log2(v)) > 0]
        worst.append(("log2 2^%d" % k, _rel(CM.routine("log2", v), np.log2(v))))
    t = -64.0 * np.arange(0, (1 << 20) + 1, dtype=np.float64) / (1 << 20)
    worst.append(("exp2 [-64, 0]", _rel(CM.routine("exp2", t), np.exp2(t))))
    t = rng.uniform(-64.0, 0.0, 200000)
    worst.append(("exp2 random", _rel(CM.routine("exp2", t), np.exp2(t))))
    assert CM.routine("exp2", [0.0, -1.0, -64.0, 3.0]).tolist() == [1.0, 0.5, 2.0 ** -64, 8.0]
    name, w = max(worst, key=lambda p: p[1])
    print("log2 / exp2 against libm: worst relative error %.3g (%s), 2^-40 = %.3g" % (w, name, ROUTINE_REL))
    for name, w in worst:
        assert w <= ROUTINE_REL, (name, w)
    assert CM.routine("exp2", [float("nan"), -5000.0, 5000.0]).tolist() == [2.0 ** -1000, 2.0 ** -1000, 2.0 ** 1000]   # clamped, never wild


# ------------------------------------------------------------------------------------------------- the twin and the oracle
def _grid_call(rate, device=CPU, mode="out"):
    g = R.grid(rate)
    clips = [x for _, _, _, x in g]
    x, offsets = C.pack(clips)
    out, rec, _ = C.call(x, offsets, [len(c) for c in clips], [NAMES.index(name) for name, _, _, _ in g], _params(rate), device, mode)
    return g, offsets, out, rec


@pytest.mark.parametrize("rate", R.RATES)
def test_twin_against_the_fp64_oracle(rate):
    g, offsets, out, rec = _grid_call(rate)
    want = R.grid_expected(rate)
    recs = C.recs_of(rec)
    worst = differ = total = 0
    acted = set()
    for (name, n, kind, x), o, (e, gain), r in zip(g, offsets, want, recs):
        y = out[o: o + n]
        cell = (rate, name, n, kind)
        assert np.all(np.isfinite(y)), cell
        u = R.ulps(y, e)
        worst, differ, total = max(worst, int(u.max())), differ + int((u > 0).sum()), total + n
        assert u.max() <= ULPS, cell
        assert not r.nonfinite and r.peak_in == np.abs(x).max() and r.peak_out == np.abs(y).max(), cell
        assert r.min_gain == np.float32(gain.min()) or abs(float(r.min_gain) / gain.min() - 1.0) < 2.0 ** -23, cell
        assert r.compressed == bool(r.min_gain < 1), cell
        if r.compressed:
            acted.add((name, kind))
        if kind == "quiet":
            assert not r.compressed and r.min_gain == 1 and gain.max() == 1.0, cell
    print("twin vs oracle at %d Hz: worst %d ulps, %d of %d samples differ" % (rate, worst, differ, total))
    for name in NAMES:                      # the loud signals do pass every set's threshold
        assert {(name, k) for k in ("noise", "gated220", "square")} <= acted, name


def test_a_clip_under_its_threshold_comes_back_bit_for_bit():
    rate = 32000
    for name in ("voice", "fast", "inf"):                   # 0 dB of makeup: 1 x is exact
        x = R.grid_signal("quiet", R.CHUNK + 1, rate, name)
        co = np.array(R.coefficients(R.SETS[name], rate))
        out, rec, _ = C.call(x, [0], [len(x)], [0], [co], CPU)
        r = C.recs_of(rec)[0]
        assert out.tobytes() == x.tobytes() and not r.compressed and not r.nonfinite and r.min_gain == 1
        assert r.peak_in.tobytes() == r.peak_out.tobytes() == np.abs(x).max().tobytes()
    x = R.grid_signal("quiet", 3000, rate, "slow").copy()   # +3 dB of makeup: the gain is the makeup alone
    y, r = CM.compress(x, rate, Compressor(*R.SETS["slow"]), device="cpu")
    assert not r.compressed and r.min_gain == 1 and y.tobytes() == R.to_f32(10.0 ** (3.0 / 20.0) * x.astype(np.float64)).tobytes()


def test_the_detector_falls_through_the_denormals_to_zero():
    x, co = R.denormal_clip()
    e = np.array(R.detector(x, co))
    tiny = np.finfo(np.float64).tiny
    assert ((e > 0) & (e < tiny)).sum() > 20 and e[-1] == 0.0 and e.max() > co[2], "the clip does not do what it is for"
    want, gain = R.compress(x, co)
    out, rec, _ = C.call(x, [0], [len(x)], [0], [np.array(co)], CPU)
    assert R.ulps(out, want).max() <= ULPS and np.all(np.isfinite(out))
    settled = int(np.nonzero(e > co[2])[0].max()) + 1                       # from here on e <= T
    assert 0 < settled < len(x) and out[settled:].tobytes() == x[settled:].tobytes()
    r = C.recs_of(rec)[0]
    assert r.compressed and abs(float(r.min_gain) / gain.min() - 1.0) < 2.0 ** -23
    # the same clip with a tail that is not zero: exact input bits once e <= T
    x2 = x.copy()
    x2[2000:] = np.float32(1e-30) * np.where(np.arange(len(x) - 2000) % 2 == 0, 1.0, -1.0).astype(np.float32)
    out2, _, _ = C.call(x2, [0], [len(x2)], [0], [np.array(co)], CPU)
    assert out2[2000:].tobytes() == x2[2000:].tobytes() and R.ulps(out2, R.compress(x2, co)[0]).max() <= ULPS


# -------------------------------------------------------------------------------------------------------- other properties
def _mixed(rate=32000):
    """nine clips over three parameter sets, some of them copied: (clips, index, params)"""
    rng = np.random.default_rng(11)
    noise = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    clips = [noise(R.CHUNK + 1), noise(777), np.zeros(0, np.float32), noise(R.SPAN), R.grid_signal("gated220", 3 * R.SPAN + 5, rate, "voice"),
             noise(R.RUN), noise(2 * R.CHUNK), noise(1), noise(R.SPAN - 1)]
    index = [0, 1, 2, 2, 1, 0, -1, 1, 2]
    return clips, index, _params(rate)[:3]


def test_packed_clips_equal_single_calls_in_place_too_and_nothing_else_moves():
    clips, index, params = _mixed()
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    out, rec, x_after = C.call(x, offsets, lengths, index, params, CPU)
    assert x_after.tobytes() == x.tobytes()
    mask = np.zeros(len(x), bool)
    for i, (c, o, d) in enumerate(zip(clips, offsets, index)):
        mask[o: o + len(c)] = True
        one, rec1, _ = C.call(c, [0], [len(c)], [0 if d >= 0 else -1], [params[max(d, 0)]], CPU)
        assert out[o: o + len(c)].tobytes() == one.tobytes() and rec[16 * i: 16 * i + 16] == rec1, i
    assert np.all(out[~mask] == C.FILL * 2), "written outside a clip"
    got_in, rec_in, _ = C.call(x, offsets, lengths, index, params, CPU, "inplace")
    assert rec_in == rec and got_in[mask].tobytes() == out[mask].tobytes() and np.all(got_in[~mask] == C.FILL)
    recs = C.recs_of(rec)
    assert [r.compressed for r in recs] == [True, True, False, True, True, True, False, True, True]
    o = offsets[6]
    assert out[o: o + lengths[6]].tobytes() == clips[6].tobytes() and recs[6].peak_in == recs[6].peak_out == np.abs(clips[6]).max()
    assert recs[6].min_gain == 1 and recs[2].peak_in == recs[2].peak_out == 0 and recs[2].min_gain == 1


def test_nonfinite_and_empty_clips_come_back_bit_for_bit():
    rate = 32000
    co = _params(rate)[0]
    rng = np.random.default_rng(5)
    nan = rng.uniform(-1, 1, R.CHUNK + 100).astype(np.float32)
    nan[R.SPAN + 3] = np.nan
    inf = rng.uniform(-1, 1, 3000).astype(np.float32)
    inf[2999] = -np.inf
    both = nan.copy()
    both[5] = np.inf
    good = rng.uniform(-1, 1, 5000).astype(np.float32)
    clips = [good, nan, np.zeros(0, np.float32), inf, good, both]
    x, offsets = C.pack(clips)
    want = R.compress(good, R.coefficients(R.SETS["voice"], rate))[0]
    for mode in ("out", "inplace"):
        out, rec, _ = C.call(x, offsets, [len(c) for c in clips], [0] * len(clips), [co], CPU, mode)
        recs = C.recs_of(rec)
        for c, o, r, bad in zip(clips, offsets, recs, (False, True, False, True, False, True)):
            y = out[o: o + len(c)]
            assert (r.nonfinite, r.compressed) == ((True, False) if bad else (False, len(c) > 0))
            if bad:
                assert y.tobytes() == c.tobytes() and r.peak_in.tobytes() == r.peak_out.tobytes() and not np.isfinite(r.peak_in) and r.min_gain == 1
        assert np.isnan(recs[1].peak_in) and np.isinf(recs[3].peak_in) and np.isnan(recs[5].peak_in)
        assert recs[2].peak_in == recs[2].peak_out == 0 and recs[2].min_gain == 1
        for o in (offsets[0], offsets[4]):                              # the neighbours are what they are alone
            assert R.ulps(out[o: o + 5000], want).max() <= ULPS


def test_the_c_entry_rejects_bad_tables():
    x = np.zeros(64, np.float32)
    good = np.array(R.coefficients(R.SETS["voice"], 32000))

    def rc(params, index=(0,), lengths=(64,), offsets=(0,)):
        L = N.lib()
        clips, tab = CM._tables(offsets, lengths, index, params)
        need = L.gsv_compressor_work_bytes(clips, len(lengths), tab, len(params)) or 1 << 16
        xt, out = torch.from_numpy(x.copy()), torch.zeros(64)
        work, rec = torch.zeros(need, dtype=torch.uint8), torch.zeros(16 * len(lengths), dtype=torch.uint8)
        return L.gsv_compressor_host(xt.data_ptr(), 64, clips, len(lengths), tab, len(params), out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)

    assert rc([good]) == 0
    for j, values in enumerate(((0.0, 1.0, -0.1, 1.5), (0.0, 1.0, -0.1, 1.5), (0.0, -1.0, 1e-320), (-1.0001, 0.1), (0.0, -2.0))):
        for v in values + (float("nan"), float("inf")):
            bad = good.copy()
            bad[j] = v
            assert rc([bad]) == 1, (j, v)
    edge = good.copy()
    edge[3] = -1.0                                                      # ratio inf
    assert rc([edge]) == 0 and rc([good, edge], index=(1,)) == 0
    assert rc([good], index=(1,)) == 1 and rc([good], index=(-2,)) == 1 and rc([good], lengths=(65,)) == 1 and rc([good], offsets=(1,)) == 1
    assert rc([], index=(-1,)) == 0                                     # measure only needs no parameter set
    L = N.lib()
    clips, tab = CM._tables([0], [64], [0], [good])
    w = torch.zeros(1 << 16, dtype=torch.uint8)
    need = L.gsv_compressor_work_bytes(clips, 1, tab, 1)
    xt, out, rec = torch.from_numpy(x), torch.zeros(64), torch.zeros(16, dtype=torch.uint8)          # alive over the calls below
    args = (xt.data_ptr(), 64, clips, 1, tab, 1, out.data_ptr(), rec.data_ptr())
    assert 0 < need < 1 << 16 and L.gsv_compressor_host(*args, w.data_ptr(), need - 1) == 1 and L.gsv_compressor_host(*args, w.data_ptr() + 8, need) == 1
    assert L.gsv_compressor_host(*args, w.data_ptr(), need) == 0
    assert L.gsv_compressor_work_bytes(clips, 0, tab, 1) == 0 and L.gsv_compressor_work_bytes(clips, 1, None, 1) == 0
    with pytest.raises(RuntimeError, match="parameter set 0"):
        CM.run_packed(torch.from_numpy(x.copy()), [0], [64], [0], [np.array([0.5, 0.5, 0.1, 0.5, 1.0])], torch.zeros(64))
    with pytest.raises(ValueError):
        CM.run_packed(torch.from_numpy(x.copy()), [0], [64], [0], [np.zeros(4)], torch.zeros(64))


def test_the_identity_returns_the_input_and_issues_no_call(monkeypatch):
    x = np.random.default_rng(3).uniform(-1, 1, 1000).astype(np.float32)
    monkeypatch.setattr(CM, "run_packed", lambda *a, **k: pytest.fail("a call was issued"))
    for c in (Compressor(ratio=1.0), Compressor(-40.0, 1.0, 5.0, 50.0, 0.0), None):
        y, rec = CM.compress(x, 32000, c, device="cpu")
        assert y is not x and y.tobytes() == x.tobytes() and not rec.compressed and rec.min_gain == 1
        assert rec.peak_in == rec.peak_out == np.abs(x).max()
    ys, recs = CM.compress([x, x[:10]], 32000, [Compressor(ratio=1.0), None])
    assert ys[1].tobytes() == x[:10].tobytes() and len(recs) == 2
    t = torch.from_numpy(x)
    y, rec = CM.compress(t, 32000, Compressor(ratio=1.0))
    assert isinstance(y, torch.Tensor) and y.data_ptr() != t.data_ptr() and torch.equal(y, t)
    assert CM.compress([], 32000, "voice") == ([], [])
    bad = x.copy()
    bad[7] = np.nan
    assert CM.compress(bad, 32000, None)[1].nonfinite


def test_module_lists_share_parameter_sets_and_keep_types():
    rate = 32000
    a, b, c = (np.random.default_rng(s).uniform(-1, 1, n).astype(np.float32) for s, n in ((1, 5000), (2, R.SPAN + 9), (3, 300)))
    c2 = Compressor(*R.SETS["fast"])
    ys, recs = CM.compress([a, b.reshape(1, -1), torch.from_numpy(c), a], rate, ["voice", c2, None, Compressor.preset("voice")], device="cpu")
    assert isinstance(ys[0], np.ndarray) and ys[1].shape == (1, R.SPAN + 9) and isinstance(ys[2], torch.Tensor)
    assert ys[0].tobytes() == ys[3].tobytes() and [r.compressed for r in recs] == [True, True, False, True]
    assert ys[2].numpy().tobytes() == c.tobytes()
    y0, r0 = CM.compress(a, rate, "voice", device="cpu")
    assert y0.tobytes() == ys[0].tobytes() and r0.peak_out == recs[0].peak_out == np.abs(y0).max() and r0.min_gain == recs[0].min_gain
    assert R.ulps(ys[1].reshape(-1), R.compress(b, R.coefficients(R.SETS["fast"], rate))[0]).max() <= ULPS


# ------------------------------------------------------------------------------------------------------------- the curve
def test_the_static_curve_and_a_square_wave_that_settles_to_it():
    for name, p in R.SETS.items():
        c = Compressor(*p)
        thr, ratio, mk = p[0], p[1], p[4]
        below = np.array([-90.0, thr - 20.0, thr - 1e-9, thr])
        assert np.array_equal(CM.curve(c, below), below + mk), name                   # the diagonal
        above = thr + np.array([0.0, 1.0, 6.0, 40.0])
        got = CM.curve(c, above)
        assert np.allclose(np.diff(got) / np.diff(above), 1.0 / ratio, rtol=0, atol=1e-12), name
        assert got[0] == thr + mk and CM.curve(name if name == "voice" else c, 0.0).shape == ()
    v = CM.curve("voice", [[-18.0, 0.0]])
    assert v.shape == (1, 2) and v[0, 0] == -18.0 and v[0, 1] == pytest.approx(-18.0 + 18.0 / 3.5, abs=1e-12)
    # 2 s of a full-scale square wave: |x| = 1 throughout, so p = 1 from the first sample and e -> 1; the gain settles to the curve's
    rate = 32000
    x = np.where((np.arange(2 * rate) // 50) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for name in ("voice", "fast", "slow", "inf"):
        c = Compressor(*R.SETS[name])
        y, rec = CM.compress(x, rate, c, device="cpu")
        want = 10.0 ** (float(CM.curve(c, 0.0)) / 20.0)                             # the output level of a 0 dB input
        tail = np.abs(y[-rate // 2:].astype(np.float64))
        assert np.max(np.abs(tail / want - 1.0)) < 1e-6, (name, tail.max(), want)
        g = want / 10.0 ** (c.makeup_db / 20.0)
        assert rec.compressed and abs(float(rec.min_gain) / g - 1.0) < 1e-6, name


# ------------------------------------------------------------------------------------------------------------- AudioClip
def test_audioclip_compressed_carries_the_record():
    from gsv_tts_lite_amd.tts import AudioClip
    rate = 32000
    x = (0.5 * np.random.default_rng(9).uniform(-1, 1, rate)).astype(np.float32)
    subs = [{"text": "a", "start_s": 0.0, "end_s": 0.5}]
    clip = AudioClip(None, x, rate, 1.0, subs, "a")
    assert clip.comp is None
    out = clip.compressed("voice")
    want, rec = CM.compress(x, rate, Compressor.preset("voice"))
    assert out is not clip and out.audio_data.tobytes() == want.tobytes() and clip.audio_data.tobytes() == x.tobytes()
    assert out.subtitles is subs and out.orig_text == "a" and out.audio_len_s == 1.0 and out.samplerate == rate
    assert out.comp.compressed and out.comp.min_gain == rec.min_gain < 1 and out.comp.peak_out == np.abs(out.audio_data).max() == rec.peak_out
    assert out.comp.peak_in == np.abs(x).max()
    chain = clip.equalised("voice").compressed(Compressor(-30.0, 4.0)).normalised(-20.0, peak_limit=math.inf).limited_to(-1.0)
    assert chain.eq is not None and chain.comp is not None and chain.comp.compressed and chain.lufs is not None and chain.dbtp is not None
    assert clip.compressed().equalised("voice").comp is not None
    same = clip.compressed(Compressor(ratio=1.0))
    assert same.audio_data.tobytes() == x.tobytes() and not same.comp.compressed
    for bad in ([Compressor()], None, "radio", -18.0):
        with pytest.raises(ValueError):
            clip.compressed(bad)
