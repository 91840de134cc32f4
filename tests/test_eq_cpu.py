"""CPU checks of the equaliser (csrc/eq.h behind gsv_eq_host, eq.py): the designs against the cookbook written out here, the host
twin against the fp64 restatement tests/eq_ref.py over rates, section counts, lengths and signals, packed lists, in place, guards,
non-finite and empty clips, saturation, the identity, AudioClip.  No GPU: the host twin is built from the scalar routines the
device kernels share, and tests/test_hip_eq.py pins the device to it bit for bit.

Bounds, all measured against the fp64 oracle and written next to their margin:

  twin    The twin's fp32 samples against the oracle's fp64 rounded to fp32, over the whole grid (eq_ref: 4 rates x 3 section
          counts x 12 lengths x 5 signals, 3.4 M samples).  Two fp64 evaluations of one cascade differ by an ABSOLUTE amount (about
          1e-11 of the clip's peak here: the oracle against its own restatement as a loop 2e-12, the twin against the serial
          cascade 5e-11 in tools/eq_host_check.cpp), so (a) a sample within 2^-8 of the clip's peak flips its fp32 rounding only when
          the fp64 value sits that close to a rounding boundary, and is then 1 ulp off; (b) a sample far below the peak -- a zero
          crossing, the tail of an impulse response -- can be several of ITS ulps off without either side being wrong.
          Measured: (a) worst 1 ulp; (b) worst 55 ulps (the "voice" preset at 192 kHz, an impulse's tail); samples that differ at
          all: 4.5e-4 of the grid.  Bounds: (a) 2 ulps, (b) 110 ulps, share 1.8e-3 -- 2x, 2x and 4x, since all three are rounding
          coincidences.
  fft     eq.response against numpy's rfft of the oracle's impulse response, 65 536 samples at 32 kHz (the response has decayed
          below 1e-100 by then): worst |difference| 2.6e-14 for one section, 6.8e-13 for "voice", 2.3e-11 for the six sections
          (|H| up to 2.3).  Bound 1e-10: 4x the worst."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_ref as R  # noqa: E402
import eq_cases as C  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402
from gsv_tts_lite_amd.eq import EQ, Band  # noqa: E402

CPU = torch.device("cpu")
NEAR_ULPS, FAR_ULPS, SHARE = 2, 110, 1.8e-3         # measured 1, 55, 4.5e-4 (the docstring)
FFT_TOL = 1e-10                                     # measured 2.3e-11


def _eq(bands):
    return EQ([Band(k, f, q=q, gain_db=g) for k, f, q, g in bands])


def _within_bounds(y, e):
    """the twin's bounds of the docstring for one clip"""
    u = R.ulps(y, e)
    high = np.abs(e) >= np.abs(e).max() / 256
    return u[high].max() <= NEAR_ULPS and u.max() <= FAR_ULPS


# ---------------------------------------------------------------------------------------------------------------- designs
def test_voice_preset_is_the_cookbook_written_out():
    rate = 32000
    got = EQM.design(EQ.preset("voice", rate), rate)
    assert got.dtype == np.float64 and got.shape == (3, 5)
    # high pass 80 Hz, Q = 1 / sqrt 2
    w0 = 2 * math.pi * 80.0 / rate
    al, c = math.sin(w0) / (2 * (1 / math.sqrt(2))), math.cos(w0)
    a0 = 1 + al
    want = [[(1 + c) / 2 / a0, -(1 + c) / a0, (1 + c) / 2 / a0, -2 * c / a0, (1 - al) / a0]]
    for f0, q, g in ((300.0, 1.0, 2.5), (7000.0, 2.0, -3.0)):
        A = 10.0 ** (g / 40.0)
        w0 = 2 * math.pi * f0 / rate
        al, c = math.sin(w0) / (2 * q), math.cos(w0)
        a0 = 1 + al / A
        want.append([(1 + al * A) / a0, -2 * c / a0, (1 - al * A) / a0, -2 * c / a0, (1 - al / A) / a0])
    assert got.tolist() == want
    assert EQM.design(EQ.preset("voice", 8000), 8000).tolist()[2] == list(R.section("peak", 3600.0, 2.0, -3.0, 8000))   # clamped
    for count in R.COUNTS:
        for rate in R.RATES:
            assert EQM.design(_eq(R.bands_for(count, rate)), rate).tolist() == [list(s) for s in R.coefficients(R.bands_for(count, rate), rate)]


def test_response_at_the_design_points():
    db = lambda h: 20.0 * math.log10(abs(h))
    for rate in (8000, 32000, 192000):
        for f0, q, g in ((300.0, 1.0, 2.5), (1000.0, 4.0, -12.0), (0.4 * rate, 0.3, 40.0)):
            assert abs(db(EQM.response(EQ([Band("peak", f0, q=q, gain_db=g)]), rate, f0)) - g) < 1e-12
        for f0 in (80.0, 1000.0):
            assert abs(db(EQM.response(EQ([Band("highpass", f0)]), rate, f0)) - 10.0 * math.log10(0.5)) < 1e-9
            assert abs(db(EQM.response(EQ([Band("lowpass", f0)]), rate, f0)) + 3.0103) < 1e-5
    h = EQM.response(EQ.preset("voice", 32000), 32000, [[10.0, 300.0], [7000.0, 15000.0]])
    assert h.shape == (2, 2) and h.dtype == np.complex128 and abs(h[0, 0]) < 0.03 and abs(abs(h[1, 1]) - 1) < 0.02


@pytest.mark.parametrize("count", R.COUNTS)
def test_response_is_the_fft_of_the_oracles_impulse_response(count):
    rate, n = 32000, 65536
    bands = R.bands_for(count, rate)
    imp = np.zeros(n, np.float32)
    imp[0] = 1.0
    h = R.cascade64(imp, R.coefficients(bands, rate))
    assert np.abs(h[-256:]).max() < 1e-100
    worst = float(np.abs(np.fft.rfft(h) - EQM.response(_eq(bands), rate, np.arange(n // 2 + 1) * (rate / n))).max())
    print("fft: %d sections, worst |difference| %.3g" % (count, worst))
    assert worst < FFT_TOL


# ----------------------------------------------------------------------------------------------------------------- domain
def test_out_of_range_fields_raise():
    for bad in (lambda: Band("notch", 100.0), lambda: Band("peak", 9.9), lambda: Band("peak", float("nan")), lambda: Band("peak", 100.0, q=0.09),
                lambda: Band("peak", 100.0, q=40.1), lambda: Band("peak", 100.0, gain_db=40.5), lambda: Band("lowshelf", 100.0, gain_db=-41),
                lambda: Band("peak", 100.0, gain_db=float("nan")), lambda: EQ([Band("peak", 100.0)] * 7), lambda: EQ(["voice"]),
                lambda: EQ.preset("radio", 32000), lambda: EQ.preset("voice", 3999), lambda: EQ.preset("voice", 768001),
                lambda: EQM.design(EQ([Band("peak", 3601.0, gain_db=1)]), 8000), lambda: EQM.design(EQ([]), 1000),
                lambda: EQM.response(EQ([]), 900000, [1.0]), lambda: EQM.equalise(np.zeros(4, np.float32), 32000, [Band("peak", 100.0, gain_db=1)]),
                lambda: EQM.equalise([np.zeros(4, np.float32)] * 2, 32000, ["voice"]), lambda: EQM.equalise(np.zeros(4, np.float32), 100, "voice"),
                lambda: EQM.resolve(3.0, 32000), lambda: EQM.resolve([Band("peak", 100.0)], 32000)):
        with pytest.raises(ValueError):
            bad()
    assert Band("peak", 10.0, q=0.1, gain_db=-40).coefficients(4000) and Band("highshelf", 0.45 * 768000, q=40, gain_db=40).coefficients(768000)


def test_the_c_entry_rejects_what_it_must():
    x = np.zeros(64, np.float32)
    good = np.asarray(R.coefficients(R.voice(32000), 32000))

    def rc(designs, index=(0,), lengths=(64,), offsets=(0,)):
        L = N.lib()
        clips, des = EQM._tables(offsets, lengths, index, designs)
        need = L.gsv_eq_work_bytes(clips, len(lengths), des, len(designs)) or 1 << 16
        xt, out = torch.from_numpy(x.copy()), torch.zeros(64)
        work, rec = torch.zeros(need, dtype=torch.uint8), torch.zeros(16 * len(lengths), dtype=torch.uint8)
        return L.gsv_eq_host(xt.data_ptr(), 64, clips, len(lengths), des, len(designs), out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)

    assert rc([good]) == 0
    for j in range(5):
        for v in (float("nan"), float("inf")):
            bad = good.copy()
            bad[1, j] = v
            assert rc([bad]) == 1, (j, v)
    for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (0.0, 1.5), (2.0, 1.0 - 1e-9), (-1.9, 0.9), (1.9, 0.9), (0.5, -0.6)):
        bad = good.copy()
        bad[2, 3:] = (a1, a2)
        assert rc([bad]) == 1, (a1, a2)
    edge = good.copy()
    edge[2, 3:] = (1.899999, 0.9)
    assert rc([edge]) == 0
    assert rc([good], index=(1,)) == 1 and rc([good], index=(-2,)) == 1 and rc([good], lengths=(65,)) == 1 and rc([good], offsets=(1,)) == 1
    assert rc([], index=(-1,)) == 0                                     # measure only needs no design
    L = N.lib()
    clips, des = EQM._tables([0], [64], [0], [good])
    des[0].n_sections = 7
    assert L.gsv_eq_work_bytes(clips, 1, des, 1) > 0                    # the size does not depend on the coefficients ...
    des[0].n_sections = 0
    w = torch.zeros(1 << 16, dtype=torch.uint8)
    assert L.gsv_eq_host(torch.from_numpy(x).data_ptr(), 64, clips, 1, des, 1, torch.zeros(64).data_ptr(), torch.zeros(16, dtype=torch.uint8).data_ptr(),
                         w.data_ptr(), 1 << 16) == 1                    # ... the call does
    with pytest.raises(RuntimeError, match="unit circle"):
        EQM.run_packed(torch.from_numpy(x.copy()), [0], [64], [0], [np.array([[1.0, 0, 0, 0, 1.0]])], torch.zeros(64))


# ------------------------------------------------------------------------------------------------- the twin and the oracle
def _grid_call(rate, count, device=CPU):
    g = R.grid(rate)
    clips = [x for _, _, x in g]
    x, offsets = C.pack(clips)
    co = np.asarray(R.coefficients(R.bands_for(count, rate), rate))
    out, rec, _ = C.call(x, offsets, [len(c) for c in clips], [0] * len(clips), [co], device)
    return g, offsets, out, rec


_TALLY = {}


@pytest.mark.parametrize("count", R.COUNTS)
@pytest.mark.parametrize("rate", R.RATES)
def test_twin_against_the_fp64_oracle(rate, count):
    g, offsets, out, rec = _grid_call(rate, count)
    want = R.grid_expected(rate, count)
    recs = C.recs_of(rec)
    near = far = differ = total = 0
    for (n, kind, x), o, e, r in zip(g, offsets, want, recs):
        y = out[o: o + n]
        assert r.equalised and not r.nonfinite and r.sections == count, (n, kind)
        assert r.peak_in == (np.abs(x).max() if n else 0) and r.peak_out == (np.abs(y).max() if n else 0), (n, kind)
        if not n:
            continue
        assert np.all(np.isfinite(y))
        if kind == "zeros":
            assert not y.any() and not e.any()
        u = R.ulps(y, e)
        high = np.abs(e) >= np.abs(e).max() / 256
        near = max(near, int(u[high].max()) if high.any() else 0)
        far = max(far, int(u.max()))
        differ += int((u > 0).sum())
        total += n
    _TALLY[(rate, count)] = (near, far, differ, total)
    print("twin vs oracle at %d Hz, %d sections: worst %d ulps within 2^-8 of the peak, %d anywhere; %d of %d samples differ" % (
        rate, count, near, far, differ, total))
    assert near <= NEAR_ULPS and far <= FAR_ULPS
    assert differ <= 4 * SHARE * total                  # no single cell above four times the grid's bound
    if len(_TALLY) == len(R.RATES) * len(R.COUNTS):     # the last cell: the share over the whole grid
        d, t = sum(v[2] for v in _TALLY.values()), sum(v[3] for v in _TALLY.values())
        print("twin vs oracle, whole grid: worst %d / %d ulps, share %.3g" % (max(v[0] for v in _TALLY.values()),
                                                                               max(v[1] for v in _TALLY.values()), d / t))
        assert d <= SHARE * t


def test_the_oracle_is_its_own_loop():
    """scipy's lfilter is the definition's three lines: against the plain Python loop, to what two fp64 evaluations differ by"""
    for rate, count in ((8000, 6), (192000, 3)):
        co = R.coefficients(R.bands_for(count, rate), rate)
        x = R.grid_signal("noise", R.SPAN + 1, rate)[:3000]
        assert np.abs(R.cascade64(x, co) - R.cascade_loop(x, co)).max() < 1e-10


# -------------------------------------------------------------------------------------------------------- other properties
def _mixed(rate=32000):
    """nine clips over three designs, one of them copied: (clips, index, designs)"""
    rng = np.random.default_rng(11)
    noise = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    clips = [noise(R.CHUNK + 1), noise(777), np.zeros(0, np.float32), noise(R.SPAN), R.grid_signal("sine60", 3 * R.SPAN + 5, rate), noise(R.RUN),
             noise(2 * R.CHUNK), noise(1), noise(R.SPAN - 1)]
    index = [0, 1, 2, 2, 1, 0, -1, 1, 2]
    designs = [np.asarray(R.coefficients(R.bands_for(c, rate), rate)) for c in (1, 3, 6)]
    return clips, index, designs


def test_packed_clips_equal_single_calls_in_place_too_and_nothing_else_moves():
    clips, index, designs = _mixed()
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    out, rec, x_after = C.call(x, offsets, lengths, index, designs, CPU)
    assert x_after.tobytes() == x.tobytes()
    mask = np.zeros(len(x), bool)
    for i, (c, o, d) in enumerate(zip(clips, offsets, index)):
        mask[o: o + len(c)] = True
        one, rec1, _ = C.call(c, [0], [len(c)], [0 if d >= 0 else -1], [designs[max(d, 0)]], CPU)
        assert out[o: o + len(c)].tobytes() == one.tobytes() and rec[16 * i: 16 * i + 16] == rec1, i
    assert np.all(out[~mask] == C.FILL * 2), "written outside a clip"
    got_in, rec_in, _ = C.call(x, offsets, lengths, index, designs, CPU, "inplace")
    assert rec_in == rec and got_in[mask].tobytes() == out[mask].tobytes() and np.all(got_in[~mask] == C.FILL)
    recs = C.recs_of(rec)
    assert [r.sections for r in recs] == [1, 3, 6, 6, 3, 1, 0, 3, 6] and [r.equalised for r in recs] == [d >= 0 for d in index]
    o = offsets[6]
    assert out[o: o + lengths[6]].tobytes() == clips[6].tobytes() and recs[6].peak_in == recs[6].peak_out == np.abs(clips[6]).max()


def test_nonfinite_and_empty_clips_come_back_bit_for_bit():
    rate = 32000
    co = np.asarray(R.coefficients(R.voice(rate), rate))
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
    for mode in ("out", "inplace"):
        out, rec, _ = C.call(x, offsets, [len(c) for c in clips], [0] * len(clips), [co], CPU, mode)
        recs = C.recs_of(rec)
        for c, o, r, bad in zip(clips, offsets, recs, (False, True, False, True, False, True)):
            y = out[o: o + len(c)]
            assert (r.nonfinite, r.equalised, r.sections) == ((True, False, 0) if bad else (False, True, 3))
            if bad:
                assert y.tobytes() == c.tobytes() and r.peak_in.tobytes() == r.peak_out.tobytes() and not np.isfinite(r.peak_in)
        assert np.isnan(recs[1].peak_in) and np.isinf(recs[3].peak_in) and np.isnan(recs[5].peak_in)
        assert recs[2].peak_in == recs[2].peak_out == 0
        want = R.equalise(good, R.coefficients(R.voice(rate), rate))
        for o in (offsets[0], offsets[4]):                              # the neighbours are what they are alone
            assert _within_bounds(out[o: o + 5000], want)


def test_a_boost_near_flt_max_saturates_and_stays_finite():
    rate = 32000
    x = np.full(4000, 3e38, np.float32)
    x[1::2] *= -1                                                   # fs / 2 ... and a tone at the band's centre
    x[2000:] = (3e38 * np.sin(2 * np.pi * 1000.0 * np.arange(2000) / rate)).astype(np.float32)
    y, rec = EQM.equalise(x, rate, EQ([Band("peak", 1000.0, q=1.0, gain_db=12.0)]), device="cpu")
    fmax = np.finfo(np.float32).max
    assert np.all(np.isfinite(y)) and np.abs(y).max() == fmax and rec.peak_out == fmax and rec.equalised and not rec.nonfinite
    want = R.equalise(x, [R.section("peak", 1000.0, 1.0, 12.0, rate)])
    assert (np.abs(want) == fmax).sum() > 100 and np.array_equal(np.abs(y) == fmax, np.abs(want) == fmax) and _within_bounds(y, want)


def test_the_identity_returns_the_input_and_issues_no_call(monkeypatch):
    x = np.random.default_rng(3).uniform(-1, 1, 1000).astype(np.float32)
    monkeypatch.setattr(EQM, "run_packed", lambda *a, **k: pytest.fail("a call was issued"))
    for e in (EQ([]), EQ([Band("peak", 300.0, gain_db=0.0), Band("lowshelf", 100.0), Band("highshelf", 5000.0, q=2.0, gain_db=-0.0)]), None):
        y, rec = EQM.equalise(x, 32000, e, device="cpu")
        assert y is not x and y.tobytes() == x.tobytes() and rec.sections == 0 and not rec.equalised and rec.peak_in == rec.peak_out == np.abs(x).max()
    ys, recs = EQM.equalise([x, x[:10]], 32000, [EQ([]), None])
    assert ys[1].tobytes() == x[:10].tobytes() and len(recs) == 2
    t = torch.from_numpy(x)
    y, rec = EQM.equalise(t, 32000, EQ([]))
    assert isinstance(y, torch.Tensor) and y.data_ptr() != t.data_ptr() and torch.equal(y, t)
    assert EQM.design(EQ([Band("peak", 300.0), Band("highpass", 80.0)]), 32000).shape == (1, 5) and EQM.design(EQ([]), 32000).shape == (0, 5)
    assert EQM.equalise([], 32000, "voice") == ([], [])


def test_module_lists_share_designs_and_keep_types():
    rate = 32000
    a, b, c = (np.random.default_rng(s).uniform(-1, 1, n).astype(np.float32) for s, n in ((1, 5000), (2, R.SPAN + 9), (3, 300)))
    e2 = EQ([Band("lowshelf", 200.0, gain_db=3.0), Band("peak", 300.0)])
    ys, recs = EQM.equalise([a, b.reshape(1, -1), torch.from_numpy(c), a], rate, ["voice", e2, None, EQ.preset("voice", rate)], device="cpu")
    assert isinstance(ys[0], np.ndarray) and ys[1].shape == (1, R.SPAN + 9) and isinstance(ys[2], torch.Tensor)
    assert ys[0].tobytes() == ys[3].tobytes() and [r.sections for r in recs] == [3, 1, 0, 3]
    assert ys[2].numpy().tobytes() == c.tobytes()
    y0, r0 = EQM.equalise(a, rate, "voice", device="cpu")
    assert y0.tobytes() == ys[0].tobytes() and r0.peak_out == recs[0].peak_out == np.abs(y0).max()
    assert _within_bounds(ys[1].reshape(-1), R.equalise(b, [R.section("lowshelf", 200.0, 1 / math.sqrt(2), 3.0, rate)]))


def test_audioclip_equalised_carries_the_record():
    from gsv_tts_lite_amd.tts import AudioClip
    rate = 32000
    x = (0.5 * np.random.default_rng(9).uniform(-1, 1, rate)).astype(np.float32)
    subs = [{"text": "a", "start_s": 0.0, "end_s": 0.5}]
    clip = AudioClip(None, x, rate, 1.0, subs, "a")
    assert clip.eq is None
    out = clip.equalised("voice")
    want, rec = EQM.equalise(x, rate, EQ.preset("voice", rate))
    assert out is not clip and out.audio_data.tobytes() == want.tobytes() and clip.audio_data.tobytes() == x.tobytes()
    assert out.subtitles is subs and out.orig_text == "a" and out.audio_len_s == 1.0 and out.samplerate == rate
    assert out.eq.sections == 3 and out.eq.peak_out == np.abs(out.audio_data).max() == rec.peak_out and out.eq.peak_in == np.abs(x).max()
    both = out.normalised(-20.0, peak_limit=math.inf).limited_to(-1.0)
    assert both.eq is out.eq and both.lufs is not None and both.dbtp is not None
    same = clip.equalised(EQ([]))
    assert same.audio_data.tobytes() == x.tobytes() and same.eq.sections == 0
    for bad in ([Band("peak", 100.0, gain_db=1)], None, "radio"):
        with pytest.raises(ValueError):
            clip.equalised(bad)
