"""The reverb's host twin (csrc/reverb.h behind gsv_reverb_host) against the serial fp64 oracle of tests/reverb_ref.py,
and the module around it.  No GPU: test_hip_reverb.py holds the device to this twin in bytes.

The bound.  Per sample |twin - oracle| <= ulp32(oracle) + 1e-12 max(1, peak_in G), G = reverb_ref.gain_bound: the largest |y| a
clip of peak 1 can reach.  Both sides compute the fp64 value w = gw s + gd v and round it to fp32 once.  The twin's w differs from
the oracle's only by fp64 rounding: it evaluates the damping filter as a scan over runs of 32 samples where the oracle runs it
sample by sample, and it uses fma where the oracle rounds the product first.  Every intermediate -- a line's contents, a filter's
state, the sums -- is bounded by peak_in G (G sums the magnitudes of the whole impulse response), each operation adds at most
2^-53 of that, and the network is contractive (fb < 1, |0.5| < 1), so an error made at one sample comes back at most G-fold over
all later ones: a few thousand operations per sample's history give |dw| <~ 1e-13 peak_in G, under the second term.  The two
fp32 roundings of values that close land on the same float or, next to a tie, on neighbours: the first term.  The max(1, .) keeps
the bound from shrinking under the quiet clip, whose w are far above fp64's denormals but whose |dw| is not worth a tighter claim.
Measured: every sample of the grid equal, 0 ulps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_ref as R  # noqa: E402
import reverb_cases as C  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import reverb as RV  # noqa: E402
from gsv_tts_lite_amd.reverb import Reverb  # noqa: E402

CPU = torch.device("cpu")


def _assert_close(got, want, x, ps, cell):
    if len(want) == 0:
        return
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-12 * max(1.0, float(np.abs(x).max()) * R.gain_bound(ps))
    worst = int(np.argmax(err - tol))
    assert np.all(err <= tol), (cell, worst, got[worst], want[worst])


# ------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", list(R.SETS))
def test_twin_against_the_serial_oracle(name):
    ps = R.SETS[name][0]
    g = R.grid(name)
    clips = [c[3] for c in g]
    x, offsets = C.pack(clips)
    out, rec, x_after = C.call(x, offsets, [len(c) for c in clips], [0] * len(clips), [C.params_of(ps)], CPU)
    assert x_after.tobytes() == x.tobytes()
    for (_, n, kind, xc, y), o, r in zip(g, offsets, C.recs_of(rec)):
        got = out[o: o + n]
        _assert_close(got, y, xc, ps, (name, n, kind))
        assert r.reverbed and not r.nonfinite
        assert r.peak_in == (np.abs(xc).max() if n else 0) and r.peak_out == (np.abs(got).max() if n else 0)


def test_the_longest_legal_line_against_the_oracle():
    x1, y = R.long_cell()
    assert max(R.LONG[0]) == 28160 <= RV.MAX_DELAY and 28160 > N.RVB_SPAN
    out, rec, _ = C.call(*C.pack([x1]), [len(x1)], [0], [C.params_of(R.LONG)], CPU)
    _assert_close(out[C.GUARD: C.GUARD + len(x1)], y, x1, R.LONG, "long")
    assert np.abs(y[28160:].astype(np.float64) - 1.94 * x1[28160:]).max() > 1e-4      # the line has wrapped: the wet part is there


def test_the_delays_and_gains_of_the_module_are_the_definitions():
    for rate in (8000, 32000, 48000, 768000):
        for vals in (R.VOICE, R.HALL, (0.5, 0.5, 0.33, 0.4, 1.0), (0.3, 0.9, 0.2, 0.1, 0.0)):
            delays, gains = Reverb(*vals).parameters(rate)
            ps = R.parameter_set(*vals, rate)
            assert tuple(delays) == ps[0] + ps[1] and delays.dtype == np.int32
            assert gains.tobytes() == np.array(ps[2:], np.float64).tobytes()
    assert Reverb.preset("voice").parameters(32000)[1].tolist() == [0.2, 0.28 * 0.1 + 0.7, 0.015, 1.5 * 0.03 * 2.0, 1.94]
    assert Reverb().parameters(768000)[0].max() == 28160
    for bad in (3999, 768001, 44100.5):
        with pytest.raises(ValueError):
            Reverb().parameters(bad)


# ------------------------------------------------------------------------------------------------------------- closed forms
def test_the_voice_impulse_response_at_32_khz():
    h = RV.impulse_response("voice", 32000, 2000)
    assert h.dtype == np.float32 and h.shape == (2000,)
    assert h[0] == np.float32(1.94)
    assert not h[1:809].any()                                           # the shortest comb line is 32000 * 1116 // 44100 = 809
    # the first arrival: gin through one comb, its sign flipped by each of the four all-passes, times the wet gain
    want = np.float32(0.015 * 0.09)
    assert abs(float(h[809]) - float(want)) <= float(np.spacing(want)) and h[809] > 0
    assert RV.impulse_response(Reverb(wet_level=0.0, dry_level=0.5), 32000, 4).tolist() == [1.0, 0.0, 0.0, 0.0]
    assert RV.impulse_response("voice", 32000, 0).shape == (0,)
    with pytest.raises(ValueError):
        RV.impulse_response("radio", 32000, 10)


def test_no_wet_signal_is_the_dry_gain_alone():
    x = np.random.default_rng(4).uniform(-1, 1, 3000).astype(np.float32)
    for dry in (0.0, 0.25, 0.97, 1.0):
        y, rec = RV.reverberate(x, 32000, Reverb(wet_level=0.0, dry_level=dry), device="cpu")
        want = (2.0 * dry * x.astype(np.float64)).astype(np.float32)
        # the wet term is a zero of either sign (gw = 0 times a finite s), so it moves no value; only the sign of a zero can differ
        assert np.array_equal(y, want) and y[want != 0].tobytes() == want[want != 0].tobytes(), dry
        assert rec.reverbed and rec.peak_out == np.abs(y).max()


def test_the_identity_returns_the_input_and_issues_no_call(monkeypatch):
    x = np.random.default_rng(3).uniform(-1, 1, 1000).astype(np.float32)
    monkeypatch.setattr(RV, "run_packed", lambda *a, **k: pytest.fail("a call was issued"))
    ident = Reverb(wet_level=0.0, dry_level=0.5)
    assert ident.is_identity and not Reverb(wet_level=0.0).is_identity and not Reverb(dry_level=0.5).is_identity
    for r in (ident, Reverb(0.9, 0.1, 0.0, 0.5, 0.3), None):
        y, rec = RV.reverberate(x, 32000, r, device="cpu")
        assert y is not x and y.tobytes() == x.tobytes() and not rec.reverbed and not rec.nonfinite
        assert rec.peak_in == rec.peak_out == np.abs(x).max()
    ys, recs = RV.reverberate([x, x[:10]], 32000, [ident, None])
    assert ys[1].tobytes() == x[:10].tobytes() and len(recs) == 2
    t = torch.from_numpy(x)
    y, rec = RV.reverberate(t, 32000, ident)
    assert isinstance(y, torch.Tensor) and y.data_ptr() != t.data_ptr() and torch.equal(y, t)
    assert RV.reverberate([], 32000, "voice") == ([], [])
    bad = x.copy()
    bad[7] = np.nan
    assert RV.reverberate(bad, 32000, None)[1].nonfinite
    assert RV.resolve(ident) is None and RV.resolve(None) is None and isinstance(RV.resolve("voice"), Reverb)


# ------------------------------------------------------------------------------------------------------------- the call
def _mixed():
    rng = np.random.default_rng(7)
    noise = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    clips = [noise(2500), noise(777), np.zeros(0, np.float32), noise(1), R.signal("gated220", 3001, 48000), noise(258), noise(900), noise(64),
             noise(4099)]
    index = [0, 1, 2, 2, 1, 0, -1, 1, 2]
    params = [C.params_of(R.SETS[n][0]) for n in ("voice32", "voice8", "tiny")]
    return clips, index, params


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
    assert [r.reverbed for r in recs] == [True, True, True, True, True, True, False, True, True]
    o = offsets[6]
    assert out[o: o + lengths[6]].tobytes() == clips[6].tobytes() and recs[6].peak_in == recs[6].peak_out == np.abs(clips[6]).max()
    assert recs[2].peak_in == recs[2].peak_out == 0


def test_nonfinite_and_empty_clips_come_back_bit_for_bit():
    ps = R.SETS["voice32"][0]
    rng = np.random.default_rng(5)
    nan = rng.uniform(-1, 1, 4000).astype(np.float32)
    nan[2051] = np.nan
    inf = rng.uniform(-1, 1, 3000).astype(np.float32)
    inf[2999] = -np.inf
    both = nan.copy()
    both[5] = np.inf
    good = rng.uniform(-1, 1, 2500).astype(np.float32)
    clips = [good, nan, np.zeros(0, np.float32), inf, good, both]
    x, offsets = C.pack(clips)
    want = R.reverb(good, ps)
    for mode in ("out", "inplace"):
        out, rec, _ = C.call(x, offsets, [len(c) for c in clips], [0] * len(clips), [C.params_of(ps)], CPU, mode)
        recs = C.recs_of(rec)
        for c, o, r, bad in zip(clips, offsets, recs, (False, True, False, True, False, True)):
            y = out[o: o + len(c)]
            assert (r.nonfinite, r.reverbed) == ((True, False) if bad else (False, True))
            if bad:
                assert y.tobytes() == c.tobytes() and r.peak_in.tobytes() == r.peak_out.tobytes() and not np.isfinite(r.peak_in)
        assert np.isnan(recs[1].peak_in) and np.isinf(recs[3].peak_in) and np.isnan(recs[5].peak_in)
        assert recs[2].peak_in == recs[2].peak_out == 0
        for o in (offsets[0], offsets[4]):                              # the neighbours are what they are alone
            _assert_close(out[o: o + len(good)], want, good, ps, mode)


def test_every_refusal_of_the_c_entry_has_its_message():
    x = np.zeros(64, np.float32)
    good = C.params_of(R.SETS["tiny"][0])
    L = N.lib()

    def rc(params, index=(0,), lengths=(64,), offsets=(0,)):
        clips, tab = RV._tables(offsets, lengths, index, params)
        need = L.gsv_reverb_work_bytes(clips, len(lengths), tab, len(params)) or 1 << 16
        xt, out = torch.from_numpy(x.copy()), torch.zeros(64)
        work, rec = torch.zeros(need, dtype=torch.uint8), torch.zeros(16 * len(lengths), dtype=torch.uint8)
        code = L.gsv_reverb_host(xt.data_ptr(), 64, clips, len(lengths), tab, len(params), out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)
        return code, (L.gsv_last_error() or b"").decode()

    def with_delay(j, v):
        d = good[0].copy()
        d[j] = v
        return d, good[1]

    def with_gain(j, v):
        g = good[1].copy()
        g[j] = v
        return good[0], g

    assert rc([good])[0] == 0
    for j in range(12):                                                 # a delay outside 1..32768
        for v in (0, -1, 32769, 2 ** 31 - 1):
            code, msg = rc([with_delay(j, v)])
            assert code == 1 and "parameter set 0" in msg and "delay outside 1..32768" in msg, (j, v, msg)
        assert rc([with_delay(j, 32768)])[0] == 0 and rc([with_delay(j, 1)])[0] == 0
    for j in (0, 1):                                                    # d or fb outside [0, 1)
        for v in (-1e-9, 1.0, 1.5, float("nan"), float("inf")):
            code, msg = rc([with_gain(j, v)])
            assert code == 1 and "in [0, 1)" in msg, (j, v, msg)
        assert rc([with_gain(j, 0.0)])[0] == 0 and rc([with_gain(j, 1.0 - 2.0 ** -53)])[0] == 0
    for j in (2, 3, 4):                                                 # a gain that is not finite
        for v in (float("nan"), float("inf"), -float("inf")):
            code, msg = rc([with_gain(j, v)])
            assert code == 1 and "not finite" in msg, (j, v, msg)
        assert rc([with_gain(j, -3.0)])[0] == 0 and rc([with_gain(j, 0.0)])[0] == 0
    for kw in (dict(index=(1,)), dict(index=(-2,)), dict(lengths=(65,)), dict(offsets=(1,)), dict(lengths=(-1,))):
        code, msg = rc([good], **kw)                                    # an index outside the sets, a clip outside the samples
        assert code == 1 and "an index outside them" in msg, (kw, msg)
    assert rc([], index=(-1,))[0] == 0                                  # measure only needs no parameter set
    assert rc([good, good], index=(1,))[0] == 0
    clips, tab = RV._tables([0], [64], [0], [good])
    w = torch.zeros(1 << 16, dtype=torch.uint8)
    need = L.gsv_reverb_work_bytes(clips, 1, tab, 1)
    xt, out, rec = torch.from_numpy(x), torch.zeros(64), torch.zeros(16, dtype=torch.uint8)          # alive over the calls below
    args = (xt.data_ptr(), 64, clips, 1, tab, 1, out.data_ptr(), rec.data_ptr())
    assert 0 < need < 1 << 16 and need >= 64 * 72
    assert L.gsv_reverb_host(*args, w.data_ptr(), need - 1) == 1 and b"needed" in L.gsv_last_error()
    assert L.gsv_reverb_host(*args, w.data_ptr() + 8, need) == 1 and b"16-byte aligned" in L.gsv_last_error()
    assert L.gsv_reverb_host(*args, w.data_ptr(), need) == 0
    for k in (0, 2, 6, 7):                                              # x, clips, out, records
        a = list(args)
        a[k] = None
        assert L.gsv_reverb_host(*a, w.data_ptr(), need) == 1 and b"null argument" in L.gsv_last_error(), k
    a = list(args)
    a[4] = None
    assert L.gsv_reverb_host(*a, w.data_ptr(), need) == 1 and b"null argument" in L.gsv_last_error()
    assert L.gsv_reverb_host(*args, None, need) == 1 and b"null argument" in L.gsv_last_error()
    assert L.gsv_reverb_work_bytes(clips, 0, tab, 1) == 0 and L.gsv_reverb_work_bytes(clips, 1, None, 1) == 0
    assert L.gsv_reverb_work_bytes(clips, 65536, tab, 1) == 0
    with pytest.raises(RuntimeError, match="parameter set 0"):
        RV.run_packed(torch.from_numpy(x.copy()), [0], [64], [0], [with_gain(1, 1.0)], torch.zeros(64))
    with pytest.raises(ValueError):
        RV.run_packed(torch.from_numpy(x.copy()), [0], [64], [0], [(np.zeros(11, np.int32), good[1])], torch.zeros(64))
    with pytest.raises(ValueError):
        RV.run_packed(torch.from_numpy(x.copy()), [0], [64], [1], [good], torch.zeros(64))


def test_module_lists_share_parameter_sets_and_keep_types(monkeypatch):
    rate = 32000
    a, b, c = (np.random.default_rng(s).uniform(-1, 1, n).astype(np.float32) for s, n in ((1, 2500), (2, 2057), (3, 300)))
    hall = Reverb(*R.HALL)
    seen = []
    inner = RV.run_packed
    monkeypatch.setattr(RV, "run_packed", lambda x, o, l, index, params, *rest, **kw: (seen.append((list(index), len(params))),
                                                                                        inner(x, o, l, index, params, *rest, **kw))[1])
    ys, recs = RV.reverberate([a, b.reshape(1, -1), torch.from_numpy(c), a], rate, ["voice", hall, None, Reverb.preset("voice")], device="cpu")
    assert seen == [([0, 1, -1, 0], 2)]                                 # one packed call, the distinct sets once
    assert isinstance(ys[0], np.ndarray) and ys[1].shape == (1, 2057) and isinstance(ys[2], torch.Tensor)
    assert ys[0].tobytes() == ys[3].tobytes() and [r.reverbed for r in recs] == [True, True, False, True]
    assert ys[2].numpy().tobytes() == c.tobytes()
    y0, r0 = RV.reverberate(a, rate, "voice", device="cpu")
    assert y0.tobytes() == ys[0].tobytes() and r0.peak_out == recs[0].peak_out == np.abs(y0).max()
    _assert_close(ys[1].reshape(-1), R.reverb(b, R.SETS["hall"][0]), b, R.SETS["hall"][0], "hall")
    with pytest.raises(ValueError):
        RV.reverberate([a, b], rate, ["voice"])


def test_reverb_range_errors():
    for kw in (dict(room_size=-0.01), dict(room_size=1.01), dict(damping=2.0), dict(wet_level=-1.0), dict(dry_level=1.5), dict(width=float("nan")),
               dict(width=1.0001), dict(damping="soft"), dict(room_size=None), dict(wet_level=float("inf"))):
        with pytest.raises(ValueError):
            Reverb(**kw)
    r = Reverb(0.0, 1.0, 1.0, 0.0, 0.0)
    assert (r.room_size, r.damping, r.wet_level, r.dry_level, r.width) == (0.0, 1.0, 1.0, 0.0, 0.0)
    assert repr(Reverb()) == "Reverb(room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0)"
    v = Reverb.preset("voice")
    assert (v.room_size, v.damping, v.wet_level, v.dry_level, v.width) == (0.1, 0.5, 0.03, 0.97, 1.0) and RV.PRESETS == ("voice",)
    for bad in ("radio", 3.0, [v], object()):
        with pytest.raises(ValueError):
            RV.resolve(bad)
    with pytest.raises(ValueError):
        Reverb.preset("hall")


# ------------------------------------------------------------------------------------------------------------- AudioClip
def test_audioclip_ambient_carries_the_record_and_keeps_the_others():
    from gsv_tts_lite_amd.tts import AudioClip
    rate = 32000
    x = (0.4 * np.random.default_rng(9).uniform(-1, 1, 4000)).astype(np.float32)
    subs = [{"text": "a", "start_s": 0.0, "end_s": 0.1}]
    clip = AudioClip(None, x, rate, 0.125, subs, "a")
    assert clip.ambience is None
    out = clip.ambient()
    want, rec = RV.reverberate(x, rate, "voice")
    assert out is not clip and out.audio_data.tobytes() == want.tobytes() and clip.audio_data.tobytes() == x.tobytes()
    assert len(out.audio_data) == len(x) and out.subtitles is subs and out.orig_text == "a" and out.audio_len_s == 0.125
    assert out.ambience.reverbed and out.ambience.peak_out == np.abs(out.audio_data).max() == rec.peak_out and out.ambience.peak_in == np.abs(x).max()
    chain = clip.equalised("voice").compressed("voice").ambient(Reverb(0.3, 0.2, 0.1, 0.5)).normalised(-20.0).limited_to(-1.0)
    assert chain.eq is not None and chain.comp is not None and chain.ambience.reverbed and chain.lufs is not None and chain.dbtp is not None
    assert clip.ambient().equalised("voice").compressed("voice").ambience is not None
    same = clip.ambient(Reverb(wet_level=0.0, dry_level=0.5))
    assert same.audio_data.tobytes() == x.tobytes() and not same.ambience.reverbed
    for bad in ([Reverb()], None, "radio", 0.5):
        with pytest.raises(ValueError):
            clip.ambient(bad)
