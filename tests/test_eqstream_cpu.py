"""CPU checks of the stream equaliser (csrc/eqstream.h behind gsv_eqstream_push_host, eq.StreamEQ).  No GPU: the host
twin is built from the scalar routines the device kernels share, and tests/test_hip_eqstream.py pins the device to it byte for byte.

The contract: the samples a stream emits, concatenated, are the bytes eq.equalise (gsv_eq_host) returns for the same samples as one
clip with the same design, however the stream was cut into pushes; a push of n samples emits n; a flush emits nothing extra and
returns the state to fresh.  So no tolerance appears here: the clip twin is held to the fp64 oracle by test_eq_cpu.py, and these
tests hold the stream to the clip twin bit for bit.

The cuttings.  Every signal of tests/eq_ref.py's grid (12 lengths x 5 kinds at 32 kHz) goes through every cutting of the contract.
The cuttings of about a span or a chunk, the random ones, the flushing empty push and the push that completes two chunks run with
1, 3 and 6 sections.  The pushes of about a run (15, 16, 17 samples: three thousand pushes for the longest signal, each of which
reruns the open chunk on the host twin) run over every signal with the one-section design, and with 3 and 6 sections over the
lengths up to a span + 1: what a cut can break -- the stash, the span and chunk edges, the chain -- does not depend on the section
count, which the other cuttings cover."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_ref as R  # noqa: E402
import eqstream_cases as C  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402
from gsv_tts_lite_amd.eq import EQ, Band  # noqa: E402

RUN, SPAN, CHUNK = C.RUN, C.SPAN, C.CHUNK
RATE = 32000
FMAX = np.finfo(np.float32).max
EQUALISED, EVER, NONFINITE = N.EQS_EQUALISED, N.EQS_NONFINITE_EVER, N.EQS_NONFINITE


def _bits(v):
    return np.float32(v).view(np.uint32)


def test_constants_and_record_layout():
    assert (EQM.RUN, EQM.SPAN, EQM.CHUNK) == (RUN, SPAN, CHUNK)
    assert EQM.STREAM_RECORD_BYTES == C.REC == 32
    assert N.lib().gsv_eqstream_state_bytes() % 16 == 0 and N.lib().gsv_eqstream_state_bytes() > 2 * CHUNK * 4


@pytest.mark.parametrize("count", R.COUNTS)
def test_whole_stream_equals_the_clip_twin(count):
    st = C.RawStream(C.eq_for(count, RATE), RATE)
    for n in R.LENGTHS:
        for kind in R.KINDS:
            x = R.grid_signal(kind, n, RATE)
            y, recs = st.run(x, [n])
            want, crec = C.clip_twin(count, kind, n, RATE)
            rec = C.record(recs[0])
            what = (count, n, kind, rec, crec)
            assert y.tobytes() == want.tobytes(), what
            assert rec.emitted == n and rec.total == n and rec.equalised and not rec.nonfinite and not rec.nonfinite_ever, what
            assert _bits(rec.peak_in_run) == _bits(crec.peak_in) and _bits(rec.peak_out_run) == _bits(crec.peak_out), what
            assert _bits(rec.peak_in) == _bits(crec.peak_in) and _bits(rec.peak_out) == _bits(crec.peak_out), what


@pytest.mark.parametrize("rate", (8000, 192000))
def test_whole_stream_equals_the_clip_twin_at_other_rates(rate):
    e = EQ.preset("voice", rate)
    st = EQM.StreamEQ("voice", rate, "cpu")
    rng = np.random.default_rng(rate)
    for n in (SPAN + 1, CHUNK + 1):
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        want, crec = EQM.equalise(x, rate, e, device="cpu")
        y = st.push(x, flush=True)
        assert y.tobytes() == want.tobytes() and st.rec.total == n
        assert st.rec.peak_in_run == crec.peak_in and st.rec.peak_out_run == crec.peak_out
        y2, rec2 = EQM.equalise_stream(x, rate, e, cuts=C.cut_every(n, SPAN - 1))
        assert y2.tobytes() == want.tobytes() and rec2.total == n and rec2.peak_out_run == crec.peak_out


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("count", R.COUNTS)
def test_cut_invariance(count, kind):
    st = C.RawStream(C.eq_for(count, RATE), RATE)
    for n in R.LENGTHS:
        x = R.grid_signal(kind, n, RATE)
        want, crec = C.clip_twin(count, kind, n, RATE)
        for j, cuts in enumerate(C.cuttings(n, fine=count == 1 or n <= SPAN + 1)):
            # through the state the stream before left flushed; every other cutting in place
            y, recs = st.run(x, cuts, inplace=bool(j & 1))
            what = (count, kind, n, cuts[:8])
            assert y.tobytes() == want.tobytes(), what
            totals = np.array([np.frombuffer(r, np.int64)[3] for r in recs])
            assert np.array_equal(totals, np.cumsum(cuts)), what
            last = C.record(recs[-1])
            assert _bits(last.peak_in_run) == _bits(crec.peak_in) and _bits(last.peak_out_run) == _bits(crec.peak_out), what
            assert last.total == n and not last.nonfinite_ever, what


def test_a_second_stream_through_a_flushed_state_equals_a_fresh_states():
    e = C.eq_for(3, RATE)
    x = R.grid_signal("noise", 3 * CHUNK + 5, RATE)
    cuts = C.cut_every(len(x), 3333)
    a, ra = C.RawStream(e, RATE).run(x, cuts)
    used = C.RawStream(e, RATE)
    used.run(R.grid_signal("sine60", CHUNK + 1, RATE), C.cut_every(CHUNK + 1, 1000))
    used.run(R.grid_signal("impulse", 17, RATE), [17, 0])
    b, rb = used.run(x, cuts)
    assert a.tobytes() == b.tobytes() and ra == rb
    assert a.tobytes() == C.clip_twin(3, "noise", 3 * CHUNK + 5, RATE)[0].tobytes()
    # a flush emits nothing extra: the empty flushing push behind a stream hands out no sample and reports the stream's length
    st = EQM.StreamEQ(e, RATE, "cpu")
    assert len(st.push(x[:100])) == 100 and len(st.push(np.zeros(0, np.float32), flush=True)) == 0
    assert st.rec.emitted == 0 and st.rec.total == 100 and st.rec.peak_in == 0 and st.rec.peak_out == 0
    assert st.push(x[:100], flush=True).tobytes() == EQM.equalise(x[:100], RATE, e, device="cpu")[0].tobytes()


def test_per_push_records():
    e = C.eq_for(3, RATE)
    x = R.grid_signal("noise", 3 * CHUNK + 5, RATE) * np.float32(0.5)
    x[20000] = 0.9
    st = EQM.StreamEQ(e, RATE, "cpu")
    cuts = [0, 1, 15, SPAN, 0, CHUNK + 7, 3 * CHUNK + 5 - (1 + 15 + SPAN + CHUNK + 7), 0]
    at, pin, pout = 0, np.float32(0), np.float32(0)
    for k, n in enumerate(cuts):
        y = st.push(x[at: at + n], flush=k + 1 == len(cuts))
        r = st.rec
        assert isinstance(y, np.ndarray) and y.dtype == np.float32 and len(y) == n == r.emitted
        at += n
        assert r.total == at and r.equalised and not r.nonfinite and not r.nonfinite_ever
        assert r.peak_in == (np.abs(x[at - n: at]).max() if n else 0) and r.peak_out == (np.abs(y).max() if n else 0)
        pin, pout = max(pin, r.peak_in), max(pout, r.peak_out)
        assert r.peak_in_run == pin and r.peak_out_run == pout
    assert pin == np.float32(0.9) and at == len(x)
    # the next stream starts from nothing
    st.push(x[:10])
    assert st.rec.total == 10 and st.rec.peak_in_run == np.abs(x[:10]).max()


@pytest.mark.parametrize("count", (1, 6))
def test_a_sample_that_is_not_finite_is_copied_and_runs_as_zero(count):
    e = C.eq_for(count, RATE)
    n = 2 * CHUNK + 3
    base = np.random.default_rng(11).uniform(-1.0, 1.0, n).astype(np.float32)
    bad = {CHUNK: np.float32(np.nan), CHUNK - 1: np.float32(np.inf), CHUNK + SPAN + 7: np.float32(-np.inf),
           2 * CHUNK - 1: np.float32(-np.nan), 2 * CHUNK: np.float32(np.inf), 5: np.float32(np.nan)}
    x, z = base.copy(), base.copy()
    for at, v in bad.items():
        x[at], z[at] = v, 0.0
    want, crec = EQM.equalise(z, RATE, e, device="cpu")
    good = np.ones(n, bool)
    good[list(bad)] = False
    st = C.RawStream(e, RATE)
    for j, cuts in enumerate([[n], C.cut_every(n, SPAN), C.cut_every(n, CHUNK - 1), C.cut_every(n, 4097), C.cut_random(n, 5)]):
        y, recs = st.run(x, cuts, inplace=bool(j & 1))
        what = (count, cuts[:6])
        assert y[good].tobytes() == want[good].tobytes(), what
        assert y[~good].tobytes() == x[~good].tobytes(), what            # bit for bit, the NaN's sign and payload too
        ever, at = False, 0
        for c, raw in zip(cuts, recs):
            r = C.record(raw)
            here = bool((~good[at: at + c]).any())
            ever = ever or here
            assert r.nonfinite == here and r.nonfinite_ever == ever and r.equalised, what
            assert np.isfinite(r.peak_in) and np.isfinite(r.peak_out) and np.isfinite(r.peak_in_run) and np.isfinite(r.peak_out_run)
            sl = slice(at, at + c)
            assert r.peak_in == (np.abs(x[sl][good[sl]]).max() if good[sl].any() else 0), what
            assert r.peak_out == (np.abs(y[sl][good[sl]]).max() if good[sl].any() else 0), what
            at += c
        last = C.record(recs[-1])
        assert last.peak_in_run == np.abs(z[good]).max() and last.peak_out_run == np.abs(want[good]).max()
    # the flag does not outlive the flush
    _, recs = st.run(base, [100, n - 100])
    assert all(C.record(r).equalised and not C.record(r).nonfinite and not C.record(r).nonfinite_ever for r in recs)


def test_a_boost_near_flt_max_saturates_as_the_clip_does():
    x = np.full(4000, 3e38, np.float32)
    x[1::2] *= -1
    x[2000:] = (3e38 * np.sin(2 * np.pi * 1000.0 * np.arange(2000) / RATE)).astype(np.float32)
    x[10], x[11] = FMAX, -FMAX
    e = EQ([Band("peak", 1000.0, q=1.0, gain_db=12.0)])
    want, crec = EQM.equalise(x, RATE, e, device="cpu")
    assert (np.abs(want) == FMAX).sum() > 100
    for cuts in ([4000], C.cut_every(4000, 333)):
        y, rec = EQM.equalise_stream(x, RATE, e, cuts=cuts)
        assert y.tobytes() == want.tobytes() and np.all(np.isfinite(y))
        assert rec.peak_out_run == FMAX == crec.peak_out and rec.peak_in_run == FMAX and not rec.nonfinite_ever


def test_in_place_equals_out_of_place():
    e = C.eq_for(6, RATE)
    x = R.grid_signal("noise", 3 * CHUNK + 5, RATE)
    for cuts in ([len(x)], C.cut_every(len(x), SPAN + 1), C.cut_random(len(x), 3)):
        a, ra = C.RawStream(e, RATE).run(x, cuts, inplace=False)
        b, rb = C.RawStream(e, RATE).run(x, cuts, inplace=True)
        assert a.tobytes() == b.tobytes() and ra == rb


def test_a_held_length_is_honoured_and_clamped():
    e = C.eq_for(3, RATE)
    x = R.grid_signal("noise", SPAN + 1, RATE)
    want = EQM.equalise(x, RATE, e, device="cpu")[0]
    for held, n in ((40, 40), (-3, 0), (1 << 30, SPAN + 1), (SPAN, SPAN)):
        st = C.RawStream(e, RATE)
        o, raw = st.push(x, held=held)
        r = C.record(raw)
        assert r.emitted == n == r.total and o[:n].tobytes() == want[:n].tobytes()
        assert np.all(o[n:] == np.float32(2 * C.FILL)), "written behind the held length"
        o2, raw2 = st.push(x[n:], flush=True)
        assert o2[: len(x) - n].tobytes() == want[n:].tobytes() and C.record(raw2).total == len(x)


def test_argument_checks():
    L = N.lib()
    need = L.gsv_eqstream_state_bytes()
    state = torch.zeros(need + 16, dtype=torch.uint8)
    sp = state.data_ptr()
    assert sp % 16 == 0
    err = lambda: L.gsv_last_error().decode()
    des = C.design_struct(EQ.preset("voice", RATE), RATE)
    assert L.gsv_eqstream_init_host(None, need, des) == 1 and "null" in err()
    assert L.gsv_eqstream_init_host(sp, need, None) == 1 and "null" in err()
    assert L.gsv_eqstream_init_host(sp, need - 1, des) == 1 and "state" in err()
    assert L.gsv_eqstream_init_host(sp + 4, need, des) == 1 and "aligned" in err()

    def broken(change):
        d = C.design_struct(EQ.preset("voice", RATE), RATE)
        change(d[0])
        return d
    for change in (lambda d: setattr(d, "n_sections", 0), lambda d: setattr(d, "n_sections", 7),
                   lambda d: d.coef[1].__setitem__(0, float("nan")), lambda d: d.coef[0].__setitem__(4, 1.0),
                   lambda d: d.coef[2].__setitem__(3, 2.5), lambda d: d.coef[0].__setitem__(2, float("inf"))):
        assert L.gsv_eqstream_init_host(sp, need, broken(change)) == 1 and "sections" in err()
    x, out = torch.zeros(100), torch.full((100,), 3.0)
    rec = torch.zeros(4, dtype=torch.int64)
    ok = [sp, x.data_ptr(), 100, None, 0, out.data_ptr(), rec.data_ptr()]
    # zeros: not a state init made -- not read through, flags -1, out not written
    assert L.gsv_eqstream_push_host(*ok) == 0
    assert np.frombuffer(rec.numpy().tobytes(), np.int32)[:2].tolist() == [0, -1] and bool((out == 3.0).all())
    assert L.gsv_eqstream_init_host(sp, need, des) == 0
    assert L.gsv_eqstream_push_host(*ok) == 0
    assert np.frombuffer(rec.numpy().tobytes(), np.int32)[:2].tolist() == [100, EQUALISED] and bool((out == 0.0).all())
    for i, bad, word in [(0, None, "null"), (1, None, "null"), (5, None, "null"), (6, None, "null"), (2, -1, "chunk of -1"),
                         (2, (1 << 20) + 1, "chunk of"), (0, sp + 4, "aligned"), (6, rec.data_ptr() + 4, "aligned")]:
        args = list(ok)
        args[i] = bad
        assert L.gsv_eqstream_push_host(*args) == 1 and word in err(), (i, bad, err())
    args = list(ok)         # an empty push needs neither chunk nor out
    args[1], args[2], args[5] = None, 0, None
    assert L.gsv_eqstream_push_host(*args) == 0 and np.frombuffer(rec.numpy().tobytes(), np.int64)[3] == 100


def test_python_entries_raise_on_what_is_no_equaliser():
    x = np.zeros(8, np.float32)
    for bad in (EQ([]), EQ([Band("peak", 300.0, gain_db=0.0)]), None, [Band("peak", 100.0, gain_db=1)], "radio", 3.0):
        with pytest.raises(ValueError):
            EQM.StreamEQ(bad, RATE, "cpu")
        with pytest.raises(ValueError):
            EQM.equalise_stream(x, RATE, bad)
    for rate in (3999, 768001, 32000.5, True):
        with pytest.raises(ValueError):
            EQM.StreamEQ("voice", rate, "cpu")
        with pytest.raises(ValueError):
            EQM.equalise_stream(x, rate, "voice")
    for cuts in ([3, 4], [9, -1], []):
        with pytest.raises(ValueError):
            EQM.equalise_stream(x, RATE, "voice", cuts=cuts)
    st = EQM.StreamEQ("voice", RATE)
    assert not st.on_device and st.rec is None and isinstance(st.push_tensor(torch.zeros(5)), torch.Tensor)


def test_stream_keyword_validates(tmp_path):
    from gsv_tts import TTS
    t = TTS(models_dir=str(tmp_path), device="cpu")
    ref = ("spk.wav", "prompt.wav", "prompt.")
    band = Band("peak", 100.0, gain_db=1)
    for bad in ([band], "radio", 3.0, band):
        with pytest.raises(ValueError, match="eq"):
            next(t.infer_stream(*ref, "text.", eq=bad))
    for bad in (["voice", "radio"], ["voice", 3.0], [band, band], "radio"):
        with pytest.raises(ValueError, match="eq"):
            next(t.infer_stream_batched(*ref, ["one.", "two."], eq=bad))
    with pytest.raises(ValueError, match="eq has 3 entries for 2 requests"):
        next(t.infer_stream_batched(*ref, ["one.", "two."], eq=["voice", None, "voice"]))
