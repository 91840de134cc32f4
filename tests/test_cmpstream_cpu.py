"""CPU checks of the stream compressor (csrc/cmpstream.h behind gsv_cmpstream_push_host, compressor.StreamCompressor).
No GPU: the host twin is built from the scalar routines the device kernels share, and tests/test_hip_cmpstream.py pins the device
to it byte for byte.

The contract: the samples a stream emits, concatenated, are the bytes compressor.compress (gsv_compressor_host) returns for the
same samples as one clip with the same parameters, however the stream was cut into pushes; a push of n samples emits n; a flush
emits nothing extra and returns the state to fresh.  So no tolerance appears here: the clip twin is held to the serial fp64 oracle
by test_compressor_cpu.py, and these tests hold the stream to the clip twin bit for bit.

The cuttings.  Every parameter set and signal kind of tests/compressor_ref.py at 32 kHz goes through the stream lengths 0, 1, a
run + 1, a span + 1, a chunk, a chunk + 1 and two chunks + a span + 5 under every cutting of the contract.  The pushes of about a
run (15, 16, 17 samples, each of which reruns the open chunk on the host twin) run over the lengths up to a span + 1, and for the
"voice" set over the gated tone -- whose attacks and releases cross the span and chunk edges -- also at a chunk + 1, where they
cross the first chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compressor_ref as R  # noqa: E402
import cmpstream_cases as C  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import compressor as CM  # noqa: E402
from gsv_tts_lite_amd.compressor import Compressor  # noqa: E402

RUN, SPAN, CHUNK = C.RUN, C.SPAN, C.CHUNK
RATE = 32000
LIVE, EVER, NONFINITE, COMPRESSED = N.CMS_STREAM, N.CMS_NONFINITE_EVER, N.CMS_NONFINITE, N.CMS_COMPRESSED
_bits = C.bits


def _same_running(rec, crec):
    return (_bits(rec.peak_in_run) == _bits(crec.peak_in) and _bits(rec.peak_out_run) == _bits(crec.peak_out)
            and _bits(rec.min_gain_run) == _bits(crec.min_gain))


def test_constants_and_record_layout():
    assert (CM.RUN, CM.SPAN, CM.CHUNK) == (RUN, SPAN, CHUNK)
    assert CM.STREAM_RECORD_BYTES == C.REC == 40
    need = N.lib().gsv_cmpstream_state_bytes()
    assert need % 16 == 0 and need > 2 * CHUNK * 4
    assert C.LENGTHS == (0, 1, RUN + 1, SPAN + 1, CHUNK, CHUNK + 1, 2 * CHUNK + SPAN + 5)


@pytest.mark.parametrize("name", list(R.SETS))
def test_whole_stream_equals_the_clip_twin(name):
    st = C.RawStream(C.comp_for(name), RATE)
    acted = False
    for n in C.LENGTHS:
        for kind in R.KINDS:
            x = R.grid_signal(kind, n, RATE, name)
            y, recs = st.run(x, [n])
            want, crec = C.clip_twin(name, kind, n, RATE)
            rec = C.record(recs[0])
            what = (name, n, kind, rec, crec)
            assert y.tobytes() == want.tobytes(), what
            assert rec.emitted == n and rec.total == n and rec.live and not rec.nonfinite and not rec.nonfinite_ever, what
            assert _same_running(rec, crec), what
            assert _bits(rec.peak_in) == _bits(crec.peak_in) and _bits(rec.peak_out) == _bits(crec.peak_out), what
            assert _bits(rec.min_gain) == _bits(crec.min_gain) and rec.compressed == crec.compressed == bool(rec.min_gain < 1), what
            acted = acted or rec.compressed
    assert acted, "no cell of the set passes its threshold: the test shows nothing"


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(R.SETS))
def test_cut_invariance(name, kind):
    st = C.RawStream(C.comp_for(name), RATE)
    for n in C.LENGTHS:
        x = R.grid_signal(kind, n, RATE, name)
        want, crec = C.clip_twin(name, kind, n, RATE)
        if kind == "gated220" and n > CHUNK:
            assert crec.min_gain < 1, "the gated tone must drive the compressor"
        fine = n <= SPAN + 1 or (name == "voice" and kind == "gated220" and n == CHUNK + 1)
        for j, cuts in enumerate(C.cuttings(n, fine=fine)):
            # through the state the stream before left flushed; every other cutting in place
            y, recs = st.run(x, cuts, inplace=bool(j & 1))
            what = (name, kind, n, cuts[:8])
            assert y.tobytes() == want.tobytes(), what
            totals = np.array([np.frombuffer(r, np.int64)[4] for r in recs])
            assert np.array_equal(totals, np.cumsum(cuts)), what
            last = C.record(recs[-1])
            assert _same_running(last, crec), (what, last, crec)
            assert last.total == n and not last.nonfinite_ever, what


@pytest.mark.parametrize("rate", (8000, 48000))
def test_whole_stream_equals_the_clip_twin_at_other_rates(rate):
    st = CM.StreamCompressor("voice", rate, "cpu")
    for n in (SPAN + 1, CHUNK + 1):
        x = np.array(R.grid_signal("gated220", n, rate, "voice"))
        want, crec = CM.compress(x, rate, "voice", device="cpu")
        y = st.push(x, flush=True)
        assert y.tobytes() == want.tobytes() and st.rec.total == n and crec.compressed
        assert _same_running(st.rec, crec)
        y2, rec2 = CM.compress_stream(x, rate, "voice", cuts=C.cut_every(n, SPAN - 1))
        assert y2.tobytes() == want.tobytes() and rec2.total == n and _same_running(rec2, crec)


def test_a_second_stream_through_a_flushed_state_equals_a_fresh_states():
    c = C.comp_for("voice")
    n = 2 * CHUNK + SPAN + 5
    x = np.array(R.grid_signal("gated220", n, RATE, "voice"))
    cuts = C.cut_every(n, 3333)
    a, ra = C.RawStream(c, RATE).run(x, cuts)
    used = C.RawStream(c, RATE)
    used.run(R.grid_signal("noise", CHUNK + 1, RATE, "voice"), C.cut_every(CHUNK + 1, 1000))
    used.run(R.grid_signal("square", 17, RATE, "voice"), [17, 0])
    b, rb = used.run(x, cuts)
    assert a.tobytes() == b.tobytes() and ra == rb
    assert a.tobytes() == C.clip_twin("voice", "gated220", n, RATE)[0].tobytes()
    # a flush emits nothing extra: the empty flushing push behind a stream hands out no sample and reports the stream's length
    st = CM.StreamCompressor(c, RATE, "cpu")
    assert len(st.push(x[:100])) == 100 and len(st.push(np.zeros(0, np.float32), flush=True)) == 0
    r = st.rec
    assert r.emitted == 0 and r.total == 100 and r.peak_in == 0 and r.peak_out == 0 and r.min_gain == 1 and not r.compressed
    assert st.push(x[:100], flush=True).tobytes() == CM.compress(np.array(x[:100]), RATE, c, device="cpu")[0].tobytes()


def test_per_push_records():
    c = C.comp_for("voice")
    n = 2 * CHUNK + SPAN + 5
    x = np.array(R.grid_signal("gated220", n, RATE, "voice"))
    st = CM.StreamCompressor(c, RATE, "cpu")
    cuts = [0, 1, 15, SPAN, 0, CHUNK + 7, n - (1 + 15 + SPAN + CHUNK + 7), 0]
    at, pin, pout, gmin = 0, np.float32(0), np.float32(0), np.float32(1)
    for k, m in enumerate(cuts):
        y = st.push(x[at: at + m], flush=k + 1 == len(cuts))
        r = st.rec
        assert isinstance(y, np.ndarray) and y.dtype == np.float32 and len(y) == m == r.emitted
        at += m
        assert r.total == at and r.live and not r.nonfinite and not r.nonfinite_ever
        assert r.peak_in == (np.abs(x[at - m: at]).max() if m else 0) and r.peak_out == (np.abs(y).max() if m else 0)
        assert r.min_gain <= 1 and r.compressed == bool(r.min_gain < 1) and (m or r.min_gain == 1)
        pin, pout, gmin = max(pin, r.peak_in), max(pout, r.peak_out), min(gmin, r.min_gain)
        assert r.peak_in_run == pin and r.peak_out_run == pout and r.min_gain_run == gmin
    crec = C.clip_twin("voice", "gated220", n, RATE)[1]
    assert at == n and gmin == crec.min_gain < 1 and pout == crec.peak_out
    # the next stream starts from nothing
    st.push(x[:10])
    assert st.rec.total == 10 and st.rec.peak_in_run == np.abs(x[:10]).max() and st.rec.min_gain_run == st.rec.min_gain > gmin


@pytest.mark.parametrize("name", ("voice", "fast"))
def test_a_sample_that_is_not_finite_is_copied_and_runs_as_zero(name):
    c = C.comp_for(name)
    n = 2 * CHUNK + 3
    base = np.array(R.grid_signal("gated220", n, RATE, name))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # a run edge, a span edge and a chunk edge, each from both sides, with NaN, +inf and -inf
    bad = {RUN - 1: nan, RUN: inf, SPAN - 1: -inf, SPAN: -nan, CHUNK - 1: inf, CHUNK: nan, CHUNK + SPAN + 7: -inf,
           2 * CHUNK - 1: -nan, 2 * CHUNK: inf, 5: nan}
    x, z = base.copy(), base.copy()
    for at, v in bad.items():
        x[at], z[at] = v, 0.0
    want, crec = CM.compress(z, RATE, c, device="cpu")
    assert crec.compressed
    good = np.ones(n, bool)
    good[list(bad)] = False
    alone = np.diff([0] + sorted(set(sum(([at, at + 1] for at in bad), []))) + [n]).tolist()     # every such sample a push of its own
    st, clean = C.RawStream(c, RATE), C.RawStream(c, RATE)
    for j, cuts in enumerate([[n], C.cut_every(n, SPAN), C.cut_every(n, CHUNK - 1), C.cut_every(n, 4097), C.cut_random(n, 5), alone]):
        y, recs = st.run(x, cuts, inplace=bool(j & 1))
        yz, recs_z = clean.run(z, cuts, inplace=bool(j & 1))
        what = (name, cuts[:6])
        assert yz.tobytes() == want.tobytes(), what
        assert y[good].tobytes() == want[good].tobytes(), what
        assert y[~good].tobytes() == x[~good].tobytes(), what            # bit for bit, the NaN's sign and payload too
        ever, at = False, 0
        for m, raw, raw_z in zip(cuts, recs, recs_z):
            r, rz = C.record(raw), C.record(raw_z)
            sl = slice(at, at + m)
            here = bool((~good[sl]).any())
            ever = ever or here
            assert r.nonfinite == here and r.nonfinite_ever == ever and r.live, what
            assert all(np.isfinite(v) for v in (r.peak_in, r.peak_out, r.min_gain, r.peak_in_run, r.peak_out_run, r.min_gain_run))
            assert r.peak_in == (np.abs(x[sl][good[sl]]).max() if good[sl].any() else 0), what
            assert r.peak_out == (np.abs(y[sl][good[sl]]).max() if good[sl].any() else 0), what
            if not here:            # a push without such a sample: the record of the stream with zeros in their places
                assert (r.peak_in, r.peak_out, r.min_gain, r.compressed) == (rz.peak_in, rz.peak_out, rz.min_gain, rz.compressed), what
            elif not good[sl].any():        # a push of such samples alone: nothing measured, no gain counted
                assert (r.peak_in, r.peak_out, r.min_gain, r.compressed) == (0, 0, 1, False), what
            assert r.min_gain >= rz.min_gain, what
            at += m
        last = C.record(recs[-1])
        assert last.peak_in_run == np.abs(z[good]).max() and last.peak_out_run == np.abs(want[good]).max()
        if cuts is alone:           # the smallest gain of the stream leaves these samples out: that of the pushes without them
            assert last.min_gain_run == min(C.record(rz).min_gain for m, rz, at in
                                            zip(cuts, recs_z, np.cumsum([0] + cuts[:-1])) if m and good[at: at + m].all())
    # the flag does not outlive the flush
    _, recs = st.run(base, [100, n - 100])
    assert all(C.record(r).live and not C.record(r).nonfinite and not C.record(r).nonfinite_ever for r in recs)


def test_denormals_pushed_in_pieces_equal_the_clip():
    x, co = R.denormal_clip()
    x = np.array(x)
    d = R.DENORMAL
    want, crec = CM.compress(x, d["rate"], Compressor(*d["params"]), device="cpu")
    assert crec.compressed
    for j, cuts in enumerate(([len(x)], C.cut_every(len(x), 61), C.cut_every(len(x), 1000), C.cut_random(len(x), 2))):
        st = C.RawStream(None, d["rate"], coefficients=np.array(co, np.float64))
        y, recs = st.run(x, cuts, inplace=bool(j & 1))
        assert y.tobytes() == want.tobytes(), cuts[:6]
        assert _same_running(C.record(recs[-1]), crec)


def test_in_place_equals_out_of_place():
    c = C.comp_for("fast")
    n = 2 * CHUNK + SPAN + 5
    x = R.grid_signal("gated220", n, RATE, "fast")
    for cuts in ([n], C.cut_every(n, SPAN + 1), C.cut_random(n, 3)):
        a, ra = C.RawStream(c, RATE).run(x, cuts, inplace=False)
        b, rb = C.RawStream(c, RATE).run(x, cuts, inplace=True)
        assert a.tobytes() == b.tobytes() and ra == rb


def test_a_held_length_is_honoured_and_clamped():
    c = C.comp_for("voice")
    x = R.grid_signal("gated220", SPAN + 1, RATE, "voice")
    want = C.clip_twin("voice", "gated220", SPAN + 1, RATE)[0]
    for held, n in ((40, 40), (-3, 0), (1 << 30, SPAN + 1), (SPAN, SPAN)):
        st = C.RawStream(c, RATE)
        o, raw = st.push(x, held=held)
        r = C.record(raw)
        assert r.emitted == n == r.total and o[:n].tobytes() == want[:n].tobytes()
        assert np.all(o[n:] == np.float32(2 * C.FILL)), "written behind the held length"
        o2, raw2 = st.push(x[n:], flush=True)
        assert o2[: len(x) - n].tobytes() == want[n:].tobytes() and C.record(raw2).total == len(x)


def test_argument_checks():
    L = N.lib()
    need = L.gsv_cmpstream_state_bytes()
    state = torch.zeros(need + 16, dtype=torch.uint8)
    sp = state.data_ptr()
    assert sp % 16 == 0
    err = lambda: L.gsv_last_error().decode()
    par = C.params_struct(Compressor.preset("voice"), RATE)
    assert L.gsv_cmpstream_init_host(None, need, par) == 1 and "null" in err()
    assert L.gsv_cmpstream_init_host(sp, need, None) == 1 and "null" in err()
    assert L.gsv_cmpstream_init_host(sp, need - 1, par) == 1 and "state" in err()
    assert L.gsv_cmpstream_init_host(sp + 4, need, par) == 1 and "aligned" in err()
    for field, v in (("attack", 0.0), ("attack", 1.0), ("release", float("nan")), ("release", 1.5), ("threshold", 0.0),
                     ("threshold", float("inf")), ("slope", 0.1), ("slope", -1.5), ("makeup", 0.0), ("makeup", float("inf"))):
        broken = C.params_struct(Compressor.preset("voice"), RATE)
        setattr(broken[0], field, v)
        assert L.gsv_cmpstream_init_host(sp, need, broken) == 1 and "threshold" in err(), (field, v)
    x, out = torch.full((100,), 0.5), torch.full((100,), 3.0)
    rec = torch.zeros(5, dtype=torch.int64)
    ok = [sp, x.data_ptr(), 100, None, 0, out.data_ptr(), rec.data_ptr()]
    # zeros: not a state init made -- not read through, flags -1, out not written
    assert L.gsv_cmpstream_push_host(*ok) == 0
    assert np.frombuffer(rec.numpy().tobytes(), np.int32)[:2].tolist() == [0, -1] and bool((out == 3.0).all())
    assert bool((state == 0).all())
    bad = CM.stream_record(rec.view(torch.uint8))
    assert not (bad.live or bad.compressed or bad.nonfinite or bad.nonfinite_ever) and bad.emitted == 0
    assert L.gsv_cmpstream_init_host(sp, need, par) == 0
    assert L.gsv_cmpstream_push_host(*ok) == 0
    head = np.frombuffer(rec.numpy().tobytes(), np.int32)[:2].tolist()
    assert head == [100, LIVE | COMPRESSED] and bool((out < 0.5).any()) and bool((out > 0.0).all())
    for i, wrong, word in [(0, None, "null"), (1, None, "null"), (5, None, "null"), (6, None, "null"), (2, -1, "chunk of -1"),
                           (2, (1 << 20) + 1, "chunk of"), (0, sp + 4, "aligned"), (6, rec.data_ptr() + 4, "aligned")]:
        args = list(ok)
        args[i] = wrong
        assert L.gsv_cmpstream_push_host(*args) == 1 and word in err(), (i, wrong, err())
    args = list(ok)         # an empty push needs neither chunk nor out
    args[1], args[2], args[5] = None, 0, None
    assert L.gsv_cmpstream_push_host(*args) == 0 and np.frombuffer(rec.numpy().tobytes(), np.int64)[4] == 100


def test_compress_stream_with_and_without_cuts_equals_compress():
    n = CHUNK + 77
    x = np.array(R.grid_signal("gated220", n, RATE, "voice"))
    for c in ("voice", Compressor(-30.0, 8.0, 0.5, 50.0, 6.0)):
        want, crec = CM.compress(x, RATE, c, device="cpu")
        assert crec.compressed and want.tobytes() != x.tobytes()
        for cuts in (None, [n], [0, 100, 0, SPAN, n - 100 - SPAN], C.cut_every(n, 999) + [0]):
            y, rec = CM.compress_stream(x, RATE, c, cuts=cuts)
            assert y.dtype == np.float32 and y.tobytes() == want.tobytes(), cuts
            assert rec.total == n and _same_running(rec, crec)
        y, rec = CM.compress_stream(torch.from_numpy(x), RATE, c)
        assert y.tobytes() == want.tobytes()


def test_the_identity_is_no_stream_compressor_and_issues_no_call(monkeypatch):
    """an identity compressor resolves to no stage: StreamCompressor refuses it before any library call"""
    calls = []
    real = N.lib

    def counting():
        calls.append(1)
        return real()
    monkeypatch.setattr(N, "lib", counting)
    for ident in (Compressor(ratio=1.0), Compressor(-40.0, 1.0, 5.0, 50.0, 0.0), None):
        assert CM.resolve(ident) is None
        with pytest.raises(ValueError):
            CM.StreamCompressor(ident, RATE, "cpu")
        with pytest.raises(ValueError):
            CM.compress_stream(np.zeros(8, np.float32), RATE, ident)
    assert calls == []


def test_python_entries_raise_on_what_is_no_compressor():
    x = np.zeros(8, np.float32)
    for wrong in ("radio", 3.0, [Compressor()]):
        with pytest.raises(ValueError):
            CM.StreamCompressor(wrong, RATE, "cpu")
        with pytest.raises(ValueError):
            CM.compress_stream(x, RATE, wrong)
    for rate in (3999, 768001, 32000.5, True):
        with pytest.raises(ValueError):
            CM.StreamCompressor("voice", rate, "cpu")
    for cuts in ([3, 4], [9, -1], []):
        with pytest.raises(ValueError):
            CM.compress_stream(x, RATE, "voice", cuts=cuts)
    st = CM.StreamCompressor("voice", RATE)
    assert not st.on_device and st.rec is None and isinstance(st.push_tensor(torch.zeros(5)), torch.Tensor)


def test_stream_keyword_validates(tmp_path):
    from gsv_tts import TTS
    t = TTS(models_dir=str(tmp_path), device="cpu")
    ref = ("spk.wav", "prompt.wav", "prompt.")
    for wrong in ([Compressor()], "radio", 3.0):
        with pytest.raises(ValueError, match="compress"):
            next(t.infer_stream(*ref, "text.", compress=wrong))
    for wrong in (["voice", "radio"], ["voice", 3.0], "radio"):
        with pytest.raises(ValueError, match="compress"):
            next(t.infer_stream_batched(*ref, ["one.", "two."], compress=wrong))
    with pytest.raises(ValueError, match="compress has 3 entries for 2 requests"):
        next(t.infer_stream_batched(*ref, ["one.", "two."], compress=["voice", None, "voice"]))
