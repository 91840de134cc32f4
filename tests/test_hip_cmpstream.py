"""GPU parity of the stream compressor (csrc/cmpstream.h behind gsv_cmpstream_push) against its host twin gsv_cmpstream_push_host,
which tests/test_cmpstream_cpu.py pins to the clip compressor bit for bit: the same samples and the same record bytes under the
same cuttings, nothing written behind the push's samples, the record or the stated state, a device-held length honoured, in place,
the equaliser's record as the n_dev of a compressor push, and stream.ChunkEmitter(eq=, compress=, level=, limit=, track=) driving
all five behind gsv_stream_emit.

Shapes.  The pushes of 15 to 17 samples run over the streams up to a span + a run + 1 (the run scan, the span carry and the stash
parity under many pushes); the coarse cuttings run up to two chunks + a span + 5 (both chains, a push that completes two chunks at
once, several blocks).  The signal is the gated tone, whose attacks and releases cross the span and chunk edges."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compressor_ref as R  # noqa: E402
import cmpstream_cases as C  # noqa: E402

from oracle.gen_golden_inputs import facade_audio  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import compressor as CM  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402

pytestmark = pytest.mark.gpu

RUN, SPAN, CHUNK = C.RUN, C.SPAN, C.CHUNK
RATE = 32000
FINE_MAX = SPAN + RUN + 1
LENGTHS = C.LENGTHS[:3] + (SPAN + 1, FINE_MAX) + C.LENGTHS[4:]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cuttings(n):
    """the contract's cuttings without the pushes of about a run over more than a run + 1 (the test below), and a stretch of
    run-sized pushes across the first span edge and the first chunk edge"""
    res = [[n]] + C.cuttings(n, fine=n <= RUN + 1)
    for edge in (SPAN, CHUNK):
        if n > edge + 40:
            res.append([edge - 40] + [RUN - 1, RUN, RUN + 1, RUN, RUN + 1] + [n - (edge - 40) - (5 * RUN + 1)])
    return res


def _both(d, h, x, cuts, inplace, want, what):
    yd, rd = d.run(x, cuts, inplace=inplace)
    yh, rh = h.run(x, cuts, inplace=inplace)
    assert yd.tobytes() == yh.tobytes() == want.tobytes(), what
    assert rd == rh, what


@pytest.mark.parametrize("name", list(R.SETS))
def test_device_samples_and_records_equal_the_host_twin(dev, name):
    c = C.comp_for(name)
    d, h = C.RawStream(c, RATE, dev), C.RawStream(c, RATE, "cpu")
    for n in LENGTHS:
        x = R.grid_signal("gated220", n, RATE, name)
        want, crec = C.clip_twin(name, "gated220", n, RATE)
        for j, cuts in enumerate(_cuttings(n)):
            _both(d, h, x, cuts, bool(j & 1), want, (name, n, cuts[:8]))
        assert n <= CHUNK or crec.compressed


@pytest.mark.parametrize("step", C.FINE)
@pytest.mark.parametrize("n", (SPAN + 1, FINE_MAX))
def test_pushes_of_about_a_run(dev, n, step):
    """a few hundred pushes of 15, 16 or 17 samples, each of which reruns the open chunk: the run scan, the span carry (the longer
    stream) and the stash's two copies used in turn"""
    c = C.comp_for("voice")
    d, h = C.RawStream(c, RATE, dev), C.RawStream(c, RATE, "cpu")
    x = R.grid_signal("gated220", n, RATE, "voice")
    want, crec = C.clip_twin("voice", "gated220", n, RATE)
    _both(d, h, x, C.cut_every(n, step), step == RUN, want, (n, step))
    assert crec.compressed


@pytest.mark.parametrize("kind", ("noise", "square", "quiet"))
def test_the_other_signal_kinds(dev, kind):
    c = C.comp_for("voice")
    d, h = C.RawStream(c, RATE, dev), C.RawStream(c, RATE, "cpu")
    n = 2 * CHUNK + SPAN + 5
    x = R.grid_signal(kind, n, RATE, "voice")
    want = C.clip_twin("voice", kind, n, RATE)[0]
    for j, cuts in enumerate(([n], C.cut_every(n, SPAN + 1), C.cut_every(n, CHUNK - 1), C.cut_random(n, 9))):
        yd, rd = d.run(x, cuts, inplace=bool(j & 1))
        yh, rh = h.run(x, cuts, inplace=bool(j & 1))
        assert yd.tobytes() == yh.tobytes() == want.tobytes() and rd == rh, (kind, cuts[:8])


def test_a_signal_with_samples_that_are_not_finite(dev):
    c = C.comp_for("voice")
    n = 2 * CHUNK + 3
    x = np.array(R.grid_signal("gated220", n, RATE, "voice"))
    for at, v in ((5, np.nan), (RUN, np.inf), (SPAN - 1, -np.inf), (CHUNK - 1, np.inf), (CHUNK, -np.nan), (CHUNK + SPAN + 7, -np.inf),
                  (2 * CHUNK, np.nan)):
        x[at] = v
    d, h = C.RawStream(c, RATE, dev), C.RawStream(c, RATE, "cpu")
    for j, cuts in enumerate([[n], C.cut_every(n, SPAN), C.cut_every(n, CHUNK - 1), C.cut_random(n, 5)]):
        yd, rd = d.run(x, cuts, inplace=bool(j & 1))
        yh, rh = h.run(x, cuts, inplace=bool(j & 1))
        assert yd.tobytes() == yh.tobytes() and rd == rh, cuts[:8]
    last = C.record(rd[-1])
    assert last.nonfinite_ever and last.min_gain_run < 1


def test_denormals(dev):
    x, co = R.denormal_clip()
    x = np.array(x)
    for cuts in ([len(x)], C.cut_every(len(x), 1000)):
        d = C.RawStream(None, R.DENORMAL["rate"], dev, coefficients=np.array(co, np.float64))
        h = C.RawStream(None, R.DENORMAL["rate"], "cpu", coefficients=np.array(co, np.float64))
        yd, rd = d.run(x, cuts)
        yh, rh = h.run(x, cuts)
        assert yd.tobytes() == yh.tobytes() and rd == rh


def test_a_device_held_length_is_honoured(dev):
    c = C.comp_for("voice")
    x = R.grid_signal("gated220", CHUNK + 1, RATE, "voice")
    want = C.clip_twin("voice", "gated220", CHUNK + 1, RATE)[0]
    for held, n in ((40, 40), (-3, 0), (1 << 30, CHUNK + 1), (SPAN + 3, SPAN + 3)):
        for inplace in (False, True):
            st = C.RawStream(c, RATE, dev)
            o, raw = st.push(x, held=held, inplace=inplace)
            r = C.record(raw)
            assert r.emitted == n == r.total and o[:n].tobytes() == want[:n].tobytes()
            # nothing behind the held length is written: in place the samples stay, out of place the fill
            assert o[n: len(x)].tobytes() == (x[n:] if inplace else np.full(len(x) - n, 2 * C.FILL, np.float32)).tobytes()
            o2, raw2 = st.push(x[n:], flush=True)
            assert o2[: len(x) - n].tobytes() == want[n:].tobytes() and C.record(raw2).total == len(x)


def test_device_argument_checks(dev):
    L = N.lib()
    need = L.gsv_cmpstream_state_bytes()
    state = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    st = N.current_stream_ptr(dev)
    par = C.params_struct(CM.Compressor.preset("voice"), RATE)
    broken = C.params_struct(CM.Compressor.preset("voice"), RATE)
    broken[0].slope = 0.5
    out, x = torch.full((10,), C.FILL, device=dev), torch.zeros(10, device=dev)
    rec = torch.zeros(5, dtype=torch.int64, device=dev)
    sp = state.data_ptr()
    bad = [L.gsv_cmpstream_init(None, need, par, st), L.gsv_cmpstream_init(sp, need, None, st), L.gsv_cmpstream_init(sp, need - 1, par, st),
           L.gsv_cmpstream_init(sp + 4, need, par, st), L.gsv_cmpstream_init(sp, need, broken, st),
           L.gsv_cmpstream_push(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp, None, 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp, x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp, x.data_ptr(), (1 << 20) + 1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp, x.data_ptr(), 10, None, 0, None, rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp + 4, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_cmpstream_push(sp, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr() + 4, st),
           L.gsv_cmpstream_push(sp, x.data_ptr(), 10, None, 0, out.data_ptr(), None, st)]
    assert bad == [1] * len(bad), bad
    # a state nobody initialised is not read through: the record says so and `out` stays as it was
    assert L.gsv_cmpstream_push(sp, x.data_ptr(), 10, None, 1, out.data_ptr(), rec.data_ptr(), st) == 0
    assert rec.cpu().numpy().view(np.int32)[:2].tolist() == [0, -1] and bool((out == C.FILL).all())
    assert bool((state == 0).all())


def test_the_equalisers_record_is_the_length_of_a_compressor_push(dev):
    """eq -> compress (both in place) on the device, the compressor reading its length from the equaliser's record with no host
    read between, and a level push reading the compressor's: the host chain's bytes"""
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd import level as LV
    x = np.array(R.grid_signal("gated220", CHUNK + 1, RATE, "voice"))
    cuts = [30, 1000, 0, SPAN, len(x) - 1030 - SPAN]
    e = EQM.EQ.preset("voice", RATE)
    lv = lambda d: StreamLeveller(-20.0, RATE, d, seed=-12.0)
    se, sc, sl = EQM.StreamEQ(e, RATE, dev), CM.StreamCompressor("voice", RATE, dev), lv(dev)
    he, hc, hl = EQM.StreamEQ(e, RATE, "cpu"), CM.StreamCompressor("voice", RATE, "cpu"), lv("cpu")
    xd, at = torch.from_numpy(x).to(dev), 0
    same = lambda p, q: all(getattr(p, f) == getattr(q, f) for f in CM.CmpStreamRecord.__slots__)
    for k, n in enumerate(cuts):
        flush = k + 1 == len(cuts)
        cap = n + 8                                      # the stages behind see a capacity above the real length
        buf = torch.full((cap,), 3.0e38, device=dev)
        buf[:n] = xd[at: at + n]
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        erec = torch.zeros(4, dtype=torch.int64, device=dev)
        crec = torch.zeros(5, dtype=torch.int64, device=dev)
        lrec = torch.zeros(LV.RECORD_BYTES // 8 + 1, dtype=torch.int64, device=dev)
        se.enqueue(buf.data_ptr(), cap, n_dev.data_ptr(), flush, buf.data_ptr(), erec.data_ptr())
        sc.enqueue(buf.data_ptr(), cap, erec.data_ptr(), flush, buf.data_ptr(), crec.data_ptr())
        mid = buf.clone()
        sl.enqueue(buf.data_ptr(), cap, crec.data_ptr(), flush, buf.data_ptr(), lrec.data_ptr())
        squeezed = hc.push(he.push(x[at: at + n], flush), flush)
        levelled = hl.push(squeezed, flush)
        got_mid, got = mid.cpu().numpy(), buf.cpu().numpy()
        assert got_mid[:n].tobytes() == squeezed.tobytes() and np.all(got_mid[n:] == np.float32(3.0e38)), k
        assert got[:n].tobytes() == levelled.tobytes() and np.all(got[n:] == np.float32(3.0e38)), k
        assert same(CM.stream_record(crec.view(torch.uint8)), hc.rec), k
        at += n
    assert hc.rec.min_gain_run < 1 and hc.rec.total == len(x)


def _emitter_jobs(emitters, dev):
    """the five-chunk signal of tests/test_hip_limstream.py's emitter test and a second segment through every emitter"""
    ov, n_chunk, mute = 640, 6400, 1234
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    sm[:4000] *= 0.01
    jobs, pos, shifts = [], 0, [0, 13, 200, 0, 77]
    for c, sh in enumerate(shifts):
        final = c == len(shifts) - 1
        start = pos - sh if c else 0
        chunk = torch.from_numpy(sm[start: start + n_chunk].copy()).to(dev)
        kw = dict(trim_head=c == 0, mute_samples=mute if final else 0)
        jobs.append(([e.push(chunk[None, None], final, flush=False, **kw) for e in emitters], False))
        pos = start + n_chunk if final else start + n_chunk - ov
    for e in emitters:
        e.new_segment()
    silent = torch.zeros(3000, device=dev)
    jobs.append(([e.push(silent, False, trim_head=True) for e in emitters], False))
    last = torch.from_numpy(sm[5000: 5000 + n_chunk].copy()).to(dev)
    jobs.append(([e.push(last, True, mute_samples=mute, flush=True) for e in emitters], True))
    return jobs


def test_chunk_emitter_with_all_five_stages(dev):
    """the samples are the plain emitter's, equalised, compressed, levelled and limited push by push on the host in that order, the
    packets those of the limited samples; with the compressor alone the clips keep their lengths"""
    from gsv_tts_lite_amd import limiter as LM
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    ov = 640
    fmt = TrackFormat(48000, 1, 20)
    e = EQM.EQ([EQM.Band("highpass", 80.0), EQM.Band("peak", 300.0, q=1.0, gain_db=9.0)])
    c = CM.Compressor(-30.0, 4.0, 1.0, 100.0, 3.0)
    lv = lambda d: StreamLeveller(-10.0, RATE, d, seed=-30.0, peak_limit=float("inf"))
    plain = ChunkEmitter(ov)
    only = ChunkEmitter(ov, compress=CM.StreamCompressor(c, RATE, dev))
    full = ChunkEmitter(ov, track=TrackResampler(fmt, RATE, dev), level=lv(dev), limit=LM.StreamLimiter(-6.0, RATE, dev),
                        eq=EQM.StreamEQ(e, RATE, dev), compress=CM.StreamCompressor(c, RATE, dev))
    h_c, h_eq, h_c2, h_level, h_lim, h_track = CM.StreamCompressor(c, RATE, "cpu"), EQM.StreamEQ(e, RATE, "cpu"), \
        CM.StreamCompressor(c, RATE, "cpu"), lv("cpu"), LM.StreamLimiter(-6.0, RATE, "cpu"), TrackResampler(fmt, RATE, "cpu")
    same = lambda p, q, cls: all(getattr(p, f) == getattr(q, f) for f in cls.__slots__)
    total = 0
    for i, ((hp, ho, hf), flush) in enumerate(_emitter_jobs((plain, only, full), dev)):
        a, b, d = hp.result(), ho.result(), hf.result()
        assert len(a) == 3 and len(b) == 3 and len(d) == 4 and hp.comp is None
        assert a[1:] == b[1:] == d[1:3]
        want = h_c.push(a[0], flush)
        assert b[0].dtype == np.float32 and b[0].tobytes() == want.tobytes() and same(ho.comp, h_c.rec, CM.CmpStreamRecord), (i, ho.comp, h_c.rec)
        assert ho.level is None and ho.limit is None and ho.eq is None
        want2 = h_lim.push(h_level.push(h_c2.push(h_eq.push(a[0], flush), flush), flush), flush)
        assert d[0].tobytes() == want2.tobytes(), i
        assert same(hf.eq, h_eq.rec, EQM.EqStreamRecord) and same(hf.comp, h_c2.rec, CM.CmpStreamRecord), (i, hf.comp, h_c2.rec)
        assert same(hf.limit, h_lim.rec, LM.StreamLimiterRecord) and hf.level.gain_last == h_level.rec.gain_last
        assert np.array_equal(d[3], h_track.push(want2, flush)), i
        total += len(a[0])
        assert ho.comp.total == hf.comp.total == total          # one stream over both segments
    assert h_c.rec.min_gain_run < 1 and h_c.rec.total == total


def test_chunk_emitter_without_a_compressor_is_what_it_was(dev):
    """compress=None against the emitter constructed without the argument: the same places in the buffer, the same records and bytes"""
    from gsv_tts_lite_amd import limiter as LM
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    fmt = TrackFormat(48000, 1, 20)
    e = EQM.EQ.preset("voice", RATE)
    make = lambda **kw: ChunkEmitter(640, track=TrackResampler(fmt, RATE, dev), level=StreamLeveller(-10.0, RATE, dev, seed=-30.0),
                                     limit=LM.StreamLimiter(-6.0, RATE, dev), eq=EQM.StreamEQ(e, RATE, dev), **kw)
    for (ha, hb), _ in _emitter_jobs((make(), make(compress=None)), dev):
        assert (ha._pcm_at, ha._level_at, ha._limit_at, ha._eq_at, ha._comp_at) == (hb._pcm_at, hb._level_at, hb._limit_at, hb._eq_at, None)
        ha._event.synchronize()
        hb._event.synchronize()
        end = ha._pcm_at + 4        # the records and the samples in front of the packets: every byte the copy carried
        used_a, used_b = ha._bufs[1][:end].clone(), hb._bufs[1][:end].clone()
        a, b = ha.result(), hb.result()
        n, at = len(a[0]), ha._limit_at
        for lo, hi in ((0, 4), (ha._eq_at, ha._eq_at + 8), (ha._level_at, ha._level_at + 10), (at, at + 8 + n), (ha._pcm_at, end)):
            assert used_a[lo:hi].numpy().tobytes() == used_b[lo:hi].numpy().tobytes(), (lo, hi)
        assert a[0].tobytes() == b[0].tobytes() and a[1:3] == b[1:3] and np.array_equal(a[3], b[3])
        assert ha.comp is None and hb.comp is None
    bare = ChunkEmitter(640)
    assert bare.compress is None and bare.push(torch.zeros(3000, device=dev), True)._comp_at is None
