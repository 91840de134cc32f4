"""GPU parity of the stream equaliser (csrc/eqstream.h behind gsv_eqstream_push) against its host twin gsv_eqstream_push_host,
which tests/test_eqstream_cpu.py pins to the clip equaliser bit for bit: the same samples and the same record bytes under the same
cuttings, nothing written behind the push's samples, the record or the stated state, a device-held length honoured, in place, the
record as the n_dev of a level and of a track push, and stream.ChunkEmitter(eq=, level=, limit=, track=) driving all four behind
gsv_stream_emit.

Shapes: 1 sample, a run + 1, a span + 1, a chunk + 1 (the first push that completes a chunk: the pass from zero state and the
chain) and three chunks + 5 (several blocks, a push that completes two chunks at once) with 1, 3 and 6 sections."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_ref as R  # noqa: E402
import eqstream_cases as C  # noqa: E402

from oracle.gen_golden_inputs import facade_audio  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402

pytestmark = pytest.mark.gpu

RUN, SPAN, CHUNK = C.RUN, C.SPAN, C.CHUNK
RATE = 32000
LENGTHS = (1, RUN + 1, SPAN + 1, CHUNK + 1, 3 * CHUNK + 5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cuttings(n):
    """the contract's cuttings, the pushes of about a run only where they are a few hundred at the most"""
    res = [[n]] + C.cuttings(n, fine=n <= SPAN + 1)
    if n > SPAN + 1:        # a stretch of run-sized pushes across the first span edge and the first chunk edge
        for edge in (SPAN, CHUNK):
            if n > edge + 40:
                res.append([edge - 40] + [RUN - 1, RUN, RUN + 1, RUN, RUN + 1] + [n - (edge - 40) - (5 * RUN + 1)])
    return res


@pytest.mark.parametrize("count", (1, 3, 6))
def test_device_samples_and_records_equal_the_host_twin(dev, count):
    e = C.eq_for(count, RATE)
    d, h = C.RawStream(e, RATE, dev), C.RawStream(e, RATE, "cpu")
    for n in LENGTHS:
        x = R.grid_signal("noise", n, RATE)
        want = C.clip_twin(count, "noise", n, RATE)[0]
        for j, cuts in enumerate(_cuttings(n)):
            inplace = bool(j & 1)
            yd, rd = d.run(x, cuts, inplace=inplace)
            yh, rh = h.run(x, cuts, inplace=inplace)
            assert yd.tobytes() == yh.tobytes() == want.tobytes(), (count, n, cuts[:8])
            assert rd == rh, (count, n, cuts[:8])


def test_a_signal_with_samples_that_are_not_finite(dev):
    e = C.eq_for(3, RATE)
    n = 2 * CHUNK + 3
    x = np.random.default_rng(11).uniform(-1.0, 1.0, n).astype(np.float32)
    for at, v in ((5, np.nan), (CHUNK - 1, np.inf), (CHUNK, -np.nan), (CHUNK + SPAN + 7, -np.inf), (2 * CHUNK, np.nan)):
        x[at] = v
    d, h = C.RawStream(e, RATE, dev), C.RawStream(e, RATE, "cpu")
    for j, cuts in enumerate([[n], C.cut_every(n, SPAN), C.cut_every(n, CHUNK - 1), C.cut_random(n, 5)]):
        yd, rd = d.run(x, cuts, inplace=bool(j & 1))
        yh, rh = h.run(x, cuts, inplace=bool(j & 1))
        assert yd.tobytes() == yh.tobytes() and rd == rh, cuts[:8]
    assert C.record(rd[-1]).nonfinite_ever


def test_a_device_held_length_is_honoured(dev):
    e = C.eq_for(3, RATE)
    x = R.grid_signal("noise", CHUNK + 1, RATE)
    want = C.clip_twin(3, "noise", CHUNK + 1, RATE)[0]
    for held, n in ((40, 40), (-3, 0), (1 << 30, CHUNK + 1), (SPAN + 3, SPAN + 3)):
        for inplace in (False, True):
            st = C.RawStream(e, RATE, dev)
            o, raw = st.push(x, held=held, inplace=inplace)
            r = C.record(raw)
            assert r.emitted == n == r.total and o[:n].tobytes() == want[:n].tobytes()
            # nothing behind the held length is written: in place the samples stay, out of place the fill
            assert o[n: len(x)].tobytes() == (x[n:] if inplace else np.full(len(x) - n, 2 * C.FILL, np.float32)).tobytes()
            o2, raw2 = st.push(x[n:], flush=True)
            assert o2[: len(x) - n].tobytes() == want[n:].tobytes() and C.record(raw2).total == len(x)


def test_device_argument_checks(dev):
    L = N.lib()
    need = L.gsv_eqstream_state_bytes()
    state = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    st = N.current_stream_ptr(dev)
    des = C.design_struct(EQM.EQ.preset("voice", RATE), RATE)
    broken = C.design_struct(EQM.EQ.preset("voice", RATE), RATE)
    broken[0].coef[0][4] = 1.0
    out, x = torch.full((10,), C.FILL, device=dev), torch.zeros(10, device=dev)
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    sp = state.data_ptr()
    bad = [L.gsv_eqstream_init(None, need, des, st), L.gsv_eqstream_init(sp, need, None, st), L.gsv_eqstream_init(sp, need - 1, des, st),
           L.gsv_eqstream_init(sp + 4, need, des, st), L.gsv_eqstream_init(sp, need, broken, st),
           L.gsv_eqstream_push(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_eqstream_push(sp, None, 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_eqstream_push(sp, x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_eqstream_push(sp, x.data_ptr(), (1 << 20) + 1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_eqstream_push(sp, x.data_ptr(), 10, None, 0, None, rec.data_ptr(), st),
           L.gsv_eqstream_push(sp + 4, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_eqstream_push(sp, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr() + 4, st),
           L.gsv_eqstream_push(sp, x.data_ptr(), 10, None, 0, out.data_ptr(), None, st)]
    assert bad == [1] * len(bad), bad
    # a state nobody initialised is not read through: the record says so and `out` stays as it was
    assert L.gsv_eqstream_push(sp, x.data_ptr(), 10, None, 1, out.data_ptr(), rec.data_ptr(), st) == 0
    assert rec.cpu().numpy().view(np.int32)[:2].tolist() == [0, -1] and bool((out == C.FILL).all())
    assert bool((state == 0).all())


def test_the_record_is_the_length_of_a_level_and_of_a_track_push(dev):
    """eq -> level (in place) -> track on the device, each reading its length from the equaliser's record: the host chain's bytes"""
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    fmt = TrackFormat(48000, 2, 20)
    x = R.grid_signal("noise", CHUNK + 1, RATE)
    cuts = [30, 1000, 0, SPAN, len(x) - 1030 - SPAN]
    e = C.eq_for(3, RATE)
    lv = lambda d: StreamLeveller(-20.0, RATE, d, seed=-12.0)
    se, sl, tr = EQM.StreamEQ(e, RATE, dev), lv(dev), TrackResampler(fmt, RATE, dev)
    he, hl, ht = EQM.StreamEQ(e, RATE, "cpu"), lv("cpu"), TrackResampler(fmt, RATE, "cpu")
    xd, at = torch.from_numpy(x).to(dev), 0
    from gsv_tts_lite_amd import level as LV
    for k, n in enumerate(cuts):
        flush = k + 1 == len(cuts)
        cap = n + 8                                      # the stages behind see a capacity above the real length
        buf = torch.full((cap,), 3.0e38, device=dev)
        buf[:n] = xd[at: at + n]
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        rec = torch.zeros(4, dtype=torch.int64, device=dev)
        lrec = torch.zeros(LV.RECORD_BYTES // 8 + 1, dtype=torch.int64, device=dev)
        pcm = torch.full((tr.capacity(cap),), 0x5A5A, dtype=torch.int16, device=dev)
        trec = torch.zeros(4, dtype=torch.int32, device=dev)
        se.enqueue(buf.data_ptr(), cap, n_dev.data_ptr(), flush, buf.data_ptr(), rec.data_ptr())
        sl.enqueue(buf.data_ptr(), cap, rec.data_ptr(), flush, buf.data_ptr(), lrec.data_ptr())
        tr.enqueue(buf.data_ptr(), cap, rec.data_ptr(), flush, pcm.data_ptr(), trec.data_ptr())
        levelled = hl.push(he.push(x[at: at + n], flush), flush)
        want = ht.push(levelled, flush)
        got = buf.cpu().numpy()
        assert got[:n].tobytes() == levelled.tobytes() and np.all(got[n:] == np.float32(3.0e38)), k
        r = EQM.stream_record(rec.view(torch.uint8))
        assert (r.emitted, r.total, r.peak_out_run) == (he.rec.emitted, he.rec.total, he.rec.peak_out_run)
        packets = trec.tolist()[0]
        assert trec.tolist() == list(ht.rec) and packets == want.shape[0], (k, trec.tolist(), ht.rec)
        width = fmt.packet * fmt.channels
        assert np.array_equal(pcm.cpu().numpy()[: packets * width].reshape(packets, width), want), k
        at += n


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


def test_chunk_emitter_with_equaliser_leveller_limiter_and_track(dev):
    """the samples are the plain emitter's, equalised, levelled and limited push by push on the host in that order, the packets
    those of the limited samples; with the equaliser alone the clips keep their lengths"""
    from gsv_tts_lite_amd import limiter as LM
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    ov = 640
    fmt = TrackFormat(48000, 1, 20)
    e = EQM.EQ([EQM.Band("highpass", 80.0), EQM.Band("peak", 300.0, q=1.0, gain_db=9.0)])
    lv = lambda d: StreamLeveller(-10.0, RATE, d, seed=-30.0, peak_limit=float("inf"))
    plain = ChunkEmitter(ov)
    only = ChunkEmitter(ov, eq=EQM.StreamEQ(e, RATE, dev))
    full = ChunkEmitter(ov, track=TrackResampler(fmt, RATE, dev), level=lv(dev), limit=LM.StreamLimiter(-6.0, RATE, dev),
                        eq=EQM.StreamEQ(e, RATE, dev))
    h_eq, h_eq2, h_level, h_lim, h_track = EQM.StreamEQ(e, RATE, "cpu"), EQM.StreamEQ(e, RATE, "cpu"), lv("cpu"), \
        LM.StreamLimiter(-6.0, RATE, "cpu"), TrackResampler(fmt, RATE, "cpu")
    same = lambda p, q, cls: all(getattr(p, f) == getattr(q, f) for f in cls.__slots__)
    total = 0
    for i, ((hp, ho, hf), flush) in enumerate(_emitter_jobs((plain, only, full), dev)):
        a, b, c = hp.result(), ho.result(), hf.result()
        assert len(a) == 3 and len(b) == 3 and len(c) == 4 and hp.eq is None
        assert a[1:] == b[1:] == c[1:3]
        want = h_eq.push(a[0], flush)
        assert b[0].dtype == np.float32 and b[0].tobytes() == want.tobytes() and same(ho.eq, h_eq.rec, EQM.EqStreamRecord), (i, ho.eq, h_eq.rec)
        assert ho.level is None and ho.limit is None
        want2 = h_lim.push(h_level.push(h_eq2.push(a[0], flush), flush), flush)
        assert c[0].tobytes() == want2.tobytes(), i
        assert same(hf.eq, h_eq2.rec, EQM.EqStreamRecord) and same(hf.limit, h_lim.rec, LM.StreamLimiterRecord), (i, hf.eq, h_eq2.rec)
        assert hf.level.gain_last == h_level.rec.gain_last
        assert np.array_equal(c[3], h_track.push(want2, flush)), i
        total += len(a[0])
        assert ho.eq.total == hf.eq.total == total          # one stream over both segments
    assert h_lim.rec.limited_ever and h_eq.rec.total == total


def test_chunk_emitter_without_an_equaliser_is_what_it_was(dev):
    """eq=None against the emitter constructed without the argument: the same places in the buffer, the same records and bytes"""
    from gsv_tts_lite_amd import limiter as LM
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    fmt = TrackFormat(48000, 1, 20)
    make = lambda **kw: ChunkEmitter(640, track=TrackResampler(fmt, RATE, dev), level=StreamLeveller(-10.0, RATE, dev, seed=-30.0),
                                     limit=LM.StreamLimiter(-6.0, RATE, dev), **kw)
    for (ha, hb), _ in _emitter_jobs((make(), make(eq=None)), dev):
        assert (ha._pcm_at, ha._level_at, ha._limit_at, ha._eq_at) == (hb._pcm_at, hb._level_at, hb._limit_at, None)
        ha._event.synchronize()
        hb._event.synchronize()
        end = ha._pcm_at + 4        # the records and the samples in front of the packets: every byte the copy carried
        used_a, used_b = ha._bufs[1][:end].clone(), hb._bufs[1][:end].clone()
        a, b = ha.result(), hb.result()
        n, at = len(a[0]), ha._limit_at
        for lo, hi in ((0, 4), (ha._level_at, ha._level_at + 10), (at, at + 8 + n), (ha._pcm_at, end)):
            assert used_a[lo:hi].numpy().tobytes() == used_b[lo:hi].numpy().tobytes(), (lo, hi)
        assert a[0].tobytes() == b[0].tobytes() and a[1:3] == b[1:3] and np.array_equal(a[3], b[3])
        assert ha.eq is None and hb.eq is None
    bare = ChunkEmitter(640)
    assert bare.eq is None and bare.push(torch.zeros(3000, device=dev), True)._eq_at is None
