"""GPU parity of the stream limiter (csrc/limstream.h behind gsv_limstream_push) against its host twin gsv_limstream_push_host, which
tests/test_limstream_cpu.py pins to the clip limiter and to the fp64 definition: the same samples and the same record bytes for the
same chunking, nothing written behind `out`'s capacity or behind what the record names, a device-held length honoured, the record
as the n_dev of a track push, and stream.ChunkEmitter(level=, limit=, track=) driving all three behind gsv_stream_emit.

Shapes: 4 tiles + 47 samples (the release chained over several tiles), a tile + 1, 97 (single-sample pushes), 13, 1 and 0 at the
default 48 / 66-sample look-aheads, where a block redoes one tile in front of its own; and look-aheads of 1500 and 4096 samples,
where it redoes two and up to five and the hold's halo is longer than a tile."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as R  # noqa: E402
import limstream_ref as SR  # noqa: E402

from oracle.gen_golden_inputs import facade_audio  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = LM.TILE
GUARD = 16
FILL = -7.25
CEILING = -1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _Raw:
    """the raw device calls on one state, with guard words behind `out`'s capacity and behind the emitted samples checked after
    every push"""

    def __init__(self, dev, rate, **kw):
        self.lm = LM.StreamLimiter(CEILING, rate, dev, **kw)
        self.dev = dev

    def push(self, chunk, n_cap, flush, n_dev=None):
        """chunk: device fp32 with at least n_cap samples -> (samples, the record's bytes)"""
        cap = int(N.lib().gsv_limstream_out_capacity(n_cap, self.lm.lookahead))
        assert cap == n_cap + self.lm.delay
        out = torch.full((cap + GUARD,), FILL, dtype=torch.float32, device=self.dev)
        rec = torch.full((4 + 2,), -5, dtype=torch.int64, device=self.dev)
        self.lm.enqueue(chunk.data_ptr() if n_cap else 0, n_cap, None if n_dev is None else n_dev.data_ptr(), flush, out.data_ptr(),
                        rec.data_ptr())
        rec, out = rec.cpu().numpy(), out.cpu().numpy()
        assert np.all(rec[4:] == -5), "written behind the record"
        raw = rec[:4].view(np.uint8)
        emitted = LM.stream_record(raw).emitted
        assert 0 <= emitted <= cap and np.all(out[emitted:] == np.float32(FILL)), "written behind what the record names"
        return out[:emitted], raw.tobytes()


def _host(x, rate, cuts, **kw):
    lm = LM.StreamLimiter(CEILING, rate, "cpu", **kw)
    got, at = [], 0
    for k, n in enumerate(cuts):
        y = lm.push(x[at: at + n], flush=k + 1 == len(cuts))
        got.append((y, lm.rec))
        at += n
    return got


def _host_bytes(x, rate, cuts, **kw):
    """the host twin through the raw call, so that the record's bytes can be compared"""
    lm = LM.StreamLimiter(CEILING, rate, "cpu", **kw)
    L, got, at = N.lib(), [], 0
    for k, n in enumerate(cuts):
        chunk = torch.from_numpy(np.ascontiguousarray(x[at: at + n]))
        out = torch.zeros(n + lm.delay)
        rec = torch.zeros(4, dtype=torch.int64)
        N.check(L.gsv_limstream_push_host(lm.state.data_ptr(), chunk.data_ptr() or None, n, None, int(k + 1 == len(cuts)),
                                          out.data_ptr(), rec.data_ptr()))
        raw = rec.numpy().view(np.uint8)
        got.append((out.numpy()[: LM.stream_record(raw).emitted].copy(), raw.tobytes()))
        at += n
    return got


def _compare(dev, x, rate, cuts, what, **kw):
    want = _host_bytes(x, rate, cuts, **kw)
    raw, xd, at = _Raw(dev, rate, **kw), torch.from_numpy(x).to(dev), 0
    limited = False
    for k, (n, (wy, wrec)) in enumerate(zip(cuts, want)):
        got, rec = raw.push(xd[at: at + n], n, k + 1 == len(cuts))
        assert rec == wrec, (what, k, at, n, LM.stream_record(np.frombuffer(rec, np.uint8)), LM.stream_record(np.frombuffer(wrec, np.uint8)))
        assert got.tobytes() == wy.tobytes(), (what, k, at, n)
        limited = limited or LM.stream_record(np.frombuffer(rec, np.uint8)).limited
        at += n
    return limited


@pytest.mark.parametrize("rate", [32000, 44100])
def test_device_samples_and_records_equal_the_host_twin(dev, rate):
    D = LM.times(rate)[0] + 5
    n = 4 * TILE + 47
    acted = 0
    for kind in ("sine997", "noise", "click_tile", "nan", "quiet"):
        x = R.grid_signal(kind, n, rate)
        plans = [[n], SR.cut_every(n, D - 1), SR.cut_every(n, D + 1), SR.cut_every(n, TILE - 1), SR.cut_every(n, TILE),
                 SR.cut_every(n, TILE + 1), SR.cut_random(n, 11), SR.cut_random(n, 12), SR.cut_every(n, 700) + [0]]
        if kind not in ("sine997", "nan"):
            plans = plans[:1] + plans[3:7]
        for cuts in plans:
            acted += _compare(dev, x, rate, cuts, (rate, kind, cuts[:6]))
    assert acted >= 20           # the limiter was at work: the comparison is not one of copies
    for m, kind in ((TILE + 1, "click_last"), (97, "noise"), (97, "click_first"), (13, "sine997"), (1, "click_first"), (0, "zeros")):
        x = R.grid_signal(kind, m, rate)
        for cuts in ([m], SR.cut_every(m, 1), SR.cut_every(m, D), SR.cut_random(m, 5)):
            _compare(dev, x, rate, cuts, (rate, kind, m, cuts[:6]))


@pytest.mark.parametrize("lookahead_ms,release_ms", [(1500 / 32.0, 20.0), (128.0, 100.0), (0.0, 0.0)])
def test_long_and_shortest_lookaheads(dev, lookahead_ms, release_ms):
    rate, n = 32000, 6 * TILE + 5
    kw = dict(lookahead_ms=lookahead_ms, release_ms=release_ms)
    L = LM.times(rate, **kw)[0]
    assert L in (1500, 4096, 1)
    for kind in ("noise", "click_tile"):
        x = R.grid_signal(kind, n, rate)
        acted = 0
        for cuts in ([n], SR.cut_every(n, TILE + 1), SR.cut_every(n, L + 4), SR.cut_random(n, 3), [3000, 0, 2000, n - 5000, 0]):
            acted += _compare(dev, x, rate, cuts, (L, kind, cuts[:6]), **kw)
        assert acted == 5


def test_a_typical_chunk_and_a_second_stream_through_the_same_state(dev):
    rate = 32000
    x = np.concatenate([R.grid_signal("sine997", 16000, rate), R.grid_signal("noise", 16000, rate), R.grid_signal("quiet", 8000, rate)])
    want = _host(x, rate, [16000, 16000, 8000])
    lm = LM.StreamLimiter(CEILING, rate, dev)
    for rep in range(2):        # the flush left the state fresh
        at = 0
        for k, (n, (wy, wrec)) in enumerate(zip([16000, 16000, 8000], want)):
            got = lm.push(x[at: at + n], flush=k == 2)
            assert got.tobytes() == wy.tobytes(), (rep, k)
            assert all(getattr(lm.rec, f) == getattr(wrec, f) for f in LM.StreamLimiterRecord.__slots__), (rep, k, lm.rec, wrec)
            at += n
    y, rec = LM.limit_stream(torch.from_numpy(x).to(dev), rate, CEILING)
    assert y.tobytes() == np.concatenate([w[0] for w in want]).tobytes() and rec.limited and rec.total == len(x)


def test_a_device_held_length_is_honoured(dev):
    rate = 32000
    x = R.grid_signal("sine997", 2000, rate)
    lengths = [613, 0, 1, 700, 686]                       # the real lengths; every call names a capacity of 700
    assert sum(lengths) == 2000
    want = _host_bytes(x, rate, lengths)
    raw, at = _Raw(dev, rate), 0
    for k, (n, (wy, wrec)) in enumerate(zip(lengths, want)):
        chunk = np.full(700, np.float32(3.0e38))            # poison behind the real length
        chunk[n:][::2] = np.nan
        chunk[:n] = x[at: at + n]
        n_dev = torch.tensor([n, 12345, -7, 99], dtype=torch.int32, device=dev)
        got, rec = raw.push(torch.from_numpy(chunk).to(dev), 700, k == len(lengths) - 1, n_dev)
        assert rec == wrec and got.tobytes() == wy.tobytes(), (at, n)
        at += n
    # a length past the capacity is the capacity; a negative one is 0
    a, _ = raw.push(torch.from_numpy(x[:700].copy()).to(dev), 700, True, torch.tensor([100000], dtype=torch.int32, device=dev))
    assert a.tobytes() == _host_bytes(x[:700], rate, [700])[0][0].tobytes()
    z, rz = raw.push(torch.from_numpy(x[:700].copy()).to(dev), 700, True, torch.tensor([-3], dtype=torch.int32, device=dev))
    assert len(z) == 0 and LM.stream_record(np.frombuffer(rz, np.uint8)).total == 0


def test_device_argument_checks(dev):
    L = N.lib()
    need = L.gsv_limstream_state_bytes(48, 1600)
    state = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    st = N.current_stream_ptr(dev)
    out, x = torch.full((63,), FILL, device=dev), torch.zeros(10, device=dev)
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    sp = state.data_ptr()
    bad = [L.gsv_limstream_init(None, need, -1.0, 48, 1600, st), L.gsv_limstream_init(sp, need - 1, -1.0, 48, 1600, st),
           L.gsv_limstream_init(sp + 4, need, -1.0, 48, 1600, st), L.gsv_limstream_init(sp, need, 0.5, 48, 1600, st),
           L.gsv_limstream_init(sp, need, -1.0, 4097, 1600, st),
           L.gsv_limstream_push(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_limstream_push(sp, None, 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_limstream_push(sp, x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_limstream_push(sp, x.data_ptr(), 10, None, 0, None, rec.data_ptr(), st),
           L.gsv_limstream_push(sp, x.data_ptr(), 10, None, 0, x.data_ptr(), rec.data_ptr(), st),
           L.gsv_limstream_push(sp, x.data_ptr(), 10, None, 0, out.data_ptr(), None, st)]
    assert bad == [1] * len(bad), bad
    # a state nobody initialised is not read through: the record says so and `out` stays as it was
    assert L.gsv_limstream_push(sp, x.data_ptr(), 10, None, 1, out.data_ptr(), rec.data_ptr(), st) == 0
    assert LM.stream_record(rec.view(torch.uint8)).emitted == 0 and rec.cpu().numpy().view(np.int16)[2] == -1
    assert bool((out == FILL).all())


def test_the_record_is_the_length_of_a_track_push(dev):
    """limit -> track on the device, the track reading its length from the limiter's record: the packets of the host chain"""
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    rate, fmt = 32000, TrackFormat(48000, 2, 20)
    x = R.grid_signal("noise", 3 * TILE + 5, rate)
    cuts = [30, 1000, 0, 1500, len(x) - 2530]
    lm, tr = LM.StreamLimiter(CEILING, rate, dev), TrackResampler(fmt, rate, dev)
    hl, ht = LM.StreamLimiter(CEILING, rate, "cpu"), TrackResampler(fmt, rate, "cpu")
    xd, at = torch.from_numpy(x).to(dev), 0
    for k, n in enumerate(cuts):
        flush = k + 1 == len(cuts)
        cap = lm.capacity(n)
        out = torch.full((cap,), 3.0e38, device=dev)
        rec = torch.zeros(4, dtype=torch.int64, device=dev)
        pcm = torch.full((tr.capacity(cap),), 0x5A5A, dtype=torch.int16, device=dev)
        trec = torch.zeros(4, dtype=torch.int32, device=dev)
        lm.enqueue(xd[at: at + n].data_ptr() if n else 0, n, None, flush, out.data_ptr(), rec.data_ptr())
        tr.enqueue(out.data_ptr(), cap, rec.data_ptr(), flush, pcm.data_ptr(), trec.data_ptr())
        want = ht.push(hl.push(x[at: at + n], flush), flush)
        packets = trec.tolist()[0]
        assert trec.tolist() == list(ht.rec) and packets == want.shape[0], (k, trec.tolist(), ht.rec)
        width = fmt.packet * fmt.channels
        assert np.array_equal(pcm.cpu().numpy()[: packets * width].reshape(packets, width), want), k
        at += n
    assert hl.rec.limited_ever


def test_chunk_emitter_with_leveller_limiter_and_track(dev):
    """the five-chunk signal of tests/test_hip_track.py's emitter test, lifted so that the limiter has work: the samples are the
    plain emitter's, levelled and limited push by push on the host, the packets those of the limited samples; a second segment
    goes on in the same streams"""
    from gsv_tts_lite_amd.level import StreamLeveller
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    ov, n_chunk, mute = 640, 6400, 1234
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    sm[:4000] *= 0.01
    fmt = TrackFormat(48000, 1, 20)
    lv = lambda d: StreamLeveller(-10.0, 32000, d, seed=-30.0, peak_limit=float("inf"))
    plain = ChunkEmitter(ov)
    limited = ChunkEmitter(ov, limit=LM.StreamLimiter(-6.0, 32000, dev))
    full = ChunkEmitter(ov, track=TrackResampler(fmt, 32000, dev), level=lv(dev), limit=LM.StreamLimiter(-6.0, 32000, dev))
    f_lim, f_level, f_lim2, f_track = LM.StreamLimiter(-6.0, 32000, "cpu"), lv("cpu"), LM.StreamLimiter(-6.0, 32000, "cpu"), \
        TrackResampler(fmt, 32000, "cpu")
    jobs, pos, shifts = [], 0, [0, 13, 200, 0, 77]
    for c, sh in enumerate(shifts):
        final = c == len(shifts) - 1
        start = pos - sh if c else 0
        chunk = torch.from_numpy(sm[start: start + n_chunk].copy()).to(dev)
        kw = dict(trim_head=c == 0, mute_samples=mute if final else 0)
        jobs.append(([e.push(chunk[None, None], final, flush=False, **kw) for e in (plain, limited, full)], False))
        pos = start + n_chunk if final else start + n_chunk - ov
    for e in (plain, limited, full):
        e.new_segment()
    silent = torch.zeros(3000, device=dev)
    jobs.append(([e.push(silent, False, trim_head=True) for e in (plain, limited, full)], False))
    last = torch.from_numpy(sm[5000: 5000 + n_chunk].copy()).to(dev)
    jobs.append(([e.push(last, True, mute_samples=mute, flush=True) for e in (plain, limited, full)], True))
    total = [0, 0, 0]
    same = lambda p, q: all(getattr(p, f) == getattr(q, f) for f in LM.StreamLimiterRecord.__slots__)
    for i, ((hp, hl, hf), flush) in enumerate(jobs):
        a, b, c = hp.result(), hl.result(), hf.result()
        assert len(a) == 3 and len(b) == 3 and len(c) == 4 and hp.limit is None
        assert a[1:] == b[1:] == c[1:3]
        want = f_lim.push(a[0], flush)
        assert b[0].dtype == np.float32 and b[0].tobytes() == want.tobytes() and same(hl.limit, f_lim.rec), (i, hl.limit, f_lim.rec)
        want2 = f_lim2.push(f_level.push(a[0], flush), flush)
        assert c[0].tobytes() == want2.tobytes() and same(hf.limit, f_lim2.rec), (i, hf.limit, f_lim2.rec)
        assert hf.level.gain_last == f_level.rec.gain_last and hf.level.clamped == 0
        assert np.array_equal(c[3], f_track.push(want2, flush)), i
        for j, v in enumerate((a, b, c)):
            total[j] += len(v[0])
    assert total[0] == total[1] == total[2] and f_lim2.rec.limited_ever
    d = f_lim.delay
    assert len(jobs[0][0][1].result()[0]) == len(jobs[0][0][0].result()[0]) - d           # the first clip is D shorter
    assert len(jobs[-1][0][1].result()[0]) == len(jobs[-1][0][0].result()[0]) + d         # the flushing one D longer
    assert len(jobs[5][0][1].result()[0]) == 0                                            # the silent chunk: empty in, empty out
