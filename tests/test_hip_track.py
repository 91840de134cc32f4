"""GPU parity of the real-time track output (csrc/track.h behind gsv_track_push) against its host twin gsv_track_push_host, which
tests/test_track_cpu.py pins to the fp64 definition: the same bytes and the same record for the same chunking, nothing written
behind what the record names, a device-held length honoured, and stream.ChunkEmitter(track=...) driving it behind gsv_stream_emit."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as R  # noqa: E402

from oracle.gen_golden_inputs import facade_audio  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402

pytestmark = pytest.mark.gpu

N_SAMPLES = 3001
GUARD = 16
FILL = 0x5A5A
GRID = list(itertools.product(R.PACKETS, R.CHANNELS, R.SIGNALS))
PAIRS = R.RATE_PAIRS + [(32000, 125)]        # the last: 3360 taps, a tile's span is read from memory, not staged in LDS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fmt(out_rate, packet, channels):
    return TrackFormat(rate=out_rate, channels=channels, packet_samples=packet)


class _Raw:
    """the raw device calls on one state, with guard words behind `out`'s capacity checked after every push"""

    def __init__(self, dev, in_rate, out_rate, packet, channels):
        self.dev, self.args, self.width = dev, (in_rate, out_rate, packet, channels), packet * channels
        L = N.lib()
        nbytes = L.gsv_track_state_bytes(*self.args)
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        N.check(L.gsv_track_init(self.state.data_ptr(), nbytes, *self.args, N.current_stream_ptr(dev)))

    def push(self, chunk, n_cap, flush, n_dev=None):
        """chunk: device fp32 with at least n_cap samples -> (packets int16 [k, width], rec)"""
        L = N.lib()
        cap = int(L.gsv_track_out_capacity(n_cap, *self.args))
        out = torch.full((cap + GUARD,), FILL, dtype=torch.int16, device=self.dev)
        rec = torch.full((4,), -5, dtype=torch.int32, device=self.dev)
        N.check(L.gsv_track_push(self.state.data_ptr(), chunk.data_ptr() if n_cap else None, n_cap,
                                 None if n_dev is None else n_dev.data_ptr(), int(flush), out.data_ptr(), rec.data_ptr(),
                                 N.current_stream_ptr(self.dev)))
        rec, out = rec.tolist(), out.cpu().numpy()
        assert np.all(out[cap:] == FILL), "written behind the capacity"
        used = (rec[0] * self.args[2] + rec[2]) * self.args[3]     # whole packets, then the samples the second launch moved to the carry
        assert 0 <= used <= cap and np.all(out[used:] == FILL), "written behind what the record names"
        return out[: rec[0] * self.width].reshape(rec[0], self.width), rec


def _host(x, in_rate, out_rate, packet, channels, plan):
    rs = TrackResampler(_fmt(out_rate, packet, channels), in_rate, "cpu")
    got, recs, at = [], [], 0
    for n, flush in plan:
        got.append(rs.push(x[at: at + n], flush))
        recs.append(list(rs.rec))
        at += n
    return got, recs


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_device_bytes_and_records_equal_the_host_twin(dev, in_rate, out_rate):
    o, w, width, _ = R.params(in_rate, out_rate)
    combos = itertools.cycle(GRID[PAIRS.index((in_rate, out_rate))::5] + GRID)
    for name, plan in R.chunkings(N_SAMPLES, o, width).items():
        packet, channels, kind = next(combos)
        x = R.signal(kind, N_SAMPLES)
        want, want_recs = _host(x, in_rate, out_rate, packet, channels, plan)
        raw, xd, at = _Raw(dev, in_rate, out_rate, packet, channels), torch.from_numpy(x).to(dev), 0
        for (n, flush), wp, wr in zip(plan, want, want_recs):
            got, rec = raw.push(xd[at: at + n], n, flush)
            assert rec == wr, (name, packet, channels, kind, at, n, rec, wr)
            assert np.array_equal(got, wp), (name, packet, channels, kind, at, n)
            at += n


def test_every_packet_size_channel_count_and_signal(dev):
    in_rate, out_rate = 32000, 44100
    o, w, width, _ = R.params(in_rate, out_rate)
    for i, (packet, channels, kind) in enumerate(GRID):
        x = R.signal(kind, N_SAMPLES, i)
        plan = R.chunkings(N_SAMPLES, o, width, i)["random 0..700"]
        want, want_recs = _host(x, in_rate, out_rate, packet, channels, plan)
        rs, at = TrackResampler(_fmt(out_rate, packet, channels), in_rate, dev), 0
        for (n, flush), wp, wr in zip(plan, want, want_recs):
            got = rs.push(x[at: at + n], flush)
            assert rs.rec == wr and np.array_equal(got, wp), (packet, channels, kind, at, n)
            at += n


def test_a_device_held_length_is_honoured(dev):
    in_rate, out_rate, packet, channels = 32000, 48000, 7, 2
    x = R.signal("noise", 2000)
    lengths = [613, 0, 1, 700, 686]                       # the real lengths; every call names a capacity of 700
    assert sum(lengths) == 2000
    plan = [(n, i == len(lengths) - 1) for i, n in enumerate(lengths)]
    want, want_recs = _host(x, in_rate, out_rate, packet, channels, plan)
    raw, at = _Raw(dev, in_rate, out_rate, packet, channels), 0
    for (n, flush), wp, wr in zip(plan, want, want_recs):
        chunk = np.full(700, np.float32(3.0e38))            # poison behind the real length
        chunk[n:][::2] = np.nan
        chunk[:n] = x[at: at + n]
        n_dev = torch.tensor([n, 12345, -7, 99], dtype=torch.int32, device=dev)
        got, rec = raw.push(torch.from_numpy(chunk).to(dev), 700, flush, n_dev)
        assert rec == wr and np.array_equal(got, wp), (at, n, rec, wr)
        at += n
    # a length past the capacity is the capacity; a negative one is 0
    a, ra = raw.push(torch.from_numpy(x[:700].copy()).to(dev), 700, True, torch.tensor([100000], dtype=torch.int32, device=dev))
    b, rb = _host(x[:700], in_rate, out_rate, packet, channels, [(700, True)])
    assert ra == rb[0] and np.array_equal(a, b[0])
    _, rz = raw.push(torch.from_numpy(x[:700].copy()).to(dev), 700, True, torch.tensor([-3], dtype=torch.int32, device=dev))
    assert rz == [0, 0, 0, 0]


def test_device_argument_checks(dev):
    L = N.lib()
    args = (32000, 48000, 960, 1)
    need = L.gsv_track_state_bytes(*args)
    state = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    st = N.current_stream_ptr(dev)
    out = torch.zeros(L.gsv_track_out_capacity(10, *args), dtype=torch.int16, device=dev)
    rec, x = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(10, device=dev)
    bad = [L.gsv_track_init(None, need, *args, st), L.gsv_track_init(state.data_ptr(), need - 1, *args, st),
           L.gsv_track_init(state.data_ptr() + 4, need, *args, st), L.gsv_track_init(state.data_ptr(), need, 32000, 48000, 0, 1, st),
           L.gsv_track_push(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_track_push(state.data_ptr(), None, 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_track_push(state.data_ptr(), x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_track_push(state.data_ptr(), x.data_ptr(), 10, None, 0, None, rec.data_ptr(), st),
           L.gsv_track_push(state.data_ptr(), x.data_ptr(), 10, None, 0, out.data_ptr(), None, st)]
    assert bad == [1] * len(bad), bad
    # a state nobody initialised is not read through: the record says so and `out` stays as it was
    out.fill_(FILL)
    assert L.gsv_track_push(state.data_ptr(), x.data_ptr(), 10, None, 1, out.data_ptr(), rec.data_ptr(), st) == 0
    assert rec.tolist() == [-1, -1, -1, -1] and bool((out == FILL).all())
    with pytest.raises(RuntimeError):
        N.check(bad[0])


def test_chunk_emitter_with_a_track(dev):
    """the five-chunk signal of tests/test_hip_stream_emit.py, head trim on the first chunk and a mute behind the last: the fp32
    samples are the ones the emitter hands out without a track, and the packets are what a TrackResampler fed those samples
    gives, push by push; a second segment goes on in the same track stream"""
    from gsv_tts_lite_amd.stream import ChunkEmitter
    ov, n_chunk, mute = 640, 6400, 1234
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    sm[:4000] *= 0.01                                        # a quiet head: the trim takes some of it
    fmt = TrackFormat(48000, 2, 20)
    plain, tracked = ChunkEmitter(ov), ChunkEmitter(ov, track=TrackResampler(fmt, 32000, dev))
    follow = TrackResampler(fmt, 32000, dev)
    jobs, pos, shifts = [], 0, [0, 13, 200, 0, 77]
    for c, sh in enumerate(shifts):
        final = c == len(shifts) - 1
        start = pos - sh if c else 0
        chunk = torch.from_numpy(sm[start: start + n_chunk].copy()).to(dev)
        kw = dict(trim_head=c == 0, mute_samples=mute if final else 0)
        jobs.append((plain.push(chunk[None, None], final, **kw), tracked.push(chunk[None, None], final, flush=False, **kw), False))
        pos = start + n_chunk if final else start + n_chunk - ov
    plain.new_segment(); tracked.new_segment()
    # the second segment: a first chunk trimmed to nothing (all silence: a zero-length push), then the text's last chunk with the flush
    silent = torch.zeros(3000, device=dev)
    jobs.append((plain.push(silent, False, trim_head=True), tracked.push(silent, False, trim_head=True), False))
    last = torch.from_numpy(sm[5000: 5000 + n_chunk].copy()).to(dev)
    jobs.append((plain.push(last, True, mute_samples=mute), tracked.push(last, True, mute_samples=mute, flush=True), True))
    total = 0
    for i, (hp, ht, flush) in enumerate(jobs):
        a, b = hp.result(), ht.result()
        assert len(a) == 3 and len(b) == 4
        assert b[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and a[1:] == b[1:3], i
        want = follow.push(b[0], flush)
        assert b[3].dtype == np.int16 and b[3].shape == want.shape and np.array_equal(b[3], want), i
        total += b[3].shape[0]
    assert jobs[0][1].result()[2] > 0 and len(jobs[5][1].result()[0]) == 0          # the head was trimmed; the silent chunk is empty
    whole = np.concatenate([t.result()[0] for _, t, _ in jobs])
    assert total == -(-R.total(len(whole), 2, 3) // 960) and follow.rec[2] == 0
