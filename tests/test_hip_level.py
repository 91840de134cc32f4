"""GPU parity of the stream leveller (csrc/level.h behind gsv_level_push) against its host twin gsv_level_push_host, which
tests/test_level_cpu.py pins to the numpy restatement of DESIGN 4.21: the same samples, the same record and the same state bytes
for the same pushes, in place and out of place, a device-held length honoured, nothing written outside the buffers, and
stream.ChunkEmitter(level=...) driving it behind gsv_stream_emit.

The shapes are the smallest that cross every boundary: hops of 800 samples at 8 kHz (runs of 2), of 1102 / 1103 at 11 025 Hz (runs of
3, the first of a hop short), of 9600 at 96 kHz (two spans of the measure block per hop), one push that holds 40 hops (the block
walks them one after the other), and a stream that runs past max_seconds=2.

The grid is thinned to keep the run at seconds: every rate meets every signal, each in one push and in a random cut, plus one of the
fixed cuts (hop-1, hop, hop+1, 4 hop-1, 4 hop+1) that rotates with the signal, plus the cut with pushes of 0 and 1 sample on every
other signal -- so each cut is met at every rate, not on every signal.  tests/test_level_cpu.py holds the twin to one answer under
every cut; here the device is held to the twin."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_ref as R  # noqa: E402
import loudness_ref as LR  # noqa: E402

from oracle.gen_golden_inputs import facade_audio  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import level as lv  # noqa: E402
from gsv_tts_lite_amd.level import StreamLeveller  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 16
FILL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rec_bytes(r):
    return bytes(r.cpu().numpy().view(np.uint8)[: lv.RECORD_BYTES])


class _Raw:
    """the raw device calls on one state: guard samples around every buffer, the state in the middle of a guarded allocation"""

    def __init__(self, dev, rate, **kw):
        self.dev = dev
        self.host = StreamLeveller(R.TARGET, rate, "cpu", **kw)                 # the twin, pushed alongside
        fresh = StreamLeveller(R.TARGET, rate, dev, **kw).state
        self.nbytes = fresh.numel()
        self.block = torch.full((self.nbytes + 512,), 0xA5, dtype=torch.uint8, device=dev)
        self.state = self.block[256: 256 + self.nbytes]
        assert self.state.data_ptr() % 16 == 0
        self.state.copy_(fresh)
        assert np.array_equal(self.state.cpu().numpy(), self.host.state.numpy()), "a fresh device state equals a fresh host state"

    def push(self, x, flush, in_place=False, n_real=None):
        """x: float32 numpy, the capacity of the call; n_real: None, or the real length on the device (< len(x))"""
        L = N.lib()
        n_cap = len(x)
        n = n_cap if n_real is None else max(0, min(n_real, n_cap))
        buf = torch.full((n_cap + 2 * GUARD,), FILL, dtype=torch.float32, device=self.dev)
        buf[GUARD: GUARD + n_cap] = torch.from_numpy(x).to(self.dev)
        out = buf if in_place else torch.full((n_cap + 2 * GUARD,), FILL, dtype=torch.float32, device=self.dev)
        rec = torch.full((lv.RECORD_BYTES // 8 + 2,), -5, dtype=torch.int64, device=self.dev)
        n_dev = None if n_real is None else torch.tensor([n_real, 12345, -7], dtype=torch.int32, device=self.dev)
        N.check(L.gsv_level_push(self.state.data_ptr(), buf[GUARD:].data_ptr() if n_cap else None, n_cap,
                                 None if n_dev is None else n_dev.data_ptr(), int(flush), out[GUARD:].data_ptr() if n_cap else None,
                                 rec[1:].data_ptr(), N.current_stream_ptr(self.dev)))
        got, src, r = out.cpu().numpy(), buf.cpu().numpy(), rec.cpu().numpy()
        assert np.all(got[:GUARD] == FILL) and np.all(got[GUARD + n_cap:] == FILL), "written outside out"
        if not in_place:
            assert np.all(got[GUARD + n: GUARD + n_cap] == FILL), "written behind the real length"
            assert np.array_equal(src[GUARD: GUARD + n_cap].view(np.uint32), x.view(np.uint32)), "the chunk was changed"
        assert r[0] == -5 and r[-1] == -5, "written outside the record"
        block = self.block.cpu().numpy()
        assert np.all(block[:256] == 0xA5) and np.all(block[256 + self.nbytes:] == 0xA5), "written outside the state"
        want = self.host.push(x[:n], flush)
        have, nan = got[GUARD: GUARD + n], np.isnan(want)
        assert np.array_equal(np.isnan(have), nan) and np.array_equal(have[~nan].view(np.uint32), want[~nan].view(np.uint32)), "samples"
        return lv.record(r[1:-1].view(np.uint8)), block[256: 256 + self.nbytes]


def _check(raw, x, plan, in_place):
    at = 0
    for i, n in enumerate(plan):
        rec, state = raw.push(x[at: at + n].copy(), i == len(plan) - 1, in_place=in_place)
        at += n
        want = raw.host.rec
        assert (rec.zbar, rec.gain_first, rec.gain_last, rec.clamped, rec.blocks, rec.above_abs, rec.kept, rec.measured, rec.nonfinite,
                rec.full) == (want.zbar, want.gain_first, want.gain_last, want.clamped, want.blocks, want.above_abs, want.kept,
                              want.measured, want.nonfinite, want.full), (i, at)
        assert np.array_equal(state, raw.host.state.numpy()), ("state bytes", i, at)


@pytest.mark.parametrize("rate", R.RATES)
def test_device_samples_records_and_state_equal_the_host_twin(dev, rate):
    hop = R.knot(1, rate)
    for i, kind in enumerate(R.KINDS):
        x = R.signal(kind, rate)
        plans = R.cuts(len(x), hop, seed=rate + i)
        names = ["one", "random"] + [list(plans)[1 + (i + j) % 5] for j in range(1)] + (["0,1,.."] if i % 2 else [])
        for j, name in enumerate(names):
            raw = _Raw(dev, rate, seed=-25.0 if (i + j) % 2 else None)
            _check(raw, x, plans[name], in_place=(i + j) % 2 == 0)
            # the flushed state starts a fresh stream: the first hops again, as a second stream on the same state
            if j == 0:
                _check(raw, x[: 5 * hop + 7], [2 * hop, 3 * hop + 7], in_place=True)


def test_hops_of_two_spans(dev):
    rate = 96000                    # a hop of 9600 samples: a span of 8192 and one of 1408 whose first run is short
    x = np.concatenate([LR.noise(rate // 2, seed=4, amp=0.05), LR.sine(60.0, 0.35, rate, amp=0.2)]).astype(np.float32)
    _check(_Raw(dev, rate), x, [len(x)], in_place=False)
    _check(_Raw(dev, rate, seed=-30.0), x, [9599, 1, 30000, 9601, len(x) - 49201], in_place=True)


def test_a_device_held_length_is_honoured(dev):
    rate = 8000
    x = R.signal("gating", rate)[: 6000]
    lengths = [613, 0, 1, 1999, 1500, 1887]                 # the real lengths; every call names a capacity of 2000
    assert sum(lengths) == 6000
    for in_place in (False, True):
        raw, at = _Raw(dev, rate, seed=-20.0), 0
        for i, n in enumerate(lengths):
            chunk = np.full(2000, np.float32(3.0e38))         # poison behind the real length
            chunk[n:][::2] = np.nan
            chunk[:n] = x[at: at + n]
            rec, state = raw.push(chunk, i == len(lengths) - 1, in_place=in_place, n_real=n)
            assert rec.zbar == raw.host.rec.zbar and not rec.nonfinite and np.array_equal(state, raw.host.state.numpy()), (i, at)
            at += n
    # a length past the capacity is the capacity; a negative one is 0
    raw = _Raw(dev, rate)
    rec, _ = raw.push(x[:2000].copy(), False, n_real=100000)
    assert rec.blocks == 0 and raw.host.rec.gain_last == rec.gain_last
    rec, state = raw.push(x[:2000].copy(), False, n_real=-3)
    assert np.array_equal(state, raw.host.state.numpy())


def test_a_stream_past_max_seconds_and_a_nan(dev):
    rate = 8000
    x = LR.noise(3 * rate + 100, seed=11, amp=0.02)
    raw = _Raw(dev, rate, max_seconds=2)
    _check(raw, x, [2 * rate - 1, rate + 1, 100], in_place=False)
    assert raw.host.rec.full and raw.host.rec.blocks == 17
    y = x.copy()
    y[12 * 800 + 5] = np.nan
    y[20 * 800] = -np.inf
    raw = _Raw(dev, rate)
    for at, n in ((0, 16000), (16000, 8100)):
        chunk = y[at: at + n].copy()
        rec, state = raw.push(chunk, False, in_place=True)
        assert rec.nonfinite and rec.blocks == 9 and rec.clamped == raw.host.rec.clamped and np.array_equal(state, raw.host.state.numpy())
    assert raw.host.rec.clamped == 1


def test_device_argument_checks(dev):
    L = N.lib()
    good = (8000, -18.0, float("nan"), 10.0, 10.0, 20.0, 1.0, 2)
    need = L.gsv_level_state_bytes(8000, 2)
    state = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    st = N.current_stream_ptr(dev)
    x, out = torch.zeros(10, device=dev), torch.full((10,), FILL, device=dev)
    rec = torch.zeros(5, dtype=torch.int64, device=dev)
    bad = [L.gsv_level_init(None, need, *good, st), L.gsv_level_init(state.data_ptr(), need - 1, *good, st),
           L.gsv_level_init(state.data_ptr() + 4, need, *good, st),
           L.gsv_level_init(state.data_ptr(), need, 3999, *good[1:], st),
           L.gsv_level_init(state.data_ptr(), need, 8000, -18.0, float("nan"), 10.0, 10.0, 20.0, -1.0, 2, st),
           L.gsv_level_push(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_level_push(state.data_ptr(), None, 10, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_level_push(state.data_ptr(), x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr(), st),
           L.gsv_level_push(state.data_ptr(), x.data_ptr(), 10, None, 0, None, rec.data_ptr(), st),
           L.gsv_level_push(state.data_ptr(), x.data_ptr(), 10, None, 0, out.data_ptr(), None, st),
           L.gsv_level_push(state.data_ptr(), x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr() + 4, st)]
    assert bad == [1] * len(bad), bad
    # a state nobody initialised is not read through: the record says so and `out` stays as it was
    assert L.gsv_level_push(state.data_ptr(), x.data_ptr(), 10, None, 1, out.data_ptr(), rec.data_ptr(), st) == 0
    assert lv._REC.names[-1] == "flags" and int(np.frombuffer(_rec_bytes(rec), lv._REC)["flags"][0]) == -1
    assert bool((out == FILL).all())
    with pytest.raises(RuntimeError):
        N.check(bad[0])


def test_chunk_emitter_with_a_leveller(dev):
    """the five-chunk signal of tests/test_hip_track.py's emitter test: the samples are the plain emitter's, levelled push by push
    by a leveller on the host; the track's packets are those of the levelled samples; a second segment goes on in the same stream"""
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    ov, n_chunk, mute = 640, 6400, 1234
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    sm[:4000] *= 0.01
    fmt = TrackFormat(48000, 1, 20)
    plain = ChunkEmitter(ov)
    levelled = ChunkEmitter(ov, level=StreamLeveller(-30.0, 32000, dev, seed=-20.0))
    both = ChunkEmitter(ov, track=TrackResampler(fmt, 32000, dev), level=StreamLeveller(-30.0, 32000, dev, seed=-20.0))
    follow, follow_track = StreamLeveller(-30.0, 32000, "cpu", seed=-20.0), TrackResampler(fmt, 32000, "cpu")
    jobs, pos, shifts = [], 0, [0, 13, 200, 0, 77]
    for c, sh in enumerate(shifts):
        final = c == len(shifts) - 1
        start = pos - sh if c else 0
        chunk = torch.from_numpy(sm[start: start + n_chunk].copy()).to(dev)
        kw = dict(trim_head=c == 0, mute_samples=mute if final else 0)
        jobs.append(([e.push(chunk[None, None], final, flush=False, **kw) for e in (plain, levelled, both)], False))
        pos = start + n_chunk if final else start + n_chunk - ov
    for e in (plain, levelled, both):
        e.new_segment()
    silent = torch.zeros(3000, device=dev)
    jobs.append(([e.push(silent, False, trim_head=True) for e in (plain, levelled, both)], False))
    last = torch.from_numpy(sm[5000: 5000 + n_chunk].copy()).to(dev)
    jobs.append(([e.push(last, True, mute_samples=mute, flush=True) for e in (plain, levelled, both)], True))
    moved = 0
    for i, ((hp, hl, hb), flush) in enumerate(jobs):
        a, b, c = hp.result(), hl.result(), hb.result()
        assert len(a) == 3 and len(b) == 3 and len(c) == 4 and hp.level is None
        want = follow.push(a[0], flush)
        assert np.array_equal(b[0].view(np.uint32), want.view(np.uint32)) and np.array_equal(c[0].view(np.uint32), want.view(np.uint32)), i
        assert a[1:] == b[1:] == c[1:3]
        for h in (hl, hb):
            assert (h.level.zbar, h.level.gain_first, h.level.gain_last, h.level.clamped, h.level.blocks, h.level.kept) == (
                follow.rec.zbar, follow.rec.gain_first, follow.rec.gain_last, follow.rec.clamped, follow.rec.blocks, follow.rec.kept), i
        assert np.array_equal(c[3], follow_track.push(want, flush)), i
        moved += int(follow.rec.gain_first != follow.rec.gain_last)
    assert moved >= 3 and follow.rec.blocks >= 5           # the gain was on the move: the comparison is not one of copies
