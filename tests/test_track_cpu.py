"""CPU checks of the real-time track output (csrc/track.h behind gsv_track_init_host / gsv_track_push_host, track.py): the
host twin against the numpy restatement tests/track_ref.py, chunking invariance bit for bit, the record of every push
against the streaming rule, the edge cases and the argument checks.  No GPU: the host twin is built from the scalar
routines the device kernels share, and tests/test_hip_track.py pins the device to it.

Tolerance of the fp64 comparison: at most 1 LSB at every sample, and differing samples on at most 2 % of a stream.  Derived,
not measured: only 14-50 taps of a row are non-negligible, so the fp32 tap sum sits within 1e-5 of the fp64 one against an
LSB of 2^-15 = 3.05e-5 -- the two can only fall on either side of a rounding boundary, one step apart; and a sum lands that
close to a boundary for well under 2 % of uniform samples (an fp32 model of the kernel differs at 0.1-0.5 % of them), where
a truncating or biased quantiser would differ at about half."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref as R  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler, pcm16  # noqa: E402

N_SAMPLES = 3001
GRID = list(itertools.product(R.PACKETS, R.CHANNELS, R.SIGNALS))


def _fmt(out_rate, packet, channels):
    return TrackFormat(rate=out_rate, channels=channels, packet_samples=packet)


def _stream(x, in_rate, out_rate, packet, channels, plan, rs=None):
    """push x through a resampler on the CPU as `plan` cuts it -> (the packets concatenated, every push's rec)"""
    rs = rs or TrackResampler(_fmt(out_rate, packet, channels), in_rate, "cpu")
    got, recs, at = [], [], 0
    for n, flush in plan:
        got.append(rs.push(x[at: at + n], flush))
        recs.append(list(rs.rec))
        at += n
    assert at == len(x)
    return np.concatenate(got), recs


@pytest.mark.parametrize("in_rate,out_rate", R.RATE_PAIRS)
def test_one_push_with_flush_is_within_one_lsb_of_the_fp64_definition(in_rate, out_rate):
    worst = 0.0
    for kind in R.SIGNALS:
        x = R.signal(kind, N_SAMPLES)
        q64 = R.quantise(R.resample64(x, in_rate, out_rate))
        for packet, channels in itertools.product(R.PACKETS, R.CHANNELS):
            want = R.packets(q64, packet, channels)
            got = pcm16(x, in_rate, _fmt(out_rate, packet, channels), device="cpu")
            assert got.dtype == np.int16 and got.shape == want.shape, (got.shape, want.shape)
            diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
            share = float((diff > 0).mean()) if diff.size else 0.0
            worst = max(worst, share)
            assert diff.max(initial=0) <= 1, (kind, packet, channels, int(diff.max()))
            assert share <= 0.02, (kind, packet, channels, share)
    print("%d -> %d: samples one LSB from the fp64 definition: at most %.3f %% of a stream" % (in_rate, out_rate, 100 * worst))


@pytest.mark.parametrize("in_rate,out_rate", R.RATE_PAIRS)
def test_packets_do_not_depend_on_the_chunking(in_rate, out_rate):
    o, w, width, _ = R.params(in_rate, out_rate)
    combos = itertools.cycle(GRID)
    for seed in range(2):
        for name, plan in R.chunkings(N_SAMPLES, o, width, seed).items():
            packet, channels, kind = next(combos)
            x = R.signal(kind, N_SAMPLES, seed)
            want = pcm16(x, in_rate, _fmt(out_rate, packet, channels), device="cpu")
            got, recs = _stream(x, in_rate, out_rate, packet, channels, plan)
            assert np.array_equal(got, want), (name, packet, channels, kind)
            rule = R.Rule(in_rate, out_rate, packet)
            for (n, flush), rec in zip(plan, recs):
                assert rec == rule.push(n, flush), (name, packet, channels, n, flush)


def test_every_packet_size_channel_count_and_signal_under_a_random_chunking():
    in_rate, out_rate = 32000, 48000
    o, w, width, _ = R.params(in_rate, out_rate)
    for i, (packet, channels, kind) in enumerate(GRID):
        x = R.signal(kind, N_SAMPLES, i)
        plan = R.chunkings(N_SAMPLES, o, width, i)["random 0..700"]
        want = pcm16(x, in_rate, _fmt(out_rate, packet, channels), device="cpu")
        got, _ = _stream(x, in_rate, out_rate, packet, channels, plan)
        assert np.array_equal(got, want), (packet, channels, kind)
        if channels == 2:
            assert np.array_equal(got[:, 0::2], got[:, 1::2])
            mono = pcm16(x, in_rate, _fmt(out_rate, packet, 1), device="cpu")
            assert np.array_equal(got[:, 0::2], mono)


def test_a_span_too_long_for_staging_takes_the_same_rule():
    """32000 -> 125 Hz: o = 256, 3360 taps; the device reads such a tile from memory instead of LDS (tests/test_hip_track.py)"""
    x = R.signal("noise", 4000)
    want = R.one_shot(x, 32000, 125, 7, 1)
    got = pcm16(x, 32000, _fmt(125, 7, 1), device="cpu")
    assert got.shape == want.shape and np.abs(got.astype(np.int32) - want).max() <= 1
    o, w, width, _ = R.params(32000, 125)
    chunked, _ = _stream(x, 32000, 125, 7, 1, R.chunkings(4000, o, width)["random 0..700"])
    assert np.array_equal(chunked, got)


def test_edge_cases():
    for in_rate, out_rate in [(32000, 48000), (32000, 32000), (32000, 8000)]:
        rs = TrackResampler(_fmt(out_rate, 7, 2), in_rate, "cpu")
        out = rs.push(np.zeros(0, np.float32), flush=True)                       # an empty stream: no packet
        assert out.shape == (0, 14) and rs.rec == [0, 0, 0, 0]
        o, w, width, _ = R.params(in_rate, out_rate)
        # a stream whose outputs fill whole packets: the flush finds an empty carry and pads nothing
        n = 7 * o * 20
        assert R.total(n, o, w) % 7 == 0
        x = R.signal("noise", n)
        a = rs.push(x, flush=False)
        b = rs.push(np.zeros(0, np.float32), flush=True)
        assert rs.rec[3] == 0 and rs.rec[2] == 0
        assert (a.shape[0] + b.shape[0]) * 7 == R.total(n, o, w)
        # the state after a flush is a fresh state
        y = R.signal("sine", 2000, 3)
        again, _ = _stream(y, in_rate, out_rate, 7, 2, [(700, False), (1300, True)], rs)
        fresh, _ = _stream(y, in_rate, out_rate, 7, 2, [(700, False), (1300, True)])
        assert np.array_equal(again, fresh)


def test_argument_checks():
    L = N.lib()
    assert L.gsv_track_state_bytes(32000, 48000, 960, 1) > 0
    for bad in [(32000, 48000, 0, 1), (32000, 48000, 4097, 1), (32000, 48000, 960, 3), (32000, 48000, 960, 0), (0, 48000, 960, 1),
                (32000, -1, 960, 1), (31999, 48001, 960, 1)]:          # the last: a table past 2^24 entries
        assert L.gsv_track_state_bytes(*bad) == 0, bad
        assert L.gsv_track_out_capacity(100, *bad) == 0, bad
    assert L.gsv_track_out_capacity(-1, 32000, 48000, 960, 1) == 0
    args = (32000, 48000, 960, 1)
    need = L.gsv_track_state_bytes(*args)
    state = torch.zeros(need, dtype=torch.uint8)
    out = torch.zeros(L.gsv_track_out_capacity(10, *args), dtype=torch.int16)
    rec = torch.zeros(4, dtype=torch.int32)
    x = torch.zeros(10)
    assert L.gsv_track_init_host(None, need, *args) == 1
    assert L.gsv_track_init_host(state.data_ptr(), need - 1, *args) == 1          # a state that is too small
    assert L.gsv_track_init_host(state.data_ptr(), need, 32000, 48000, 960, 3) == 1
    assert L.gsv_track_push_host(state.data_ptr(), x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr()) == 1   # never initialised
    assert L.gsv_track_init_host(state.data_ptr(), need, *args) == 0
    assert L.gsv_track_push_host(None, x.data_ptr(), 10, None, 0, out.data_ptr(), rec.data_ptr()) == 1
    assert L.gsv_track_push_host(state.data_ptr(), None, 10, None, 0, out.data_ptr(), rec.data_ptr()) == 1
    assert L.gsv_track_push_host(state.data_ptr(), x.data_ptr(), -1, None, 0, out.data_ptr(), rec.data_ptr()) == 1
    assert L.gsv_track_push_host(state.data_ptr(), x.data_ptr(), 10, None, 0, None, rec.data_ptr()) == 1
    assert L.gsv_track_push_host(state.data_ptr(), x.data_ptr(), 10, None, 0, out.data_ptr(), None) == 1
    assert L.gsv_track_push_host(state.data_ptr(), None, 0, None, 0, out.data_ptr(), rec.data_ptr()) == 0            # no samples: no chunk needed
    # a host-held length is honoured the way the device-held one is, clamped to the capacity
    n = torch.tensor([4], dtype=torch.int32)
    assert L.gsv_track_push_host(state.data_ptr(), x.data_ptr(), 10, n.data_ptr(), 1, out.data_ptr(), rec.data_ptr()) == 0
    assert rec.tolist() == [1, 6, 0, 954]
    for bad in [dict(rate=0), dict(channels=3), dict(packet_ms=0.01), dict(rate=44100, packet_ms=2.5), dict(packet_samples=5000)]:
        with pytest.raises(ValueError):
            TrackFormat(**bad)
    assert TrackFormat().packet == 960 and TrackFormat(44100, 2, 20).packet == 882 and TrackFormat(8000, packet_ms=2.5).packet == 20
    with pytest.raises(ValueError):
        TrackResampler(TrackFormat(48001), 31999, "cpu")


def test_audioclip_to_pcm16_equals_pcm16(monkeypatch):
    from gsv_tts_lite_amd.tts import AudioClip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # the CPU path wherever this runs
    x = R.signal("noise", 2500)
    clip = AudioClip(None, x, 32000, len(x) / 32000, [], "text")
    assert clip.pcm is None and clip.pcm_rate is None
    assert np.array_equal(clip.to_pcm16(), pcm16(x, 32000, TrackFormat(), device="cpu"))
    assert np.array_equal(clip.to_pcm16(rate=8000, channels=2, packet_ms=10), pcm16(x, 32000, TrackFormat(8000, 2, 10), device="cpu"))
    assert clip.to_pcm16().shape == (-(-R.total(2500, 2, 3) // 960), 960)
