"""CPU tests of the stream leveller (csrc/level.h behind gsv_level_push_host): the host twin -- the CPU path of
level.StreamLeveller and the device's oracle -- against the numpy restatement of the rule in tests/level_ref.py, its independence
of how the stream is cut into pushes (bit for bit), the rule's own guarantees, its agreement with the clip meter, and convergence.

The bounds are four times the worst case measured here on the CPU over the grid below (DESIGN 4.21 states both):
  knot gains  4.2e-11 relative (60 Hz sine at 44.1 kHz: the high pass's double pole)  -> 1.7e-10
  zbar        8.4e-11 relative (the same signal)                                        -> 3.4e-10"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_ref as R  # noqa: E402
import loudness_ref as LR  # noqa: E402

import __graft_entry__ as g  # noqa: E402

g.build_hip()

from gsv_tts_lite_amd import level as lv  # noqa: E402
from gsv_tts_lite_amd import loudness  # noqa: E402
from gsv_tts_lite_amd.level import StreamLeveller  # noqa: E402

GAIN_BOUND, ZBAR_BOUND = 1.7e-10, 3.4e-10
ULP = 2.0 ** -52


def _stream(x, rate, plan, **kw):
    """push x in the lengths of `plan`, the last with the flush -> (samples, records, the state's bytes before the flush's push and
    after it, the knot gains before the flush)"""
    s = StreamLeveller(R.TARGET, rate, "cpu", **kw)
    out, recs, at = [], [], 0
    for i, n in enumerate(plan):
        last = i == len(plan) - 1
        if last:
            before, knots = s.state.numpy().copy(), s.knot_gains()
        out.append(s.push(x[at: at + n], flush=last))
        recs.append(s.rec)
        at += n
    assert at == len(x)
    return np.concatenate(out), recs, before, s.state.numpy().copy(), knots


def _by_hops(x, rate, hops, **kw):
    """one push per complete hop, then the rest with the flush: a record at every knot"""
    bounds = [R.knot(h, rate) for h in range(hops + 1)]
    return _stream(x, rate, [b - a for a, b in zip(bounds, bounds[1:])] + [len(x) - bounds[-1]], **kw)


@pytest.mark.parametrize("rate", R.RATES)
@pytest.mark.parametrize("seeded", [False, True])
def test_the_twin_against_the_oracle(rate, seeded):
    worst_a = worst_z = 0.0
    for kind in R.KINDS:
        ref = R.reference(kind, rate, seeded)
        assert ref.margin >= 0.1, (kind, rate, ref.margin)          # no block near a threshold at any knot: the counts are comparable
        assert ref.hops >= 20
        x = R.signal(kind, rate)
        out, recs, _, _, _ = _by_hops(x, rate, ref.hops, seed=-25.0 if seeded else None)
        s = StreamLeveller(R.TARGET, rate, "cpu", seed=-25.0 if seeded else None)
        s.push(x[: R.knot(ref.hops, rate)])
        A = s.knot_gains()
        assert len(A) == len(ref.A) == ref.hops + 2
        for h, (rec, want) in enumerate(zip(recs, ref.knots)):
            assert (rec.blocks, rec.above_abs, rec.kept) == want[:3], (kind, h)
            if want[3] > 0:
                worst_z = max(worst_z, abs(rec.zbar / want[3] - 1.0))
            else:
                assert rec.zbar == 0.0
        worst_a = max(worst_a, float(np.max(np.abs(A / np.asarray(ref.A) - 1.0))))
        assert recs[-1].zbar == recs[-2].zbar and recs[-1].clamped == ref.clamped
        # the samples: the oracle's fp32 gain comes from a rounded fp64 one, so a product may sit one fp32 rounding off
        assert np.allclose(out, ref.out, rtol=2.0 ** -22, atol=0.0), kind
        assert math.isclose(recs[-1].lufs, ref.lufs, abs_tol=1e-8) or (recs[-1].lufs == ref.lufs == -math.inf)
    print("rate %d seeded %r: worst knot gain %.3g, worst zbar %.3g (relative)" % (rate, seeded, worst_a, worst_z))
    assert worst_a <= GAIN_BOUND and worst_z <= ZBAR_BOUND


@pytest.mark.parametrize("rate", [8000, 11025])
def test_any_cut_of_the_stream_gives_the_same_bits(rate):
    for kind in ("noise", "gating"):
        x = R.signal(kind, rate)
        hop = R.knot(1, rate)
        plans = R.cuts(len(x), hop, seed=rate)
        want = _stream(x, rate, plans["one"], seed=-25.0)
        for name, plan in plans.items():
            got = _stream(x, rate, plan, seed=-25.0)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (kind, name)
            assert got[1][-1].zbar == want[1][-1].zbar and got[1][-1].clamped == want[1][-1].clamped, (kind, name)
            assert np.array_equal(got[3], want[3]), (kind, name, "state after the flush")
        # state bytes mid-stream: the same samples in other pushes leave the same bytes
        a = StreamLeveller(R.TARGET, rate, "cpu")
        b = StreamLeveller(R.TARGET, rate, "cpu")
        n = 7 * hop + 13
        a.push(x[:n])
        for lo in range(0, n, 331):
            b.push(x[lo: min(lo + 331, n)])
            by_hops_zbar = b.rec.zbar
        assert np.array_equal(a.state.numpy(), b.state.numpy()) and a.rec.zbar == by_hops_zbar


def test_every_records_zbar_is_the_running_measure():
    rate, x = 8000, R.signal("gating", 8000)
    ref = R.reference("gating", rate)
    _, per_hop, _, _, _ = _by_hops(x, rate, ref.hops)
    zbar_after = {h + 1: r.zbar for h, r in enumerate(per_hop[:-1])}       # after h complete hops
    zbar_after[0] = 0.0
    s, at = StreamLeveller(R.TARGET, rate, "cpu"), 0
    for n in R.cuts(len(x), R.knot(1, rate), seed=5)["random"]:
        s.push(x[at: at + n])
        at += n
        assert s.rec.zbar == zbar_after[min(at // 800, ref.hops)], at


def _db(a):
    return 20.0 * math.log10(a)


def test_the_rule_itself():
    rate = 8000
    # slew and the gain range: a quiet stream lifts the gain as fast as the slew lets it and no further than max_gain_db
    quiet = (LR.noise(4 * rate, seed=3) * np.float32(1e-2)).astype(np.float32)
    s = StreamLeveller(-18.0, rate, "cpu", max_gain_db=12.0, slew_db_s=30.0)
    s.push(quiet)
    A = s.knot_gains()
    r = 10.0 ** (30.0 * 0.1 / 20.0)
    # |20 log10(A[h+1] / A[h])| <= slew * 0.1, held in the ratio domain where one ulp can be told: log10 has a rounding of its own
    assert np.all(A[1:] <= A[:-1] * r * (1 + ULP)) and np.all(A[1:] >= A[:-1] / r * (1 - ULP))
    assert np.any(A[1:] == A[:-1] * r)                      # and the slew is what held it back on the way up
    assert A.max() == 10.0 ** (12.0 / 20.0) and A[0] == 1.0 and A[1] == 1.0
    # the peak limit: a knot's gain keeps the peak so far under the limit, or is falling as fast as the slew lets it
    x = LR.sine(997.0, 5.0, rate, amp=0.05)
    x[2 * rate] = 0.9
    s = StreamLeveller(-10.0, rate, "cpu", peak_limit=0.5)
    out = s.push(x)
    A, r = s.knot_gains(), 10.0 ** (10.0 * 0.1 / 20.0)
    for h in range(1, len(A) - 1):
        P = float(np.abs(x[: R.knot(h, rate)]).max())
        assert A[h + 1] * P <= 0.5 * (1 + ULP) or A[h + 1] <= A[h] / r * (1 + ULP), h
    assert A[-1] * float(np.float32(0.9)) <= 0.5 * (1 + ULP) and A[19] * 0.05 > 0.1
    # clamped samples are counted and sit at the limit
    assert s.rec.clamped == int((np.abs(out) == np.float32(0.5)).sum()) >= 1 and s.rec.limited
    assert float(np.abs(out).max()) == 0.5
    # zeros come back bit for bit, at gain 1
    z = np.zeros(3 * rate, np.float32)
    z[::2] = -0.0
    s = StreamLeveller(-18.0, rate, "cpu")
    out = s.push(z, flush=True)
    assert np.array_equal(out.view(np.uint32), z.view(np.uint32)) and np.all(s.knot_gains() == 1.0)
    assert s.rec.lufs == -math.inf and not s.rec.measured and s.rec.gain_last == 1.0
    # a seed sets the first gain
    s = StreamLeveller(-18.0, rate, "cpu", seed=-27.5)
    s.push(z[:10])
    k, seed_z = 10.0 ** ((-18.0 + 0.691) / 10.0), 10.0 ** ((-27.5 + 0.691) / 10.0)
    assert s.knot_gains()[0] == math.sqrt(k / seed_z) and s.rec.gain_first == np.float32(math.sqrt(k / seed_z))
    assert StreamLeveller(-18.0, rate, "cpu", seed=-60.0).knot_gains()[0] == 10.0       # clamped to max_gain_db


def test_a_nan_freezes_the_gain():
    rate = 8000
    x = LR.noise(3 * rate, seed=9, amp=0.02)
    x[12 * 800 + 5] = np.nan
    x[20 * 800] = np.inf
    s = StreamLeveller(-18.0, rate, "cpu")
    out = s.push(x[: 16000])
    A = s.knot_gains()
    assert s.rec.nonfinite and len(A) == 14 and s.rec.blocks == 9         # hops 0 .. 11 were measured; knot 13 is the last
    assert np.isnan(out[12 * 800 + 5]) and np.isfinite(np.delete(out, 12 * 800 + 5)).all()
    assert np.all(out[13 * 800: 16000] == x[13 * 800: 16000] * np.float32(A[13]))
    out2 = s.push(x[16000:])
    assert s.rec.nonfinite and np.array_equal(s.knot_gains(), A) and s.rec.gain_first == s.rec.gain_last == np.float32(A[13])
    assert abs(out2[0]) == 1.0 and s.rec.clamped >= 1                     # the infinity is set to the limit
    ref = R.Run(x, rate, -18.0)
    assert ref.nonfinite and np.allclose(A, ref.A, rtol=GAIN_BOUND, atol=0.0)
    # a flush starts a fresh stream
    s.push(x[:0], flush=True)
    s.push(x[:800])
    assert not s.rec.nonfinite and len(s.knot_gains()) == 3


def test_a_full_history_freezes_the_gain():
    rate = 8000
    x = LR.noise(4 * rate, seed=11, amp=0.02)
    s = StreamLeveller(-18.0, rate, "cpu", max_seconds=2)
    s.push(x[: 2 * rate - 1])
    assert not s.rec.full and s.rec.blocks == 16
    s.push(x[2 * rate - 1: 3 * rate])
    A = s.knot_gains()
    assert s.rec.full and s.rec.blocks == 17 and len(A) == 22
    out = s.push(x[3 * rate:])
    assert s.rec.full and s.rec.blocks == 17 and np.array_equal(s.knot_gains(), A)
    assert np.array_equal(out, x[3 * rate:] * np.float32(A[21]))
    ref = R.Run(x, rate, -18.0, max_seconds=2)
    assert ref.full and len(ref.A) == 22 and np.allclose(A, ref.A, rtol=GAIN_BOUND, atol=0.0)


AGREE_BOUND = 4 * 1.5e-8        # LU: four times the worst case measured here, 1.42e-8 (the clip meter keeps its filtered signal in fp32)


def test_agreement_with_the_clip_meter():
    """the stream's final measure against loudness.measure of the same samples cut where the last measured block ends: the same
    blocks through the same gates, summed hop by hop here and block by block there"""
    worst = 0.0
    for rate in R.RATES:
        for kind in ("noise", "sine997", "sine60", "gating"):
            x = R.signal(kind, rate)
            s = StreamLeveller(R.TARGET, rate, "cpu")
            s.push(x)
            nb = s.rec.blocks
            clip = loudness.measure(x[: R.knot(nb + 3, rate)], rate, device="cpu")
            assert (clip.blocks, clip.above_abs, clip.kept) == (nb, s.rec.above_abs, s.rec.kept), (kind, rate)
            worst = max(worst, abs(s.lufs - clip.lufs))
    print("stream against clip meter: worst %.3g LU" % worst)
    assert worst <= AGREE_BOUND


CONVERGE_BOUND = 4 * 7.3e-5     # LU: four times the oracle's own deviation from the target over the last second, 7.22e-5


def test_convergence():
    rate = 32000
    x = LR.sine(997.0, 4.0, rate, amp=1.0)
    x = (x * np.float32(10.0 ** ((-30.0 - LR.Measurement(x, rate).lufs) / 20.0))).astype(np.float32)
    assert abs(LR.Measurement(x, rate).lufs + 30.0) < 1e-3
    ref = R.Run(x, rate, -18.0)
    own = abs(LR.Measurement(ref.out[-rate:], rate).lufs + 18.0)
    out, rec = lv.level(x, rate, -18.0, device="cpu")
    got = loudness.integrated_loudness(out[-rate:], rate, device="cpu")
    print("last second: %.5f LUFS; the oracle's deviation %.3g LU" % (got, own))
    assert own <= CONVERGE_BOUND / 4 * 1.01 and abs(got + 18.0) <= CONVERGE_BOUND
    assert abs(rec.lufs + 30.0) < 0.01 and abs(_db(float(rec.gain_last)) - 12.0) < 0.01 and not rec.limited


def test_no_state_outlives_its_stream():
    """the state is built per stream: a seed differs from call to call, and nothing keyed by it may be kept"""
    import gc
    import torch

    def held():
        sizes = {k: len(v) for k, v in vars(StreamLeveller).items() if isinstance(v, (dict, list, set))}
        sizes.update({"level." + k: len(v) for k, v in vars(lv).items() if isinstance(v, (dict, list, set)) and not k.startswith("__")})
        gc.collect()
        big = sum(1 for o in gc.get_objects() if type(o) is torch.Tensor and o.dtype == torch.uint8 and o.numel() > 100000)
        return sizes, big
    StreamLeveller(-18.0, 32000, "cpu", seed=-20.0).push(np.zeros(10, np.float32))
    before = held()
    for i in range(40):
        s = StreamLeveller(-18.0, 32000, "cpu", seed=-20.0 - 0.01 * i)
        s.push(np.zeros(10, np.float32), flush=True)
    del s
    assert held() == before


def test_the_seed_of_a_stream():
    from gsv_tts_lite_amd.tts import _check_loudness_seed
    assert _check_loudness_seed(None) is None and _check_loudness_seed(-math.inf) is None and _check_loudness_seed(-23.5) == -23.5
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError, match="loudness seed"):
            _check_loudness_seed(bad)


def test_argument_checks():
    from gsv_tts_lite_amd import _native as N
    L = N.lib()
    assert L.gsv_level_state_bytes(3999, 600) == 0 and L.gsv_level_state_bytes(192001, 600) == 0
    assert L.gsv_level_state_bytes(32000, 0) == 0 and L.gsv_level_state_bytes(32000, 3601) == 0
    need = L.gsv_level_state_bytes(8000, 2)
    state = np.zeros(need + 16, np.uint8)
    base = state.ctypes.data + (-state.ctypes.data) % 16
    good = (8000, -18.0, float("nan"), 10.0, 10.0, 20.0, 1.0, 2)
    assert L.gsv_level_init_host(base, need, *good) == 0
    x, rec = np.zeros(10, np.float32), np.zeros(5, np.int64)
    bad = [L.gsv_level_init_host(None, need, *good), L.gsv_level_init_host(base, need - 1, *good),
           L.gsv_level_init_host(base + 4, need, *good),
           L.gsv_level_init_host(base, need, 8000, float("nan"), float("nan"), 10.0, 10.0, 20.0, 1.0, 2),
           L.gsv_level_init_host(base, need, 8000, -18.0, float("inf"), 10.0, 10.0, 20.0, 1.0, 2),
           L.gsv_level_init_host(base, need, 8000, -18.0, float("nan"), 0.0, 10.0, 20.0, 1.0, 2),
           L.gsv_level_init_host(base, need, 8000, -18.0, float("nan"), 10.0, -1.0, 20.0, 1.0, 2),
           L.gsv_level_init_host(base, need, 8000, -18.0, float("nan"), 10.0, 10.0, -1.0, 1.0, 2),
           L.gsv_level_init_host(base, need, 8000, -18.0, float("nan"), 10.0, 10.0, 20.0, 0.0, 2),
           L.gsv_level_push_host(None, x.ctypes.data, 10, None, 0, x.ctypes.data, rec.ctypes.data),
           L.gsv_level_push_host(base, None, 10, None, 0, x.ctypes.data, rec.ctypes.data),
           L.gsv_level_push_host(base, x.ctypes.data, -1, None, 0, x.ctypes.data, rec.ctypes.data),
           L.gsv_level_push_host(base, x.ctypes.data, 10, None, 0, None, rec.ctypes.data),
           L.gsv_level_push_host(base, x.ctypes.data, 10, None, 0, x.ctypes.data, None),
           L.gsv_level_push_host(base, x.ctypes.data, 10, None, 0, x.ctypes.data, rec.ctypes.data + 4),
           L.gsv_level_push_host(rec.ctypes.data, x.ctypes.data, 10, None, 0, x.ctypes.data, rec.ctypes.data)]
    assert bad == [1] * len(bad), bad
    with pytest.raises(ValueError):
        StreamLeveller(-18.0, 2000)
    with pytest.raises(RuntimeError):
        StreamLeveller(float("nan"), 8000)
    # a host-held length is honoured, in place
    y = np.full(10, 0.25, np.float32)
    n = np.array([4], np.int32)
    assert L.gsv_level_push_host(base, y.ctypes.data, 10, n.ctypes.data, 1, y.ctypes.data, rec.ctypes.data) == 0
    assert lv.record(rec.view(np.uint8)).gain_last == 1.0 and np.all(y == 0.25)
