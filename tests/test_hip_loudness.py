"""GPU parity of the loudness meter (csrc/loudness.h behind gsv_loudness) against its host twin gsv_loudness_host, which
tests/test_loudness_cpu.py pins to the fp64 definition: the same record bytes and the same scaled samples, bit for bit, for a
packed batch of mixed-length clips; nothing written outside the clips or behind the stated workspace; in place equal to out of
place; a measure-only target leaves the samples alone.  A block walks a chunk of a clip span by span (8192 samples, two to a
chunk) and the chunks of a clip run side by side with their states chained, so the batch holds clips that end inside the first
span, exactly on a chunk boundary (2 spans at 8 and 32 kHz), one sample behind it, on a span boundary inside a chunk (3 spans at
44.1 kHz) and six chunks later (the gating signal)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import loudness as LD  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 5           # odd, so every clip starts at an odd offset
FILL = np.float32(-7.25)
SPAN = 512 * 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(rate):
    """(clips, targets): about 8 mixed-length clips"""
    k = 2 if rate < 40000 else 3                # k spans hold a whole 400 ms block at this rate
    nan = R.noise(k * SPAN + 1, seed=3).copy()
    nan[SPAN + 3] = np.nan
    clips = [R.gating_signal(rate), np.zeros(0, np.float32), R.noise(int(0.4 * rate) - 1, seed=1), R.noise(k * SPAN, seed=2), nan,
             R.sine(60.0, 2.2, rate)[: k * SPAN + 1], R.noise(int(0.55 * rate), seed=4), np.zeros(3 * SPAN // 2, np.float32),
             R.sine(997.0, 0.5, rate)]
    assert len(clips[3]) == k * SPAN and len(clips[5]) == k * SPAN + 1
    targets = [-18.0, -18.0, -18.0, 0.0, -18.0, None, -23.0, -18.0, -30.0]
    return clips, targets


def _pack(clips):
    """one buffer with GUARD words before, between and after the clips"""
    n_x = GUARD + sum(len(c) + GUARD for c in clips)
    x = np.full(n_x, FILL, np.float32)
    offsets, at = [], GUARD
    for c in clips:
        x[at: at + len(c)] = c
        offsets.append(at)
        at += len(c) + GUARD
    return x, offsets


def _call(x, offsets, lengths, targets, rate, device, mode, peak_limit=1.0):
    """the raw call -> (out buffer as numpy or None, record bytes, x afterwards); mode: 'none', 'inplace', 'out'.  On the GPU the
    workspace has guard bytes behind its stated size, checked here."""
    L = N.lib()
    n = len(lengths)
    arr = (N.LoudnessClip * n)(*[N.LoudnessClip(o, l, float("nan") if t is None else t) for o, l, t in zip(offsets, lengths, targets)])
    need = L.gsv_loudness_work_bytes(arr, n, rate)
    assert need > 0
    xt = torch.from_numpy(x.copy()).to(device)
    work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=device)
    rec = torch.full((n * 32 + 32,), 0xA5, dtype=torch.uint8, device=device)
    out = {"none": None, "inplace": xt, "out": torch.full_like(xt, float(FILL) * 2)}[mode]
    args = (xt.data_ptr(), xt.numel(), arr, n, rate, peak_limit, None if out is None else out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)
    if device.type == "cuda":
        N.check(L.gsv_loudness(*args, N.current_stream_ptr(device)))
        torch.cuda.synchronize(device)
    else:
        N.check(L.gsv_loudness_host(*args))
    assert bool((work[need:] == 0xA5).all()), "written behind the stated workspace"
    recb = rec.cpu().numpy()
    assert np.all(recb[n * 32:] == 0xA5), "written behind the records"
    return (None if out is None else out.cpu().numpy()), recb[: n * 32].tobytes(), xt.cpu().numpy()


@pytest.mark.parametrize("rate", [32000, 8000, 44100])
def test_device_records_and_samples_equal_the_twin(dev, rate):
    clips, targets = _batch(rate)
    x, offsets = _pack(clips)
    lengths = [len(c) for c in clips]
    cpu = torch.device("cpu")
    want_out, want_rec, _ = _call(x, offsets, lengths, targets, rate, cpu, "out")
    got_out, got_rec, x_after = _call(x, offsets, lengths, targets, rate, dev, "out")
    assert got_rec == want_rec
    assert x_after.tobytes() == x.tobytes()                                  # out of place: the input is not touched
    recs = LD.records(torch.frombuffer(bytearray(got_rec), dtype=torch.uint8))
    # the twin's records are the sane ones: the batch exercises every kind of clip
    assert recs[0].kept == 14 and recs[0].blocks == 27 and not recs[0].limited and recs[0].gain != 1
    assert [r.measured for r in recs] == [True, False, False, True, False, True, True, False, True]
    assert recs[3].limited and recs[4].nonfinite and recs[5].gain == 1 and recs[6].blocks == 3
    # inside the clips the twin's samples; the guards before, between and after untouched
    mask = np.zeros(len(x), bool)
    for o, n, c, r in zip(offsets, lengths, clips, recs):
        mask[o: o + n] = True
        assert got_out[o: o + n].tobytes() == want_out[o: o + n].tobytes()
        if r.gain == 1:
            assert got_out[o: o + n].tobytes() == c.tobytes()
        else:
            assert np.array_equal(got_out[o: o + n], c * r.gain)
    assert np.all(got_out[~mask] == FILL * 2), "written outside a clip"
    # in place: the same samples, the guards still the input's
    got_in, rec_in, _ = _call(x, offsets, lengths, targets, rate, dev, "inplace")
    assert rec_in == want_rec
    assert got_in[mask].tobytes() == got_out[mask].tobytes() and np.all(got_in[~mask] == FILL)
    # measure only, by a null `out` or by NaN targets: the same measurement, no sample moves
    _, rec_m, x_m = _call(x, offsets, lengths, [None] * len(clips), rate, dev, "none")
    _, rec_n, x_n = _call(x, offsets, lengths, [None] * len(clips), rate, dev, "inplace")
    assert rec_m == rec_n and x_m.tobytes() == x.tobytes() and x_n.tobytes() == x.tobytes()
    for a, b in zip(LD.records(torch.frombuffer(bytearray(rec_m), dtype=torch.uint8)), recs):
        assert a.zbar == b.zbar and a.peak.tobytes() == b.peak.tobytes() and a.gain == 1 and (a.blocks, a.above_abs, a.kept) == (b.blocks, b.above_abs, b.kept)


@pytest.mark.parametrize("rate", sorted(R.LENGTHS))
def test_the_grid_of_the_cpu_test_on_the_device(dev, rate):
    """every length of the CPU test's grid (around one block, a span and a chunk; 0 and 1 sample) with every one of its signals, as one
    packed call per rate: record bytes and scaled samples equal the twin's, guards untouched"""
    clips = [R.grid_signal(k, n, rate) for n in R.LENGTHS[rate] for k in R.KINDS]
    assert all(len(c) == n for c, n in zip(clips, [n for n in R.LENGTHS[rate] for _ in R.KINDS]))
    targets = [(-18.0, -30.0, None, 0.0)[i % 4] for i in range(len(clips))]
    targets = targets[1:] + targets[:1]                     # every signal meets every kind of target over the lengths
    x, offsets = _pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = _call(x, offsets, lengths, targets, rate, torch.device("cpu"), "out")
    got_out, got_rec, x_after = _call(x, offsets, lengths, targets, rate, dev, "out")
    for i, (n, k) in enumerate((n, k) for n in R.LENGTHS[rate] for k in R.KINDS):
        assert got_rec[32 * i: 32 * i + 32] == want_rec[32 * i: 32 * i + 32], (rate, n, k)
        o = offsets[i]
        assert got_out[o: o + n].tobytes() == want_out[o: o + n].tobytes(), (rate, n, k)
    assert got_out.tobytes() == want_out.tobytes() and x_after.tobytes() == x.tobytes()
    recs = LD.records(torch.frombuffer(bytearray(got_rec), dtype=torch.uint8))
    by = {(n, k): r for (n, k), r in zip(((n, k) for n in R.LENGTHS[rate] for k in R.KINDS), recs)}
    if rate == 32000:
        assert [by[(n, "noise")].blocks for n in (12799, 12800, 14400, 17600, 20800, 22400)] == [0, 1, 1, 3, 3, 4]
        assert all(by[(n, k)].measured for n in (12800, 14400, 22400) for k in ("noise", "sine997", "sine60"))
    assert sum(r.limited for r in recs) > 0 and sum(r.measured for r in recs) >= len(recs) // 3


def test_module_on_the_device_equals_the_cpu(dev):
    rate = 32000
    clips, targets = _batch(rate)
    ys, recs = LD.normalise(clips, rate, targets, device=dev)
    ys_c, recs_c = LD.normalise(clips, rate, targets, device="cpu")
    for y, yc, r, rc in zip(ys, ys_c, recs, recs_c):
        assert isinstance(y, np.ndarray) and y.tobytes() == yc.tobytes()
        assert (r.zbar, r.gain, r.limited, r.kept) == (rc.zbar, rc.gain, rc.limited, rc.kept)
    t = torch.from_numpy(clips[0]).to(dev)
    y, r = LD.normalise(t, rate, -18.0)                        # a device tensor stays on its device
    assert y.device == t.device and y.cpu().numpy().tobytes() == ys_c[0].tobytes()
    assert LD.integrated_loudness(t, rate) == recs_c[0].lufs
