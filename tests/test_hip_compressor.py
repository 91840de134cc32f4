"""GPU parity of the compressor (csrc/compressor.h behind gsv_compressor) against its host twin gsv_compressor_host, which
tests/test_compressor_cpu.py pins to the fp64 definition: the same record bytes and the same samples, bit for bit, over the CPU
test's whole grid -- every length around a run (16), a span (8192) and a chunk (two spans; 3 chunks + 5 chains three chunk states)
with every signal and every parameter set -- as one packed call per rate, with the denormal clip beside it; a mixed batch of nine
clips over three parameter sets and -1 with guard words before, between and behind; in place equal to out of place; a measure-only
clip moves nothing; non-finite clips come back as they were; the module on the device equals the module on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compressor_ref as R  # noqa: E402
import compressor_cases as C  # noqa: E402

from gsv_tts_lite_amd import compressor as CM  # noqa: E402

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
NAMES = list(R.SETS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _params(rate):
    return [np.array(R.coefficients(R.SETS[n], rate), np.float64) for n in NAMES]


@pytest.mark.parametrize("rate", R.RATES)
def test_the_grid_of_the_cpu_test_on_the_device(dev, rate):
    g = R.grid(rate)
    clips = [x for _, _, _, x in g]
    index = [NAMES.index(name) for name, _, _, _ in g]
    params = _params(rate)
    xd, cod = R.denormal_clip()                     # its own parameter set (a 1 ms release at 8 kHz), whatever the rate of the cell
    clips.append(xd)
    index.append(len(params))
    params.append(np.array(cod))
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = C.call(x, offsets, lengths, index, params, CPU)
    got_out, got_rec, x_after = C.call(x, offsets, lengths, index, params, dev)
    for i, (n, o) in enumerate(zip(lengths, offsets)):
        cell = (rate,) + (g[i][:3] if i < len(g) else ("denormal",))
        assert got_rec[16 * i: 16 * i + 16] == want_rec[16 * i: 16 * i + 16], cell
        assert got_out[o: o + n].tobytes() == want_out[o: o + n].tobytes(), cell
    assert got_out.tobytes() == want_out.tobytes() and x_after.tobytes() == x.tobytes()
    recs = C.recs_of(got_rec)
    assert all(r.compressed == (k != "quiet") for r, (_, n, k, _) in zip(recs, g) if k == "quiet" or n > R.CHUNK) and recs[-1].compressed
    got_in, rec_in, _ = C.call(x, offsets, lengths, index, params, dev, "inplace")
    assert rec_in == want_rec
    mask = np.zeros(len(x), bool)
    for n, o in zip(lengths, offsets):
        mask[o: o + n] = True
    assert got_in[mask].tobytes() == want_out[mask].tobytes() and np.all(got_in[~mask] == C.FILL)


def test_a_mixed_batch_over_three_parameter_sets(dev):
    rate = 48000
    rng = np.random.default_rng(11)
    noise = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    nan = noise(R.CHUNK + 100)
    nan[R.SPAN + 3] = np.nan
    inf = noise(3000)
    inf[2999] = -np.inf
    clips = [noise(R.CHUNK + 1), noise(777), np.zeros(0, np.float32), nan, R.grid_signal("gated220", 3 * R.SPAN + 5, rate, "voice"), inf,
             noise(2 * R.CHUNK), noise(1), noise(5 * R.CHUNK - R.SPAN - 1)]
    index = [0, 1, 2, 2, 1, 0, -1, 1, 2]
    params = _params(rate)[:3]
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = C.call(x, offsets, lengths, index, params, CPU)
    mask = np.zeros(len(x), bool)
    for n, o in zip(lengths, offsets):
        mask[o: o + n] = True
    for mode in ("out", "inplace"):
        got, rec, x_after = C.call(x, offsets, lengths, index, params, dev, mode)
        assert rec == want_rec
        assert got[mask].tobytes() == want_out[mask].tobytes()
        assert np.all(got[~mask] == (C.FILL * 2 if mode == "out" else C.FILL)), "written outside a clip"
        if mode == "out":
            assert x_after.tobytes() == x.tobytes()
    recs = C.recs_of(rec)
    assert [r.compressed for r in recs] == [True, True, False, False, True, False, False, True, True]
    assert [r.nonfinite for r in recs] == [False, False, False, True, False, True, False, False, False]
    for i in (3, 5, 6):                                 # NaN, infinity, measure only: bit for bit what came in
        o = offsets[i]
        assert got[o: o + lengths[i]].tobytes() == clips[i].tobytes()
    assert recs[6].peak_in == recs[6].peak_out == np.abs(clips[6]).max() and recs[6].min_gain == 1
    o = offsets[8]
    assert recs[8].peak_out == np.abs(got[o: o + lengths[8]]).max() and recs[8].min_gain < 1
    # measure only over the whole batch, in place: records of the peaks, no sample moves
    got, rec, _ = C.call(x, offsets, lengths, [-1] * len(clips), [], dev, "inplace")
    assert got.tobytes() == x.tobytes() and rec == C.call(x, offsets, lengths, [-1] * len(clips), [], CPU, "inplace")[1]


def test_module_on_the_device_equals_the_cpu(dev):
    rate = 32000
    rng = np.random.default_rng(2)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in (5000, R.CHUNK + 7, 0, 300)]
    cs = ["voice", CM.Compressor(*R.SETS["slow"]), "voice", None]
    ys, recs = CM.compress(clips, rate, cs, device=dev)
    ys_c, recs_c = CM.compress(clips, rate, cs, device="cpu")
    for y, yc, r, rc in zip(ys, ys_c, recs, recs_c):
        assert isinstance(y, np.ndarray) and y.tobytes() == yc.tobytes()
        assert (r.peak_in, r.peak_out, r.min_gain, r.compressed) == (rc.peak_in, rc.peak_out, rc.min_gain, rc.compressed)
    assert recs[0].compressed and recs[1].compressed and not recs[2].compressed and not recs[3].compressed
    t = torch.from_numpy(clips[0]).to(dev)
    y, r = CM.compress(t, rate, "voice")                    # a device tensor stays on its device
    assert y.device == t.device and y.cpu().numpy().tobytes() == ys_c[0].tobytes() and r.peak_out == recs_c[0].peak_out
