"""GPU parity of the reverb (csrc/reverb.h behind gsv_reverb) against its host twin gsv_reverb_host, which tests/test_reverb_cpu.py
pins to the serial fp64 definition: the same record bytes and the same samples, bit for bit, over the CPU test's whole grid --
every length around the shortest and the longest delay, up to three wraps of the longest line, with every signal -- as one packed
call per parameter family, plus the cell with the longest legal line (28 160 samples: the combs read their lines back from the
workspace, in spans with a short last one); a mixed batch of nine clips over three parameter sets and -1 with guard words before,
between and behind; in place equal to out of place; non-finite clips come back as they were; the module on the device equals the
module on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverb_ref as R  # noqa: E402
import reverb_cases as C  # noqa: E402

from gsv_tts_lite_amd import reverb as RV  # noqa: E402

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
FAMILIES = {"voice": ("voice8", "voice32", "voice48"), "hall": ("hall",), "tiny": ("tiny",)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cells(names):
    """the clips of the named sets without their oracle (the twin is the reference here) -> (labels, clips, index, params)"""
    labels, clips, index = [], [], []
    for k, name in enumerate(names):
        ps, rate = R.SETS[name]
        for n in R.lengths(ps):
            for s, kind in enumerate(R.KINDS):
                labels.append((name, n, kind))
                clips.append(R.signal(kind, n, rate, seed=s))
                index.append(k)
    return labels, clips, index, [C.params_of(R.SETS[name][0]) for name in names]


def _mask(x, lengths, offsets):
    mask = np.zeros(len(x), bool)
    for n, o in zip(lengths, offsets):
        mask[o: o + n] = True
    return mask


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_grid_of_the_cpu_test_on_the_device(dev, family):
    labels, clips, index, params = _cells(FAMILIES[family])
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = C.call(x, offsets, lengths, index, params, CPU)
    got_out, got_rec, x_after = C.call(x, offsets, lengths, index, params, dev)
    for i, (n, o) in enumerate(zip(lengths, offsets)):
        assert got_rec[16 * i: 16 * i + 16] == want_rec[16 * i: 16 * i + 16], labels[i]
        assert got_out[o: o + n].tobytes() == want_out[o: o + n].tobytes(), labels[i]
    assert got_out.tobytes() == want_out.tobytes() and x_after.tobytes() == x.tobytes()
    assert all(r.reverbed and not r.nonfinite for r in C.recs_of(got_rec))
    got_in, rec_in, _ = C.call(x, offsets, lengths, index, params, dev, "inplace")
    assert rec_in == want_rec
    mask = _mask(x, lengths, offsets)
    assert got_in[mask].tobytes() == want_out[mask].tobytes() and np.all(got_in[~mask] == C.FILL)


def test_the_longest_legal_line(dev):
    x1, _ = R.long_cell(False)
    assert max(R.LONG[0]) == 28160 > RV.N.RVB_SPAN and len(x1) == 2 * 28160 + 5
    x, offsets = C.pack([x1])
    want_out, want_rec, _ = C.call(x, offsets, [len(x1)], [0], [C.params_of(R.LONG)], CPU)
    for mode in ("out", "inplace"):
        got, rec, _ = C.call(x, offsets, [len(x1)], [0], [C.params_of(R.LONG)], dev, mode)
        assert rec == want_rec
        o = offsets[0]
        assert got[o: o + len(x1)].tobytes() == want_out[o: o + len(x1)].tobytes()
        assert np.all(got[:o] == (C.FILL * 2 if mode == "out" else C.FILL)) and np.all(got[o + len(x1):] == got[0])


def test_a_mixed_batch_over_three_parameter_sets(dev):
    rng = np.random.default_rng(11)
    noise = lambda n: rng.uniform(-1, 1, n).astype(np.float32)
    nan = noise(4000)
    nan[2049] = np.nan
    inf = noise(3000)
    inf[2999] = -np.inf
    clips = [noise(5001), noise(777), np.zeros(0, np.float32), nan, R.signal("gated220", 6151, 48000), inf, noise(9000), noise(1), noise(12345)]
    index = [0, 1, 2, 2, 1, 0, -1, 1, 2]
    params = [C.params_of(R.SETS[n][0]) for n in ("voice32", "voice48", "tiny")]
    x, offsets = C.pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = C.call(x, offsets, lengths, index, params, CPU)
    mask = _mask(x, lengths, offsets)
    for mode in ("out", "inplace"):
        got, rec, x_after = C.call(x, offsets, lengths, index, params, dev, mode)
        assert rec == want_rec
        assert got[mask].tobytes() == want_out[mask].tobytes()
        assert np.all(got[~mask] == (C.FILL * 2 if mode == "out" else C.FILL)), "written outside a clip"
        if mode == "out":
            assert x_after.tobytes() == x.tobytes()
    recs = C.recs_of(rec)
    assert [r.reverbed for r in recs] == [True, True, True, False, True, False, False, True, True]
    assert [r.nonfinite for r in recs] == [False, False, False, True, False, True, False, False, False]
    for i in (3, 5, 6):                                 # NaN, infinity, measure only: bit for bit what came in
        o = offsets[i]
        assert got[o: o + lengths[i]].tobytes() == clips[i].tobytes()
    assert recs[6].peak_in == recs[6].peak_out == np.abs(clips[6]).max()
    o = offsets[8]
    assert recs[8].peak_out == np.abs(got[o: o + lengths[8]]).max() and recs[8].peak_in == np.abs(clips[8]).max()
    # measure only over the whole batch, in place: records of the peaks, no sample moves
    got, rec, _ = C.call(x, offsets, lengths, [-1] * len(clips), [], dev, "inplace")
    assert got.tobytes() == x.tobytes() and rec == C.call(x, offsets, lengths, [-1] * len(clips), [], CPU, "inplace")[1]


def test_module_on_the_device_equals_the_cpu(dev):
    rate = 32000
    rng = np.random.default_rng(2)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in (5000, 2500, 0, 300)]
    rs = ["voice", RV.Reverb(*R.HALL), "voice", None]
    ys, recs = RV.reverberate(clips, rate, rs, device=dev)
    ys_c, recs_c = RV.reverberate(clips, rate, rs, device="cpu")
    for y, yc, r, rc in zip(ys, ys_c, recs, recs_c):
        assert isinstance(y, np.ndarray) and y.tobytes() == yc.tobytes()
        assert (r.peak_in, r.peak_out, r.reverbed, r.nonfinite) == (rc.peak_in, rc.peak_out, rc.reverbed, rc.nonfinite)
    assert [r.reverbed for r in recs] == [True, True, True, False]
    t = torch.from_numpy(clips[0]).to(dev)
    y, r = RV.reverberate(t, rate, "voice")                 # a device tensor stays on its device
    assert y.device == t.device and y.cpu().numpy().tobytes() == ys_c[0].tobytes() and r.peak_out == recs_c[0].peak_out
