"""GPU parity of the true-peak limiter (csrc/limiter.h behind gsv_limiter) against its host twin gsv_limiter_host, which
tests/test_limiter_cpu.py pins to the fp64 definition: the same record bytes and the same samples, bit for bit, over the CPU test's
grid as one packed call with mixed ceilings; nothing written outside the clips or behind the stated workspace; in place equal to
out of place; measuring alone moves no sample.  Then the facade: true_peak= on TTS.infer, infer_vc and infer_batched.

The grid's lengths sit on every edge of the kernels: the 12 taps and the 6-sample halo of the envelope block (0, 1, 11, 12, 13), the
look-ahead of 48 (47, 48, 49, 95, 97), the scan tile of 1024 (TILE - 1, TILE, TILE + 1) and a third tile with a halo that reaches
back over a tile edge (2 TILE + 47); at 44.1 kHz the look-ahead is 66 and the release 2205 samples, more than two tiles."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as R  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 5           # odd, so clips start at odd offsets
FILL = np.float32(-7.25)
CEILINGS = (-1.0, -3.0, None, -0.1)
EPS, S = 2.0 ** -24, R.phase_sum()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def _call(x, offsets, lengths, ceilings, rate, device, mode):
    """the raw call -> (out buffer as numpy or None, record bytes, x afterwards); mode: 'none', 'inplace', 'out'.  The workspace and
    the records have guard bytes behind their stated sizes, checked here."""
    L = N.lib()
    n = len(lengths)
    arr = (N.LimiterClip * n)(*[N.LimiterClip(o, l, float("nan") if c is None else c) for o, l, c in zip(offsets, lengths, ceilings)])
    need = L.gsv_limiter_work_bytes(arr, n)
    assert need > 0
    look, rel = LM.times(rate)
    xt = torch.from_numpy(x.copy()).to(device)
    work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=device)
    rec = torch.full((n * 32 + 32,), 0xA5, dtype=torch.uint8, device=device)
    out = {"none": None, "inplace": xt, "out": torch.full_like(xt, float(FILL) * 2)}[mode]
    args = (xt.data_ptr(), xt.numel(), arr, n, look, rel, None if out is None else out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)
    if device.type == "cuda":
        N.check(L.gsv_limiter(*args, N.current_stream_ptr(device)))
        torch.cuda.synchronize(device)
    else:
        N.check(L.gsv_limiter_host(*args))
    assert bool((work[need:] == 0xA5).all()), "written behind the stated workspace"
    recb = rec.cpu().numpy()
    assert np.all(recb[n * 32:] == 0xA5), "written behind the records"
    return (None if out is None else out.cpu().numpy()), recb[: n * 32].tobytes(), xt.cpu().numpy()


@pytest.mark.parametrize("rate", [32000, 44100])
def test_device_records_and_samples_equal_the_twin(dev, rate):
    grid = [(n, k) for n in R.LENGTHS for k in R.KINDS]
    clips = [R.grid_signal(k, n, rate) for n, k in grid]
    ceilings = [CEILINGS[(i + i // len(R.KINDS)) % 4] for i in range(len(clips))]     # every signal meets every ceiling over the lengths
    x, offsets = _pack(clips)
    lengths = [len(c) for c in clips]
    want_out, want_rec, _ = _call(x, offsets, lengths, ceilings, rate, torch.device("cpu"), "out")
    got_out, got_rec, x_after = _call(x, offsets, lengths, ceilings, rate, dev, "out")
    for i, (n, k) in enumerate(grid):
        assert got_rec[32 * i: 32 * i + 32] == want_rec[32 * i: 32 * i + 32], (rate, n, k, ceilings[i])
        o = offsets[i]
        assert got_out[o: o + n].tobytes() == want_out[o: o + n].tobytes(), (rate, n, k, ceilings[i])
    assert got_out.tobytes() == want_out.tobytes() and x_after.tobytes() == x.tobytes()     # guards and input untouched
    recs = LM.records(torch.frombuffer(bytearray(got_rec), dtype=torch.uint8))
    mask = np.zeros(len(x), bool)
    for (n, k), o, c, r, clip in zip(grid, offsets, ceilings, recs, clips):
        mask[o: o + n] = True
        assert r.nonfinite == (k == "nan" and n > 0)
        if c is None or r.nonfinite or k in ("zeros", "quiet"):
            assert not r.limited and got_out[o: o + n].tobytes() == clip.tobytes()
        elif k.startswith("click") and n:
            assert r.limited and r.dbtp_out <= c + 1e-5
    assert np.all(got_out[~mask] == FILL * 2), "written outside a clip"
    assert sum(r.limited for r in recs) >= len(recs) // 3 and sum(r.trim < 1 for r in recs) > 0
    # in place: the same samples, the guards still the input's
    got_in, rec_in, _ = _call(x, offsets, lengths, ceilings, rate, dev, "inplace")
    assert rec_in == want_rec
    assert got_in[mask].tobytes() == got_out[mask].tobytes() and np.all(got_in[~mask] == FILL)
    # measure only, by a null `out` or by NaN ceilings: the same true peak, no sample moves
    _, rec_m, x_m = _call(x, offsets, lengths, ceilings, rate, dev, "none")
    _, rec_n, x_n = _call(x, offsets, lengths, [None] * len(clips), rate, dev, "inplace")
    assert rec_m == rec_n and x_m.tobytes() == x.tobytes() and x_n.tobytes() == x.tobytes()
    assert rec_m == _call(x, offsets, lengths, ceilings, rate, torch.device("cpu"), "none")[1]
    for a, b in zip(LM.records(torch.frombuffer(bytearray(rec_m), dtype=torch.uint8)), recs):
        assert a.true_peak_in.tobytes() == b.true_peak_in.tobytes() and not a.limited and a.nonfinite == b.nonfinite


def test_module_on_the_device_equals_the_cpu(dev):
    rate = 32000
    g = lambda k, n: R.grid_signal(k, n, rate)
    clips = [g("click_last", R.TILE + 1), g("quiet", 97), g("noise", 2 * R.TILE + 47), np.zeros(0, np.float32), g("nan", 49),
             g("sine997", R.TILE - 1), g("quarter", R.TILE)]
    ceilings = [-1.0, -1.0, -3.0, -1.0, -1.0, None, -0.1]
    ys, recs = LM.limit(clips, rate, ceilings, device=dev)
    ys_c, recs_c = LM.limit(clips, rate, ceilings, device="cpu")
    for y, yc, r, rc in zip(ys, ys_c, recs, recs_c):
        assert isinstance(y, np.ndarray) and y.tobytes() == yc.tobytes()
        for f in LM.LimiterRecord.__slots__:
            assert np.array_equal(getattr(r, f), getattr(rc, f), equal_nan=True), (f, r, rc)
    assert LM.true_peak(clips[:4], rate, device=dev) == LM.true_peak(clips[:4], rate, device="cpu")
    t = torch.from_numpy(clips[2]).to(dev)
    y, r = LM.limit(t, rate, -3.0)                             # a device tensor stays on its device
    assert y.device == t.device and y.cpu().numpy().tobytes() == ys_c[2].tobytes()
    assert LM.true_peak(t, rate) == recs_c[2].dbtp_in


# ---------------------------------------------------------------------------------------------------------------------------------
# the facade: the toy front end and the synthetic 6-layer models exactly as tests/test_hip_tts_loudness.py sets them up (copied)
# ---------------------------------------------------------------------------------------------------------------------------------
TWO_SEGMENTS = "willow violet. xenon tango yonder?"
THREE = [TWO_SEGMENTS, "pixel delta beta?", "yonder willow!"]
REF = ("spk.wav", "prompt.wav", "prompt text.")


def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


@pytest.fixture(scope="module")
def tts():
    assert torch.cuda.is_available()
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 160), (4, 160)], sovits_cache=[50, 55], device="cuda:0", dtype="float32")
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_toy_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    return tts


def _under(clip, ceiling):
    """the clip's own reading and the fp64 meter's, both under the ceiling within the meter's bound"""
    T = 10.0 ** (ceiling / 20.0)
    bound = 14 * EPS * S * T
    assert 10.0 ** (clip.dbtp / 20.0) <= T + bound and R.true_peak(clip.audio_data) <= T + bound, (clip.dbtp, ceiling)


def test_infer_with_a_loudness_target_and_a_ceiling(tts):
    kw = dict(top_k=1, noise_scale=0.0, return_subtitles=True)
    base = tts.infer(*REF, TWO_SEGMENTS, **kw)
    assert base.dbtp is None and base.limited is None and base.lufs is None
    assert tts.infer(*REF, TWO_SEGMENTS, true_peak=None, **kw).audio_data.tobytes() == base.audio_data.tobytes()
    acted = 0
    for target in (-14.0, -3.0):
        clip = tts.infer(*REF, TWO_SEGMENTS, loudness=target, true_peak=-1.0, **kw)
        free = base.normalised(target, peak_limit=math.inf)         # the normalisation no peak limit constrains
        want, rec = LM.limit(free.audio_data, 32000, -1.0)
        assert clip.audio_data.tobytes() == want.tobytes()
        assert clip.lufs == free.lufs and clip.gain == free.gain and clip.limited == rec.limited and clip.dbtp == rec.dbtp_out
        assert clip.limited == (free.true_peak() > -1.0)
        assert clip.subtitles == base.subtitles and clip.audio_len_s == base.audio_len_s
        _under(clip, -1.0)
        acted += clip.limited
        print("target %.0f LUFS: %.2f dBTP unconstrained -> %.4f dBTP, limited %r, %.2f LUFS out" % (
            target, free.true_peak(), clip.dbtp, clip.limited, clip.loudness()))
    assert acted >= 1                                               # at -3 LUFS the limiter has work
    # alone: the clip the call would have returned, limited
    ceiling = min(-1.0, math.floor(base.true_peak() - 3.0))         # three dB and more under the clip's peak
    alone = tts.infer(*REF, TWO_SEGMENTS, true_peak=ceiling, **kw)
    want, rec = LM.limit(base.audio_data, 32000, ceiling)
    assert alone.audio_data.tobytes() == want.tobytes() and alone.limited and rec.limited and alone.lufs is None and alone.gain is None
    assert alone.audio_data.tobytes() == base.limited_to(ceiling).audio_data.tobytes()
    _under(alone, ceiling)
    with pytest.raises(ValueError):
        tts.infer(*REF, TWO_SEGMENTS, top_k=1, true_peak=0.5)


def test_infer_vc_and_infer_batched_with_a_ceiling(tts):
    base = tts.infer_vc(*REF, noise_scale=0.0)
    clip = tts.infer_vc(*REF, noise_scale=0.0, loudness=-3.0, true_peak=-2.0)
    want, rec = LM.limit(base.normalised(-3.0, peak_limit=math.inf).audio_data, 32000, -2.0)
    assert clip.audio_data.tobytes() == want.tobytes() and clip.limited and clip.dbtp == rec.dbtp_out and clip.subtitles == base.subtitles
    _under(clip, -2.0)
    kw = dict(top_k=1, noise_scale=0.0, cut_minlen=8)
    plain = tts.infer_batched(*REF, THREE, **kw)
    targets, ceilings = [-3.0, -16.0, None], [-1.0, None, min(-1.0, math.floor(plain[2].true_peak() - 3.0))]
    got = tts.infer_batched(*REF, THREE, loudness=targets, true_peak=ceilings, **kw)
    only = tts.infer_batched(*REF, THREE, loudness=targets, **kw)
    for clip, b, o, t, c in zip(got, plain, only, targets, ceilings):
        if c is None:
            assert clip.audio_data.tobytes() == o.audio_data.tobytes() and clip.dbtp is None and clip.limited == o.limited
            continue
        free = b if t is None else b.normalised(t, peak_limit=math.inf)
        want, rec = LM.limit(free.audio_data, 32000, c)
        assert clip.audio_data.tobytes() == want.tobytes() and clip.limited and clip.dbtp == rec.dbtp_out
        assert clip.lufs == free.lufs and clip.gain == free.gain
        _under(clip, c)
    with pytest.raises(ValueError):
        tts.infer_batched(*REF, THREE, true_peak=[-1.0, None], **kw)
