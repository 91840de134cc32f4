"""CPU checks of the speaker-verification path: the plain-torch restatement tests/sv_ref.py against the reference's
ERes2NetV2 module (tests/golden/sv.npz, tools/gen_golden_sv.py), properties of the resample / fbank restatement (which
torchaudio, absent here, cannot pin), loader.read_sv and the configuration checks of sv.infer_config.  No GPU.

Tolerance: 1e-3 max abs on forward3's output (|values| up to ~70).  The golden rows are the reference module in fp32;
the fp64 restatement sits 1.5e-4 from them, which is the fp32 spread itself (the fp32 restatement is as far from fp64)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

TOL = 1e-3


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "sv.npz"))


@pytest.mark.parametrize("name", ["m64_T1", "m64_T37", "m64_T298", "m16_T37"])
def test_restatement_vs_golden(gold, name):
    m = 16 if name.startswith("m16") else 64
    T, step = int(gold[name + "_T"]), int(gold[name + "_step"])
    emb = sv_ref.forward3(synth.sv_weights(int(gold["seed"]), m), synth.sv_feat(T, T, int(gold["seed"])))
    assert emb.shape == (32 * m * 10,)
    assert np.abs(emb.numpy()[::step] - gold[name + "_emb"]).max() <= TOL


def test_restatement_taps_vs_golden(gold):
    seed = int(gold["seed"])
    taps = {}
    sv_ref.forward3(synth.sv_weights(seed, 64), synth.sv_feat(37, 37, seed), taps=taps)
    for tap in ("layer1", "layer3", "fuse34"):
        (c0, f0, t0), (cs, fs, ts) = gold["m64_T37_%s_slice" % tap]
        got = taps[tap][c0::cs, f0::fs, t0::ts].numpy()
        assert np.abs(got - gold["m64_T37_" + tap]).max() <= TOL, tap


@pytest.mark.parametrize("orig,new", [(32000, 16000), (48000, 16000), (16000, 32000), (44100, 16000)])
@pytest.mark.parametrize("n", [1, 5, 100, 32001])
def test_resample_length(orig, new, n):
    y = sv_ref.resample(np.ones(n), orig, new)
    assert y.shape == (math.ceil(new * n / orig),) == (sv_ref.resample_length(n, orig, new),)


def test_resample_kernel_shape():
    k, width = sv_ref.resample_kernel(32000, 16000)
    assert width == math.ceil(6 * 2 / 0.99) == 13
    assert k.shape == (1, 2 * 13 + 2)
    k, width = sv_ref.resample_kernel(44100, 16000)     # gcd 100: 441 -> 160 phases
    assert k.shape == (160, 2 * width + 441)


def _tone_amp(f, sr_in=32000, sr_out=16000):
    t = np.arange(sr_in) / sr_in
    y = sv_ref.resample(np.sin(2 * math.pi * f * t), sr_in, sr_out)
    mid = y[2000:-2000]
    return math.sqrt(2 * np.mean(mid ** 2))


def test_resample_keeps_1khz_attenuates_7950hz():
    assert abs(_tone_amp(1000.0) - 1.0) < 1e-3
    assert _tone_amp(7950.0) < 0.6           # past the 0.99 * 8 kHz cutoff
    assert _tone_amp(12000.0) < 1e-2         # far above the new Nyquist


@pytest.mark.parametrize("n,T", [(399, 0), (400, 1), (559, 1), (560, 2), (16000, 98), (48000, 298)])
def test_fbank_frames(n, T):
    assert sv_ref.fbank_frames(n) == T
    assert sv_ref.fbank(synth.synth_audio(1, n)).shape == (T, 80)


def test_mel_banks():
    b = sv_ref.mel_banks()
    assert b.shape == (80, 257)
    assert (b[:, 256] == 0).all() and (b >= 0).all() and (b <= 1).all()
    assert (b.sum(1) > 0).all()
    assert (b[:, 0] == 0).all()                  # bin 0 (0 Hz) is below 20 Hz


def test_fbank_tone_peaks_in_its_bin():
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(20.0), mel(8000.0)
    for f in (300.0, 1000.0, 4000.0):
        fb = sv_ref.fbank(np.sin(2 * math.pi * f * np.arange(16000) / 16000.0))
        centre = (mel(f) - lo) / ((hi - lo) / 81) - 1
        assert abs(int(fb.mean(0).argmax()) - centre) <= 1.0, f


def test_fbank_zero_frames_are_log_eps():
    x = synth.synth_audio(2, 16000).astype(np.float64)
    x[4000:8000] = 0.0
    fb = sv_ref.fbank(x)
    zero = [t for t in range(fb.shape[0]) if t * 160 >= 4000 and t * 160 + 400 <= 8000]
    assert zero and (fb[zero] == math.log(sv_ref.FLT_EPS)).all()
    assert (fb[0] > math.log(sv_ref.FLT_EPS)).all()


def test_read_sv_accepts_and_refuses(tmp_path):
    from gsv_tts_lite_amd.loader import read_sv
    p = synth.write_sv_ckpt(str(tmp_path / "sv" / "ok.ckpt"), seed=3, m_channels=16)
    w = read_sv(p)
    assert "conv1.weight" in w and not any(k.endswith("num_batches_tracked") for k in w)
    assert tuple(w["layer4.0.convs.0.weight"].shape) == (48, 48, 3, 3)
    with pytest.raises(FileNotFoundError):
        read_sv(str(tmp_path / "missing.ckpt"))
    bad = tmp_path / "bad.ckpt"
    torch.save({"state_dict": {"conv1.weight": torch.zeros(16, 1, 3, 3)}}, str(bad))
    with pytest.raises(ValueError):
        read_sv(str(bad))
    obj = tmp_path / "obj.ckpt"
    torch.save({"model": object}, str(obj))                # not loadable with weights_only=True
    with pytest.raises(ValueError):
        read_sv(str(obj))
    junk = tmp_path / "junk.ckpt"
    junk.write_bytes(b"not a torch file")
    with pytest.raises(ValueError):
        read_sv(str(junk))


def _sd(**kw):
    return {k: torch.from_numpy(v) for k, v in synth.sv_weights(5, 16, **kw).items()}


def test_infer_config_and_refusals():
    from gsv_tts_lite_amd.sv import infer_config
    c = infer_config(_sd())
    assert (c.m_channels, list(c.blocks), list(c.width), c.scale, c.expansion, c.feat_dim) == (
        16, [3, 4, 6, 3], [6, 12, 24, 48], 4, 4, 80)
    c = infer_config(_sd(blocks=(1, 2, 1, 2)))
    assert list(c.blocks) == [1, 2, 1, 2]
    with pytest.raises(ValueError, match="scale"):
        infer_config(_sd(scale=2))
    with pytest.raises(ValueError, match="expansion"):
        infer_config(_sd(expansion=2))
    with pytest.raises(ValueError, match="feat_dim"):
        infer_config(_sd(feat_dim=64))
