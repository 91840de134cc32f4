"""GPU parity of CN-HuBERT (csrc/hubert.h behind gsv_hubert_*): last_hidden_state against transformers.HubertModel
(tests/golden/hubert.npz, at the frames it stores) and, in full, against the plain-torch restatement tests/hubert_ref.py
at lengths that move each conv's floor and at 30 s; bit-reproducibility and workspace reuse;
TTS.cache_prompt_audio(audio=...) to the reference's prompt codes, and infer_vc from that prompt.
Tolerance: 2e-4 max abs on the layer-normed output (rms ~1).  The fp32 restatement's own spread against float64 is
~5e-6 on these weights, so the bound leaves a 40x margin for the MFMA / VALU summation orders and nothing more."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubert_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "hubert.npz"))


@pytest.fixture(scope="module")
def model(dev, gold):
    from gsv_tts_lite_amd.hubert import CNHubertNative
    cfg = synth.hubert_config()
    w = synth.hubert_weights(cfg, int(gold["seed"]))
    return CNHubertNative(w, cfg, dev), w, cfg


def _np(ssl):
    assert ssl.dtype == torch.float32 and ssl.dim() == 3 and ssl.shape[0] == 1
    return ssl[0].transpose(0, 1).cpu().numpy()   # [Th][H]


@pytest.mark.parametrize("name,i", [("bare400", 0), ("bare8000", 1)])
def test_golden_bare(model, gold, name, i):
    m, _, _ = model
    n = int(gold[name + "_n"])
    assert m.frames(n) == int(gold[name + "_Th"])
    got = _np(m(torch.from_numpy(synth.synth_audio(100 + i, n, int(gold["seed"])))))
    assert got.shape == (int(gold[name + "_Th"]), 768)
    assert np.abs(got[gold[name + "_rows"]] - gold[name + "_last"]).max() <= TOL


def test_golden_prompts(model, gold):
    m, _, _ = model
    seed = int(gold["seed"])
    got3 = _np(m.prompt_ssl(torch.from_numpy(synth.synth_wav16k(2, 3.0, seed))))
    assert got3.shape[0] == m.frames(16000 * 3 + 4800) == int(gold["prompt3s_Th"])
    assert np.abs(got3[gold["prompt3s_rows"]] - gold["prompt3s_last"]).max() <= TOL
    got10 = _np(m.prompt_ssl(torch.from_numpy(synth.synth_wav16k(3, 10.0, seed))))
    assert got10.shape[0] == m.frames(16000 * 10 + 4800) == int(gold["prompt10s_Th"])
    assert np.abs(got10[gold["prompt10s_rows"]] - gold["prompt10s_last"]).max() <= TOL


@pytest.mark.parametrize("n", [400, 401, 719, 720, 16000 + 4800 + 3, 2 * 16000 + 4800 + 3, 30 * 16000 + 4800])
def test_vs_restatement(model, n):
    m, w, cfg = model
    a = synth.synth_audio(7, n)
    want, _ = hubert_ref.forward(w, cfg, a)
    got = _np(m(torch.from_numpy(a)))
    assert got.shape == tuple(want.shape) and got.shape[0] == hubert_ref.frames(cfg, n) == m.frames(n)
    assert np.isfinite(got).all()
    assert np.abs(got - want.numpy()).max() <= TOL


def test_bit_reproducible_and_workspace_reuse(model, dev):
    m, _, _ = model
    lens = [8000, 52800, 164800, 52800, 401]
    first = {}
    for n in lens:
        a = torch.from_numpy(synth.synth_audio(8, n)).to(dev)
        out = m(a).clone()
        if n in first:
            assert torch.equal(out, first[n]), n
        else:
            first[n] = out
            assert torch.equal(m(a), out), n
    with pytest.raises(ValueError):
        m(torch.zeros(399, device=dev))


def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def test_tts_prompt_audio_and_infer_vc(dev, gold, tmp_path):
    from gsv_tts import TTS
    seed = int(gold["seed"])
    synth.write_hubert_dir(str(tmp_path / "chinese-hubert-base"), seed=seed)
    tts = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(tmp_path), device=str(dev), dtype="bfloat16")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=%d" % seed)
    tts.set_text_frontend(_toy_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    phones = _toy_frontend("prompt text.")[0]
    for name, i, secs in (("prompt3s", 2, 3.0), ("prompt10s", 3, 10.0)):
        tts.cache_prompt_audio(name + ".wav", "prompt text.", audio=torch.from_numpy(synth.synth_wav16k(i, secs, seed)),
                               phones1=phones)
        assert tts.cnhubert_model is None          # always_load_cnhubert=False: dropped after the call
        prompt = tts.prompt_audio_cache[name + ".wav"]["prompt"]
        want, margin = gold[name + "_codes"], gold[name + "_margin"]
        assert prompt.dtype == torch.int64 and tuple(prompt.shape) == (1, want.shape[0])
        ok = margin > 1e-2
        assert ok.mean() > 0.9
        assert np.array_equal(prompt[0].cpu().numpy()[ok], want[ok])
    tts.always_load_cnhubert = True
    tts.cache_prompt_audio("again.wav", "prompt text.", audio=torch.from_numpy(synth.synth_wav16k(2, 3.0, seed)), phones1=phones)
    assert tts.cnhubert_model is not None
    assert torch.equal(tts.prompt_audio_cache["again.wav"]["prompt"], tts.prompt_audio_cache["prompt3s.wav"]["prompt"])
    vc = tts.infer_vc("spk.wav", "prompt3s.wav", "prompt text.", noise_scale=0.0)
    assert np.isfinite(vc.audio_data).all() and len(vc.audio_data) > 6400
    assert np.abs(vc.audio_data).max() > 1e-3
