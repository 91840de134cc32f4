"""GPU checks of the batched reference-audio models (gsv_hubert_forward_batch, gsv_sv_forward_batch / embed_batch behind
CNHubertNative.batch / prompt_ssl_batch and SVNative.forward3_batch / embed_batch) and of the list forms of
TTS.cache_prompt_audio / cache_spk_audio.  Every clip of a batch must be bit-identical (torch.equal) to the single-clip
call on that clip, whatever else is in the batch and in any order; the golden / restatement bounds are those of
tests/test_hip_hubert.py (2e-4) and tests/test_hip_sv.py (2e-3)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubert_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_HUB = 2e-4
TOL_SV = 2e-3
PAD = 4800


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hgold(golden_dir):
    return np.load(os.path.join(golden_dir, "hubert.npz"))


@pytest.fixture(scope="module")
def sgold(golden_dir):
    return np.load(os.path.join(golden_dir, "sv.npz"))


@pytest.fixture(scope="module")
def hub(dev, hgold):
    from gsv_tts_lite_amd.hubert import CNHubertNative
    cfg = synth.hubert_config()
    w = synth.hubert_weights(cfg, int(hgold["seed"]))
    return CNHubertNative(w, cfg, dev), w, cfg


@pytest.fixture(scope="module")
def svm(dev, sgold):
    from gsv_tts_lite_amd.sv import SVNative
    w = synth.sv_weights(int(sgold["seed"]), 64)
    return SVNative(w, dev), w


def _rows(ssl):
    return ssl[0].transpose(0, 1).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ CN-HuBERT
def test_hubert_batch_equals_single(hub, hgold, dev):
    m, w, cfg = hub
    seed = int(hgold["seed"])
    clips = [torch.from_numpy(synth.synth_audio(20 + i, n)).to(dev) for i, n in enumerate((400, 401, 719, 8000))]
    clips.append(torch.from_numpy(synth.synth_wav16k(2, 3.0, seed)).to(dev))
    clips.append(torch.from_numpy(synth.synth_wav16k(3, 10.0, seed)).to(dev))
    clips[4] = torch.cat([clips[4], clips[4].new_zeros(PAD)])
    clips[5] = torch.cat([clips[5], clips[5].new_zeros(PAD)])
    single = [m(a).clone() for a in clips]
    got = m.batch(clips)
    assert len(got) == len(clips)
    for i, (g, s) in enumerate(zip(got, single)):
        assert g.shape == s.shape == (1, 768, m.frames(clips[i].numel())), i
        assert torch.equal(g, s), i
    for order in ([5, 4, 3, 2, 1, 0], [2, 5, 0, 3, 1, 4]):
        again = m.batch([clips[i] for i in order])
        for j, i in enumerate(order):
            assert torch.equal(again[j], single[i]), (order, i)
    assert torch.equal(m.batch(clips[3:4])[0], single[3])
    # the prompt clips against transformers.HubertModel at the golden rows
    for name, i in (("prompt3s", 4), ("prompt10s", 5)):
        got_r = _rows(got[i])
        assert got_r.shape[0] == int(hgold[name + "_Th"])
        assert np.abs(got_r[hgold[name + "_rows"]] - hgold[name + "_last"]).max() <= TOL_HUB, name
    # one mid-length clip against the restatement
    want, _ = hubert_ref.forward(w, cfg, clips[3].cpu().numpy())
    assert np.abs(_rows(got[3]) - want.numpy()).max() <= TOL_HUB


def test_hubert_batch_30s(hub, dev):
    m, _, _ = hub
    a = torch.from_numpy(synth.synth_audio(30, 30 * 16000 + PAD)).to(dev)
    single = m(a).clone()
    got = m.batch([a])[0]
    assert got.shape == (1, 768, 1514)
    assert torch.equal(got, single)


def test_hubert_prompt_ssl_batch_and_reproducible(hub, dev):
    m, _, _ = hub
    wavs = [torch.from_numpy(synth.synth_wav16k(40 + i, s)).to(dev) for i, s in enumerate((0.5, 3.0, 1.2))]
    a = [t.clone() for t in m.prompt_ssl_batch(wavs)]
    b = m.prompt_ssl_batch(wavs)
    for i, w in enumerate(wavs):
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(a[i], m.prompt_ssl(w)), i


def test_hubert_past_the_cap(hub, dev):
    from gsv_tts_lite_amd import _native as N
    m, _, _ = hub
    clips = [torch.from_numpy(synth.synth_audio(200 + i, 400 + 97 * i)).to(dev) for i in range(N.AUX_MAX_CLIPS + 6)]
    got = m.batch(clips)
    assert len(got) == len(clips)
    for i, a in enumerate(clips):
        assert torch.equal(got[i], m(a)), i


def test_hubert_bad_clip_names_its_index(hub, dev):
    m, _, _ = hub
    with pytest.raises(ValueError, match="clip 2"):
        m.batch([torch.zeros(800, device=dev), torch.zeros(1600, device=dev), torch.zeros(399, device=dev)])


# ------------------------------------------------------------------------------------------------------------ ERes2NetV2
def test_forward3_batch_golden_and_single(svm, sgold):
    m, _ = svm
    seed = int(sgold["seed"])
    names = ["m64_T1", "m64_T37", "m64_T298", "m64_T998"]
    feats = [torch.from_numpy(synth.sv_feat(int(sgold[n + "_T"]), int(sgold[n + "_T"]), seed)) for n in names]
    got = m.forward3_batch(feats)
    assert got.shape == (4, 20480)
    for i, n in enumerate(names):
        step = int(sgold[n + "_step"])
        assert np.abs(got[i].cpu().numpy()[::step] - sgold[n + "_emb"]).max() <= TOL_SV, n
        assert torch.equal(got[i:i + 1], m.forward3(feats[i])), n
    rev = m.forward3_batch(feats[::-1])
    assert torch.equal(rev, got.flip(0))
    assert torch.equal(m.forward3_batch(feats), got)                 # two identical calls


def test_forward3_batch_m16(dev, sgold):
    from gsv_tts_lite_amd.sv import SVNative
    seed = int(sgold["seed"])
    m = SVNative(synth.sv_weights(seed, 16), dev)
    feats = [torch.from_numpy(synth.sv_feat(T, T, seed)) for T in (37, 298)]
    got = m.forward3_batch(feats)
    for i, f in enumerate(feats):
        assert torch.equal(got[i:i + 1], m.forward3(f)), i
    assert np.abs(got[0].cpu().numpy() - sgold["m16_T37_emb"]).max() <= TOL_SV


@pytest.mark.parametrize("rate", [32000, 16000])
def test_embed_batch_equals_single(svm, dev, rate):
    m, _ = svm
    one_frame = 400 * rate // 16000
    clips = [torch.from_numpy(synth.synth_audio(50 + i, n)).to(dev) for i, n in
             enumerate((one_frame, 3 * rate, 10 * rate, 30 * rate))]
    got = m.embed_batch(clips, rate)
    assert got.shape == (4, m.emb_dim)
    for i, a in enumerate(clips):
        assert torch.equal(got[i:i + 1], m.embed(a, rate)), i
    shuffled = [2, 0, 3, 1]
    again = m.embed_batch([clips[i] for i in shuffled], rate)
    for j, i in enumerate(shuffled):
        assert torch.equal(again[j], got[i]), i


def test_embed_batch_past_the_cap_and_bad_clip(svm, dev):
    from gsv_tts_lite_amd import _native as N
    m, _ = svm
    clips = [torch.from_numpy(synth.synth_audio(300 + i, 800 + 331 * i)).to(dev) for i in range(N.AUX_MAX_CLIPS + 6)]
    got = m.embed_batch(clips, 32000)
    for i, a in enumerate(clips):
        assert torch.equal(got[i:i + 1], m.embed(a, 32000)), i
    with pytest.raises(ValueError, match="clip 1"):
        m.embed_batch([clips[0], torch.zeros(797, device=dev)], 32000)


# ------------------------------------------------------------------------------------------------------------ facade
def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def test_facade_lists(dev, tmp_path):
    from gsv_tts import TTS
    seed = 1234
    synth.write_hubert_dir(str(tmp_path / "chinese-hubert-base"), seed=seed)
    synth.write_sv_ckpt(str(tmp_path / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"), seed=seed)
    tts = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(tmp_path), device=str(dev), dtype="bfloat16")
    pro = "synthetic://sovits?version=v2Pro&seed=%d" % seed
    v2 = "synthetic://sovits?version=v2&seed=%d" % seed
    tts.load_sovits_model(pro, v2)
    tts.set_text_frontend(_toy_frontend)
    phones = _toy_frontend("prompt text.")[0]
    # prompts: one batched call against four single-key calls
    pw = [torch.from_numpy(synth.synth_wav16k(60 + i, s, seed)) for i, s in enumerate((3.0, 1.0, 10.0, 2.5))]
    keys = ["b%d.wav" % i for i in range(4)]
    tts.cache_prompt_audio(keys, "prompt text.", audio=pw, phones1=phones, sovits_model=pro)
    assert tts.cnhubert_model is None
    for i, k in enumerate(keys):
        tts.cache_prompt_audio("s%d.wav" % i, "prompt text.", audio=pw[i], phones1=phones, sovits_model=pro)
        a, b = tts.prompt_audio_cache[k], tts.prompt_audio_cache["s%d.wav" % i]
        assert torch.equal(a["prompt"], b["prompt"]), k
        assert a["phones1"] == b["phones1"] and a["text"] == b["text"] and torch.equal(a["bert1"], b["bert1"])
    # speakers: v2Pro computes sv_emb in one batched pass; v2 gets none
    sw = [torch.from_numpy(synth.synth_audio(70 + i, n)) for i, n in enumerate((32000 * 3, 32000, 32000 * 5, 20000))]
    skeys = ["spk%d" % i for i in range(4)]
    tts.cache_spk_audio(skeys, sovits_model=pro, audio=sw)
    assert tts.sv_model is None
    for i, k in enumerate(skeys):
        tts.cache_spk_audio("one%d" % i, sovits_model=pro, audio=sw[i])
        a, b = tts.spk_audio_cache[k], tts.spk_audio_cache["one%d" % i]
        assert torch.equal(a["sv_emb"], b["sv_emb"]), k
        assert torch.equal(a["ge"][pro], b["ge"][pro]), k
    tts.cache_spk_audio(["v2a", "v2b"], sovits_model=v2, audio=sw[:2])
    for i, k in enumerate(["v2a", "v2b"]):
        assert "sv_emb" not in tts.spk_audio_cache[k]
        tts.cache_spk_audio("v2one%d" % i, sovits_model=v2, audio=sw[i])
        assert torch.equal(tts.spk_audio_cache[k]["ge"][v2], tts.spk_audio_cache["v2one%d" % i]["ge"][v2])
    vc = tts.infer_vc("spk0", "b0.wav", "prompt text.", noise_scale=0.0, sovits_model=pro)   # a prompt cached in a batch
    assert np.isfinite(vc.audio_data).all() and len(vc.audio_data) > 6400
