"""GPU checks of FLAC files as reference audio: the frames decoded on the device (flac_frames_kernel behind
flacio.load_flac / load_flacs) bit for bit against wavio.load_wav of the WAV file holding the same integers, batches
against single loads, and the facade reading .flac paths equal to the same calls on .wav paths."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_writer as fw  # noqa: E402
import wav_writer as ww  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234
PRO = "synthetic://sovits?version=v2Pro&seed=%d" % SEED
GRID = fw.grid()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def wav_of(path, x, bps, rate):
    """the WAV file with the same integers: s16 for 16 bits, packed s24 for 24, u8 (+128) for 8; 12 and 20 bits
    left-justified in s16 / s24"""
    if bps == 8:
        return ww.write(path, x + 128, "u8", rate)
    if bps <= 16:
        return ww.write(path, x << (16 - bps), "s16", rate)
    return ww.write(path, x << (24 - bps), "s24", rate)


# ------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("name", sorted(GRID))
def test_decode_equals_the_wav_of_the_same_integers(dev, tmp_path, name):
    from gsv_tts_lite_amd.flacio import load_flac
    from gsv_tts_lite_amd.wavio import load_wav
    x, bps, rate, kw = GRID[name]
    got, sr = load_flac(fw.write(tmp_path / "a.flac", x, bps, rate, **kw), dev)
    want, _ = load_wav(wav_of(tmp_path / "a.wav", x, bps, rate), dev)
    assert sr == rate and got.dtype == torch.float32 and got.device == dev and got.shape == (len(x),)
    assert torch.equal(got, want)
    if x.shape[1] == 1:
        assert torch.equal(got.cpu(), torch.from_numpy((x[:, 0] / 2.0 ** (bps - 1)).astype(np.float32)))


def test_batch_equals_single(dev, tmp_path):
    from gsv_tts_lite_amd import _native as N
    from gsv_tts_lite_amd.flacio import load_flac, load_flacs
    names = ["bits8_ch1", "bits12_ch2", "bits16_ch1", "bits20_ch2", "bits24_ch1", "bs16", "bs255", "bs1000", "bs4608", "variable",
             "stereo_ms", "lpc32_shift14_24bit", "len1", "len%d" % (3 * 4096 + 5), "rice0"]
    paths = [fw.write(tmp_path / (n + ".flac"), GRID[n][0], GRID[n][1], GRID[n][2], **GRID[n][3]) for n in names]
    single = [load_flac(p, dev) for p in paths]
    order = list(np.random.default_rng(5).permutation(len(paths)))
    for o in (list(range(len(paths))), order):
        got = load_flacs([paths[i] for i in o], dev)
        for j, i in enumerate(o):
            assert got[j][1] == single[i][1] == GRID[names[i]][2]
            assert torch.equal(got[j][0], single[i][0]), (o, names[i])
    many = [paths[i % len(paths)] for i in range(N.AUX_MAX_CLIPS + 1)]           # 65 clips: past one call's cap
    for k, (w, sr) in enumerate(load_flacs(many, dev)):
        assert torch.equal(w, single[k % len(paths)][0]), k


# ------------------------------------------------------------------------------------------------------------ errors
def test_a_flipped_residual_bit_names_file_and_frame(dev, tmp_path):
    from gsv_tts_lite_amd.flacio import load_flac, load_flacs
    x = fw.tone(1000, 2, 16, seed=9)
    data, table = fw.flac_bytes(x, 16, 44100, block_size=192, sub=fw.Sub("fixed", order=2, params=6))
    (tmp_path / "good.flac").write_bytes(data)
    raw = bytearray(data)
    raw[table[3][0] + table[3][1] - 30] ^= 0x01         # the low bit of a Rice remainder: the structure stays intact
    (tmp_path / "r.flac").write_bytes(raw)
    with pytest.raises(ValueError, match=r"r\.flac: frame 3: CRC-16 mismatch"):
        load_flac(str(tmp_path / "r.flac"), dev)
    with pytest.raises(ValueError, match=r"r\.flac: frame 3: CRC-16 mismatch"):
        load_flacs([str(tmp_path / "good.flac"), str(tmp_path / "r.flac")], dev)


def test_a_truncated_file_is_refused_before_any_launch(dev, tmp_path):
    from gsv_tts_lite_amd.flacio import load_flac
    x = fw.tone(1000, 2, 16, seed=9)
    data, table = fw.flac_bytes(x, 16, 44100, block_size=192, sub=fw.Sub("fixed", order=2, params=6))
    (tmp_path / "t.flac").write_bytes(data[:table[2][0] + table[2][1] // 2])
    with pytest.raises(ValueError, match=r"t\.flac: frame 2"):
        load_flac(str(tmp_path / "t.flac"), dev)


# ------------------------------------------------------------------------------------------------------------ facade
def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


@pytest.fixture(scope="module")
def tts(dev, tmp_path_factory):
    from gsv_tts import TTS
    path = tmp_path_factory.mktemp("models")
    synth.write_hubert_dir(str(path / "chinese-hubert-base"), seed=SEED)
    synth.write_sv_ckpt(str(path / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"), seed=SEED)
    t = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(path), device=str(dev), dtype="bfloat16",
            always_load_cnhubert=True, always_load_sv=True)
    t.load_sovits_model(PRO)
    t.set_text_frontend(_toy_frontend)
    return t


def _pair(tmp_path, stem, ch, rate, seconds, i, **kw):
    """the same speech-like s16 integers as stem.flac and stem.wav"""
    n = int(rate * seconds)
    w = np.stack([synth.synth_audio(i + c, n) for c in range(ch)], axis=1).astype(np.float64)
    x = np.clip(np.round(w * 2.0 ** 15), -2.0 ** 15, 2.0 ** 15 - 1).astype(np.int64)
    kw.setdefault("sub", fw.Sub("lpc", order=8, precision=12, shift=10, method=0, params=11))
    return (fw.write(tmp_path / (stem + ".flac"), x, 16, rate, **kw), ww.write(tmp_path / (stem + ".wav"), x, "s16", rate))


def test_facade_reads_flac_as_it_reads_wav(tts, tmp_path):
    af, aw = _pair(tmp_path, "a", 2, 44100, 1.5, 3, assignment="ms")
    tts.cache_spk_audio(af, sovits_model=PRO)
    tts.cache_spk_audio(aw, sovits_model=PRO)
    a, b = tts.spk_audio_cache[af], tts.spk_audio_cache[aw]
    assert torch.equal(a["ge"][PRO], b["ge"][PRO]) and torch.equal(a["sv_emb"], b["sv_emb"])
    text = "prompt text."
    pf, pw = _pair(tmp_path, "p", 1, 16000, 1.5, 7)
    tts.cache_prompt_audio(pf, text, phones1=_toy_frontend(text)[0], sovits_model=PRO)
    tts.cache_prompt_audio(pw, text, phones1=_toy_frontend(text)[0], sovits_model=PRO)
    a, b = tts.prompt_audio_cache[pf], tts.prompt_audio_cache[pw]
    assert a["prompt"].shape[1] > 10 and torch.equal(a["prompt"], b["prompt"]) and a["phones1"] == b["phones1"]
    assert tts.verify_speaker(af, aw) == tts.verify_speaker(aw, aw)


def test_lists_mixing_wav_and_flac_equal_single_calls(tts, tmp_path):
    (tmp_path / "l").mkdir()
    (tmp_path / "s").mkdir()
    spec = [(1, 32000, 1.0, 40), (2, 44100, 1.2, 41), (1, 16000, 1.4, 42), (2, 48000, 1.0, 43)]
    lst = [_pair(tmp_path / "l", "c%d" % i, *sp) for i, sp in enumerate(spec)]
    one = [_pair(tmp_path / "s", "c%d" % i, *sp) for i, sp in enumerate(spec)]
    keys = [lst[0][0], lst[1][1], lst[2][1], lst[3][0]]              # flac, wav, wav, flac
    single = [one[0][0], one[1][1], one[2][1], one[3][0]]
    tts.cache_spk_audio(keys, sovits_model=PRO)
    for p, q in zip(keys, single):
        tts.cache_spk_audio(q, sovits_model=PRO)
        assert torch.equal(tts.spk_audio_cache[p]["sv_emb"], tts.spk_audio_cache[q]["sv_emb"]), p
        assert torch.equal(tts.spk_audio_cache[p]["ge"][PRO], tts.spk_audio_cache[q]["ge"][PRO]), p
    texts = ["first prompt.", "second one.", "third!", "and a fourth."]
    tts.cache_prompt_audio(keys, texts, sovits_model=PRO)
    for p, q, t in zip(keys, single, texts):
        tts.cache_prompt_audio(q, t, sovits_model=PRO)
        assert torch.equal(tts.prompt_audio_cache[p]["prompt"], tts.prompt_audio_cache[q]["prompt"]), p
