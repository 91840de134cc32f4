"""CPU checks of the WAV reader (gsv_tts_lite_amd.wavio): the RIFF/WAVE parser on every supported format tag and
container variant, the refusals (compressed audio named, more than two channels, malformed files), the CPU device
refused before any conversion, and the facade's behaviour for keys that are not files.  No GPU."""
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wav_writer as ww  # noqa: E402

from gsv_tts_lite_amd import wavio  # noqa: E402


def _parse_and_check(path, x, fmt, rate):
    info, raw = wavio.parse_wav(path)
    assert wavio.FORMATS[info.format] == fmt
    assert (info.channels, info.sample_rate, info.n_frames) == (x.shape[1], rate, x.shape[0])
    nb = info.n_frames * info.channels * wavio.SAMPLE_BYTES[info.format]
    assert raw[info.data_offset:info.data_offset + nb] == ww.encode(x, fmt)
    return info


@pytest.mark.parametrize("fmt", ww.FORMATS)
@pytest.mark.parametrize("ch", [1, 2])
def test_every_format_and_tag(tmp_path, fmt, ch):
    x = ww.samples(fmt, 37, ch)
    _parse_and_check(ww.write(tmp_path / "a.wav", x, fmt, 22050), x, fmt, 22050)


@pytest.mark.parametrize("fmt", ww.FORMATS)
def test_extensible(tmp_path, fmt):
    x = ww.samples(fmt, 19, 2, seed=3)
    _parse_and_check(ww.write(tmp_path / "e.wav", x, fmt, 48000, extensible=True), x, fmt, 48000)


def test_container_width_rounds_up(tmp_path):
    """20 valid bits in a 3-byte container read as s24, as ffmpeg does"""
    x = ww.samples("s24", 9, 1)
    path = ww.write(tmp_path / "w.wav", x, "s24", 16000, bits=20)
    _parse_and_check(path, x, "s24", 16000)


def test_unknown_chunks_and_pad_bytes(tmp_path):
    x = ww.samples("s16", 11, 2)
    odd = ww.chunk(b"junk", b"abc")                  # 3 bytes + the pad byte
    lst = ww.chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 5) + b"test\0\0")
    path = ww.write(tmp_path / "c.wav", x, "s16", 32000, before_fmt=(lst, odd), before_data=(odd, lst,
                    ww.chunk(b"fact", struct.pack("<I", 11)), ww.chunk(b"cue ", struct.pack("<I", 0))),
                    after=lst + odd)
    _parse_and_check(path, x, "s16", 32000)


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_streamed_data_size_runs_to_the_end(tmp_path, size):
    x = ww.samples("s24", 13, 2)
    _parse_and_check(ww.write(tmp_path / "s.wav", x, "s24", 44100, data_size=size), x, "s24", 44100)


def test_data_size_past_the_end_and_truncated_frame(tmp_path):
    x = ww.samples("s16", 10, 2)
    data = ww.encode(x, "s16")
    with open(tmp_path / "t.wav", "wb") as f:          # a last frame cut after 3 of its 4 bytes, the size claiming more
        f.write(ww.wav_bytes(data + b"\x01\x02\x03", "s16", 2, 16000, data_size=len(data) + 400)[:-1])
    _parse_and_check(str(tmp_path / "t.wav"), x, "s16", 16000)
    with open(tmp_path / "u.wav", "wb") as f:          # an odd data size: the truncated frame and the pad byte are dropped
        f.write(ww.wav_bytes(data + b"\x7f", "s16", 2, 16000))
    _parse_and_check(str(tmp_path / "u.wav"), x, "s16", 16000)


@pytest.mark.parametrize("head, name", [
    (b"ID3\x04\x00\x00\x00\x00\x00\x21" + bytes(64), "MP3"),
    (b"\xff\xfb\x90\x64" + bytes(64), "MP3"),
    (b"OggS\x00\x02" + bytes(64), "Ogg"),
    (b"fLaC\x00\x00\x00\x22" + bytes(64), "FLAC"),
    (b"RIFF\x10\x00\x00\x00AVI LIST" + bytes(8), "AVI"),
    (b"RF64\xff\xff\xff\xffWAVEds64" + bytes(64), "RF64"),
])
def test_compressed_and_foreign_files_are_named(tmp_path, head, name):
    p = tmp_path / "x.bin"
    p.write_bytes(head)
    with pytest.raises(NotImplementedError, match=name) as e:
        wavio.parse_wav(str(p))
    assert "outside this build" in str(e.value)
    with pytest.raises(NotImplementedError, match=name):
        wavio.load_wav(str(p), "cpu")                # parsed before the device is looked at


@pytest.mark.parametrize("tag, name", [(7, "mu-law"), (6, "A-law"), (2, "ADPCM"), (0x11, "ADPCM"), (0x55, "MP3")])
def test_compressed_wav_tags(tmp_path, tag, name):
    p = tmp_path / "c.wav"
    p.write_bytes(ww.wav_bytes(bytes(64), "u8", 1, 8000, tag=tag, bits=8))
    with pytest.raises(NotImplementedError, match=name):
        wavio.parse_wav(str(p))
    p.write_bytes(ww.wav_bytes(bytes(64), "u8", 1, 8000, tag=tag, bits=8, extensible=True))
    with pytest.raises(NotImplementedError, match="0x%04X" % tag):
        wavio.parse_wav(str(p))


@pytest.mark.parametrize("ch", [3, 6])
def test_more_than_two_channels(tmp_path, ch):
    x = ww.samples("s16", 8, ch)
    with pytest.raises(NotImplementedError, match="%d channels" % ch):
        wavio.parse_wav(ww.write(tmp_path / "m.wav", x, "s16", 48000))


def test_unsupported_widths_and_malformed_files(tmp_path):
    p = tmp_path / "b.wav"
    p.write_bytes(ww.wav_bytes(bytes(64), "s32", 1, 8000, bits=64))             # s64 integer PCM
    with pytest.raises(NotImplementedError, match="64-bit integer PCM"):
        wavio.parse_wav(str(p))
    p.write_bytes(ww.wav_bytes(bytes(64), "f32", 1, 8000, bits=16))             # half floats
    with pytest.raises(NotImplementedError, match="16-bit IEEE float"):
        wavio.parse_wav(str(p))
    p.write_bytes(b"RIFF" + struct.pack("<I", 4 + 8 + 4) + b"WAVE" + ww.chunk(b"data", bytes(4)))
    with pytest.raises(ValueError, match="'fmt '"):
        wavio.parse_wav(str(p))
    p.write_bytes(b"RIFF" + struct.pack("<I", 4 + 24) + b"WAVE" + ww.fmt_chunk("s16", 1, 8000))
    with pytest.raises(ValueError, match="'data'"):
        wavio.parse_wav(str(p))
    p.write_bytes(ww.wav_bytes(b"\x01", "s16", 1, 8000))
    with pytest.raises(ValueError, match="no complete audio frame"):
        wavio.parse_wav(str(p))


def test_cpu_device_is_refused(tmp_path):
    path = ww.write(tmp_path / "ok.wav", ww.samples("s16", 100, 1), "s16", 16000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        wavio.load_wav(path, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        wavio.load_wavs([path, path], torch.device("cpu"))
    assert wavio.load_wavs([], "cuda:0") == []


def test_a_bad_file_in_a_list_is_named_before_any_upload(tmp_path):
    good = ww.write(tmp_path / "ok.wav", ww.samples("s16", 100, 1), "s16", 16000)
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"OggS" + bytes(40))
    with pytest.raises(NotImplementedError, match="bad.wav"):
        wavio.load_wavs([good, str(bad)], "cuda:0")


# ------------------------------------------------------------------------------------------------------------ facade
@pytest.fixture
def tts(tmp_path, monkeypatch):
    import gsv_tts_lite_amd.hubert as hubert
    import gsv_tts_lite_amd.sv as sv
    from gsv_tts import TTS

    def spy(name):
        def load(*a, **k):
            raise AssertionError("%s was called" % name)
        return load

    monkeypatch.setattr(hubert, "load_cnhubert", spy("load_cnhubert"))
    monkeypatch.setattr(sv, "load_sv", spy("load_sv"))
    t = TTS(models_dir=str(tmp_path), device="cpu")
    t.load_sovits_model = spy("load_sovits_model")
    return t


def test_keys_that_are_no_files_keep_their_errors(tts, tmp_path):
    missing = str(tmp_path / "missing.wav")
    wav = ww.write(tmp_path / "ok.wav", ww.samples("s16", 100, 1), "s16", 32000)
    with pytest.raises(NotImplementedError, match="decoding / resampling audio files is outside this build's scope"):
        tts.cache_spk_audio(missing)
    with pytest.raises(NotImplementedError, match="16 kHz"):
        tts.cache_prompt_audio(missing, "prompt text.", phones1=[1, 2, 3])
    with pytest.raises(NotImplementedError, match="decoding"):
        tts.verify_speaker(missing, missing)
    with pytest.raises(NotImplementedError, match="key 1"):
        tts.cache_spk_audio([wav, str(tmp_path)])               # a directory is no file
    with pytest.raises(NotImplementedError, match="decoding"):
        tts.cache_prompt_audio([missing, missing], "t", phones1=[1])
    assert tts.spk_audio_cache == {} and tts.prompt_audio_cache == {}


def test_wav_keys_on_the_cpu_fail_loudly(tts, tmp_path):
    path = ww.write(tmp_path / "spk.wav", ww.samples("s16", 32000, 1), "s16", 32000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_spk_audio(path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_prompt_audio(path, "prompt text.", phones1=[1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_spk_audio([path, path])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_prompt_audio([path], "prompt text.", phones1=[1, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.verify_speaker(path, path)
    mp3 = tmp_path / "spk.mp3"
    mp3.write_bytes(b"ID3" + bytes(40))
    with pytest.raises(NotImplementedError, match="MP3"):
        tts.cache_spk_audio(str(mp3))
    assert tts.spk_audio_cache == {} and tts.prompt_audio_cache == {}


def test_prompt_list_of_files_needs_phones_or_a_frontend(tts, tmp_path):
    path = ww.write(tmp_path / "p.wav", ww.samples("s16", 16000, 1), "s16", 16000)
    with pytest.raises(NotImplementedError, match="G2P"):
        tts.cache_prompt_audio([path, path], "prompt text.")
    with pytest.raises(NotImplementedError, match="G2P"):   # a waveform key in the list: phones1 must be given
        tts.cache_prompt_audio([path, "k"], "prompt text.", audio=[None, torch.zeros(1600)])
    with pytest.raises(ValueError, match="sample_rate has 1 entries for 2 keys"):
        tts.cache_spk_audio([path, path], sample_rate=[16000])
