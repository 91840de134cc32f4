"""CPU checks of the FLAC writer: flacio.build_header against the reader's own header parser and against the test
writer; the serial encoder gsv_flac_encode_host (the scalar pieces of csrc/flacenc.h, which the GPU kernel shares) round
trip through parse_flac and gsv_flac_decode_host, byte for byte against tests/flac_writer.py given the reported choice,
and its choice against a brute-force argmin; the argument checks; AudioClip.save.  No GPU."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_writer as fw  # noqa: E402
import flacenc_cases as E  # noqa: E402
from flacenc_cases import decode_host  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio  # noqa: E402

RATES = (8000, 32000, 44100, 11025, 12345)


# ------------------------------------------------------------------------------------------------------------ headers
@pytest.mark.parametrize("bits", E.BITS)
def test_header_is_the_inverse_of_the_reader(bits):
    for bs in (1, 15, 16, 192, 255, 256, 257, 1000, 4096, 4608):
        x = np.zeros((bs, 1), dtype=np.int64)
        for rate in RATES:
            info = flacio.FlacInfo(1, bits, rate, 0, bs, bs, 0, 0, bytes(16))
            for number in (0, 127, 128, 2047, 2048, 65535, 65536, 2 ** 31 - 1):
                h = flacio.build_header(bs, rate, bits, number)
                assert 6 <= len(h) <= 16
                assert flacio._header(h, 0, info, False, number) == bs, (bs, rate, number)
                assert flacio._header(h, 0, info, False, number + 1) is None
                assert fw.frame_bytes(x, bits, rate, number, sub=fw.Sub("constant"))[:len(h)] == h, (bs, rate, number)


# --------------------------------------------------------------------------------------------------------- round trip
@pytest.fixture(scope="module", params=[(b, w) for b in E.BLOCKS for w in E.BITS], ids=lambda p: "B%d_%dbit" % p)
def encoded(request):
    """the whole grid of one block size and width through flacio.encode_flacs on the CPU, and through the ABI with the
    choices -> (block, bits, [(name, x, rate)], files, [Encoded per call])"""
    block, bits = request.param
    clips = [(name, x, RATES[i % len(RATES)]) for i, (name, x) in enumerate(E.grid_clips(block, bits))]
    files = flacio.encode_flacs([x for _, x, _ in clips], [r for _, _, r in clips], bits=bits, block_size=block, device="cpu")
    calls = []
    for c0 in range(0, len(clips), N.AUX_MAX_CLIPS):
        part = clips[c0:c0 + N.AUX_MAX_CLIPS]
        calls.append(E.encode_abi([x for _, x, _ in part], [r for _, _, r in part], [bits] * len(part), [block] * len(part)))
        assert calls[-1].rc == 0
    return block, bits, clips, files, calls


def test_round_trip(encoded, tmp_path):
    block, bits, clips, files, calls = encoded
    assert len(clips) == len(E.SIGNALS) * len(E.LENGTHS) > N.AUX_MAX_CLIPS
    for (name, x, rate), data in zip(clips, files):
        path = tmp_path / (name + ".flac")
        path.write_bytes(data)
        info, frames, raw = flacio.parse_flac(str(path))
        sizes = [f.length for f in frames]
        assert data[:4] == b"fLaC" and data[4:8] == b"\x80\x00\x00\x22"
        assert data[8:42] == fw.streaminfo(block, block, min(sizes), max(sizes), rate, 1, bits, len(x), bytes(16)), name
        assert info.md5 == bytes(16) and len(frames) == -(-len(x) // block)
        assert all(f.block_size == block for f in frames[:-1]) and frames[-1].block_size == len(x) - block * (len(frames) - 1)
        rc, (got,), status = decode_host([(info, frames, raw)])
        assert rc == 0 and not status.any(), (name, status)
        assert np.array_equal(got[:, 0], E.quantise(x, bits)), name


def test_files_are_the_abi_frames(encoded):
    """encode_flacs (64 clips per call, the container around them) holds exactly the frames the ABI call returns"""
    block, bits, clips, files, calls = encoded
    c = 0
    for e in calls:
        assert e.offsets[0] == 0 and e.offsets[-1] <= e.bound and np.all(np.diff(e.offsets) >= 6 + 1 + 2)
        f = 0
        for nf in e.per_clip:
            assert files[c][42:] == bytes(e.data[e.offsets[f]:e.offsets[f + nf]]), clips[c][0]
            f += nf
            c += 1
    assert c == len(clips)


def test_frames_equal_the_writer_given_the_choice(encoded):
    """header, CRC-8, subframe and CRC-16: the test writer, forced to the reported choice, writes the same bytes"""
    block, bits, clips, files, calls = encoded
    c = 0
    for e in calls:
        f = 0
        for nf in e.per_clip:
            name, x, rate = clips[c]
            q = E.quantise(x, bits)
            for k in range(nf):
                want = fw.frame_bytes(q[k * block:(k + 1) * block, None], bits, rate, k, sub=E.sub_of(e.choice(f + k)))
                assert e.frame(f + k) == want, (name, k, e.choice(f + k))
            f += nf
            c += 1


def test_quantiser_edges():
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 1.0, -1.0, 0.99999, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768,
                  -1.5 / 32768, 1e-30, -0.0, 3e38], dtype=np.float32)
    x = np.concatenate([x, np.frombuffer(np.array([0x7F800001, 0xFFC00001], dtype=np.uint32).tobytes(), dtype=np.float32)])
    assert list(E.quantise(x, 16)) == [0, 0, 32767, -32768, 32767, -32768, 32767, 0, 2, 2, 0, -2, 0, 0, 32767, 0, 0]
    for bits in E.BITS:
        e = E.encode_abi([x], [32000], [bits], [4096])
        assert e.rc == 0 and e.choice(0)[0] in ("fixed", "verbatim")
        want = fw.frame_bytes(E.quantise(x, bits)[:, None], bits, 32000, 0, sub=E.sub_of(e.choice(0)))
        assert e.frame(0) == want


# -------------------------------------------------------------------------------------------------------- the optimum
@pytest.mark.parametrize("bits", E.BITS)
@pytest.mark.parametrize("n", (4096, 1000, 37))
def test_choice_is_the_brute_force_argmin(n, bits):
    names = ("tone", "noise", "const", "outlier")
    xs = [E.signal(s, n, seed=3) for s in names]
    e = E.encode_abi(xs, [32000] * len(xs), [bits] * len(xs), [4608] * len(xs))         # one frame per clip
    assert e.rc == 0
    seen = set()
    for f, (s, x) in enumerate(zip(names, xs)):
        choice, sub_bits = E.brute_force(E.quantise(x, bits), bits)
        assert e.choice(f) == choice, s
        assert len(e.frame(f)) == e.ftab[f].header_len + (sub_bits + 7) // 8 + 2, s
        seen.add(choice[0])
    assert seen == {"fixed", "verbatim", "constant"}
    tone = e.choice(0)
    assert tone[0] == "fixed" and tone[1] >= 1 and tone[2] <= {4096: 6, 1000: 3, 37: 0}[n]


# ---------------------------------------------------------------------------------------------------- argument checks
def _err():
    return N.lib().gsv_last_error().decode()


def _call_host(clips, ftab, n_samples=None, out_bytes=None, n_clips=None):
    L = N.lib()
    total = sum(c.n_samples for c in clips) if n_samples is None else n_samples
    x = np.zeros(max(total, 1), dtype=np.float32)
    out = np.zeros(1 << 16, dtype=np.uint8)
    offsets = np.zeros(len(ftab) + 1, dtype=np.int64)
    return L.gsv_flac_encode_host(x.ctypes.data, total, clips, len(clips) if n_clips is None else n_clips, ftab, len(ftab),
                                  out.ctypes.data, len(out) if out_bytes is None else out_bytes, offsets.ctypes.data, None)


def _tables(lengths=(100, 40), bits=(16, 24), block=64):
    clips, ftab, _ = flacio.enc_tables(list(lengths), [32000] * len(lengths), list(bits), [block] * len(lengths))
    return clips, ftab


def test_abi_argument_checks_name_the_entry():
    ERR_ARG = 1
    clips, ftab = _tables()
    assert _call_host(clips, ftab) == 0
    assert _call_host(clips, ftab, n_clips=0) == ERR_ARG and "0 clips" in _err()
    many, mtab = _tables(lengths=[16] * 65, bits=[16] * 65, block=16)
    assert _call_host(many, mtab) == ERR_ARG and "65 clips" in _err()
    clips, ftab = _tables()
    clips[1].bits_per_sample = 20
    assert _call_host(clips, ftab) == ERR_ARG and "clip 1: 20 bits" in _err()
    clips, ftab = _tables()
    assert _call_host(clips, ftab, n_samples=139) == ERR_ARG and "clip 1" in _err() and "139 samples given" in _err()
    clips, ftab = _tables()
    ftab[0].first_sample, ftab[1].first_sample = 64, 0          # a clip's frames out of order
    assert _call_host(clips, ftab) == ERR_ARG and "frame 0: starts at sample 64" in _err()
    clips, ftab = _tables()
    ftab[1].block_size = 35                                     # clip 0 is left one sample short
    assert _call_host(clips, ftab) == ERR_ARG and "clip 0: its frames hold 99 of 100" in _err()
    clips, ftab = _tables()
    ftab[1].block_size = 37                                     # one past the clip's end
    assert _call_host(clips, ftab) == ERR_ARG and "frame 1: ends at sample 101" in _err()
    for bad in (0, 4609):
        clips, ftab = _tables()
        ftab[2].block_size = bad
        assert _call_host(clips, ftab) == ERR_ARG and "frame 2: block size %d" % bad in _err()
    for bad in (5, 17):
        clips, ftab = _tables()
        ftab[1].header_len = bad
        assert _call_host(clips, ftab) == ERR_ARG and "frame 1: header of %d bytes" % bad in _err()
    clips, ftab = _tables()
    ftab[2].clip = 2
    assert _call_host(clips, ftab) == ERR_ARG and "frame 2: clip 2 of 2" in _err()
    clips, ftab = _tables()
    L = N.lib()
    bound = L.gsv_flac_encode_bound(clips, 2, ftab, len(ftab))
    assert bound == sum(ftab[f].header_len + 1 + ftab[f].block_size * (2 if ftab[f].clip == 0 else 3) + 2 for f in range(len(ftab)))
    assert _call_host(clips, ftab, out_bytes=bound) == 0
    assert _call_host(clips, ftab, out_bytes=bound - 1) == ERR_ARG and "out_bytes %d (%d needed" % (bound - 1, bound) in _err()
    # the device entry point refuses before anything is launched: the pointers are never followed
    need = L.gsv_flac_encode_workspace(clips, 2, ftab, len(ftab))
    assert need >= bound
    fake = 0x10000
    assert L.gsv_flac_encode(fake, 140, clips, 2, ftab, len(ftab), fake, bound, fake, None, fake, need - 1, None) == ERR_ARG
    assert "workspace of %d bytes (%d needed" % (need - 1, need) in _err()
    assert L.gsv_flac_encode(fake, 140, clips, 2, ftab, len(ftab), fake, bound, fake, None, fake + 8, need, None) == ERR_ARG
    assert "16-byte aligned" in _err()
    assert L.gsv_flac_encode(fake, 140, clips, 2, ftab, len(ftab), fake, bound - 1, fake, None, fake, need, None) == ERR_ARG
    assert "out_bytes" in _err()
    clips[0].bits_per_sample = 8
    assert L.gsv_flac_encode_bound(clips, 2, ftab, len(ftab)) == 0 and L.gsv_flac_encode_workspace(clips, 2, ftab, len(ftab)) == 0


def test_python_argument_checks_name_the_clip():
    ok = np.zeros(100, dtype=np.float32)
    for kw, waves, what in (
            ({}, [ok, np.zeros((2, 50), dtype=np.float32)], r"clip 1: 2 dimensions"),
            ({}, [ok, ok, torch.zeros(0)], r"clip 2: 0 samples"),
            ({"bits": 20}, [ok], r"clip 0: 20 bits"),
            ({"bits": [16, 8]}, [ok, ok], r"clip 1: 8 bits"),
            ({"block_size": 15}, [ok], r"clip 0: block size 15"),
            ({"block_size": [4096, 4609]}, [ok, ok], r"clip 1: block size 4609"),
            ({"rate": 0}, [ok], r"clip 0: sample rate 0"),
            ({"rate": [32000, 655351]}, [ok, ok], r"clip 1: sample rate 655351"),
            ({}, [ok, [0.0, 1.0]], r"clip 1: a list")):
        kw = dict(kw)
        rate = kw.pop("rate", 32000)
        with pytest.raises(ValueError, match=what):
            flacio.encode_flacs(waves, rate, device="cpu", **kw)
    with pytest.raises(ValueError, match="2 sample rates for 1 clips"):
        flacio.encode_flacs([ok], [1, 2], device="cpu")
    assert flacio.encode_flacs([], [], device="cpu") == []
    data = flacio.encode_flac(ok, 655350, bits=24, block_size=16, device="cpu")
    assert data[:4] == b"fLaC" and int.from_bytes(data[18:26], "big") >> 44 == 655350


# ----------------------------------------------------------------------------------------------------------- AudioClip
def _have_soundfile():
    try:
        import soundfile  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.mark.skipif(_have_soundfile(), reason="with soundfile AudioClip.save hands the path to sf.write")
def test_audioclip_save_flac_and_wav(tmp_path):
    from gsv_tts_lite_amd.tts import AudioClip
    audio = E.signal("tone", 32000 + 17, seed=9)
    audio[5] = 1.5
    clip = AudioClip(None, audio, 32000, len(audio) / 32000, [{"text": "a", "start_s": 0.0, "end_s": 1.0}], "a")
    for name in ("a.flac", "B.FLAC"):
        path = str(tmp_path / name)
        clip.save(path, is_save_subtitles=name == "a.flac")
        info, frames, raw = flacio.parse_flac(path)
        assert (info.channels, info.bits_per_sample, info.sample_rate, info.n_samples) == (1, 16, 32000, len(audio))
        rc, (got,), status = decode_host([(info, frames, raw)])
        assert rc == 0 and not status.any() and np.array_equal(got[:, 0], E.quantise(audio, 16))
        assert clip.to_flac() == raw
    assert os.path.exists(str(tmp_path / "a.json")) and not os.path.exists(str(tmp_path / "B.json"))
    raw24 = clip.to_flac(bits=24)
    assert raw24[:4] == b"fLaC" and (int.from_bytes(raw24[18:26], "big") >> 36) & 31 == 23
    clip.save(str(tmp_path / "a.wav"))
    want = str(tmp_path / "want.wav")
    with wave.open(want, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(32000)
        w.writeframes((np.clip(audio, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
    assert open(str(tmp_path / "a.wav"), "rb").read() == open(want, "rb").read()
    assert open(str(tmp_path / "a.wav"), "rb").read(4) == b"RIFF"
