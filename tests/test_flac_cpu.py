"""CPU checks of FLAC files as reference audio: the container parser and frame indexer (flacio.parse_flac), the frame
decoder of csrc/flacdec.h run by the CPU (gsv_flac_decode_host: the very routine the GPU kernel runs) against the
integers tests/flac_writer.py encoded, the ABI's argument checks, and the facade's routing of .flac keys.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_writer as fw  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio  # noqa: E402

GRID = fw.grid()


def decode_host(parsed):
    """gsv_flac_decode_host over parsed = [(info, frames, raw)] -> (rc, [x_i [n, ch] int32], status [n_frames])"""
    packed, clips, ftab, _ = flacio.tables(parsed)
    pcm = np.full(sum(i.n_samples * i.channels for i, _, _ in parsed), 0x5A5A5A5A, dtype=np.int32)
    status = np.full(len(ftab), -1, dtype=np.int32)
    buf = (ctypes.c_ubyte * len(packed)).from_buffer(packed)
    rc = N.lib().gsv_flac_decode_host(ctypes.addressof(buf), len(packed), clips, len(clips), ftab, len(ftab), pcm.ctypes.data,
                                      status.ctypes.data)
    out, at = [], 0
    for info, _, _ in parsed:
        out.append(pcm[at:at + info.n_samples * info.channels].reshape(-1, info.channels))
        at += info.n_samples * info.channels
    return rc, out, status


def test_crc_check_values():
    assert fw.crc8(b"123456789") == 0xF4
    assert fw.crc16(b"123456789") == 0xFEE8


@pytest.mark.parametrize("name", sorted(GRID))
def test_round_trip(tmp_path, name):
    x, bps, rate, kw = GRID[name]
    data, table = fw.flac_bytes(x, bps, rate, **kw)
    path = tmp_path / (name + ".flac")
    path.write_bytes(data)
    info, frames, raw = flacio.parse_flac(str(path))
    assert (info.channels, info.bits_per_sample, info.sample_rate, info.n_samples) == (x.shape[1], bps, rate, len(x))
    assert info.md5 == fw.md5_of(x, bps)
    assert [tuple(f) for f in frames] == table
    rc, (got,), status = decode_host([(info, frames, raw)])
    assert rc == 0 and not status.any(), status
    assert np.array_equal(got, x)


def test_several_clips_in_one_call(tmp_path):
    names = ["bits24_ch1", "stereo_ms", "len17", "bits8_ch2", "variable"]
    parsed = []
    for n in names:
        x, bps, rate, kw = GRID[n]
        parsed.append(flacio.parse_flac(fw.write(tmp_path / (n + ".flac"), x, bps, rate, **kw)))
    rc, got, status = decode_host(parsed)
    assert rc == 0 and not status.any()
    for n, g in zip(names, got):
        assert np.array_equal(g, GRID[n][0]), n


# --------------------------------------------------------------------------------------------------------- container
def test_extra_metadata_blocks_are_skipped(tmp_path):
    x = fw.tone(700, 2, 16, seed=1)
    meta = [(1, bytes(100)), (4, b"\x05\0\0\0vendo\0\0\0\0"), (3, bytes(36)), (6, b"\xff\xf8" * 40), (99, b"unknown")]
    info, frames, raw = flacio.parse_flac(fw.write(tmp_path / "m.flac", x, 16, 32000, block_size=576, metadata=meta,
                                                   sub=fw.Sub("fixed", order=2, params=6)))
    assert info.n_samples == 700 and len(frames) == 2
    assert np.array_equal(decode_host([(info, frames, raw)])[1][0], x)


def test_unknown_total_and_trailing_junk(tmp_path):
    x = fw.tone(1000, 1, 16, seed=2)
    junk = bytes(np.random.default_rng(0).integers(0, 256, 128, dtype=np.uint8))
    for i, kw in enumerate((dict(total_samples=0), dict(after=junk), dict(total_samples=0, after=junk),
                            dict(frame_sizes_known=False, after=junk))):
        info, frames, raw = flacio.parse_flac(fw.write(tmp_path / ("%d.flac" % i), x, 16, 16000, block_size=192,
                                                       sub=fw.Sub("fixed", order=1, params=8), **kw))
        assert info.n_samples == 1000 and len(frames) == 6, kw
        rc, (got,), status = decode_host([(info, frames, raw)])
        assert rc == 0 and not status.any() and np.array_equal(got, x), kw


def test_a_planted_sync_code_is_no_frame(tmp_path):
    x = fw.noise(600, 2, 16, seed=3)
    x[100:130, 0] = -8                  # 0xFFF8 0xFFF8 ... in the VERBATIM subframe: sync code, frame number 0x78 ...
    x[200:230, 0] = -7                  # and the variable-blocking sync
    info, frames, raw = flacio.parse_flac(fw.write(tmp_path / "s.flac", x, 16, 44100, block_size=192, sub=fw.Sub("verbatim")))
    assert raw.count(b"\xff\xf8") > 30 and len(frames) == 4
    assert np.array_equal(decode_host([(info, frames, raw)])[1][0], x)


def test_multi_byte_frame_and_sample_numbers(tmp_path):
    x = fw.tone(16 * 140 + 3, 1, 16, seed=4)                 # frame numbers past 127: two bytes
    info, frames, raw = flacio.parse_flac(fw.write(tmp_path / "f.flac", x, 16, 8000, block_size=16, sub=fw.Sub("fixed", order=1, params=9)))
    assert len(frames) == 141
    assert np.array_equal(decode_host([(info, frames, raw)])[1][0], x)
    y = fw.tone(70000, 1, 16, seed=5)                         # sample numbers past 2^16: two, three and four bytes
    info, frames, raw = flacio.parse_flac(fw.write(tmp_path / "v.flac", y, 16, 8000, variable=True, block_sizes=[100, 2000, 4608, 60000, 1000],
                                                   sub=fw.Sub("fixed", order=1, params=9)))
    assert [f.first_sample for f in frames] == [0, 100, 2100, 6708, 66708, 67708, 68708, 69708]
    assert np.array_equal(decode_host([(info, frames, raw)])[1][0], y)
    # the longest codings: a 6-byte frame number and a 7-byte sample number
    assert len(fw.utf8_number(2 ** 31 - 1)) == 6 and len(fw.utf8_number(2 ** 36 - 1)) == 7
    for variable, first in ((False, 2 ** 31 - 1), (True, 2 ** 36 - 16)):
        fr = fw.frame_bytes(x[:16], 16, 8000, first, variable=variable, sub=fw.Sub("verbatim"))
        clips = (N.FlacClip * 1)(N.FlacClip(1, 16, 16, 0, 0))
        ftab = (N.FlacFrame * 1)(N.FlacFrame(0, 16, 0, len(fr), 0, 0, 0))
        pcm, status = np.zeros(16, dtype=np.int32), np.zeros(1, dtype=np.int32)
        assert N.lib().gsv_flac_decode_host(fr, len(fr), clips, 1, ftab, 1, pcm.ctypes.data, status.ctypes.data) == 0
        assert status[0] == 0 and np.array_equal(pcm, x[:16, 0])


# ------------------------------------------------------------------------------------------------------------ errors
def test_what_is_outside_is_named(tmp_path):
    x3 = fw.tone(100, 3, 16, seed=6)
    with pytest.raises(NotImplementedError, match="3 channels"):
        flacio.parse_flac(fw.write(tmp_path / "c3.flac", x3, 16, 48000, block_size=192))
    # 32 bits per sample: only STREAMINFO says so (the writer's frames stop at 24)
    data, _ = fw.flac_bytes(fw.tone(100, 1, 24, seed=7), 24, 48000, block_size=192)
    raw = bytearray(data)
    v = int.from_bytes(raw[18:26], "big") | (31 << 36)
    raw[18:26] = v.to_bytes(8, "big")
    (tmp_path / "b32.flac").write_bytes(raw)
    with pytest.raises(NotImplementedError, match="32 bits per sample"):
        flacio.parse_flac(str(tmp_path / "b32.flac"))
    (tmp_path / "o.flac").write_bytes(b"OggS" + bytes(60))
    with pytest.raises(NotImplementedError, match="Ogg"):
        flacio.parse_flac(str(tmp_path / "o.flac"))
    (tmp_path / "i.flac").write_bytes(b"ID3\x04\0\0\0\0\0\x0a" + bytes(10) + data)
    with pytest.raises(NotImplementedError, match="ID3v2 tag"):
        flacio.parse_flac(str(tmp_path / "i.flac"))
    with pytest.raises(NotImplementedError, match="i.flac"):
        flacio.load_flacs([str(tmp_path / "i.flac")], "cuda:0")          # named before any upload


def test_malformed_files_name_the_frame(tmp_path):
    x = fw.tone(1000, 2, 16, seed=8)
    data, table = fw.flac_bytes(x, 16, 44100, block_size=192, sub=fw.Sub("fixed", order=2, params=6))
    p = tmp_path / "x.flac"
    p.write_bytes(b"fLaC" + fw.metadata_block(1, bytes(20), last=True) + data[42:])
    with pytest.raises(ValueError, match="no STREAMINFO"):
        flacio.parse_flac(str(p))
    p.write_bytes(data[:42])
    with pytest.raises(ValueError, match="no audio frame"):
        flacio.parse_flac(str(p))
    off, ln = table[2][0], table[2][1]
    p.write_bytes(data[:off + ln // 2])                       # cut inside frame 2
    with pytest.raises(ValueError, match=r"x\.flac: frame 2: .*ends inside the audio"):
        flacio.parse_flac(str(p))
    p.write_bytes(data[:table[3][0]])                         # cut at a frame boundary: frames 0-2 whole, 424 samples short
    with pytest.raises(ValueError, match=r"x\.flac: frame 2"):
        flacio.parse_flac(str(p))
    p.write_bytes(data[:42] + bytes(40) + data[42:])          # bytes between the metadata and frame 0: no header there
    with pytest.raises(ValueError, match=r"x\.flac: frame 0: no valid frame header at byte 42"):
        flacio.parse_flac(str(p))
    # bytes between two frames: the indexer bridges them to the next header, the decoder reports the frame in front
    p.write_bytes(data[:table[1][0]] + bytes(40) + data[table[1][0]:])
    parsed = flacio.parse_flac(str(p))
    assert parsed[1][0].length == table[0][1] + 40
    rc, _, status = decode_host([parsed])
    assert rc == 0 and list(np.flatnonzero(status)) == [0] and status[0] == 10      # structure ends before the frame does


def test_a_flipped_residual_bit_is_a_crc16_mismatch(tmp_path):
    x = fw.tone(1000, 2, 16, seed=9)
    data, table = fw.flac_bytes(x, 16, 44100, block_size=192, sub=fw.Sub("fixed", order=2, params=6))
    raw = bytearray(data)
    off, ln = table[3][0], table[3][1]
    raw[off + ln - 30] ^= 0x01                  # the low bit of a Rice remainder: the structure stays intact
    p = tmp_path / "r.flac"
    p.write_bytes(raw)
    parsed = flacio.parse_flac(str(p))
    assert [tuple(f) for f in parsed[1]] == table
    rc, (got,), status = decode_host([parsed])
    assert rc == 0 and list(np.flatnonzero(status)) == [3] and status[3] == N.FLAC_CRC16
    assert not got[3 * 192:4 * 192].any()                              # the failed frame is zero-filled
    assert np.array_equal(got[:3 * 192], x[:3 * 192]) and np.array_equal(got[4 * 192:], x[4 * 192:])
    with pytest.raises(ValueError, match=r"r\.flac: frame 3: CRC-16 mismatch"):
        raise flacio.status_error(str(p), 3, int(status[3]))


def test_hostile_structures_end_with_their_status():
    """reserved codes, an order larger than the block, partitions that do not divide it, an overlong unary run, a lying
    block size: each a distinct nonzero status and a zero-filled frame"""
    x = fw.tone(192, 1, 16, seed=10)

    def status_of(fr, bs=192, bps=16):
        clips = (N.FlacClip * 1)(N.FlacClip(1, bps, bs, 0, 0))
        ftab = (N.FlacFrame * 1)(N.FlacFrame(0, bs, 0, len(fr), 0, 0, 0))
        pcm, status = np.full(bs, 7, dtype=np.int32), np.zeros(1, dtype=np.int32)
        assert N.lib().gsv_flac_decode_host(bytes(fr), len(fr), clips, 1, ftab, 1, pcm.ctypes.data, status.ctypes.data) == 0
        assert status[0] == 0 or not pcm.any()
        return int(status[0])

    def mend(fr, header=5):
        fr = bytearray(fr)
        fr[header] = fw.crc8(fr[:header])
        fr[-2:] = fw.crc16(fr[:-2]).to_bytes(2, "big")
        return fr

    good = bytearray(fw.frame_bytes(x, 16, 44100, 0, sub=fw.Sub("fixed", order=2, params=6)))
    assert status_of(good) == 0
    assert status_of(good[:-1]) != 0 and status_of(good[:5]) == 1 and status_of(good + b"\0") in (10, 11)
    bad = bytearray(good); bad[1] = 0xFA
    assert status_of(bad) == 2                                         # reserved bit behind the sync code
    for byte, val in ((2, 0x09), (2, 0x1F), (3, 0xB8), (3, 0x06), (3, 0x0E)):     # block size 0, rate 15, channels 11, size 3 / 7
        bad = bytearray(good); bad[byte] = val
        assert status_of(mend(bad)) == 3, (byte, val)
    bad = bytearray(good); bad[4] = 0x80                               # a continuation byte as the coded number
    assert status_of(mend(bad)) == 3
    bad = bytearray(good); bad[5] ^= 0xFF
    assert status_of(bad) == 4                                         # CRC-8
    assert status_of(good, bs=191) == 5 and status_of(good, bps=24) == 5     # block size / sample size against the tables
    for val, want in ((0x04, 3), (0x1A, 3), (0x40, 3), (0x80, 3)):     # reserved subframe types, the pad bit
        bad = bytearray(good); bad[6] = val
        assert status_of(mend(bad)) == want, val
    short = fw.frame_bytes(x[:3], 16, 44100, 0, sub=fw.Sub("fixed", order=2, params=6))
    bad = bytearray(short); bad[7] = 0x18                              # FIXED order 4 in a block of 3 (explicit size: header is 7 bytes)
    assert status_of(mend(bad, 6), bs=3) == 6
    lpc = bytearray(fw.frame_bytes(x, 16, 44100, 0, sub=fw.Sub("lpc", order=1, precision=15, shift=14, params=9)))
    assert lpc[6] == 0x40 and status_of(lpc) == 0                      # LPC order 1; 16 warm-up bits; then precision, shift
    bad = bytearray(lpc); bad[9] |= 0xF0
    assert status_of(mend(bad)) == 3                                   # precision code 15
    bad = bytearray(lpc); bad[9] = (bad[9] & 0xF0) | 0x08
    assert status_of(mend(bad)) == 3                                   # negative shift
    # FIXED 2: subframe byte, 2 x 16 warm-up bits, then method (2 bits) and partition order (4 bits) in byte 11
    assert good[11] >> 6 == 0
    bad = bytearray(good); bad[11] |= 0x80
    assert status_of(mend(bad)) == 3                                   # residual method 2
    bad = bytearray(good); bad[11] = (bad[11] & 0xC3) | (7 << 2)
    assert status_of(mend(bad)) == 7                                   # 128 partitions do not divide 192
    unary = bytearray(good); unary[13:-2] = bytes(len(unary) - 15)
    assert status_of(mend(unary)) == 1                                 # a unary run to the end of the frame


# --------------------------------------------------------------------------------------------------------------- ABI
def test_abi_argument_checks():
    L = N.lib()
    x = fw.tone(400, 1, 16, seed=11)
    data, table = fw.flac_bytes(x, 16, 16000, block_size=192)
    pcm, status = np.zeros(400, dtype=np.int32), np.zeros(3, dtype=np.int32)

    def call(clips, frames, n_bytes=len(data)):
        c = (N.FlacClip * len(clips))(*clips)
        f = (N.FlacFrame * len(frames))(*frames)
        return L.gsv_flac_decode_host(data, n_bytes, c, len(clips), f, len(frames), pcm.ctypes.data, status.ctypes.data)

    clip = N.FlacClip(1, 16, 400, 0, 0)
    rows = [N.FlacFrame(0, bs, off, ln, first, 0, 0) for off, ln, first, bs in table]
    assert call([clip], rows) == 0 and not status.any() and np.array_equal(pcm, x[:, 0])
    assert call([clip], [rows[1], rows[0], rows[2]]) == 1 and b"frame 0" in L.gsv_last_error()      # out of order
    assert call([clip], rows[:2]) == 1 and b"clip 0" in L.gsv_last_error()                           # does not tile
    assert call([clip], rows, n_bytes=table[2][0] + table[2][1] - 1) == 1 and b"frame 2" in L.gsv_last_error()
    assert b"run past" in L.gsv_last_error()
    assert call([N.FlacClip(3, 16, 400, 0, 0)], rows) == 1 and b"channels" in L.gsv_last_error()
    assert call([N.FlacClip(1, 32, 400, 0, 0)], rows) == 1 and b"bits" in L.gsv_last_error()
    assert call([N.FlacClip(1, 7, 400, 0, 0)], rows) == 1
    assert call([clip] * (N.AUX_MAX_CLIPS + 1), rows) == 1
    assert call([clip], [N.FlacFrame(1, 192, 0, 10, 0, 0, 0)]) == 1 and b"clip 1" in L.gsv_last_error()
    assert L.gsv_flac_decode_workspace((N.FlacClip * 1)(clip), 1, 3) >= 3 * 32 + 400 * 4


def test_cpu_device_is_refused(tmp_path):
    x = fw.tone(300, 1, 16, seed=12)
    path = fw.write(tmp_path / "ok.flac", x, 16, 16000, block_size=192)
    with pytest.raises(RuntimeError, match="no CPU path"):
        flacio.load_flac(path, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        flacio.load_flacs([path, path], torch.device("cpu"))
    assert flacio.load_flacs([], "cuda:0") == []


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


def test_flac_keys_on_the_cpu_fail_loudly(tts, tmp_path):
    """a .flac key reaches the FLAC reader (which has no CPU path); before this feature it was refused as a file that
    needs a codec library (NotImplementedError)"""
    import wav_writer as ww
    path = fw.write(tmp_path / "spk.flac", fw.tone(32000, 1, 16, seed=13), 16, 32000)
    wav = ww.write(tmp_path / "spk.wav", ww.samples("s16", 3200, 1), "s16", 32000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_spk_audio(path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_prompt_audio(path, "prompt text.", phones1=[1, 2, 3])
    with pytest.raises(RuntimeError, match="FLAC frames are decoded on the MI355X only"):
        tts.cache_spk_audio([path, path])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_spk_audio([wav, path])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_prompt_audio([path], "prompt text.", phones1=[1, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.verify_speaker(path, path)
    three = fw.write(tmp_path / "three.flac", fw.tone(300, 3, 16, seed=14), 16, 32000, block_size=192)
    with pytest.raises(NotImplementedError, match="3 channels"):
        tts.cache_spk_audio(three)
    assert tts.spk_audio_cache == {} and tts.prompt_audio_cache == {}
