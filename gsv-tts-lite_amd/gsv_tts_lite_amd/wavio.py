"""WAV files as reference audio: what TTS._load_audio (gsv_tts/TTS.py:1811-1823) gets from PyAV for a WAV file -- mono
fp32 at the file's own rate -- with the RIFF/WAVE container parsed on the host (struct) and the samples converted on the
device (gsv_wav_to_mono*, csrc/wavpcm.h).

    wav, sr = load_wav("spk.wav", "cuda:0")            # fp32 [n_frames] on the device, the file's rate
    clips = load_wavs(["a.wav", "b.wav"], "cuda:0")     # [(wav, sr)]: one packed upload, one launch per 64 clips

Only the data chunk's bytes cross to the device, as they are in the file.  Read: format tags 1 (integer PCM: u8, s16,
packed s24, s32), 3 (IEEE float: f32, f64) and 0xFFFE (WAVE_FORMAT_EXTENSIBLE with the PCM or float sub-format), one or
two channels.  Compressed audio (MP3, Ogg, FLAC, A-law, mu-law, ADPCM) and more than two channels raise
NotImplementedError here: they need a decoder, or ffmpeg's downmix matrices, outside this module.  (Native FLAC files
have their own reader beside this one, flacio.py, and the facade sends a file that starts with "fLaC" there; this module
stays WAV-only.)  No CPU path."""
import struct
from collections import namedtuple

import torch

from . import _native as N

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")        # index = GSV_PCM_* code
SAMPLE_BYTES = (1, 2, 3, 4, 4, 8)

WavInfo = namedtuple("WavInfo", "format channels sample_rate n_frames data_offset")   # format: a FORMATS index

TAG_PCM, TAG_FLOAT, TAG_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
# KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT: the format tag as the GUID's first four bytes, then this tail
_GUID_TAIL = bytes.fromhex("00001000800000aa00389b71")
_TAG_NAMES = {0x0002: "Microsoft ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10",
              0x0050: "MPEG audio", 0x0055: "MP3", 0x0161: "WMA", 0x2000: "AC-3", 0xF1AC: "FLAC"}


def _outside(path, what):
    return NotImplementedError("%s: %s; decoding it needs a codec library outside this build's scope (only PCM and "
                               "IEEE-float WAV files are read)" % (path, what))


def _sniff(head: bytes) -> str:
    """what a file that is not RIFF/WAVE looks like"""
    if head[:3] == b"ID3" or (len(head) >= 2 and head[0] == 0xFF and head[1] & 0xE0 == 0xE0):
        return "ID3/MP3 (MPEG audio)"
    if head[:4] == b"OggS":
        return "OggS (Ogg: Vorbis / Opus)"
    if head[:4] == b"fLaC":
        return "fLaC (FLAC)"
    if head[:4] in (b"RF64", b"BW64"):
        return "%s (64-bit WAV)" % head[:4].decode()
    if head[:4] == b"FORM":
        return "FORM (AIFF)"
    if head[:4] == b"RIFF":
        return "a RIFF file of form %r, not WAVE" % head[8:12].decode("latin-1")
    return "not a RIFF/WAVE file (it starts with %r)" % bytes(head[:4])


def _sample_format(path, tag, bits):
    if tag == TAG_PCM:
        nbytes = (bits + 7) // 8                     # ffmpeg rounds the container width up to whole bytes
        if 1 <= nbytes <= 4:
            return nbytes - 1                        # u8, s16, s24, s32
        raise _outside(path, "%d-bit integer PCM" % bits)
    if tag == TAG_FLOAT:
        if bits in (32, 64):
            return FORMATS.index("f32" if bits == 32 else "f64")
        raise _outside(path, "%d-bit IEEE float" % bits)
    raise _outside(path, "a WAV file of format tag 0x%04X (%s)" % (tag, _TAG_NAMES.get(tag, "compressed or unknown")))


def parse_wav(path):
    """-> (WavInfo, the file's bytes).  NotImplementedError for what needs a decoder (names it) and for more than two
    channels; ValueError for a malformed RIFF/WAVE file or one without a complete frame.  Unknown chunks (LIST, fact,
    cue , ...) are skipped with their pad byte; a data size of 0 or 0xFFFFFFFF (a streamed writer) or one past the end of
    the file runs to the end of the file, and a truncated last frame is dropped."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise _outside(path, "it looks like " + _sniff(raw[:12]))
    fmt = data = None
    pos = 12
    while pos + 8 <= len(raw):
        cid = raw[pos:pos + 4]
        size = struct.unpack_from("<I", raw, pos + 4)[0]
        body = pos + 8
        if cid == b"data":
            end = len(raw) if size in (0, 0xFFFFFFFF) else min(body + size, len(raw))
            data = (body, end)
            if end == len(raw):
                break
        elif cid == b"fmt ":
            fmt = raw[body:body + size]
        pos = body + size + (size & 1)
    if fmt is None or len(fmt) < 16:
        raise ValueError("%s: RIFF/WAVE file without a complete 'fmt ' chunk" % path)
    if data is None:
        raise ValueError("%s: RIFF/WAVE file without a 'data' chunk" % path)
    tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", fmt)
    if tag == TAG_EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError("%s: WAVE_FORMAT_EXTENSIBLE 'fmt ' chunk of %d bytes (40 expected)" % (path, len(fmt)))
        sub = fmt[24:40]
        if sub[4:] != _GUID_TAIL:
            raise _outside(path, "a WAVE_FORMAT_EXTENSIBLE file of sub-format GUID %s" % sub.hex())
        tag = struct.unpack_from("<I", sub)[0]
    fi = _sample_format(path, tag, bits)
    if channels > 2:
        raise _outside(path, "%d channels (only mono and stereo are mixed down; ffmpeg's matrices for other layouts "
                             "are not guessed)" % channels)
    if channels < 1 or rate < 1:
        raise ValueError("%s: %d channels at %d Hz" % (path, channels, rate))
    n_frames = (data[1] - data[0]) // (SAMPLE_BYTES[fi] * channels)
    if n_frames < 1:
        raise ValueError("%s: the data chunk holds no complete audio frame" % path)
    if n_frames > 0x7FFFFFFF:
        raise ValueError("%s: %d frames (at most 2^31 - 1)" % (path, n_frames))
    return WavInfo(fi, channels, rate, n_frames, data[0]), raw


def _device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    if dev.type != "cuda":
        raise RuntimeError("WAV samples are converted on the MI355X only (gsv_wav_to_mono); got device %s -- there is no "
                           "CPU path" % dev)
    return dev


def _nbytes(info: WavInfo) -> int:
    return info.n_frames * info.channels * SAMPLE_BYTES[info.format]


def load_wav(path, device=None):
    """TTS._load_audio for a WAV file -> (fp32 mono [n_frames] on `device`, sample rate)"""
    return load_wavs([path], device)[0]


def load_wavs(paths, device=None):
    """load_wav of every path -> [(fp32 mono [n_frames_i] on `device`, sample rate)]: every file parsed first, then the
    data chunks packed into one upload and converted in one launch per AUX_MAX_CLIPS clips.  Each waveform is a view of
    one packed tensor and bit-identical to load_wav of its file."""
    parsed = [parse_wav(p) for p in paths]
    dev = _device(device)
    if not parsed:
        return []
    sizes = [_nbytes(info) for info, _ in parsed]
    packed = bytearray(sum(sizes))
    off = 0
    for (info, raw), nb in zip(parsed, sizes):
        packed[off:off + nb] = raw[info.data_offset:info.data_offset + nb]
        off += nb
    pcm = torch.frombuffer(packed, dtype=torch.uint8).to(dev)
    out = torch.empty(sum(info.n_frames for info, _ in parsed), dtype=torch.float32, device=dev)
    L = N.lib()
    st = N.current_stream_ptr(dev)
    b0 = f0 = 0           # bytes and frames before the chunk
    for c0 in range(0, len(parsed), N.AUX_MAX_CLIPS):
        chunk = parsed[c0:c0 + N.AUX_MAX_CLIPS]
        clips = (N.WavClip * len(chunk))()
        b = 0
        for j, (info, _) in enumerate(chunk):
            clips[j] = N.WavClip(b, info.n_frames, info.format, info.channels)
            b += _nbytes(info)
        N.check(L.gsv_wav_to_mono_batch(pcm[b0:].data_ptr(), b, clips, len(chunk), out[f0:].data_ptr(), st))
        b0 += b
        f0 += sum(info.n_frames for info, _ in chunk)
    res, f = [], 0
    for info, _ in parsed:
        res.append((out[f:f + info.n_frames], info.sample_rate))
        f += info.n_frames
    return res
