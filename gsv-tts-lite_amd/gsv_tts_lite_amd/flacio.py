"""FLAC files as reference audio: what TTS._load_audio (gsv_tts/TTS.py:1811-1823) gets from PyAV for a FLAC file -- mono
fp32 at the file's own rate -- with the container parsed and the frames INDEXED on the host (no sample is decoded here)
and every frame decoded on the device (gsv_flac_decode, csrc/flacdec.h: one lane per frame), then converted by the WAV
path's own kernel.  A FLAC clip is bit-identical to the WAV file that holds the same integers.

    wav, sr = load_flac("spk.flac", "cuda:0")            # fp32 [n_samples] on the device, the file's rate
    clips = load_flacs(["a.flac", "b.flac"], "cuda:0")    # [(wav, sr)]: one packed upload, one decode per 64 clips

Read: native FLAC, one or two channels, 8..24 bits per sample, fixed or variable block size.  More than two channels,
32 bits per sample, Ogg-encapsulated FLAC and a file with an ID3v2 tag in front raise NotImplementedError.  The
STREAMINFO MD5 is parsed and exposed (FlacInfo.md5) but NOT verified: that would need the integers back on the host.
What is verified: each header's CRC-8 (here, while indexing) and each frame's CRC-16 (on the device).  No CPU path."""
import struct
from collections import namedtuple

import torch

from . import _native as N
from .wavio import _outside

FlacInfo = namedtuple("FlacInfo", "channels bits_per_sample sample_rate n_samples min_block max_block min_frame max_frame md5")
FlacFrame = namedtuple("FlacFrame", "offset length first_sample block_size")      # offset: into the file

_BLOCK = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608}
_RATE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_BITS = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}


def _crc8(data) -> int:
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def _crc8_table():
    t = []
    for x in range(256):
        for _ in range(8):
            x = ((x << 1) ^ 0x07) & 0xFF if x & 0x80 else x << 1
        t.append(x)
    return t


_CRC8 = _crc8_table()


def _header(raw, pos, info, variable, expect):
    """the frame header at raw[pos:], accepted only when sync and reserved bits are right, its fields agree with
    STREAMINFO, its coded number is `expect` (frame index, or first sample in variable blocking) and its CRC-8 passes
    -> block size, or None"""
    h = raw[pos:pos + 16]               # 4 fixed bytes, a number of up to 7, up to 2 + 2 explicit bytes, the CRC-8
    if len(h) < 6 or h[0] != 0xFF or h[1] != (0xF9 if variable else 0xF8):
        return None
    bs_code, sr_code = h[2] >> 4, h[2] & 15
    ch_code, ss_code = h[3] >> 4, (h[3] >> 1) & 7
    if h[3] & 1 or bs_code == 0 or sr_code == 15 or ch_code > 10 or ss_code in (3, 7):
        return None
    if (ch_code + 1 if ch_code < 8 else 2) != info.channels or (ss_code and _BITS[ss_code] != info.bits_per_sample):
        return None
    ones = 0
    while ones < 8 and h[4] & (0x80 >> ones):
        ones += 1
    if ones == 1 or ones == 8 or (ones == 7 and not variable):
        return None
    extra = max(ones - 1, 0)
    n_bs = 1 if bs_code == 6 else 2 if bs_code == 7 else 0
    n_sr = 1 if sr_code == 12 else 2 if sr_code in (13, 14) else 0
    p = 5 + extra                       # behind the coded number
    if len(h) < p + n_bs + n_sr + 1:
        return None
    num = h[4] & (0x7F >> ones) if ones else h[4]
    for c in h[5:p]:
        if c & 0xC0 != 0x80:
            return None
        num = (num << 6) | (c & 0x3F)
    if num != expect:
        return None
    if bs_code == 6:
        bs = h[p] + 1
    elif bs_code == 7:
        bs = (h[p] << 8 | h[p + 1]) + 1
    else:
        bs = _BLOCK[bs_code] if bs_code < 6 else 256 << (bs_code - 8)
    p += n_bs
    if sr_code == 0:
        rate = info.sample_rate
    elif sr_code == 12:
        rate = h[p] * 1000
    elif sr_code == 13:
        rate = h[p] << 8 | h[p + 1]
    elif sr_code == 14:
        rate = (h[p] << 8 | h[p + 1]) * 10
    else:
        rate = _RATE[sr_code]
    p += n_sr
    if rate != info.sample_rate or bs > info.max_block or bs > 65535:
        return None
    if _crc8(h[:p]) != h[p]:
        return None
    return bs


def parse_flac(path):
    """-> (FlacInfo, [FlacFrame], the file's bytes).  The frame index is built without decoding: from the running
    position a header is accepted only when it is consistent with STREAMINFO, carries the expected next frame / sample
    number and passes its CRC-8; a frame ends where the next accepted header begins (bytes.find for the sync code, from
    min_frame_size past the current header when STREAMINFO gives one); the device's CRC-16 check catches a false
    boundary.  A total of 0 samples in STREAMINFO (unknown) becomes the sum of the block sizes; bytes behind the last
    frame are ignored once the total is reached.  NotImplementedError for what is outside this build (names it);
    ValueError, naming the path and the frame, for a file without STREAMINFO or frames, a gap the indexer cannot
    bridge, or fewer samples than STREAMINFO promises.  The last frame's length is an upper bound (no header follows
    it): the decoder takes its CRC-16 from where its structure ends (GSV_FLAC_OPEN_END)."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:3] == b"ID3":
        raise _outside(path, "an ID3v2 tag in front of the audio%s" % (
            " (a FLAC stream follows it; strip the tag)" if b"fLaC" in raw[:1 << 20] else ""))
    if raw[:4] == b"OggS":
        raise _outside(path, "an Ogg container (Ogg-encapsulated FLAC, Vorbis or Opus)")
    if raw[:4] != b"fLaC":
        raise ValueError("%s: not a FLAC file (it starts with %r)" % (path, bytes(raw[:4])))
    pos, info, last = 4, None, False
    first = True
    while not last:
        if pos + 4 > len(raw):
            raise ValueError("%s: the metadata blocks run past the end of the file" % path)
        last, kind = bool(raw[pos] & 0x80), raw[pos] & 0x7F
        size = int.from_bytes(raw[pos + 1:pos + 4], "big")
        body = raw[pos + 4:pos + 4 + size]
        if first and (kind != 0 or len(body) < 34):
            raise ValueError("%s: no STREAMINFO block in front (block type %d of %d bytes)" % (path, kind, size))
        if first:
            min_b, max_b = struct.unpack_from(">HH", body)
            min_f, max_f = int.from_bytes(body[4:7], "big"), int.from_bytes(body[7:10], "big")
            v = int.from_bytes(body[10:18], "big")
            info = FlacInfo(((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v >> 44, v & ((1 << 36) - 1), min_b, max_b, min_f,
                            max_f, bytes(body[18:34]))
        first = False
        pos += 4 + size
    if info.channels > 2:
        raise _outside(path, "FLAC with %d channels (only mono and stereo are mixed down; ffmpeg's matrices for other "
                             "layouts are not guessed)" % info.channels)
    if info.bits_per_sample > 24:
        raise _outside(path, "FLAC at %d bits per sample (8..24 are decoded)" % info.bits_per_sample)
    if info.bits_per_sample < 8 or info.sample_rate < 1 or info.max_block < 1:
        raise ValueError("%s: STREAMINFO of %d bits per sample at %d Hz, blocks of up to %d" % (
            path, info.bits_per_sample, info.sample_rate, info.max_block))
    total = info.n_samples
    frames, sample = [], 0
    variable = None
    while pos < len(raw) and (total == 0 or sample < total):
        if variable is None:
            variable = len(raw) > pos + 1 and raw[pos + 1] == 0xF9
        bs = _header(raw, pos, info, variable, sample if variable else len(frames))
        if bs is None:
            if total == 0 and frames:
                break                                   # unknown total: what follows the last frame is not audio
            raise ValueError("%s: frame %d: no valid frame header at byte %d" % (path, len(frames), pos))
        sample += bs
        nxt_expect = sample if variable else len(frames) + 1
        at = pos + max(info.min_frame, 6)
        end = None
        sync = b"\xff\xf9" if variable else b"\xff\xf8"
        if total == 0 or sample < total:
            while True:
                at = raw.find(sync, at)
                if at < 0:
                    break
                if _header(raw, at, info, variable, nxt_expect) is not None:
                    end = at
                    break
                at += 1
        if end is None:
            # the last frame: its bytes run to the end of the file at most; the decoder finds where it closes
            if total and sample < total:
                raise ValueError("%s: frame %d: no header of the next frame behind byte %d: the file ends inside the "
                                 "audio (%d of %d samples)" % (path, len(frames), pos, sample, total))
            end = len(raw)
        frames.append([pos, end - pos, sample - bs, bs])
        pos = end
    if not frames:
        raise ValueError("%s: no audio frame behind the metadata" % path)
    if total and sample < total:
        raise ValueError("%s: frame %d: the file ends after %d of the %d samples STREAMINFO promises" % (
            path, len(frames), sample, total))
    if total and sample > total:                        # a last block reaching past the total: not what encoders write
        raise ValueError("%s: frame %d: the frames hold %d samples, STREAMINFO says %d" % (path, len(frames) - 1, sample, total))
    if total == 0:
        info = info._replace(n_samples=sample)
    if info.n_samples > 0x7FFFFFFF:
        raise ValueError("%s: %d samples (at most 2^31 - 1)" % (path, info.n_samples))
    return info, [FlacFrame(*f) for f in frames], raw


def _device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    if dev.type != "cuda":
        raise RuntimeError("FLAC frames are decoded on the MI355X only (gsv_flac_decode); got device %s -- there is no "
                           "CPU path" % dev)
    return dev


def tables(parsed):
    """the ctypes tables of one gsv_flac_decode / gsv_flac_decode_host call over parsed = [(info, frames, raw)]: the
    frames' bytes packed back to back -> (packed bytes, FlacClip array, FlacFrame array, [(clip, frame index)])"""
    packed = bytearray()
    clips = (N.FlacClip * len(parsed))()
    rows, out = [], 0
    for c, (info, frames, raw) in enumerate(parsed):
        clips[c] = N.FlacClip(info.channels, info.bits_per_sample, info.n_samples, 0, out)
        out += info.n_samples
        for k, fr in enumerate(frames):
            rows.append((c, k, N.FlacFrame(c, fr.block_size, len(packed), fr.length, fr.first_sample,
                                           N.FLAC_OPEN_END if k == len(frames) - 1 else 0, 0)))
            packed += raw[fr.offset:fr.offset + fr.length]
    ftab = (N.FlacFrame * len(rows))(*[r[2] for r in rows])
    return packed, clips, ftab, [(r[0], r[1]) for r in rows]


def status_error(path, frame, code):
    what = N.FLAC_STATUS[code] if 0 <= code < len(N.FLAC_STATUS) else "status %d" % code
    return ValueError("%s: frame %d: %s (status %d); the file is damaged or not what its headers say" % (path, frame, what, code))


def load_flac(path, device=None):
    """TTS._load_audio for a FLAC file -> (fp32 mono [n_samples] on `device`, sample rate)"""
    return load_flacs([path], device)[0]


def load_flacs(paths, device=None):
    """load_flac of every path -> [(fp32 mono [n_i] on `device`, sample rate)]: every file parsed and indexed first, then
    the frames' bytes of all files packed into one upload and decoded in one gsv_flac_decode per AUX_MAX_CLIPS clips;
    the status array is read once, and the first frame that failed raises ValueError naming its file, its index and what
    the status means (CRC-16 mismatch, overrun, reserved code, ...).  Each waveform is a view of one packed tensor and
    bit-identical to load_flac of its file.  The STREAMINFO MD5 is not verified (module docstring)."""
    paths = list(paths)
    parsed = [parse_flac(p) for p in paths]
    dev = _device(device)
    if not parsed:
        return []
    L = N.lib()
    st = N.current_stream_ptr(dev)
    chunks = [tables(parsed[c0:c0 + N.AUX_MAX_CLIPS]) for c0 in range(0, len(parsed), N.AUX_MAX_CLIPS)]
    packed = bytearray()
    for ch in chunks:
        packed += ch[0]
    data = torch.frombuffer(packed, dtype=torch.uint8).to(dev)
    out = torch.empty(sum(info.n_samples for info, _, _ in parsed), dtype=torch.float32, device=dev)
    status = torch.empty(sum(len(ch[3]) for ch in chunks), dtype=torch.int32, device=dev)
    need = max(L.gsv_flac_decode_workspace(ch[1], len(ch[1]), len(ch[2])) for ch in chunks)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    b0 = s0 = f0 = 0
    for pk, clips, ftab, rows in chunks:
        N.check(L.gsv_flac_decode(data[b0:].data_ptr(), len(pk), clips, len(clips), ftab, len(ftab), out[s0:].data_ptr(),
                                  status[f0:].data_ptr(), ws.data_ptr(), need, st))
        b0 += len(pk)
        s0 += sum(c.n_samples for c in clips)
        f0 += len(rows)
    codes = status.cpu()
    bad = torch.nonzero(codes).flatten()
    if len(bad):
        i = int(bad[0])
        code = int(codes[i])
        for c0, (_, _, _, rows) in zip(range(0, len(parsed), N.AUX_MAX_CLIPS), chunks):
            if i < len(rows):
                raise status_error(paths[c0 + rows[i][0]], rows[i][1], code)
            i -= len(rows)
    res, s = [], 0
    for info, _, _ in parsed:
        res.append((out[s:s + info.n_samples], info.sample_rate))
        s += info.n_samples
    return res
