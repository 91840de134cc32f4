"""FLAC files as reference audio: what TTS._load_audio (gsv_tts/TTS.py:1811-1823) gets from PyAV for a FLAC file -- mono
fp32 at the file's own rate -- with the container parsed and the frames INDEXED on the host (no sample is decoded here)
and every frame decoded on the device (gsv_flac_decode, csrc/flacdec.h: one lane per frame), then converted by the WAV
path's own kernel.  A FLAC clip is bit-identical to the WAV file that holds the same integers.

    wav, sr = load_flac("spk.flac", "cuda:0")            # fp32 [n_samples] on the device, the file's rate
    clips = load_flacs(["a.flac", "b.flac"], "cuda:0")    # [(wav, sr)]: one packed upload, one decode per 64 clips

Read: native FLAC, one or two channels, 8..24 bits per sample, fixed or variable block size.  More than two channels,
32 bits per sample, Ogg-encapsulated FLAC and a file with an ID3v2 tag in front raise NotImplementedError.  The
STREAMINFO MD5 is parsed and exposed (FlacInfo.md5) but NOT verified: that would need the integers back on the host.
What is verified: each header's CRC-8 (here, while indexing) and each frame's CRC-16 (on the device).  No CPU path.

Writing goes the other way: the container and every frame header are built here, the frames are encoded on
the device (gsv_flac_encode, csrc/flacenc.h: one wave per frame) -- or by the same arithmetic on the CPU
(gsv_flac_encode_host) when the device is a CPU or there is no GPU:

    data = encode_flac(wave, 32000)                        # bytes of a .flac file: mono, 16 bits, blocks of 4096
    files = encode_flacs([w0, w1], [32000, 44100], bits=[16, 24])   # one packed upload, one encode per 64 clips
    save_flac("out.flac", wave, 32000)

Written: native FLAC, fixed blocking, one channel, 16 or 24 bits, CONSTANT / FIXED / VERBATIM subframes chosen per frame
by exact bit count.  load_flac(encode_flac(w)) is w bit for bit when w came from a file of that width.  The STREAMINFO
MD5 is written as sixteen zero bytes ("not computed"): it would need the integers on the host."""
import struct
from collections import namedtuple

import numpy as np
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


# ------------------------------------------------------------------------------------------------------------- writing
_BLOCK_CODE = {v: k for k, v in list(_BLOCK.items()) + [(c, 256 << (c - 8)) for c in range(8, 16)]}
_RATE_CODE = {v: k for k, v in _RATE.items()}
_BITS_CODE = {v: k for k, v in _BITS.items()}
ENC_MIN_BLOCK, ENC_MAX_BLOCK = 16, N.FLAC_ENC_MAX_BLOCK
ENC_MAX_RATE = 655350


def _coded_number(v) -> bytes:
    """the UTF-8-style coding of a frame number of up to 31 bits, 1-6 bytes"""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    return bytes([(0xFF << (8 - n)) & 0xFF | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)])


def build_header(block_size, rate, bits, number) -> bytes:
    """the header of frame `number` of a mono fixed-blocking stream, CRC-8 included: the inverse of _header.  Block size
    and rate take their table codes when they have one; otherwise the block size is explicit (8 or 16 bits) and the
    rate code is 0 (from STREAMINFO)."""
    if not 1 <= block_size <= 65536 or bits not in _BITS_CODE or not 0 <= number < 1 << 31:
        raise ValueError("frame header of block size %d at %d bits, frame %d" % (block_size, bits, number))
    bs_code = _BLOCK_CODE.get(block_size, 6 if block_size <= 256 else 7)
    h = bytes([0xFF, 0xF8, bs_code << 4 | _RATE_CODE.get(rate, 0), _BITS_CODE[bits] << 1]) + _coded_number(number)
    if bs_code == 6:
        h += bytes([block_size - 1])
    elif bs_code == 7:
        h += struct.pack(">H", block_size - 1)
    return h + bytes([_crc8(h)])


def streaminfo(block_size, min_frame, max_frame, rate, bits, n_samples) -> bytes:
    """the 34 bytes of a mono stream's STREAMINFO; the MD5 is sixteen zero bytes (not computed)"""
    v = (rate << 44) | ((bits - 1) << 36) | n_samples
    return (struct.pack(">HH", block_size, block_size) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") +
            v.to_bytes(8, "big") + bytes(16))


_ENC_FRAME = np.dtype([("clip", "<i4"), ("block_size", "<i4"), ("first_sample", "<i4"), ("header_len", "<i4"), ("header", "u1", 16)])


def enc_tables(lengths, rates, bits, block_sizes):
    """the ctypes tables of one gsv_flac_encode / gsv_flac_encode_host call over clips packed back to back: every
    clip's frames in order, each of its block size but the last -> (FlacEncClip array, FlacEncFrame array, [frames per
    clip]).  The second array is a view of a numpy buffer that its `_buf` attribute keeps alive."""
    clips = (N.FlacEncClip * len(lengths))()
    rows, per_clip, at = [], [], 0
    for c, (n, rate, b, bs) in enumerate(zip(lengths, rates, bits, block_sizes)):
        clips[c] = N.FlacEncClip(at, n, b)
        at += n
        nf = (n + bs - 1) // bs
        per_clip.append(nf)
        for k in range(nf):
            rows.append((c, min(bs, n - k * bs), k * bs, build_header(min(bs, n - k * bs), rate, b, k)))
    tab = np.zeros(len(rows), dtype=_ENC_FRAME)
    tab["clip"] = [r[0] for r in rows]
    tab["block_size"] = [r[1] for r in rows]
    tab["first_sample"] = [r[2] for r in rows]
    tab["header_len"] = [len(r[3]) for r in rows]
    tab["header"] = np.frombuffer(b"".join(r[3].ljust(16, b"\0") for r in rows), dtype=np.uint8).reshape(-1, 16)
    ftab = (N.FlacEncFrame * len(rows)).from_buffer(tab)
    ftab._buf = tab
    return clips, ftab, per_clip


def _per_clip(value, n, what):
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError("%d %s for %d clips" % (len(value), what, n))
        return [int(v) for v in value]
    return [int(value)] * n


def _files(per_clip, lengths, rates, bits, block_sizes, offsets, data):
    """frames packed back to back + their offsets -> one file's bytes per clip"""
    out, f = [], 0
    for nf, n, rate, b, bs in zip(per_clip, lengths, rates, bits, block_sizes):
        sizes = [offsets[f + k + 1] - offsets[f + k] for k in range(nf)]
        info = streaminfo(bs, min(sizes), max(sizes), rate, b, n)
        out.append(b"fLaC" + bytes([0x80]) + len(info).to_bytes(3, "big") + info + bytes(data[offsets[f]:offsets[f + nf]]))
        f += nf
    return out


def encode_flacs(waves, sample_rates, bits=16, block_size=4096, device=None):
    """every clip of `waves` (1-D torch tensors or numpy arrays, fp32 in [-1, 1]) as the bytes of a FLAC file -> [bytes].
    sample_rates, bits (16 | 24) and block_size (16..4608) are one value for all clips or one per clip.  The frames are
    encoded on `device` (default: where the tensors are, else cuda:0 when there is a GPU, else the CPU): device tensors
    that are views of one packed fp32 tensor are read in place, anything else is packed once (host arrays: one upload);
    one gsv_flac_encode per AUX_MAX_CLIPS clips, its frame offsets and bytes read back once each.  On a CPU device
    gsv_flac_encode_host does the same arithmetic, byte for byte.  ValueError, before any device work and naming the
    clip's index, for an input that is not 1-D, an empty clip, bits other than 16 / 24, a block size or rate out of
    range.  Each file is byte-identical to encode_flac of its clip."""
    waves = list(waves)
    n = len(waves)
    rates, bits, bss = _per_clip(sample_rates, n, "sample rates"), _per_clip(bits, n, "bit widths"), _per_clip(block_size, n, "block sizes")
    for c, (w, rate, b, bs) in enumerate(zip(waves, rates, bits, bss)):
        if not isinstance(w, (torch.Tensor, np.ndarray)):
            raise ValueError("clip %d: a %s (a 1-D torch tensor or numpy array is expected)" % (c, type(w).__name__))
        if w.ndim != 1:
            raise ValueError("clip %d: %d dimensions, shape %s (mono: one dimension)" % (c, w.ndim, tuple(w.shape)))
        if w.shape[0] < 1 or w.shape[0] > 0x7FFFFFFF:
            raise ValueError("clip %d: %d samples (1..2^31 - 1)" % (c, w.shape[0]))
        if b not in (16, 24):
            raise ValueError("clip %d: %d bits per sample (16 or 24 are written)" % (c, b))
        if not ENC_MIN_BLOCK <= bs <= ENC_MAX_BLOCK:
            raise ValueError("clip %d: block size %d (%d..%d)" % (c, bs, ENC_MIN_BLOCK, ENC_MAX_BLOCK))
        if not 1 <= rate <= ENC_MAX_RATE:
            raise ValueError("clip %d: sample rate %d Hz (1..%d)" % (c, rate, ENC_MAX_RATE))
    if not waves:
        return []
    if device is not None:
        dev = torch.device(device)
    else:
        on = [w.device for w in waves if isinstance(w, torch.Tensor) and w.device.type == "cuda"]
        dev = on[0] if on else torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    lengths = [int(w.shape[0]) for w in waves]
    L = N.lib()
    out = []
    if dev.type != "cuda":
        for c0 in range(0, n, N.AUX_MAX_CLIPS):
            sl = slice(c0, c0 + N.AUX_MAX_CLIPS)
            x = np.ascontiguousarray(np.concatenate([_host_f32(w) for w in waves[sl]]))
            clips, ftab, per_clip = enc_tables(lengths[sl], rates[sl], bits[sl], bss[sl])
            bound = L.gsv_flac_encode_bound(clips, len(clips), ftab, len(ftab))
            data, offsets = np.empty(bound, dtype=np.uint8), np.empty(len(ftab) + 1, dtype=np.int64)
            N.check(L.gsv_flac_encode_host(x.ctypes.data, len(x), clips, len(clips), ftab, len(ftab), data.ctypes.data, bound,
                                           offsets.ctypes.data, None))
            out += _files(per_clip, lengths[sl], rates[sl], bits[sl], bss[sl], offsets.tolist(), data)
        return out
    st = N.current_stream_ptr(dev)
    for c0 in range(0, n, N.AUX_MAX_CLIPS):
        sl = slice(c0, c0 + N.AUX_MAX_CLIPS)
        clips, ftab, per_clip = enc_tables(lengths[sl], rates[sl], bits[sl], bss[sl])
        x, base, total = _pack(waves[sl], dev)
        if base is not None:                    # views of one tensor: where each clip starts in it
            for c, w in enumerate(waves[sl]):
                clips[c].in_offset = (w.data_ptr() - base) // 4
        bound = L.gsv_flac_encode_bound(clips, len(clips), ftab, len(ftab))
        need = L.gsv_flac_encode_workspace(clips, len(clips), ftab, len(ftab))
        data = torch.empty(bound, dtype=torch.uint8, device=dev)
        offsets = torch.empty(len(ftab) + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        N.check(L.gsv_flac_encode(x.data_ptr() if base is None else base, total, clips, len(clips), ftab, len(ftab),
                                  data.data_ptr(), bound, offsets.data_ptr(), None, ws.data_ptr(), need, st))
        off = offsets.cpu().tolist()
        out += _files(per_clip, lengths[sl], rates[sl], bits[sl], bss[sl], off, data[:off[-1]].cpu().numpy())
    return out


def _host_f32(w):
    if isinstance(w, torch.Tensor):
        w = w.detach().to("cpu", torch.float32).numpy()
    return np.ascontiguousarray(w, dtype=np.float32)


def _pack(waves, dev):
    """the clips as one fp32 device buffer -> (tensor or None, base address or None, samples in it).  Tensors that are
    already contiguous fp32 views of one storage on `dev` are read in place (base: the lowest address among them);
    host arrays are concatenated on the host and go up in one copy; anything else is packed with one torch.cat."""
    if all(isinstance(w, torch.Tensor) and w.device == dev and w.dtype == torch.float32 and w.is_contiguous() for w in waves):
        if len({w.untyped_storage().data_ptr() for w in waves}) == 1:
            base = min(w.data_ptr() for w in waves)
            end = max(w.data_ptr() + 4 * w.shape[0] for w in waves)
            return None, base, (end - base) // 4
    if all(isinstance(w, np.ndarray) or w.device.type == "cpu" for w in waves):
        x = torch.from_numpy(np.concatenate([_host_f32(w) for w in waves])).to(dev)
    else:
        x = torch.cat([(w.detach() if isinstance(w, torch.Tensor) else torch.from_numpy(_host_f32(w))).to(dev, torch.float32)
                       for w in waves])
    return x, None, x.shape[0]


def encode_flac(wave, sample_rate, bits=16, block_size=4096, device=None) -> bytes:
    """one clip as the bytes of a FLAC file (encode_flacs)"""
    return encode_flacs([wave], [sample_rate], bits, block_size, device)[0]


def save_flacs(paths, waves, sample_rates, bits=16, block_size=4096, device=None):
    """encode_flacs, each clip written to its path"""
    paths, waves = list(paths), list(waves)
    if len(waves) != len(paths):
        raise ValueError("%d paths for %d clips" % (len(paths), len(waves)))
    files = encode_flacs(waves, sample_rates, bits, block_size, device)
    for p, data in zip(paths, files):
        with open(p, "wb") as f:
            f.write(data)


def save_flac(path, wave, sample_rate, bits=16, block_size=4096, device=None):
    """one clip written as a FLAC file (encode_flacs)"""
    save_flacs([path], [wave], [sample_rate], bits, block_size, device)
