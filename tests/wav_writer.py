"""Test-side WAV files, written with numpy and struct: every container variant gsv_tts_lite_amd.wavio must read, built
from integers (or floats) the test chose, and the fp32 mono samples those must convert to, computed in numpy from the
same numbers: x / 2^k per sample (u8: (x - 128) / 2^7), stereo mixed as L * g + R * g with g = sqrt(1/2), both products
rounded before the sum (fp32; fp64 for f64, then cast)."""
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
TAG_BITS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64)}
GUID_TAIL = bytes.fromhex("00001000800000aa00389b71")
GAIN = np.sqrt(0.5)             # the documented stereo -> mono coefficient


def samples(fmt, n, ch, seed=0):
    """[n, ch] values of format fmt, the extremes of the integer range first"""
    rng = np.random.default_rng(seed)
    if fmt in ("f32", "f64"):
        x = rng.standard_normal((n, ch)) * 0.6
        x.flat[:4] = [1.5, -1.25, 0.0, 1.0][:x.size]
        return x.astype(np.float32 if fmt == "f32" else np.float64)
    lo, hi = {"u8": (0, 255), "s16": (-2 ** 15, 2 ** 15 - 1), "s24": (-2 ** 23, 2 ** 23 - 1),
              "s32": (-2 ** 31, 2 ** 31 - 1)}[fmt]
    x = rng.integers(lo, hi, size=(n, ch), endpoint=True, dtype=np.int64)
    x.flat[:4] = [lo, hi, lo + 1, (lo + hi + 1) // 2][:x.size]
    return x


def encode(x, fmt) -> bytes:
    """[n, ch] -> the interleaved little-endian bytes of a data chunk"""
    if fmt == "s24":
        return x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return x.astype({"u8": "<u1", "s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[fmt]).tobytes()


def expected(x, fmt):
    """[n, ch] -> fp32 mono [n], what the device conversion must give bit for bit"""
    if fmt == "f64":
        d = x.astype(np.float64)
        return (d[:, 0] if x.shape[1] == 1 else d[:, 0] * GAIN + d[:, 1] * GAIN).astype(np.float32)
    if fmt == "f32":
        f = x.astype(np.float32)
    elif fmt == "u8":
        f = ((x - 128) / 2.0 ** 7).astype(np.float32)
    else:
        f = (x / 2.0 ** {"s16": 15, "s24": 23, "s32": 31}[fmt]).astype(np.float32)
    if x.shape[1] == 1:
        return f[:, 0]
    g = np.float32(GAIN)
    return f[:, 0] * g + f[:, 1] * g


def chunk(cid: bytes, body: bytes, size=None) -> bytes:
    """one RIFF chunk, with its pad byte when the body has an odd length"""
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(fmt, ch, rate, extensible=False, tag=None, bits=None) -> bytes:
    t, b = TAG_BITS.get(fmt, (None, None))
    t, b = (t if tag is None else tag), (b if bits is None else bits)
    block = (b + 7) // 8 * ch
    if not extensible:
        return chunk(b"fmt ", struct.pack("<HHIIHH", t, ch, rate, rate * block, block, b))
    body = struct.pack("<HHIIHH", 0xFFFE, ch, rate, rate * block, block, b)
    body += struct.pack("<HHI", 22, b, 0x4 if ch == 1 else 0x3) + struct.pack("<I", t) + GUID_TAIL
    return chunk(b"fmt ", body)


def wav_bytes(data: bytes, fmt, ch, rate, extensible=False, before_fmt=(), before_data=(), data_size=None, after=b"",
              tag=None, bits=None) -> bytes:
    body = (b"WAVE" + b"".join(before_fmt) + fmt_chunk(fmt, ch, rate, extensible, tag, bits) + b"".join(before_data) +
            chunk(b"data", data, data_size) + after)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write(path, x, fmt, rate, **kw):
    """a WAV file of the samples x [n, ch] in format fmt at rate; -> str(path)"""
    with open(path, "wb") as f:
        f.write(wav_bytes(encode(x, fmt), fmt, x.shape[1], rate, **kw))
    return str(path)
