"""What both FLAC-writer test files share: the signal x length x block size x bits grid, the quantiser written in numpy,
the brute-force argmin of the subframe choice, and the calls of the two ABI entry points with the choices
read back."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flac_writer as fw  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio  # noqa: E402

LENGTHS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 37)
BLOCKS = (16, 192, 1000, 4096, 4608)
BITS = (16, 24)
SIGNALS = ("tone", "noise", "zeros", "const", "outlier", "ramp", "special")
KINDS = ("constant", "verbatim", "fixed")


def signal(name, n, seed=0):
    """fp32 [n]"""
    rng = np.random.default_rng([seed, n, SIGNALS.index(name)])
    t = np.arange(n)
    if name == "tone":                  # a tone plus small noise
        x = 0.4 * np.sin(2 * np.pi * t * 0.0071 + seed) + 0.2 * np.sin(2 * np.pi * t * 0.0313) + rng.uniform(-2e-4, 2e-4, n)
    elif name == "noise":               # clamps at both ends
        x = rng.uniform(-1.2, 1.2, n)
        x[:2] = [1.2, -1.2][:n]
    elif name == "zeros":
        x = np.zeros(n)
    elif name == "const":
        x = np.full(n, 0.25 + 3 / 32768)
    elif name == "outlier":             # a long unary run
        x = np.zeros(n)
        x[n // 2] = 1.0
    elif name == "ramp":                # (k + 1/2) / 2^15: exact half-way points of the 16-bit quantiser
        x = (t - n // 2 + 0.5) / 2.0 ** 15
    else:                               # a NaN and both infinities among ordinary samples
        x = 0.3 * np.sin(2 * np.pi * t * 0.011) + rng.uniform(-1e-3, 1e-3, n)
        for i, v in zip((n // 3, n // 2, n - 1), (np.nan, np.inf, -np.inf)):
            x[i] = v
    return x.astype(np.float32)


def quantise(x, bits):
    """the contract's quantiser -> int64 [n]"""
    x = np.asarray(x, dtype=np.float32)
    full = np.float32(2.0 ** (bits - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.rint(np.where(np.isnan(x), np.float32(0), x) * full)
    return np.clip(s, -full, full - 1).astype(np.int64)


def grid_clips(block, bits):
    """the grid's clips for one block size and width -> [(name, x)]"""
    return [("%s_%d" % (s, n), signal(s, n, seed=block + bits)) for s in SIGNALS for n in LENGTHS]


class Encoded:
    """one ABI call's results on the host: data (uint8), offsets (int64 [F + 1]), choices, frames per clip"""

    def frame(self, f):
        return bytes(self.data[self.offsets[f]:self.offsets[f + 1]])

    def choice(self, f):
        c = self.choices[f]
        return (KINDS[c.kind], c.order, c.porder, c.method, list(c.k[:1 << c.porder]) if c.kind == N.FLAC_ENC_FIXED else [])


def timed_entry():
    """gsv_flac_encode_timed, the measuring twin of gsv_flac_encode that tools/flac_encode_time.py uses: exported by the
    library, not declared in the ABI header, so it is bound here by name"""
    fn = N.lib().gsv_flac_encode_timed
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    fn.argtypes = [vp, sz, ctypes.POINTER(N.FlacEncClip), i, ctypes.POINTER(N.FlacEncFrame), i, vp, sz, vp, vp, vp, sz, vp, i,
                   ctypes.POINTER(ctypes.c_float)]
    fn.restype = i
    return fn


def encode_abi(xs, rates, bits, blocks, dev=None, timed=None):
    """gsv_flac_encode_host (dev None) or gsv_flac_encode (a torch cuda device) over up to 64 clips -> Encoded.  timed: 0 or
    1 goes through gsv_flac_encode_timed instead, with that value as its serial_crc flag; e.ms holds its three times."""
    lengths = [len(x) for x in xs]
    clips, ftab, per_clip = flacio.enc_tables(lengths, rates, bits, blocks)
    L = N.lib()
    bound = L.gsv_flac_encode_bound(clips, len(clips), ftab, len(ftab))
    packed = np.ascontiguousarray(np.concatenate(xs), dtype=np.float32)
    e = Encoded()
    e.per_clip, e.ftab, e.clips, e.bound = per_clip, ftab, clips, bound
    if dev is None:
        data = np.full(bound, 0xA5, dtype=np.uint8)
        offsets = np.full(len(ftab) + 1, -1, dtype=np.int64)
        choices = (N.FlacEncChoice * len(ftab))()
        e.rc = L.gsv_flac_encode_host(packed.ctypes.data, len(packed), clips, len(clips), ftab, len(ftab), data.ctypes.data, bound,
                                      offsets.ctypes.data, ctypes.addressof(choices))
    else:
        import torch
        x = torch.from_numpy(packed).to(dev)
        data_d = torch.full((bound,), 0xA5, dtype=torch.uint8, device=dev)
        off_d = torch.full((len(ftab) + 1,), -1, dtype=torch.int64, device=dev)
        ch_d = torch.full((len(ftab) * ctypes.sizeof(N.FlacEncChoice),), 0xA5, dtype=torch.uint8, device=dev)
        need = L.gsv_flac_encode_workspace(clips, len(clips), ftab, len(ftab))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if timed is None:
            e.rc = L.gsv_flac_encode(x.data_ptr(), len(packed), clips, len(clips), ftab, len(ftab), data_d.data_ptr(), bound,
                                     off_d.data_ptr(), ch_d.data_ptr(), ws.data_ptr(), need, N.current_stream_ptr(dev))
        else:
            ms = (ctypes.c_float * 3)(-1, -1, -1)
            e.rc = timed_entry()(x.data_ptr(), len(packed), clips, len(clips), ftab, len(ftab), data_d.data_ptr(), bound,
                                 off_d.data_ptr(), ch_d.data_ptr(), ws.data_ptr(), need, N.current_stream_ptr(dev), timed, ms)
            e.ms = list(ms)
        torch.cuda.synchronize(dev)
        data, offsets = data_d.cpu().numpy(), off_d.cpu().numpy()
        choices = (N.FlacEncChoice * len(ftab)).from_buffer_copy(ch_d.cpu().numpy().tobytes())
    e.data, e.offsets, e.choices = data, offsets, choices
    return e


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


def sub_of(choice):
    kind, order, porder, method, ks = choice
    if kind != "fixed":
        return fw.Sub(kind)
    return fw.Sub("fixed", order=order, method=method, porder=porder, params=[int(k) for k in ks])


def brute_force(q, bits):
    """the argmin of the contract over one frame's integers -> (choice as Encoded.choice gives it, subframe bits)"""
    q = np.asarray(q, dtype=np.int64)
    n = len(q)
    if np.all(q == q[0]):
        return ("constant", 0, 0, 0, []), 8 + bits
    method, kmax, pbits = (0, 15, 4) if bits == 16 else (1, 31, 5)
    best = None
    for o in range(min(4, n - 1) + 1):
        r = q.copy()
        for _ in range(o):
            r = np.concatenate([r[:1] * 0, np.diff(r)])
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        u[:o] = 0                                       # warm-up samples are not residuals
        for p in range(7):
            if n % (1 << p) or (p > 0 and (n >> p) <= o):
                continue
            total, ks = 8 + o * bits + 2 + 4, []
            for j, part in enumerate(u.reshape(1 << p, -1)):
                ln = len(part) - (o if j == 0 else 0)
                costs = [int((part >> k).sum()) + ln * (1 + k) for k in range(kmax)]
                k = int(np.argmin(costs))               # the first minimum: the lowest k
                ks.append(k)
                total += pbits + costs[k]
            if best is None or total < best[1]:         # o, then p, ascending: ties stay with the earlier
                best = (("fixed", o, p, method, ks), total)
    if 8 + n * bits < best[1]:
        return ("verbatim", 0, 0, 0, []), 8 + n * bits
    return best
