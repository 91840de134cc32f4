"""Test-side FLAC files, written with numpy: every choice a conforming encoder may make is forced by an argument, so a
test can put each branch of the decoder (csrc/flacdec.h) in front of it with integers it chose.

    write(path, x, bps, rate, block_size=4096, sub=Sub("fixed", order=2), assignment="ms")

x is [n, channels] int64.  Nothing here searches for a good encoding: the subframe kind, predictor order, LPC
precision / shift / coefficients, wasted bits, residual method, partition order and each partition's Rice parameter or
escape width are what the caller says, and the residual is computed for them, so the file is valid whatever they are
(the writer asserts what the format demands: a CONSTANT block is constant, wasted bits are zero, a residual fits its
escape width and 32 bits).  CRC-8, CRC-16 and the STREAMINFO MD5 are computed here.  Written from the format's
definition; no other FLAC implementation was at hand.

`python tests/flac_writer.py DIR` writes the corpus of tools/flac_host_check: each grid file as DIR/<name>.flac and its
frame table as DIR/<name>.tab, and its integers (interleaved little-endian int32) as DIR/<name>.pcm."""
import hashlib
import struct
import sys

import numpy as np

BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
               16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
              96000: 11}
BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
ASSIGN = {"indep": None, "ls": 8, "rs": 9, "ms": 10}


def crc8(data: bytes) -> int:
    """polynomial 0x07, init 0"""
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else c << 1
    return c


def _crc16_table():
    t = []
    for x in range(256):
        c = x << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        t.append(c)
    return t


_T16 = _crc16_table()


def crc16(data: bytes) -> int:
    """polynomial 0x8005, init 0, unreflected"""
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def utf8_number(v: int) -> bytes:
    """the UTF-8-style coding of a frame number (31 bits) or sample number (36 bits), 1-7 bytes"""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):            # n bytes carry 7 - n + 6 (n - 1) = 5 n + 1 bits
        n += 1
    out = [(0xFF << (8 - n)) & 0xFF | (v >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


class Bits:
    """MSB-first (value, width) fields; widths above 64 are zeros in front of the low 64 bits (long unary runs)"""

    def __init__(self):
        self.v, self.w = [], []

    def put(self, value, width):
        self.v.append(np.array([int(value) & ((1 << min(width, 64)) - 1)], dtype=np.uint64))
        self.w.append(np.array([width], dtype=np.int64))

    def put_signed(self, value, width):
        self.put(int(value) & ((1 << width) - 1), width)

    def extend(self, values, widths):
        self.v.append(np.asarray(values, dtype=np.uint64))
        self.w.append(np.asarray(widths, dtype=np.int64))

    def extend_signed(self, values, width):
        v = np.asarray(values, dtype=np.int64) & np.int64((1 << width) - 1)
        self.extend(v.astype(np.uint64), np.full(len(v), width, dtype=np.int64))

    def bytes(self) -> bytes:
        """zero-padded to a whole byte"""
        v, w = np.concatenate(self.v), np.concatenate(self.w)
        keep = w > 0
        v, w = v[keep], w[keep]
        ends = np.cumsum(w)
        total = int(ends[-1]) if len(ends) else 0
        bits = np.zeros((total + 7) // 8 * 8, dtype=np.uint8)
        for j in range(int(min(w.max(), 64)) if len(w) else 0):
            m = w > j
            bits[ends[m] - 1 - j] = ((v[m] >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits).tobytes()


class Sub:
    """one subframe's forced choices.  kind: constant | verbatim | fixed | lpc.  coefs: `order` integers of `precision`
    bits (default: a deterministic decaying set scaled by 2^shift, or small integers at shift 0).  params: one entry per
    partition (or one for all): a Rice parameter, or ("esc", width)."""

    def __init__(self, kind="fixed", order=0, precision=15, shift=0, coefs=None, wasted=0, method=0, porder=0, params=4):
        self.kind, self.order, self.precision, self.shift, self.wasted = kind, order, precision, shift, wasted
        self.method, self.porder, self.params = method, porder, params
        if kind == "lpc" and coefs is None:
            coefs = default_coefs(order, precision, shift)
        self.coefs = coefs


def default_coefs(order, precision, shift):
    """deterministic and tame: about 0.9 of the last sample minus a decaying tail (sum |a| < 2), in units of 2^-shift;
    at shift 0 they are -1, 0 or 1"""
    a = np.array([0.9 if j == 0 else (-0.5 if j % 2 else 0.4) / (j + 1) ** 1.5 for j in range(order)])
    c = np.round(a * 2.0 ** shift).astype(np.int64)
    lim = 2 ** (precision - 1)
    return np.clip(c, -lim, lim - 1)


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _residual(s, coefs, shift):
    """s [n] int64 -> residual of samples order..n-1"""
    order = len(coefs)
    n = len(s)
    pred = np.zeros(n - order, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += np.int64(c) * s[order - 1 - j:n - 1 - j]
    return s[order:] - (pred >> np.int64(shift))


def _put_residual(b, r, sub, order, bs):
    b.put(sub.method, 2)
    b.put(sub.porder, 4)
    nparts = 1 << sub.porder
    assert bs % nparts == 0 and bs >> sub.porder >= order, (bs, sub.porder, order)
    assert np.all(np.abs(r) < 2 ** 31), "residual outside 32 bits"
    params = sub.params if isinstance(sub.params, list) else [sub.params] * nparts
    assert len(params) == nparts
    pbits, esc_code = (5, 31) if sub.method else (4, 15)
    at = 0
    for p, prm in enumerate(params):
        n = (bs >> sub.porder) - (order if p == 0 else 0)
        part = r[at:at + n]
        at += n
        if isinstance(prm, tuple):
            width = prm[1]
            b.put(esc_code, pbits)
            b.put(width, 5)
            if width == 0:
                assert not np.any(part)
            else:
                assert np.all(part >= -(1 << (width - 1))) and np.all(part < 1 << (width - 1)), (width, part.min(), part.max())
                b.extend_signed(part, width)
        else:
            assert 0 <= prm < esc_code
            b.put(prm, pbits)
            u = np.where(part >= 0, part << 1, ((-part) << 1) - 1).astype(np.uint64)
            q = (u >> np.uint64(prm)).astype(np.int64)
            low = u & np.uint64((1 << prm) - 1)
            b.extend((np.uint64(1) << np.uint64(prm)) | low, q + 1 + prm)      # q zeros, the 1, prm bits
    assert at == len(r)


def _put_subframe(b, s, bps, sub):
    """s [bs] int64 at bps bits"""
    bs = len(s)
    kind = sub.kind
    code = {"constant": 0, "verbatim": 1}.get(kind)
    if kind == "fixed":
        code = 8 + sub.order
    elif kind == "lpc":
        code = 32 + sub.order - 1
    b.put(0, 1)
    b.put(code, 6)
    if sub.wasted:
        assert not np.any(s & ((1 << sub.wasted) - 1)), "wasted bits are not zero"
        b.put(1, 1)
        b.put(1, sub.wasted)                     # wasted - 1 zeros, then the 1
        s = s >> sub.wasted
        bps -= sub.wasted
    else:
        b.put(0, 1)
    assert np.all(s >= -(1 << (bps - 1))) and np.all(s < 1 << (bps - 1))
    if kind == "constant":
        assert np.all(s == s[0])
        b.put_signed(s[0], bps)
    elif kind == "verbatim":
        b.extend_signed(s, bps)
    else:
        order = sub.order
        assert order <= bs
        b.extend_signed(s[:order], bps)
        if kind == "lpc":
            assert len(sub.coefs) == order and 1 <= sub.precision <= 15 and 0 <= sub.shift <= 15
            b.put(sub.precision - 1, 4)
            b.put_signed(sub.shift, 5)
            b.extend_signed(sub.coefs, sub.precision)
            coefs, shift = sub.coefs, sub.shift
        else:
            coefs, shift = FIXED[order], 0
        _put_residual(b, _residual(s, coefs, shift), sub, order, bs)


def frame_bytes(x, bps, rate, number, variable=False, assignment="indep", sub=None, bps_code=None, rate_code=None,
                block_code=None):
    """one frame of x [bs, ch]; number: the frame number (fixed) or the first sample (variable).  sub: a Sub, or one
    per channel.  bps_code / rate_code / block_code force a header code (default: the table's, else 0 / 0 / explicit)."""
    bs, ch = x.shape
    subs = list(sub) if isinstance(sub, (list, tuple)) else [sub or Sub("verbatim")] * ch
    b = Bits()
    b.put(0xFFF8 | (1 if variable else 0), 16)
    if block_code is None:
        block_code = BLOCK_CODES.get(bs, 6 if bs <= 256 else 7)
    if rate_code is None:
        rate_code = RATE_CODES.get(rate, 0)
    b.put(block_code, 4)
    b.put(rate_code, 4)
    code = ASSIGN[assignment]
    b.put(ch - 1 if code is None else code, 4)
    b.put(BPS_CODES.get(bps, 0) if bps_code is None else bps_code, 3)
    b.put(0, 1)
    for byte in utf8_number(number):
        b.put(byte, 8)
    if block_code == 6:
        b.put(bs - 1, 8)
    elif block_code == 7:
        b.put(bs - 1, 16)
    if rate_code == 12:
        b.put(rate // 1000, 8)
    elif rate_code == 13:
        b.put(rate, 16)
    elif rate_code == 14:
        b.put(rate // 10, 16)
    head = b.bytes()
    b.put(crc8(head), 8)
    x = x.astype(np.int64)
    if code is None:
        chans = [(x[:, c], bps) for c in range(ch)]
    else:
        assert ch == 2
        left, right = x[:, 0], x[:, 1]
        side = left - right
        if assignment == "ls":
            chans = [(left, bps), (side, bps + 1)]
        elif assignment == "rs":
            chans = [(side, bps + 1), (right, bps)]
        else:
            chans = [((left + right) >> 1, bps), (side, bps + 1)]
    for (s, w), sb in zip(chans, subs):
        _put_subframe(b, s, w, sb)
    body = b.bytes()
    return body + struct.pack(">H", crc16(body))


def md5_of(x, bps) -> bytes:
    """MD5 of the interleaved samples, little-endian, each in ceil(bps / 8) bytes"""
    nb = (bps + 7) // 8
    raw = x.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nb]
    return hashlib.md5(raw.tobytes()).digest()


def metadata_block(kind, body, last=False) -> bytes:
    return bytes([(0x80 if last else 0) | kind]) + struct.pack(">I", len(body))[1:] + body


def streaminfo(min_bs, max_bs, min_fs, max_fs, rate, ch, bps, total, md5) -> bytes:
    v = (rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | total
    return (struct.pack(">HH", min_bs, max_bs) + struct.pack(">I", min_fs)[1:] + struct.pack(">I", max_fs)[1:] +
            v.to_bytes(8, "big") + md5)


def flac_bytes(x, bps, rate, block_size=4096, variable=False, block_sizes=None, assignment="indep", sub=None,
               metadata=(), total_samples=None, after=b"", frame_sizes_known=True, first_number=0, **frame_kw):
    """the whole file.  block_sizes: the sizes of successive frames (variable blocking; the last is repeated), default
    block_size throughout with a short last frame.  sub / assignment may be callables of the frame index.  metadata:
    (type, body) blocks after STREAMINFO.  total_samples: STREAMINFO's field (default the true count; 0: unknown).
    -> (bytes, [(offset, length, first_sample, block_size)] of the frames)"""
    n, ch = x.shape
    frames, pos, k = [], 0, 0
    while pos < n:
        want = block_sizes[min(k, len(block_sizes) - 1)] if block_sizes else block_size
        bs = min(want, n - pos)
        a = assignment(k) if callable(assignment) else assignment
        s = sub(k) if callable(sub) else sub
        frames.append((frame_bytes(x[pos:pos + bs], bps, rate, (pos if variable else k) + first_number, variable, a, s,
                                   **frame_kw), pos, bs))
        pos += bs
        k += 1
    sizes = [len(f) for f, _, _ in frames]
    bss = [bs for _, _, bs in frames]
    max_bs = max(bss)
    min_bs = max_bs if not variable and not block_sizes else min(bss)      # fixed blocking: the last frame may be short
    info = streaminfo(min_bs, max_bs, min(sizes) if frame_sizes_known else 0, max(sizes) if frame_sizes_known else 0, rate,
                      ch, bps, n if total_samples is None else total_samples, md5_of(x, bps))
    blocks = [(0, info)] + list(metadata)
    head = b"fLaC" + b"".join(metadata_block(t, body, i == len(blocks) - 1) for i, (t, body) in enumerate(blocks))
    table, at = [], len(head)
    for f, pos, bs in frames:
        table.append((at, len(f), pos, bs))
        at += len(f)
    return head + b"".join(f for f, _, _ in frames) + after, table


def write(path, x, bps, rate, **kw):
    """-> str(path)"""
    data, _ = flac_bytes(x, bps, rate, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


# ------------------------------------------------------------------------------------------------------------ signals
def tone(n, ch, bps, seed=0, wasted=0, noise=3):
    """[n, ch] int64: a few partials and a little noise, so that predictors leave small residuals; the first samples
    are the extremes of the range (full-scale negative and positive); low `wasted` bits zero"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    full = 2 ** (bps - 1)
    w = 0.45 * np.sin(2 * np.pi * t * (0.0031 + 0.0007 * np.arange(ch)) + seed) + 0.25 * np.sin(2 * np.pi * t * 0.0113 + 1)
    x = np.round(w * (full - 1)).astype(np.int64) + rng.integers(-noise, noise, size=(n, ch), endpoint=True)
    x = np.clip(x, -full, full - 1)
    if n >= 2:
        x[0, :] = -full
        x[1, :] = full - 1
    elif n == 1:
        x[0, :] = -full
    if wasted:
        x = (x >> wasted) << wasted
    return x


def noise(n, ch, bps, seed=0):
    """[n, ch] int64 uniform over the whole range, the extremes first"""
    rng = np.random.default_rng(seed)
    full = 2 ** (bps - 1)
    x = rng.integers(-full, full - 1, size=(n, ch), endpoint=True, dtype=np.int64)
    x.flat[:2] = [-full, full - 1][:x.size]
    return x


def grid():
    """The cases both test files and the stand-alone checker use: name -> (x, bps, rate, write-kwargs).  One axis
    varies at a time around a 16-bit, 4096-block, stereo baseline."""
    g = {}
    N0 = 4096 + 37                                   # two frames, the last short
    base = dict(block_size=4096, sub=Sub("fixed", order=2, params=6), assignment="indep")

    def add(name, x, bps=16, rate=44100, **kw):
        g[name] = (x, bps, rate, dict(base, **kw))

    # lengths
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5):
        add("len%d" % n, tone(n, 2, 16, seed=n), sub=Sub("fixed", order=min(1, n - 1), params=12))
    # block sizes (255: 8-bit explicit; 1000: 16-bit explicit; 16: explicit too), last frame short
    for bs in (16, 192, 255, 576, 1000, 4096, 4608):
        add("bs%d" % bs, tone(2 * bs + 7, 2, 16, seed=bs), block_size=bs)
    add("variable", tone(3002, 2, 16, seed=5), variable=True, block_sizes=[576, 1000, 16, 255, 192])
    # bits per sample, mono and stereo, full-scale samples present
    for bps in (8, 12, 16, 20, 24):
        for ch in (1, 2):
            add("bits%d_ch%d" % (bps, ch), tone(N0, ch, bps, seed=bps + ch), bps=bps, rate=(8000, 16000, 22050, 32000, 48000)[bps // 4 - 2],
                sub=Sub("fixed", order=1, method=1, params=max(2, bps - 9)))
    add("bits_from_streaminfo", tone(N0, 2, 16, seed=3), bps_code=0, rate=12345, rate_code=0)
    add("rate_code12", tone(300, 1, 16, seed=4), rate=11000, rate_code=12, block_size=192)
    add("rate_code13", tone(300, 1, 16, seed=4), rate=11025, rate_code=13, block_size=192)
    add("rate_code14", tone(300, 1, 16, seed=4), rate=88200 + 10, rate_code=14, block_size=192)
    # subframe kinds
    add("constant", np.full((N0, 2), -32768, dtype=np.int64), sub=Sub("constant"))
    add("verbatim", noise(N0, 2, 16, seed=1), sub=Sub("verbatim"))
    add("verbatim24", noise(300, 2, 24, seed=2), bps=24, sub=Sub("verbatim"), block_size=192)
    for order in range(5):
        add("fixed%d" % order, tone(N0, 2, 16, seed=order), sub=Sub("fixed", order=order, method=1, params=14 if order == 0 else 7 + order))
    for order in (1, 2, 8, 12, 32):
        for shift in (0, 14):
            add("lpc%d_shift%d" % (order, shift), tone(N0, 2, 16, seed=order),
                sub=Sub("lpc", order=order, precision=15, shift=shift, method=1, params=16 if shift == 0 else 9))
            add("lpc%d_shift%d_24bit" % (order, shift), tone(N0, 2, 24, seed=order + 1), bps=24,
                sub=Sub("lpc", order=order, precision=15, shift=shift, method=1, params=24 if shift == 0 else 17))
    add("lpc_precision1", tone(N0, 1, 16, seed=9), sub=Sub("lpc", order=3, precision=1, shift=0, coefs=[-1, 0, -1], method=1, params=17))
    add("lpc_big_coefs_24bit", tone(N0, 2, 24, seed=11), bps=24,
        sub=Sub("lpc", order=4, precision=15, shift=13, coefs=[16383, -16384, 16383, -8200], method=1, params=22))
    for w in (1, 7):
        add("wasted%d" % w, tone(N0, 2, 16, seed=w, wasted=w), sub=Sub("fixed", order=2, wasted=w, params=4))
    add("wasted1_verbatim_constant", np.stack([noise(N0, 1, 16, seed=8)[:, 0] & ~1, np.full(N0, 6)], axis=1),
        sub=[Sub("verbatim", wasted=1), Sub("constant", wasted=1)])
    # residual coding
    quiet = tone(4096, 2, 16, seed=6, noise=0)
    quiet[2:] = quiet[2:3] + (np.arange(4094)[:, None] % 3)              # tiny differences: parameter 0 stays short
    add("rice0", quiet, sub=Sub("fixed", order=1, params=0, porder=1))
    add("rice14", noise(N0, 2, 16, seed=7), sub=Sub("fixed", order=0, params=14))
    add("rice30", noise(N0, 2, 24, seed=7), bps=24, sub=Sub("fixed", order=1, method=1, params=30))
    add("escape0", np.full((N0, 2), 1234, dtype=np.int64), sub=Sub("fixed", order=1, params=("esc", 0)))
    add("escape17", noise(N0, 2, 16, seed=12), sub=Sub("fixed", order=0, params=("esc", 17)))
    add("escape17_method1", noise(4096, 2, 16, seed=13), sub=Sub("fixed", order=0, method=1, porder=2, params=[("esc", 17), 14, ("esc", 16), 15]))
    add("porder1", tone(4096 * 2, 2, 16, seed=14), sub=Sub("fixed", order=2, porder=1, params=[5, 7]))
    # the largest partition order whose first partition is nonempty: 4096 >> 8 = 16 > 12; 4096 >> 12 = 1 > 0
    add("porder8_lpc12", tone(4096, 2, 16, seed=15), sub=Sub("lpc", order=12, precision=15, shift=14, porder=8, params=[8 + (i % 3) for i in range(256)]))
    add("porder12_fixed0", tone(4096, 1, 16, seed=16), sub=Sub("fixed", order=0, porder=12, params=[14] * 4096))
    add("porder15_fixed0", tone(32768, 1, 16, seed=17), block_size=32768, sub=Sub("fixed", order=0, method=1, porder=15, params=[15] * 32768))
    # stereo
    odd = tone(N0, 2, 16, seed=18)
    odd[:, 0] |= 1
    odd[:, 1] &= ~1                                                       # L + R odd everywhere
    odd[0], odd[1], odd[2] = (-32768, 32767), (32767, -32768), (-32767, 32766)      # side = -(2^16 - 1), 2^16 - 1
    for a in ("indep", "ls", "rs", "ms"):
        add("stereo_" + a, odd, assignment=a, sub=[Sub("fixed", order=1, method=1, params=9)] * 2)
        add("stereo24_" + a, noise(600, 2, 24, seed=19), bps=24, assignment=a, block_size=576, sub=Sub("verbatim"))
    add("stereo_8bit_ms", noise(600, 2, 8, seed=20), bps=8, assignment="ms", block_size=576, sub=Sub("verbatim"))
    add("stereo_mixed_assignments", tone(4 * 576 + 3, 2, 16, seed=21), block_size=576,
        assignment=lambda k: ("indep", "ls", "rs", "ms")[k % 4])
    return g


def main(out_dir):
    import os
    os.makedirs(out_dir, exist_ok=True)
    for name, (x, bps, rate, kw) in grid().items():
        data, table = flac_bytes(x, bps, rate, **kw)
        with open(os.path.join(out_dir, name + ".flac"), "wb") as f:
            f.write(data)
        with open(os.path.join(out_dir, name + ".tab"), "w") as f:      # channels bps n_frames, then one frame per line
            f.write("%d %d %d\n" % (x.shape[1], bps, len(table)))
            for off, ln, first, bs in table:
                f.write("%d %d %d %d\n" % (off, ln, first, bs))
        np.ascontiguousarray(x, dtype="<i4").tofile(os.path.join(out_dir, name + ".pcm"))
    print("%d files in %s" % (len(grid()), out_dir))


if __name__ == "__main__":
    main(sys.argv[1])
