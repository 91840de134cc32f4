"""The bytes of the compressor's host twins, pinned (csrc/compressor.h behind gsv_compressor_host, csrc/cmpstream.h behind
gsv_cmpstream_push_host).  No GPU.

test_compressor_cpu.py holds the clip twin to the fp64 oracle within one fp32 ulp, and the stream twin and both devices are held to
the clip twin in bytes; this holds the twins' bytes themselves still, so a change to the scans, the chains or the two routines that
moves a bit shows here.  tests/golden/compressor_twin_bytes.json carries, for three parameter sets at 32 kHz, the coefficients aA,
aR, T, s, M as raw doubles (no exp or pow is recomputed), and per length -- 1, a run + 1, a span + 1, a chunk + 1, three chunks + 5:
two chained links and a short last span -- the SHA-256 of the clip twin's samples and record and of the stream twin's records under
pushes of a span + 1, the last one flushing (its samples are asserted to be the clip's).  The input is the integer-hash signal of
test_eq_twin_bytes.py: integer arithmetic alone, so it is the same bits everywhere and the fixture stores no samples.  Per set there
is one stream-only entry, "nonfinite": the longest signal with +inf at index span - 1 and a NaN at index chunk, which a clip would
hand back unchanged and a stream takes into the detector as 0.0, copies bit for bit and keeps out of its statistics.

The fixture is written by `python tests/test_compressor_twin_bytes.py --write` (from the sets of tests/compressor_ref.py).
cmp_powers squares the coefficients in long double, so the digests hold where that is x87's 64-bit significand; elsewhere the test
skips."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "gsv-tts-lite_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import compressor as CM  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "compressor_twin_bytes.json")
RATE = 32000
SETS = ("voice", "fast", "slow")
RUN, SPAN, CHUNK = CM.RUN, CM.SPAN, CM.CHUNK
LENGTHS = (1, RUN + 1, SPAN + 1, CHUNK + 1, 3 * CHUNK + 5)
PUSH = SPAN + 1
X87 = np.finfo(np.longdouble).nmant == 63


def signal(n):
    """sample i: the top 24 bits of i * 2654435761 mod 2^32 as a signed integer, times 2^-23: exact in fp32, in [-1, 1)"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23))


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def clip_twin(coefs, x):
    """gsv_compressor_host over one clip -> (sample bytes, record bytes)"""
    xt = torch.from_numpy(x.copy())
    out = torch.empty_like(xt)
    rec = CM.run_packed(xt, [0], [len(x)], [0], [coefs], out)
    return out.numpy().tobytes(), rec.numpy().tobytes()


def stream_twin(coefs, x):
    """gsv_cmpstream_push_host in pushes of PUSH samples, the last one flushing -> (sample bytes, the records' bytes)"""
    L = N.lib()
    need = L.gsv_cmpstream_state_bytes()
    state = torch.zeros(need, dtype=torch.uint8)
    N.check(L.gsv_cmpstream_init_host(state.data_ptr(), need, CM._tables([], [], [], [coefs])[1]))
    samples, recs = [], []
    for at in range(0, len(x), PUSH):
        part = torch.from_numpy(x[at: at + PUSH].copy())
        out = torch.empty_like(part)
        rec = torch.zeros(CM.STREAM_RECORD_BYTES // 8, dtype=torch.int64)
        N.check(L.gsv_cmpstream_push_host(state.data_ptr(), part.data_ptr(), len(part), None, int(at + PUSH >= len(x)), out.data_ptr(),
                                          rec.data_ptr()))
        samples.append(out.numpy().tobytes())
        recs.append(rec.numpy().tobytes())
    return b"".join(samples), b"".join(recs)


def digests(coefs, n):
    """the clip twin's samples and record and the stream twin's records; the stream's samples must be the clip's"""
    x = signal(n)
    y, rec = clip_twin(coefs, x)
    ys, srec = stream_twin(coefs, x)
    assert ys == y, "the stream's samples are not the clip's (n = %d)" % n
    return {"samples": _sha(y), "record": _sha(rec), "stream_records": _sha(srec)}


def nonfinite_signal():
    x = signal(3 * CHUNK + 5)
    x[SPAN - 1] = np.inf
    x[CHUNK] = np.nan
    return x


def nonfinite_digests(coefs):
    """the stream twin alone over the signal with an infinity and a NaN: they come back bit for bit"""
    x = nonfinite_signal()
    ys, srec = stream_twin(coefs, x)
    y = np.frombuffer(ys, np.float32)
    for i in (SPAN - 1, CHUNK):
        assert y[i: i + 1].tobytes() == x[i: i + 1].tobytes(), "a sample that is not finite was not copied (index %d)" % i
    assert np.isfinite(np.delete(y, (SPAN - 1, CHUNK))).all()
    return {"stream_samples": _sha(ys), "stream_records": _sha(srec)}


def _load():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_input_is_what_the_fixture_was_made_from():
    x = signal(3 * CHUNK + 5)
    assert x.dtype == np.float32 and x.min() >= -1.0 and x.max() < 1.0 and x[0] == -1.0
    assert signal(RUN + 1).tobytes() == x[: RUN + 1].tobytes()
    assert _sha(x.tobytes()) == _load()["signal_sha256"]


@pytest.mark.skipif(not X87, reason="cmp_powers squares in long double: the digests were made with x87's 64-bit significand")
@pytest.mark.parametrize("name", SETS)
def test_twin_bytes_are_the_fixtures(name):
    fx = _load()
    assert (fx["rate"], fx["run"], fx["span"], fx["chunk"], fx["push"]) == (RATE, RUN, SPAN, CHUNK, PUSH)
    entry = fx["sets"][name]
    coefs = np.array([float.fromhex(v) for v in entry["coefficients"]], np.float64)
    assert coefs.shape == (5,)
    assert sorted(int(n) for n in entry["lengths"]) == sorted(LENGTHS)
    for n in LENGTHS:
        assert digests(coefs, n) == entry["lengths"][str(n)], (name, n)
    assert nonfinite_digests(coefs) == entry["nonfinite"], name


def _write():
    import compressor_ref as R
    assert X87, "write the fixture where long double has a 64-bit significand"
    fx = {"rate": RATE, "run": RUN, "span": SPAN, "chunk": CHUNK, "push": PUSH, "signal_sha256": _sha(signal(3 * CHUNK + 5).tobytes()),
          "sets": {}}
    for name in SETS:
        coefs = np.array(R.coefficients(R.SETS[name], RATE), np.float64)
        fx["sets"][name] = {"coefficients": [float(v).hex() for v in coefs], "lengths": {str(n): digests(coefs, n) for n in LENGTHS},
                             "nonfinite": nonfinite_digests(coefs)}
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_compressor_twin_bytes.py --write")
    _write()
