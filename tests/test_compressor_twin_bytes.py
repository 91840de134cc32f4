"""The bytes of the compressor's host twin, pinned (csrc/compressor.h behind gsv_compressor_host).  No GPU.

test_compressor_cpu.py holds the twin to the fp64 oracle within one fp32 ulp, and the device is held to the twin in bytes; this holds
the twin's bytes themselves still, so a change to the scans, the chains or the two routines that moves a bit shows here.
tests/golden/compressor_twin_bytes.json carries, for three parameter sets at 32 kHz, the coefficients aA, aR, T, s, M as raw doubles
(no exp or pow is recomputed), and per length -- 1, a run + 1, a span + 1, a chunk + 1, three chunks + 5: two chained links and a
short last span -- the SHA-256 of the twin's samples and of its record.  The input is the integer-hash signal of
test_eq_twin_bytes.py: integer arithmetic alone, so it is the same bits everywhere and the fixture stores no samples.

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

from gsv_tts_lite_amd import compressor as CM  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "compressor_twin_bytes.json")
RATE = 32000
SETS = ("voice", "fast", "slow")
RUN, SPAN, CHUNK = CM.RUN, CM.SPAN, CM.CHUNK
LENGTHS = (1, RUN + 1, SPAN + 1, CHUNK + 1, 3 * CHUNK + 5)
X87 = np.finfo(np.longdouble).nmant == 63


def signal(n):
    """sample i: the top 24 bits of i * 2654435761 mod 2^32 as a signed integer, times 2^-23: exact in fp32, in [-1, 1)"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23))


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def digests(coefs, n):
    """gsv_compressor_host over one clip -> the digests of its samples and of its record"""
    xt = torch.from_numpy(signal(n).copy())
    out = torch.empty_like(xt)
    rec = CM.run_packed(xt, [0], [n], [0], [coefs], out)
    return {"samples": _sha(out.numpy().tobytes()), "record": _sha(rec.numpy().tobytes())}


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
    assert (fx["rate"], fx["run"], fx["span"], fx["chunk"]) == (RATE, RUN, SPAN, CHUNK)
    entry = fx["sets"][name]
    coefs = np.array([float.fromhex(v) for v in entry["coefficients"]], np.float64)
    assert coefs.shape == (5,)
    assert sorted(int(n) for n in entry["lengths"]) == sorted(LENGTHS)
    for n in LENGTHS:
        assert digests(coefs, n) == entry["lengths"][str(n)], (name, n)


def _write():
    import compressor_ref as R
    assert X87, "write the fixture where long double has a 64-bit significand"
    fx = {"rate": RATE, "run": RUN, "span": SPAN, "chunk": CHUNK, "signal_sha256": _sha(signal(3 * CHUNK + 5).tobytes()), "sets": {}}
    for name in SETS:
        coefs = np.array(R.coefficients(R.SETS[name], RATE), np.float64)
        fx["sets"][name] = {"coefficients": [float(v).hex() for v in coefs], "lengths": {str(n): digests(coefs, n) for n in LENGTHS}}
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_compressor_twin_bytes.py --write")
    _write()
