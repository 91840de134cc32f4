"""The bytes of the reverb's host twin, pinned (csrc/reverb.h behind gsv_reverb_host).  No GPU.

test_reverb_cpu.py holds the twin to the serial fp64 oracle within its bound, and the device is held to the twin in bytes; this
holds the twin's bytes themselves still, so a change to the scan, its powers, the order of the sum or the mix that moves a bit shows
here.  tests/golden/reverb_twin_bytes.json carries, for three parameter sets, the twelve delays as integers and d, fb, gin, gw, gd as
raw doubles (nothing is recomputed), and per length -- 1, the shortest delay + 1, the longest + 1, twice the longest + 1, three times
the longest + 7: three wraps of every line -- the SHA-256 of the twin's samples and of its record.  The input is the integer-hash
signal of test_eq_twin_bytes.py: integer arithmetic alone, so it is the same bits everywhere and the fixture stores no samples.

The fixture is written by `python tests/test_reverb_twin_bytes.py --write` (from the sets of tests/reverb_ref.py).  The twin has no
long double in it -- the scan's powers are squared in fp64 -- so the digests hold wherever fp64 is IEEE, and nothing skips."""
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

from gsv_tts_lite_amd import reverb as RV  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "reverb_twin_bytes.json")
SETS = ("voice32", "hall", "tiny")
LONGEST = 3 * 1173 + 7


def signal(n):
    """sample i: the top 24 bits of i * 2654435761 mod 2^32 as a signed integer, times 2^-23: exact in fp32, in [-1, 1)"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23))


def lengths(delays):
    lo, hi = int(min(delays)), int(max(delays))
    return (1, lo + 1, hi + 1, 2 * hi + 1, 3 * hi + 7)


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def digests(params, n):
    """gsv_reverb_host over one clip -> the digests of its samples and of its record"""
    xt = torch.from_numpy(signal(n).copy())
    out = torch.empty_like(xt)
    rec = RV.run_packed(xt, [0], [n], [0], [params], out)
    return {"samples": _sha(out.numpy().tobytes()), "record": _sha(rec.numpy().tobytes())}


def _load():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_input_is_what_the_fixture_was_made_from():
    x = signal(LONGEST)
    assert x.dtype == np.float32 and x.min() >= -1.0 and x.max() < 1.0 and x[0] == -1.0
    assert signal(17).tobytes() == x[:17].tobytes()
    assert _sha(x.tobytes()) == _load()["signal_sha256"]


@pytest.mark.parametrize("name", SETS)
def test_twin_bytes_are_the_fixtures(name):
    fx = _load()
    assert fx["span"] == RV.N.RVB_SPAN
    entry = fx["sets"][name]
    delays = np.array(entry["delays"], np.int32)
    gains = np.array([float.fromhex(v) for v in entry["gains"]], np.float64)
    assert delays.shape == (12,) and gains.shape == (5,)
    assert sorted(int(n) for n in entry["lengths"]) == sorted(lengths(delays))
    for n in lengths(delays):
        assert digests((delays, gains), n) == entry["lengths"][str(n)], (name, n)


def _write():
    import reverb_ref as R
    fx = {"span": RV.N.RVB_SPAN, "signal_sha256": _sha(signal(LONGEST).tobytes()), "sets": {}}
    for name in SETS:
        combs, aps, d, fb, gin, gw, gd = R.SETS[name][0]
        delays, gains = np.array(combs + aps, np.int32), np.array([d, fb, gin, gw, gd], np.float64)
        fx["sets"][name] = {"delays": [int(v) for v in delays], "gains": [float(v).hex() for v in gains],
                            "lengths": {str(n): digests((delays, gains), n) for n in lengths(delays)}}
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_reverb_twin_bytes.py --write")
    _write()
