"""How far the compressor's detector (csrc/compressor.h) is from the branching one of JUCE / pedalboard, on the CPU.

JUCE's dsp::Compressor feeds |x| through a ballistics filter that picks its coefficient by comparing the input with its own state,

    y = |x| + c (y - |x|),   c = aA when |x| > y, else aR,

and applies the same hard-knee gain to y.  This tool restates that filter as a serial fp64 loop, runs it and the definition of
tests/compressor_ref.py (the smooth decoupled peak detector) with the same aA, aR, threshold and ratio over the test grid's signals
at their longest length, and prints the largest and the RMS difference of the two gains in dB per signal -- over all samples and
over the samples where either gain is below 1.  Nothing is asserted: the figures go into DESIGN 4.26 and the README.  No GPU.

    python tools/compressor_vs_juce.py [--rate 32000] [--set voice]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import compressor_ref as R  # noqa: E402


def branching_detector(x, co):
    """JUCE's BallisticsFilter in peak mode, fp64"""
    a_a, a_r = co[0], co[1]
    y = 0.0
    out = [0.0] * len(x)
    for n, v in enumerate(np.abs(np.asarray(x, np.float32)).astype(np.float64).tolist()):
        c = a_a if v > y else a_r
        y = v + c * (y - v)
        out[n] = y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=32000)
    ap.add_argument("--set", default="voice", choices=sorted(R.SETS))
    args = ap.parse_args()
    co = R.coefficients(R.SETS[args.set], args.rate)
    res = dict(rate=args.rate, set=args.set, samples=R.LONGEST, signals={})
    for kind in R.KINDS:
        x = R.grid_signal(kind, R.LONGEST, args.rate, args.set)
        ours = 20.0 * np.log10(R.gains(R.detector(x, co), co))
        theirs = 20.0 * np.log10(R.gains(branching_detector(x, co), co))
        d = ours - theirs
        active = (ours < 0) | (theirs < 0)
        r = dict(max_db=float(np.abs(d).max()), rms_db=float(math.sqrt(np.mean(d * d))), active_share=float(active.mean()),
                 rms_db_active=float(math.sqrt(np.mean(d[active] ** 2))) if active.any() else 0.0,
                 mean_gain_db=float(ours.mean()), mean_gain_db_juce=float(theirs.mean()))
        res["signals"][kind] = r
        print("%-9s gain difference: max %.3f dB, rms %.3f dB (%.3f dB over the %.1f %% of samples where a gain is below 1); "
              "mean gain %.2f dB here, %.2f dB branching" % (kind, r["max_db"], r["rms_db"], r["rms_db_active"], 100 * r["active_share"],
                                                             r["mean_gain_db"], r["mean_gain_db_juce"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
