"""Time the equaliser (csrc/eq.h) on the GPU, beside the loudness meter.

The device time of ONE gsv_eq call -- the upload of the rows, coefficients and matrices and all launches, the "voice" preset in
place -- with hipEvents around it: the median of --calls calls after a warm-up, with the lowest and highest beside it, for

    one 10 s clip at 32 kHz,    32 x 10 s packed,    one 60 s clip,

and, in the same run on the same card, one gsv_loudness call (measure and scale) over the same clips: the same kind of filter
with more launches behind it.  --sections 6 times a six-section cascade instead.  A JSON object with everything comes last.  There
is no CPU path: without a GPU the tool fails.

    python tools/eq_time.py [--calls 200] [--sections 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402

RATE = 32000
CASES = [("1 x 10 s", 1, 10), ("32 x 10 s", 32, 10), ("1 x 60 s", 1, 60)]
SIX = [EQM.Band("highpass", 20.0, q=0.5), EQM.Band("lowshelf", 120.0, q=0.7, gain_db=4.0), EQM.Band("peak", 300.0, q=1.0, gain_db=2.5),
       EQM.Band("peak", 2500.0, q=4.0, gain_db=-6.0), EQM.Band("highshelf", 6000.0, q=0.8, gain_db=3.0), EQM.Band("lowpass", 14400.0)]


def timed(call, calls, dev):
    for _ in range(10):
        call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2), high_us=round(1e3 * ms[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sections", type=int, default=3, choices=(3, 6))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eq_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    L = N.lib()
    e = EQM.EQ.preset("voice", RATE) if args.sections == 3 else EQM.EQ(SIX)
    co = EQM.design(e, RATE)
    res = dict(calls=args.calls, rate=RATE, sections=len(co), cases={})
    for name, clips, seconds in CASES:
        n = seconds * RATE
        rng = np.random.default_rng(5)
        x0 = torch.from_numpy((rng.uniform(-0.3, 0.3, clips * n) * np.repeat(rng.uniform(0.2, 1.0, clips), n)).astype(np.float32)).to(dev)
        stream = N.current_stream_ptr(dev)
        offsets, lengths = [c * n for c in range(clips)], [n] * clips
        tab, des = EQM._tables(offsets, lengths, [0] * clips, [co])
        need = L.gsv_eq_work_bytes(tab, clips, des, 1)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        rec = torch.empty(clips * EQM.RECORD_BYTES, dtype=torch.uint8, device=dev)
        y = torch.empty_like(x0)

        def eq_call():
            N.check(L.gsv_eq(x0.data_ptr(), x0.numel(), tab, clips, des, 1, y.data_ptr(), rec.data_ptr(), work.data_ptr(), need, stream))
        r = timed(eq_call, args.calls, dev)
        recs = EQM.records(rec)
        r.update(workspace_bytes=int(need), peak_in=float(recs[0].peak_in), peak_out=float(recs[0].peak_out))
        r["us_per_10s_of_audio"] = round(r["median_us"] * 10 / (clips * seconds), 2)

        arr = (N.LoudnessClip * clips)(*[N.LoudnessClip(c * n, n, -18.0) for c in range(clips)])
        lneed = L.gsv_loudness_work_bytes(arr, clips, RATE)
        lwork = torch.empty(lneed, dtype=torch.uint8, device=dev)
        lrec = torch.empty(clips * 32, dtype=torch.uint8, device=dev)

        def loud_call():
            N.check(L.gsv_loudness(x0.data_ptr(), x0.numel(), arr, clips, RATE, 1.0, y.data_ptr(), lrec.data_ptr(), lwork.data_ptr(), lneed, stream))
        r["loudness"] = timed(loud_call, args.calls, dev)
        res["cases"][name] = r
        print("%-10s gsv_eq %9.2f us [%9.2f, %9.2f]  = %8.2f us per 10 s of audio   gsv_loudness %9.2f us [%9.2f, %9.2f]   (peak %.3f -> %.3f)" % (
            name, r["median_us"], r["low_us"], r["high_us"], r["us_per_10s_of_audio"], r["loudness"]["median_us"], r["loudness"]["low_us"],
            r["loudness"]["high_us"], r["peak_in"], r["peak_out"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
