"""Time the loudness meter (csrc/loudness.h) on the GPU.

The device time of ONE gsv_loudness call -- the upload of the rows and all launches, measure and scale in place -- with
hipEvents around it: the median of --calls calls after a warm-up, with the lowest and highest beside it, for

    one 10 s clip at 32 kHz,    32 x 10 s packed,    one 60 s clip.

tools/voc_time.py, run in the same minute on the same card, gives the vocoder pass for the same 10 s of audio to set it against.
A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/loudness_time.py [--calls 200]
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
from gsv_tts_lite_amd import loudness as LD  # noqa: E402

RATE = 32000
CASES = [("1 x 10 s", 1, 10), ("32 x 10 s", 32, 10), ("1 x 60 s", 1, 60)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    L = N.lib()
    res = dict(calls=args.calls, rate=RATE, cases={})
    for name, clips, seconds in CASES:
        n = seconds * RATE
        rng = np.random.default_rng(5)
        x = torch.from_numpy((rng.uniform(-0.3, 0.3, clips * n) * np.repeat(rng.uniform(0.2, 1.0, clips), n)).astype(np.float32)).to(dev)
        arr = (N.LoudnessClip * clips)(*[N.LoudnessClip(c * n, n, -18.0) for c in range(clips)])
        need = L.gsv_loudness_work_bytes(arr, clips, RATE)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        rec = torch.empty(clips * 32, dtype=torch.uint8, device=dev)
        y = torch.empty_like(x)
        stream = N.current_stream_ptr(dev)

        def call():
            N.check(L.gsv_loudness(x.data_ptr(), x.numel(), arr, clips, RATE, 1.0, y.data_ptr(), rec.data_ptr(), work.data_ptr(), need, stream))
        for _ in range(10):
            call()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        recs = LD.records(rec)
        r = dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2), high_us=round(1e3 * ms[-1], 2),
                 workspace_bytes=int(need), lufs=[round(q.lufs, 3) for q in recs[:4]])
        r["us_per_10s_of_audio"] = round(r["median_us"] * 10 / (clips * seconds), 2)
        res["cases"][name] = r
        print("%-10s %9.2f us [%9.2f, %9.2f]  = %8.2f us per 10 s of audio   (first clip %.2f -> -18 LUFS, gain %.3f)" % (
            name, r["median_us"], r["low_us"], r["high_us"], r["us_per_10s_of_audio"], recs[0].lufs, recs[0].gain), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
