"""Time the true-peak limiter (csrc/limiter.h) on the GPU, next to the loudness meter on the same clips.

The device time of ONE gsv_limiter call -- the upload of the rows and all launches, limiting in place to -1 dBTP -- and of ONE
gsv_loudness call on the same clips, each with hipEvents around it: the median of --calls calls after a warm-up, with the lowest
and highest beside it, for

    one 10 s clip at 32 kHz,    32 x 10 s packed.

The clips are seeded Gaussian noise with a deviation of 0.25 to 0.5, whose true peak lies some 2 to 9 dB above the ceiling, so
every stage has work on every clip.  A JSON object with
everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/limiter_time.py [--calls 200]
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
from gsv_tts_lite_amd import limiter as LM  # noqa: E402

RATE = 32000
CASES = [("1 x 10 s", 1, 10), ("32 x 10 s", 32, 10)]


def _time(call, calls, dev):
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limiter_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    L = N.lib()
    look, rel = LM.times(RATE)
    res = dict(calls=args.calls, rate=RATE, lookahead=look, release=rel, cases={})
    for name, clips, seconds in CASES:
        n = seconds * RATE
        rng = np.random.default_rng(5)
        host = (rng.standard_normal(clips * n) * 0.5 * np.repeat(rng.uniform(0.5, 1.0, clips), n)).astype(np.float32)
        x = torch.from_numpy(host).to(dev)
        y = torch.empty_like(x)
        stream = N.current_stream_ptr(dev)
        rec = torch.empty(clips * 32, dtype=torch.uint8, device=dev)
        lim = (N.LimiterClip * clips)(*[N.LimiterClip(c * n, n, -1.0) for c in range(clips)])
        lim_need = L.gsv_limiter_work_bytes(lim, clips)
        lim_work = torch.empty(lim_need, dtype=torch.uint8, device=dev)
        loud = (N.LoudnessClip * clips)(*[N.LoudnessClip(c * n, n, -18.0) for c in range(clips)])
        loud_need = L.gsv_loudness_work_bytes(loud, clips, RATE)
        loud_work = torch.empty(loud_need, dtype=torch.uint8, device=dev)

        def limiter():          # out of place, so that every call limits the same samples
            N.check(L.gsv_limiter(x.data_ptr(), x.numel(), lim, clips, look, rel, y.data_ptr(), rec.data_ptr(), lim_work.data_ptr(), lim_need,
                                  stream))

        def loudness():
            N.check(L.gsv_loudness(x.data_ptr(), x.numel(), loud, clips, RATE, 1.0, y.data_ptr(), rec.data_ptr(), loud_work.data_ptr(),
                                   loud_need, stream))
        r = dict(gsv_loudness=_time(loudness, args.calls, dev), gsv_limiter=_time(limiter, args.calls, dev), workspace_bytes=int(lim_need))
        recs = LM.records(rec)
        r["first_clip"] = dict(dbtp_in=round(recs[0].dbtp_in, 3), dbtp_out=round(recs[0].dbtp_out, 4), min_gain=float(recs[0].min_gain),
                               trim=float(recs[0].trim))
        r["limited"] = sum(q.limited for q in recs)
        res["cases"][name] = r
        for k in ("gsv_limiter", "gsv_loudness"):
            print("%-10s %-13s %9.2f us [%9.2f, %9.2f]  = %8.2f us per 10 s of audio" % (
                name, k, r[k]["median_us"], r[k]["low_us"], r[k]["high_us"], r[k]["median_us"] * 10 / (clips * seconds)), flush=True)
        print("%-10s first clip %.2f -> %.4f dBTP, min gain %.3f, trim %.6f; %d of %d limited" % (
            name, recs[0].dbtp_in, recs[0].dbtp_out, recs[0].min_gain, recs[0].trim, r["limited"], clips), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
