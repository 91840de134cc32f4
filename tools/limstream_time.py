"""Time the stream limiter (csrc/limstream.h) on the GPU.

The device time of ONE gsv_limstream_push (its three launches) of a 16 000-sample chunk at 32 kHz with hipEvents around it -- the
median of --calls calls after a warm-up, with the lowest and highest beside it -- in the middle of a stream whose state is put back
before every call, so every call does the same work: on noise that is limited throughout, and on a quiet sine that is never limited.
Beside it, in the same process and on the same chunk: gsv_level_push (in place) and gsv_track_push (32 -> 48 kHz).  There is no
earlier version of this path to compare with; those two calls, which sit next to it in a stream, are the yardstick.

A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/limstream_time.py [--calls 100] [--samples 16000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import level as LV  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402

RATE = 32000


def _timed(call, calls, dev, before=None):
    for _ in range(10):
        if before:
            before()
        call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(calls):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2), high_us=round(1e3 * ms[-1], 2))


def _show(name, r):
    print("%-52s %9.2f us [%9.2f, %9.2f]" % (name, r["median_us"], r["low_us"], r["high_us"]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=16000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limstream_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    n = args.samples
    rng = np.random.default_rng(3)
    t = np.arange(2 * n)
    signals = {"noise, limited throughout": rng.standard_normal(2 * n).astype(np.float32) * 0.5,
               "quiet sine, never limited": (0.3 * np.sin(2 * np.pi * 997.0 * t / RATE)).astype(np.float32)}
    res = dict(calls=args.calls, samples=n, push={})
    for name, sig in signals.items():
        x = torch.from_numpy(sig).to(dev)
        lm = LM.StreamLimiter(-1.0, RATE, dev)
        lm.push_tensor(x[:n])                                      # the first half: the timed push is in the middle of a stream
        start = lm.state.clone()
        out = torch.empty(lm.capacity(n), device=dev)
        rec = torch.empty(4, dtype=torch.int64, device=dev)
        chunk = x[n:]
        key = "limstream push %d samples: %s" % (n, name)
        res["push"][key] = _show(key, _timed(lambda: lm.enqueue(chunk.data_ptr(), n, None, False, out.data_ptr(), rec.data_ptr()),
                                             args.calls, dev, lambda: lm.state.copy_(start)))
        r = LM.stream_record(rec.view(torch.uint8))
        print("    emitted %d, limited %r, min gain %.4f" % (r.emitted, r.limited, float(r.min_gain)), flush=True)
        if name.startswith("noise"):
            lv = LV.StreamLeveller(-18.0, RATE, dev)
            lv.push_tensor(x[:n])
            lstart = lv.state.clone()
            y, lrec = torch.empty(n, device=dev), torch.empty(5, dtype=torch.int64, device=dev)
            key = "level push %d samples (same chunk)" % n
            res["push"][key] = _show(key, _timed(lambda: lv.enqueue(chunk.data_ptr(), n, None, False, y.data_ptr(), lrec.data_ptr()),
                                                 args.calls, dev, lambda: lv.state.copy_(lstart)))
            rs = TrackResampler(TrackFormat(48000, 1, 20), RATE, dev)
            pcm, trec = torch.empty(rs.capacity(n), dtype=torch.int16, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
            key = "track push %d samples, 32 -> 48 kHz (same chunk)" % n
            res["push"][key] = _show(key, _timed(lambda: rs.enqueue(chunk.data_ptr(), n, None, False, pcm.data_ptr(), trec.data_ptr()),
                                                 args.calls, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
