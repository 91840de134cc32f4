"""Time the real-time track output (csrc/track.h) on the GPU.

1. The device time of ONE gsv_track_push of a 0.5 s chunk (16 000 samples at 32 kHz) per rate pair: hipEvents around each call
   (both launches), the median of --calls calls after a warm-up, with the lowest and highest beside it.
2. What tools/stream_batched_time.py reports for TTS.infer_stream_batched -- seconds of audio per second of wall time, the time to
   each text's first clip -- at 1, 16 and 32 texts, with track=TrackFormat(48000) and without, the two alternating run by run in
   the same process (without a track the loop issues the calls it issued before the track existed).  Each figure is the median
   of --reps runs with the lowest and highest run beside it.

A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/track_time.py [--calls 200] [--reps 3] [--sizes 1,16,32] [--dtype bfloat16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stream_batched_time as sbt  # noqa: E402
from gsv_tts_lite_amd import stream as stream_mod  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402
from gsv_tts_lite_amd.tts import TTS  # noqa: E402

PAIRS = [(32000, 48000), (32000, 44100), (32000, 24000), (32000, 16000), (32000, 8000), (32000, 32000), (48000, 32000)]


def push_times(dev, calls):
    out = {}
    for in_rate, out_rate in PAIRS:
        n = in_rate // 2
        fmt = TrackFormat(out_rate, 1, 20)
        rs = TrackResampler(fmt, in_rate, dev)
        x = torch.from_numpy(np.random.default_rng(3).uniform(-0.5, 0.5, n).astype(np.float32)).to(dev)
        pcm = torch.empty(rs.capacity(n), dtype=torch.int16, device=dev)
        rec = torch.empty(4, dtype=torch.int32, device=dev)
        for _ in range(10):
            rs.enqueue(x.data_ptr(), n, None, False, pcm.data_ptr(), rec.data_ptr())
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rs.enqueue(x.data_ptr(), n, None, False, pcm.data_ptr(), rec.data_ptr())
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        out["%d->%d" % (in_rate, out_rate)] = dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2),
                                                  high_us=round(1e3 * ms[-1], 2), packets=rec.tolist()[0])
        r = out["%d->%d" % (in_rate, out_rate)]
        print("push of 0.5 s  %5d -> %5d Hz: %8.2f us [%8.2f, %8.2f]  (%d packets of 20 ms)" % (in_rate, out_rate, r["median_us"], r["low_us"],
                                                                                            r["high_us"], r["packets"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1,16,32")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    res = dict(calls=args.calls, reps=args.reps, dtype=args.dtype, push=push_times(dev, args.calls), sizes={})
    sizes = [int(s) for s in args.sizes.split(",")]
    tts = TTS(gpt_cache=[(s, 512) for s in sorted(set(sizes) | {1})], sovits_cache=[50, 55], device="cuda:0", dtype=args.dtype)
    tts.load_gpt_model("synthetic://gpt?seed=1234&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(sbt._frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    vq = next(iter(tts.sovits_models.values())).vq_model
    clock = sbt._DeviceTime()
    vq.decode = clock.wrap(vq.decode)
    stream_mod.ChunkEmitter.push = clock.wrap(stream_mod.ChunkEmitter.push)
    kw = dict(stream_chunk=25, debug=False, top_k=1)
    fmt = TrackFormat(48000, 1, 20)
    for S in sizes:
        texts, seeds = sbt._texts(S), list(range(100, 100 + S))
        ways = {"no_track": lambda: tts.infer_stream_batched(*sbt.REF, texts, slots=S, seed=seeds, **kw),
                "track_48k": lambda: tts.infer_stream_batched(*sbt.REF, texts, slots=S, seed=seeds, track=fmt, **kw)}
        runs = {k: [] for k in ways}
        for fn in ways.values():
            sbt._serve(fn, S, clock)                                # warm-up: graphs captured, buffers grown
        for _ in range(args.reps):                                  # alternating: what shares the host hits both alike
            for k, fn in ways.items():
                runs[k].append(sbt._serve(fn, S, clock))
        row = {k: sbt._spread(v) for k, v in runs.items()}
        for k, r in row.items():
            print("S=%2d %-10s audio/wall %7.2f [%7.2f, %7.2f]  first clip median %.4f s [%.4f, %.4f] worst %.4f s  vocoder+epilogue %4.1f %% of "
                  "wall  (wall %.3f s, audio %.1f s)" % (S, k, r["audio_per_wall"]["median"], r["audio_per_wall"]["low"], r["audio_per_wall"]["high"],
                                                          r["first_median_s"]["median"], r["first_median_s"]["low"], r["first_median_s"]["high"],
                                                          r["first_worst_s"]["median"], 100 * r["vocoder_share"]["median"], r["wall_s"]["median"],
                                                          r["audio_s"]["median"]), flush=True)
        res["sizes"][S] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
