"""Time the stream leveller (csrc/level.h) on the GPU.

1. The device time of ONE gsv_level_push (both launches, in place) at 32 kHz with hipEvents around it -- the median of --calls
   calls after a warm-up, with the lowest and highest beside it -- for pushes of 0.5 s (the token-mode chunk), 2 s and 10 s (a
   sentence), each at the start of a stream and with 60 s of block history behind it, and for 32 streams pushed back to back.
   Beside them, in the same process: gsv_track_push (32 -> 48 kHz) for the 0.5 s chunk, gsv_loudness (the clip meter, measure
   and scale in place) for the same audio, and the vocoder pass of a 25-token chunk.
2. What tools/stream_batched_time.py reports for TTS.infer_stream_batched at --sizes texts, with loudness=-18 and without, the two
   alternating run by run in the same process (without it the loop issues the calls it issued before the leveller existed).

A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/level_time.py [--calls 200] [--reps 3] [--sizes 32] [--dtype bfloat16]
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
from gsv_tts_lite_amd import level as LV  # noqa: E402
from gsv_tts_lite_amd import loudness as LD  # noqa: E402
from gsv_tts_lite_amd import stream as stream_mod  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402
from gsv_tts_lite_amd.tts import TTS  # noqa: E402

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
    print("%-44s %9.2f us [%9.2f, %9.2f]" % (name, r["median_us"], r["low_us"], r["high_us"]), flush=True)
    return r


def push_times(dev, calls):
    out = {}
    rng = np.random.default_rng(3)
    noise = lambda n: torch.from_numpy(rng.uniform(-0.3, 0.3, n).astype(np.float32)).to(dev)
    for seconds in (0.5, 2.0, 10.0):
        n = int(seconds * RATE)
        x, y = noise(n), torch.empty(n, device=dev)
        rec = torch.empty(5, dtype=torch.int64, device=dev)
        for history in (0, 60):
            lv = LV.StreamLeveller(-18.0, RATE, dev)
            if history:
                lv.push_tensor(noise(history * RATE))
            start = lv.state.clone()
            restore = lambda: lv.state.copy_(start)                 # every call measures the same hops behind the same history
            call = lambda: lv.enqueue(x.data_ptr(), n, None, False, y.data_ptr(), rec.data_ptr())
            key = "level push %.1f s, %d s of history" % (seconds, history)
            out[key] = _show(key, _timed(call, calls, dev, restore))
    # 32 streams, a 0.5 s chunk each, back to back on one stream
    n = RATE // 2
    xs, rec = noise(32 * n), torch.empty(32 * 5, dtype=torch.int64, device=dev)
    lvs = [LV.StreamLeveller(-18.0, RATE, dev) for _ in range(32)]

    def all32():
        for i, lv in enumerate(lvs):
            lv.enqueue(xs[i * n:].data_ptr(), n, None, False, xs[i * n:].data_ptr(), rec[5 * i:].data_ptr())
    out["level push 0.5 s x 32 streams"] = _show("level push 0.5 s x 32 streams", _timed(all32, max(20, calls // 4), dev))
    # beside it: the track push of the same chunk
    fmt = TrackFormat(48000, 1, 20)
    rs = TrackResampler(fmt, RATE, dev)
    x = noise(n)
    pcm, trec = torch.empty(rs.capacity(n), dtype=torch.int16, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    out["track push 0.5 s, 32 -> 48 kHz"] = _show("track push 0.5 s, 32 -> 48 kHz",
                                                  _timed(lambda: rs.enqueue(x.data_ptr(), n, None, False, pcm.data_ptr(), trec.data_ptr()), calls, dev))
    # and the clip meter over the same audio
    for seconds in (0.5, 10.0):
        m = int(seconds * RATE)
        x = noise(m)
        key = "gsv_loudness %.1f s (measure and scale)" % seconds
        out[key] = _show(key, _timed(lambda: LD.run_packed(x, [0], [m], [-18.0], RATE, 1.0, x), max(20, calls // 4), dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="32")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("level_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    res = dict(calls=args.calls, reps=args.reps, dtype=args.dtype, push=push_times(dev, args.calls), sizes={})
    sizes = [int(s) for s in args.sizes.split(",") if s]
    tts = TTS(gpt_cache=[(s, 512) for s in sorted(set(sizes) | {1})], sovits_cache=[50, 55], device="cuda:0", dtype=args.dtype)
    tts.load_gpt_model("synthetic://gpt?seed=1234&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(sbt._frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    vq = next(iter(tts.sovits_models.values())).vq_model
    # the vocoder pass of one 25-token chunk, as the stream issues it
    ge = tts._ge_for("spk.wav", next(iter(tts.sovits_models)))
    pred = torch.from_numpy(y[:25].astype(np.int64))[None, None].to(dev)
    phones = torch.tensor(x.tolist(), dtype=torch.int64, device=dev).unsqueeze(0)

    def decode():
        with torch.inference_mode():
            vq.decode(pred, phones, ge, noise_scale=0.5, speed=1.0, stream_mode=True, valid_start_idx=0, overlap_len=5)
            vq.enc_p.y_overlap = None
    try:
        res["push"]["vocoder pass, 25-token chunk"] = _show("vocoder pass, 25-token chunk", _timed(decode, max(20, args.calls // 4), dev))
    except Exception as exc:        # the figure is a yardstick beside the others, not what this tool is about
        print("vocoder pass not timed: %r" % (exc,), flush=True)
    clock = sbt._DeviceTime()
    vq.decode = clock.wrap(vq.decode)
    stream_mod.ChunkEmitter.push = clock.wrap(stream_mod.ChunkEmitter.push)
    kw = dict(stream_chunk=25, debug=False, top_k=1)
    for S in sizes:
        texts, seeds = sbt._texts(S), list(range(100, 100 + S))
        ways = {"no_loudness": lambda: tts.infer_stream_batched(*sbt.REF, texts, slots=S, seed=seeds, **kw),
                "loudness_-18": lambda: tts.infer_stream_batched(*sbt.REF, texts, slots=S, seed=seeds, loudness=-18.0, **kw)}
        runs = {k: [] for k in ways}
        for fn in ways.values():
            sbt._serve(fn, S, clock)                                # warm-up: graphs captured, buffers grown
        for _ in range(args.reps):                                  # alternating: what shares the host hits both alike
            for k, fn in ways.items():
                runs[k].append(sbt._serve(fn, S, clock))
        row = {k: sbt._spread(v) for k, v in runs.items()}
        for k, r in row.items():
            print("S=%2d %-13s audio/wall %7.2f [%7.2f, %7.2f]  first clip median %.4f s [%.4f, %.4f] worst %.4f s  vocoder+epilogue %4.1f %% of "
                  "wall  (wall %.3f s, audio %.1f s)" % (S, k, r["audio_per_wall"]["median"], r["audio_per_wall"]["low"], r["audio_per_wall"]["high"],
                                                          r["first_median_s"]["median"], r["first_median_s"]["low"], r["first_median_s"]["high"],
                                                          r["first_worst_s"]["median"], 100 * r["vocoder_share"]["median"], r["wall_s"]["median"],
                                                          r["audio_s"]["median"]), flush=True)
        res["sizes"][S] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
