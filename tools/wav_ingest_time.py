"""Time reference-audio ingest from WAV files (wavio.load_wav / load_wavs, then sv.resample to the 32 kHz model rate),
split into its parts per clip: the host parse (file read + RIFF walk), the upload of the data chunk (H2D), the
conversion kernel (gsv_wav_to_mono_batch) and the resample; then whole load_wav calls one clip at a time against one
load_wavs over all N clips.  Host clock around work that ends in a device synchronise for the whole calls and the parse,
hipEvents for the upload, kernel and resample; warm-up excluded, median.  s16 files written into a temporary directory.
Prints one line per case and a JSON list at the end.

    python tools/wav_ingest_time.py [--reps 5] [--ns 1,16,64] [--cases 48000x2x10,44100x1x3,16000x1x10]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wav_writer as ww  # noqa: E402
from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import synth, wavio  # noqa: E402
from gsv_tts_lite_amd.sv import resample  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _median(ts)


def _event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return _median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ns", default="1,16,64")
    ap.add_argument("--cases", default="48000x2x10,44100x1x3,16000x1x10", help="rate x channels x seconds, s16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = N.lib()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in args.cases.split(","):
            rate, ch, secs = int(case.split("x")[0]), int(case.split("x")[1]), float(case.split("x")[2])
            n_fr = int(rate * secs)
            for n in [int(v) for v in args.ns.split(",")]:
                assert 1 <= n <= N.AUX_MAX_CLIPS, "one launch covers at most %d clips" % N.AUX_MAX_CLIPS
                paths = []
                for i in range(n):
                    w = np.stack([synth.synth_audio(i + c, n_fr) for c in range(ch)], axis=1)
                    paths.append(ww.write(os.path.join(tmp, "%s_%d.wav" % (case, i)), np.round(w * 32767).astype(np.int64),
                                          "s16", rate))
                parse = _host_ms(lambda: [wavio.parse_wav(p) for p in paths], args.reps, args.warmup)
                infos = [wavio.parse_wav(p) for p in paths]
                packed = bytearray(b"".join(raw[i.data_offset:i.data_offset + n_fr * ch * 2] for i, raw in infos))
                host = torch.frombuffer(packed, dtype=torch.uint8)
                h2d = _event_ms(lambda: host.to(dev), args.reps, args.warmup)
                pcm = host.to(dev)
                out = torch.empty(n * n_fr, dtype=torch.float32, device=dev)
                clips = (N.WavClip * n)(*[N.WavClip(k * n_fr * ch * 2, n_fr, N.PCM_S16, ch) for k in range(n)])
                st = N.current_stream_ptr(dev)
                kern = _event_ms(lambda: N.check(L.gsv_wav_to_mono_batch(pcm.data_ptr(), pcm.numel(), clips, n, out.data_ptr(),
                                                                         st)), args.reps, args.warmup)
                mono = [out[k * n_fr:(k + 1) * n_fr] for k in range(n)]
                rs = _event_ms(lambda: [resample(x, rate, 32000, dev) for x in mono], args.reps, args.warmup) if rate != 32000 else 0.0
                seq = _host_ms(lambda: [wavio.load_wav(p, dev) for p in paths], args.reps, args.warmup)
                bat = _host_ms(lambda: wavio.load_wavs(paths, dev), args.reps, args.warmup)
                row = dict(rate=rate, channels=ch, seconds=secs, n=n, mb_per_clip=round(n_fr * ch * 2 / 2 ** 20, 3),
                           parse_ms_per_clip=round(parse / n, 4), h2d_ms_per_clip=round(h2d / n, 4),
                           kernel_ms_per_clip=round(kern / n, 4), resample_ms_per_clip=round(rs / n, 4),
                           load_wav_ms_per_clip=round(seq / n, 4), load_wavs_ms_per_clip=round(bat / n, 4))
                rows.append(row)
                print("%5d Hz x%d %4.1f s x %2d: parse %.3f, H2D %.3f, kernel %.4f, resample %.3f ms / clip; load_wav %.3f, "
                      "load_wavs %.3f ms / clip" % (rate, ch, secs, n, parse / n, h2d / n, kern / n, rs / n, seq / n, bat / n),
                      flush=True)
                for p in paths:
                    os.remove(p)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
