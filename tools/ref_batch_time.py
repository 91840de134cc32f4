"""Time the batched reference-audio models against N sequential single-clip calls: CN-HuBERT's prompt_ssl (+ 0.3 s pad;
CNHubertNative.prompt_ssl_batch vs N x prompt_ssl) and ERes2NetV2's embed at 32 kHz (SVNative.embed_batch vs N x embed),
for N = 1, 4, 16, 64 clips of 3 s and 10 s.  hipEvents around each whole pass, warm-up passes excluded, median; synthetic
weights (the timing does not depend on their values).  Prints one line per case and a JSON list at the end.

    python tools/ref_batch_time.py [--reps 5] [--ns 1,4,16,64] [--secs 3,10] [--only hubert|sv] [--batch-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import torch  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ns", default="1,4,16,64")
    ap.add_argument("--secs", default="3,10")
    ap.add_argument("--only", default="")
    ap.add_argument("--batch-only", action="store_true", help="skip the sequential calls (for a rocprofv3 kernel split)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ns = [int(v) for v in args.ns.split(",")]
    secs = [float(v) for v in args.secs.split(",")]
    rows = []
    if args.only in ("", "hubert"):
        from gsv_tts_lite_amd.hubert import CNHubertNative
        cfg = synth.hubert_config()
        m = CNHubertNative(synth.hubert_weights(cfg), cfg, dev)
        for s in secs:
            for n in ns:
                wavs = [torch.from_numpy(synth.synth_wav16k(i, s)).to(dev) for i in range(n)]
                seq = float("nan") if args.batch_only else _median_ms(lambda: [m.prompt_ssl(w) for w in wavs], args.reps,
                                                                        args.warmup)
                bat = _median_ms(lambda: m.prompt_ssl_batch(wavs), args.reps, args.warmup)
                rows.append(dict(model="hubert prompt_ssl", seconds=s, n=n, seq_ms=round(seq, 3), batch_ms=round(bat, 3),
                                 seq_ms_per_clip=round(seq / n, 3), batch_ms_per_clip=round(bat / n, 3),
                                 speedup=round(seq / bat, 2)))
                print("hubert prompt_ssl %4.1f s x %2d: sequential %8.2f ms (%.3f / clip), batched %8.2f ms (%.3f / clip), "
                      "x%.2f" % (s, n, seq, seq / n, bat, bat / n, seq / bat), flush=True)
        del m
        torch.cuda.empty_cache()
    if args.only in ("", "sv"):
        from gsv_tts_lite_amd.sv import SVNative
        m = SVNative(synth.sv_weights(), dev)
        for s in secs:
            for n in ns:
                wavs = [torch.from_numpy(synth.synth_audio(i, int(32000 * s))).to(dev) for i in range(n)]
                seq = float("nan") if args.batch_only else _median_ms(lambda: [m.embed(w, 32000) for w in wavs], args.reps,
                                                                        args.warmup)
                bat = _median_ms(lambda: m.embed_batch(wavs, 32000), args.reps, args.warmup)
                rows.append(dict(model="sv embed 32k", seconds=s, n=n, seq_ms=round(seq, 3), batch_ms=round(bat, 3),
                                 seq_ms_per_clip=round(seq / n, 3), batch_ms_per_clip=round(bat / n, 3),
                                 speedup=round(seq / bat, 2)))
                print("sv embed          %4.1f s x %2d: sequential %8.2f ms (%.3f / clip), batched %8.2f ms (%.3f / clip), "
                      "x%.2f" % (s, n, seq, seq / n, bat, bat / n, seq / bat), flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
