"""Time the speaker-verification path on the device for 3 s / 10 s / 30 s of 32 kHz reference audio: gsv_sv_resample
(32 k -> 16 k), gsv_sv_fbank, gsv_sv_forward (ERes2NetV2.forward3) and the one-call gsv_sv_embed.  hipEvents around each
call, warm-up calls excluded, synthetic weights (the timing does not depend on their values).  The FLOP split below is
per stage (stem + layer1, layer2, layer3, layer4, layer3_ds + fuse34).

    python tools/sv_time.py [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import torch  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.sv import SVNative  # noqa: E402


def flops(T, m=64, blocks=(3, 4, 6, 3), width=(24, 48, 96, 192)):
    """multiply-adds x 2 of every conv forward3 runs on T fbank frames, per stage"""
    F, t = 80, T
    out = {"stage1": 2 * F * t * m * 9}
    cin = m
    for s in range(4):
        if s:
            F, t = (F + 1) // 2, (t + 1) // 2
        P, w = m << s, width[s]
        f = 0
        for b in range(blocks[s]):
            px = F * t
            f += 2 * px * cin * 4 * w + 4 * 2 * px * w * w * 9 + 2 * px * 4 * w * 4 * P
            if b == 0:
                f += 2 * px * cin * 4 * P
            if s >= 2:
                f += 3 * (2 * px * 2 * w * (w // 4) + 2 * px * (w // 4) * w)
            cin = 4 * P
        out["stage%d" % (s + 1)] = out.get("stage%d" % (s + 1), 0) + f
    px = F * t
    out["ds_fuse"] = 2 * px * 16 * m * 9 * 32 * m + 2 * px * 64 * m * 8 * m + 2 * px * 8 * m * 32 * m
    return out


def timed(fn, reps, warmup):
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
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = SVNative(synth.sv_weights(), dev)
    rows = []
    for secs in (3.0, 10.0, 30.0):
        wav = torch.from_numpy(synth.synth_audio(0, int(32000 * secs))).to(dev)
        wav16 = m.resample(wav, 32000)
        feat = m.fbank(wav16)
        T = feat.shape[0]
        fl = flops(T)
        total = sum(fl.values())
        r = dict(seconds=secs, frames=T, gflop=round(total / 1e9, 1),
                 gflop_split={k: round(v / 1e9, 1) for k, v in fl.items()})
        for name, fn in (("resample", lambda: m.resample(wav, 32000)), ("fbank", lambda: m.fbank(wav16)),
                         ("forward3", lambda: m.forward3(feat)), ("embed", lambda: m.embed(wav, 32000))):
            med, mn = timed(fn, args.reps, args.warmup)
            r[name + "_ms"] = round(med, 3)
            r[name + "_ms_min"] = round(mn, 3)
        r["forward3_tflops"] = round(total / r["forward3_ms"] / 1e9, 1)
        rows.append(r)
        print("sv %4.1f s (T %d): resample %.3f ms, fbank %.3f ms, forward3 %.3f ms (%.1f GFLOP -> %.1f TFLOP/s), "
              "embed %.3f ms" % (secs, T, r["resample_ms"], r["fbank_ms"], r["forward3_ms"], total / 1e9,
                                 r["forward3_tflops"], r["embed_ms"]))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
