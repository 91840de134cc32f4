"""Time CN-HuBERT's prompt_ssl (gsv_hubert_forward, + 0.3 s pad) on the device for 3 s and 10 s prompts: hipEvents
around each call, warm-up calls excluded, synthetic weights (the timing does not depend on their values).

    python tools/hubert_time.py [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import torch  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.hubert import CNHubertNative  # noqa: E402


def flops(cfg, n):
    """multiply-adds x 2 of the convs, projections, attention (QK^T and PV) and FFN for n input samples"""
    f, T = 0, n
    cin = 1
    for d, k, s in zip(cfg["conv_dim"], cfg["conv_kernel"], cfg["conv_stride"]):
        T = (T - k) // s + 1
        f += 2 * T * d * cin * k
        cin = d
    H, F, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    kpos, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    f += 2 * T * H * cin + 2 * T * H * (H // G) * kpos
    f += L * (2 * T * H * (4 * H + 2 * F) + 4 * T * T * H)
    return f, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.hubert_config()
    m = CNHubertNative(synth.hubert_weights(cfg), cfg, dev)
    rows = []
    for secs in (3.0, 10.0):
        wav = torch.from_numpy(synth.synth_wav16k(0, secs)).to(dev)
        for _ in range(args.warmup):
            m.prompt_ssl(wav)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m.prompt_ssl(wav)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        fl, Th = flops(cfg, int(16000 * secs) + 4800)
        med = times[len(times) // 2]
        rows.append(dict(seconds=secs, Th=Th, ms_median=round(med, 3), ms_min=round(times[0], 3), gflop=round(fl / 1e9, 1),
                         tflops=round(fl / med / 1e9, 1)))
        print("prompt_ssl %4.1f s (Th %d): median %.3f ms, min %.3f ms over %d calls; %.1f GFLOP -> %.1f TFLOP/s" % (
            secs, Th, med, times[0], args.reps, fl / 1e9, fl / med / 1e9))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
