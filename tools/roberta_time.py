"""Time Chinese RoBERTa's hidden_states[-3] (gsv_roberta_forward over packed texts) on the device for 1 x 32, 1 x 128,
1 x 512 and 20 x 40 tokens: hipEvents around each call, warm-up calls excluded, ids uploaded once outside the timed
region, full-size synthetic weights (the timing does not depend on their values).

    python tools/roberta_time.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import torch  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.roberta import CNRobertaNative, WordPieceTokenizer  # noqa: E402

SHAPES = [(1, 32), (1, 128), (1, 512), (20, 40)]


def flops(cfg, lens):
    """multiply-adds x 2 of the run layers' GEMMs and attention (QK^T and PV)"""
    H, F, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"] - 2
    return sum(L * (2 * T * H * (4 * H + 2 * F) + 4 * T * T * H) for T in lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.roberta_config()
    tok = WordPieceTokenizer(synth.roberta_tokenizer_json()["model"]["vocab"])
    m = CNRobertaNative(synth.roberta_weights(cfg, run_only=True), cfg, tok, dev)
    wbytes = 4 * sum(int(torch.tensor(s).prod()) for n, s in synth.roberta_spec(cfg, run_only=True).items()
                     if n.startswith("encoder."))
    rows = []
    for n, T in SHAPES:
        batch = [[101] + synth.hashed_ints("t%d" % i, T - 2, 5, 21128).tolist() + [102] for i in range(n)]
        ids_t, starts_t, starts, max_len = m._pack(batch)
        out = torch.empty(starts[-1], m.hidden_size, device=dev)
        L = N.lib()

        def call():
            N.check(L.gsv_roberta_forward(m._h, ids_t.data_ptr(), starts_t.data_ptr(), n, starts[-1], max_len, out.data_ptr(),
                                          m._ws.data_ptr(), m._ws.numel(), N.current_stream_ptr(dev)))
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        fl = flops(cfg, [T] * n)
        med = times[len(times) // 2]
        rows.append(dict(texts=n, tokens=T, ms_median=round(med, 3), ms_min=round(times[0], 3), gflop=round(fl / 1e9, 2),
                         tflops=round(fl / med / 1e9, 1), weight_tb_s=round(wbytes / med / 1e9, 2)))
        print("%2d x %3d tokens: median %.3f ms, min %.3f ms over %d calls; %.1f GFLOP -> %.1f TFLOP/s; %.2f GB of layer "
              "weights -> %.2f TB/s" % (n, T, med, times[0], args.reps, fl / 1e9, fl / med / 1e9, wbytes / 1e9, wbytes / med / 1e9))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
