"""Time the segmented vocoder call against the scalar one on a time-concatenated batch of ten utterances totalling 10 s
(250 tokens, per-token ge, slice_indices; random weights, v2Pro): device time of gsv_voc_decode at speed 1.3 and of
gsv_voc_decode_segments with ten speeds, through the C ABI with preallocated workspaces -- hipEvents, warm-up excluded,
median.  With --kernels the same calls run once more in a child process under `rocprofv3 --kernel-trace --stats`, and the
average time of dec_segments_kernel is printed beside the three launches it replaces (resample_linear_kernel,
dec_zp_kernel, dec_ge_frames_kernel).  Prints one line per figure and a JSON object at the end.

    python tools/decode_segments_time.py [--reps 5] [--warmup 2] [--dtype bfloat16] [--kernels]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.batchmath import segment_frames  # noqa: E402

LENGTHS = [16, 18, 20, 22, 24, 26, 28, 30, 32, 34]                      # 250 tokens = 10 s at 25 Hz
SPEEDS = [0.8, 0.9, 1.0, 1.05, 1.1, 1.15, 1.2, 1.25, 1.3, 1.4]
PHONES = 12
KERNELS = ("dec_segments_kernel", "resample_linear_kernel", "dec_zp_kernel", "dec_ge_frames_kernel")


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


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


def _calls(dev, dtype):
    """the two calls as closures over preallocated buffers"""
    from gsv_tts_lite_amd.sovits import SynthesizerTrn
    hps = synth.sovits_hps("v2Pro")
    vq = SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    vq.load_state_dict(synth.sovits_weights(hps, seed=7))
    vq.initialize_runtime(dtype, dev, [])
    L, h, hop = N.lib(), vq._voc._h, vq.samples_per_frame
    rng = np.random.default_rng(1)
    n, P = sum(LENGTHS), PHONES * len(LENGTHS)
    codes = torch.from_numpy(rng.integers(0, 1024, n)).to(dev)
    text = torch.from_numpy(rng.integers(1, 700, P)).to(dev)
    ge = torch.cat([torch.from_numpy(synth.synth_ge(k, 1024, 7))[0].expand(-1, l) for k, l in enumerate(LENGTHS)], 1).to(dev).contiguous()
    sl = torch.tensor([[k * PHONES, (k + 1) * PHONES] for k, l in enumerate(LENGTHS) for _ in range(2 * l)], device=dev)
    st = N.current_stream_ptr(dev)
    attn = torch.empty(4, 2 * n, P, dtype=torch.float32, device=dev)
    # scalar: one speed for the whole concatenation
    T_scalar = int(2 * n / 1.3) + 1
    need = L.gsv_voc_decode_workspace(h, n, P, n, T_scalar, 0)
    ws1 = torch.empty(need, dtype=torch.uint8, device=dev)
    out1 = torch.empty(T_scalar * hop, dtype=torch.float32, device=dev)

    def scalar():
        N.check(L.gsv_voc_decode(h, codes.data_ptr(), n, text.data_ptr(), P, ge.data_ptr(), n, sl.data_ptr(), 0.5, 1234, T_scalar, 0, 0, 0, 0, 0,
                                 out1.data_ptr(), attn.data_ptr(), ws1.data_ptr(), ws1.numel(), st))
    # segmented: ten speeds
    frames = segment_frames(LENGTHS, SPEEDS)
    table = (N.VocSegment * len(LENGTHS))(*[N.VocSegment(l, f, 0.5, 1234 + k) for k, (l, (f, _)) in enumerate(zip(LENGTHS, frames))])
    T_seg = sum(f for f, _ in frames)
    need = L.gsv_voc_decode_segments_workspace(h, n, P, n, table, len(LENGTHS))
    assert need > 0
    ws2 = torch.empty(need, dtype=torch.uint8, device=dev)
    out2 = torch.empty(T_seg * hop, dtype=torch.float32, device=dev)

    def segmented():
        N.check(L.gsv_voc_decode_segments(h, codes.data_ptr(), n, text.data_ptr(), P, ge.data_ptr(), n, sl.data_ptr(), table, len(LENGTHS),
                                          out2.data_ptr(), attn.data_ptr(), ws2.data_ptr(), ws2.numel(), st))
    return vq, scalar, segmented, T_scalar, T_seg


def _kernel_stats(args):
    """average ns per launch of the kernels of interest, from a rocprofv3 kernel trace of a child process that makes both calls"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--reps", str(args.reps), "--warmup", str(args.warmup), "--dtype", args.dtype]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        if r.returncode != 0:
            return {"error": "rocprofv3 exited with %d" % r.returncode, "tail": r.stdout.decode(errors="replace")[-400:]}
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row.get("Name", "")
                    for k in KERNELS:
                        if k in name:
                            out[k] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        return out or {"error": "no kernel_stats.csv under the profiler's output directory"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--kernels", action="store_true", help="also trace the kernels in a child process under rocprofv3")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vq, scalar, segmented, T_scalar, T_seg = _calls(dev, getattr(torch, args.dtype))
    if args.child:      # under the profiler: the same launches, no timing
        for _ in range(args.reps):
            scalar()
            segmented()
        torch.cuda.synchronize()
        return
    res = dict(dtype=args.dtype, utterances=len(LENGTHS), tokens=sum(LENGTHS), frames_scalar=T_scalar, frames_segmented=T_seg, reps=args.reps)
    res["decode_ms"] = round(_event_ms(scalar, args.reps, args.warmup), 4)
    res["decode_segments_ms"] = round(_event_ms(segmented, args.reps, args.warmup), 4)
    res["decode_ms_again"] = round(_event_ms(scalar, args.reps, 0), 4)          # the spread between two runs of the same call
    print("gsv_voc_decode (speed 1.3, %d frames): %.3f ms (again %.3f); gsv_voc_decode_segments (ten speeds, %d frames): %.3f ms"
          % (T_scalar, res["decode_ms"], res["decode_ms_again"], T_seg, res["decode_segments_ms"]), flush=True)
    res["ms_per_frame"] = dict(decode=round(res["decode_ms"] / T_scalar, 6), decode_segments=round(res["decode_segments_ms"] / T_seg, 6))
    if args.kernels:
        del vq
        res["kernels"] = k = _kernel_stats(args)
        if "error" in k:
            print("kernel trace: %s" % k["error"], flush=True)
        else:
            three = sum(k[n]["avg_us"] for n in KERNELS[1:] if n in k)
            print("dec_segments_kernel %.2f us against %.2f us for the three launches it replaces (%s)"
                  % (k.get(KERNELS[0], {}).get("avg_us", float("nan")), three,
                     ", ".join("%s %.2f" % (n, k[n]["avg_us"]) for n in KERNELS[1:] if n in k)), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
