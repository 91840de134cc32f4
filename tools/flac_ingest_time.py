"""Time reference-audio ingest from FLAC files (flacio.load_flacs) split into its parts, next to wavio.load_wavs of the
same integers as s16 WAV files in the same run: the host parse + frame index, the upload of the packed frames (H2D), the
decode call (gsv_flac_decode: table upload, flac_frames_kernel, mono conversion), the conversion alone
(gsv_wav_to_mono_batch over an s32 buffer of the same shape; the frames kernel is the decode call minus it) and the
whole load_flacs / load_wavs calls.  Host clock around work that ends in a device synchronise for the parse and the whole
calls, hipEvents for upload / decode / conversion; warm-up excluded, median.  Files are 16 bits, block 4096, LPC order 8
with one Rice parameter per frame chosen from the residual (tests/flac_writer.py; up to 4 distinct clips, repeated).
Prints one line per case and a JSON list at the end.

    python tools/flac_ingest_time.py [--reps 5] [--ns 1,16,64] [--cases 16000x1x3,44100x2x10]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flac_writer as fw  # noqa: E402
import wav_writer as ww  # noqa: E402
from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio, synth, wavio  # noqa: E402

BLOCK = 4096


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


def _write_pair(stem, x, rate):
    coefs = fw.default_coefs(8, 12, 10)

    def sub(k):
        blk = x[k * BLOCK:(k + 1) * BLOCK]
        if len(blk) <= 8:
            return fw.Sub("verbatim")
        r = np.abs(fw._residual(blk[:, 0], coefs, 10)).mean()
        return fw.Sub("lpc", order=8, precision=12, shift=10, coefs=coefs, method=0, params=int(min(14, max(0, np.ceil(np.log2(r + 1))))))

    return (fw.write(stem + ".flac", x, 16, rate, block_size=BLOCK, sub=sub, assignment="indep"),
            ww.write(stem + ".wav", x, "s16", rate))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ns", default="1,16,64")
    ap.add_argument("--cases", default="16000x1x3,44100x2x10", help="rate x channels x seconds, 16 bits")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = N.lib()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in args.cases.split(","):
            rate, ch, secs = int(case.split("x")[0]), int(case.split("x")[1]), float(case.split("x")[2])
            n_s = int(rate * secs)
            distinct = []
            for i in range(4):
                w = np.stack([synth.synth_audio(i + c, n_s) for c in range(ch)], axis=1)
                distinct.append(_write_pair(os.path.join(tmp, "%s_d%d" % (case, i)), np.round(w * 32767).astype(np.int64), rate))
            for n in [int(v) for v in args.ns.split(",")]:
                assert 1 <= n <= N.AUX_MAX_CLIPS, "one call covers at most %d clips" % N.AUX_MAX_CLIPS
                flacs, wavs = [], []
                for i in range(n):
                    f, w = os.path.join(tmp, "%s_%d.flac" % (case, i)), os.path.join(tmp, "%s_%d.wav" % (case, i))
                    shutil.copyfile(distinct[i % 4][0], f)
                    shutil.copyfile(distinct[i % 4][1], w)
                    flacs.append(f)
                    wavs.append(w)
                parse = _host_ms(lambda: [flacio.parse_flac(p) for p in flacs], args.reps, args.warmup)
                parsed = [flacio.parse_flac(p) for p in flacs]
                packed, clips, ftab, _ = flacio.tables(parsed)
                host = torch.frombuffer(packed, dtype=torch.uint8)
                h2d = _event_ms(lambda: host.to(dev), args.reps, args.warmup)
                data = host.to(dev)
                out = torch.empty(n * n_s, dtype=torch.float32, device=dev)
                status = torch.empty(len(ftab), dtype=torch.int32, device=dev)
                need = L.gsv_flac_decode_workspace(clips, n, len(ftab))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                st = N.current_stream_ptr(dev)
                dec = _event_ms(lambda: N.check(L.gsv_flac_decode(data.data_ptr(), len(packed), clips, n, ftab, len(ftab),
                                                                  out.data_ptr(), status.data_ptr(), ws.data_ptr(), need, st)),
                                args.reps, args.warmup)
                assert not status.cpu().any()
                s32 = torch.zeros(n * n_s * ch, dtype=torch.int32, device=dev)
                wclips = (N.WavClip * n)(*[N.WavClip(k * n_s * ch * 4, n_s, N.PCM_S32, ch) for k in range(n)])
                conv = _event_ms(lambda: N.check(L.gsv_wav_to_mono_batch(s32.data_ptr(), s32.numel() * 4, wclips, n, out.data_ptr(),
                                                                         st)), args.reps, args.warmup)
                whole = _host_ms(lambda: flacio.load_flacs(flacs, dev), args.reps, args.warmup)
                wav = _host_ms(lambda: wavio.load_wavs(wavs, dev), args.reps, args.warmup)
                row = dict(rate=rate, channels=ch, seconds=secs, n=n, frames=len(ftab), flac_bytes_per_clip=len(packed) // n,
                           s16_bytes_per_clip=n_s * ch * 2, parse_index_ms=round(parse, 3), h2d_ms=round(h2d, 3),
                           decode_call_ms=round(dec, 3), conversion_ms=round(conv, 3), frames_kernel_ms=round(dec - conv, 3),
                           load_flacs_ms=round(whole, 3), load_wavs_ms=round(wav, 3))
                rows.append(row)
                print("%5d Hz x%d %4.1f s x %2d (%d frames, %.2f of s16): parse+index %.3f, H2D %.3f, frames %.3f, conversion %.3f, "
                      "load_flacs %.3f ms; load_wavs %.3f ms" % (rate, ch, secs, n, len(ftab), len(packed) / n / (n_s * ch * 2), parse,
                                                                 h2d, dec - conv, conv, whole, wav), flush=True)
                for p in flacs + wavs:
                    os.remove(p)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
