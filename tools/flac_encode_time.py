"""Time writing FLAC (flacio.encode_flacs) split into its parts: the host tables and frame headers, the upload of the
packed samples (H2D; numpy input only), the encode call's parts by hipEvents (gsv_flac_encode_timed: table upload,
flac_enc_frames_kernel, scan + copy; the kernel a second time with its CRC-16 as one lane's pass, the yardstick of the
lane-split form, on 16-bit speech and on 24-bit noise, whose VERBATIM frames are the longest), the download of offsets and bytes (D2H) and the whole encode_flacs call for numpy
and for device input.  In the same run, two yardsticks on the same clips: the serial host encoder
(gsv_flac_encode_host) and the WAV fallback of AudioClip.save writing to a tmpfs path.  Host clock around work that ends
in a device synchronise, hipEvents for device parts; warm-up excluded, median.  Clips are synth.synth_audio, 16 bits,
blocks of 4096.  Prints one line per case and a JSON list at the end.

    python tools/flac_encode_time.py [--reps 5] [--ns 1,16,64] [--seconds 10] [--rate 32000]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio, synth  # noqa: E402
from gsv_tts_lite_amd.tts import AudioClip  # noqa: E402

BLOCK, BITS = 4096, 16


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _host_ms(fn, reps, warmup, sync=True):
    for _ in range(warmup):
        fn()
    if sync:
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
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
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=32000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = N.lib()
    timed = L.gsv_flac_encode_timed          # exported for this tool, not declared in the ABI header
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    timed.argtypes = [vp, sz, ctypes.POINTER(N.FlacEncClip), ci, ctypes.POINTER(N.FlacEncFrame), ci, vp, sz, vp, vp, vp, sz, vp, ci,
                      ctypes.POINTER(ctypes.c_float)]
    timed.restype = ci
    st = N.current_stream_ptr(dev)

    def kernel_parts(x, clips, ftab, data, bound, offsets, ws, need, serial):
        parts = []
        for r in range(args.warmup + args.reps):
            ms = (ctypes.c_float * 3)()
            N.check(timed(x.data_ptr(), x.numel(), clips, len(clips), ftab, len(ftab), data.data_ptr(), bound, offsets.data_ptr(),
                          None, ws.data_ptr(), need, st, serial, ms))
            if r >= args.warmup:
                parts.append(list(ms))
        return [_median([p[i] for p in parts]) for i in range(3)]

    n_s = int(args.rate * args.seconds)
    distinct = [synth.synth_audio(i, n_s).astype(np.float32) for i in range(4)]
    tmpfs = "/dev/shm" if os.path.isdir("/dev/shm") else None
    rows = []
    for n in [int(v) for v in args.ns.split(",")]:
        assert 1 <= n <= N.AUX_MAX_CLIPS, "one call covers at most %d clips" % N.AUX_MAX_CLIPS
        waves = [distinct[i % 4] for i in range(n)]
        lengths, rates, bits, blocks = [n_s] * n, [args.rate] * n, [BITS] * n, [BLOCK] * n
        tables = _host_ms(lambda: flacio.enc_tables(lengths, rates, bits, blocks), args.reps, args.warmup, sync=False)
        clips, ftab, _ = flacio.enc_tables(lengths, rates, bits, blocks)
        host = torch.from_numpy(np.concatenate(waves))
        h2d = _event_ms(lambda: host.to(dev), args.reps, args.warmup)
        x = host.to(dev)
        bound = L.gsv_flac_encode_bound(clips, n, ftab, len(ftab))
        need = L.gsv_flac_encode_workspace(clips, n, ftab, len(ftab))
        data = torch.empty(bound, dtype=torch.uint8, device=dev)
        offsets = torch.empty(len(ftab) + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        kern_serial = kernel_parts(x, clips, ftab, data, bound, offsets, ws, need, 1)[1]
        up, kern, scan = kernel_parts(x, clips, ftab, data, bound, offsets, ws, need, 0)
        total = int(offsets[-1])
        # the longest frames there are: 24-bit noise past full scale, every frame VERBATIM
        clips24, ftab24, _ = flacio.enc_tables(lengths, rates, [24] * n, blocks)
        noise = (torch.rand(n * n_s, generator=torch.Generator().manual_seed(n)) * 2.4 - 1.2).to(dev)
        bound24 = L.gsv_flac_encode_bound(clips24, n, ftab24, len(ftab24))
        need24 = L.gsv_flac_encode_workspace(clips24, n, ftab24, len(ftab24))
        data24 = torch.empty(bound24, dtype=torch.uint8, device=dev)
        ws24 = torch.empty(need24, dtype=torch.uint8, device=dev)
        kern24_serial = kernel_parts(noise, clips24, ftab24, data24, bound24, offsets, ws24, need24, 1)[1]
        kern24 = kernel_parts(noise, clips24, ftab24, data24, bound24, offsets, ws24, need24, 0)[1]
        kernel_parts(x, clips, ftab, data, bound, offsets, ws, need, 0)         # `data` and `offsets` hold the speech again

        def down():
            off = offsets.cpu()
            return data[:int(off[-1])].cpu()

        d2h = _host_ms(down, args.reps, args.warmup)
        whole_np = _host_ms(lambda: flacio.encode_flacs(waves, args.rate, bits=BITS, block_size=BLOCK, device=dev), args.reps,
                            args.warmup)
        views = [x[i * n_s:(i + 1) * n_s] for i in range(n)]
        whole_dev = _host_ms(lambda: flacio.encode_flacs(views, args.rate, bits=BITS, block_size=BLOCK, device=dev), args.reps,
                             args.warmup)
        packed = host.numpy()
        hdata, hoff = np.empty(bound, dtype=np.uint8), np.empty(len(ftab) + 1, dtype=np.int64)
        host_enc = _host_ms(lambda: N.check(L.gsv_flac_encode_host(packed.ctypes.data, len(packed), clips, n, ftab, len(ftab),
                                                                   hdata.ctypes.data, bound, hoff.ctypes.data, None)),
                            args.reps, args.warmup, sync=False)
        assert int(hoff[-1]) == total and np.array_equal(hdata[:total], data[:total].cpu().numpy()), "device bytes differ from host bytes"
        with tempfile.TemporaryDirectory(dir=tmpfs) as tmp:
            clipobjs = [AudioClip(None, w, args.rate, args.seconds, None, "") for w in waves]
            wav = _host_ms(lambda: [c.save(os.path.join(tmp, "%d.wav" % i)) for i, c in enumerate(clipobjs)], args.reps,
                           args.warmup, sync=False)
        row = dict(rate=args.rate, seconds=args.seconds, n=n, frames=len(ftab), flac_bytes=total, s16_bytes=n * n_s * 2,
                   ratio=round(total / (n * n_s * 2), 4), tables_headers_ms=round(tables, 3), h2d_ms=round(h2d, 3),
                   table_upload_ms=round(up, 3), encode_kernel_ms=round(kern, 3), encode_kernel_one_lane_crc_ms=round(kern_serial, 3),
                   noise24_kernel_ms=round(kern24, 3), noise24_kernel_one_lane_crc_ms=round(kern24_serial, 3),
                   scan_copy_ms=round(scan, 3), d2h_ms=round(d2h, 3),
                   encode_flacs_numpy_ms=round(whole_np, 3), encode_flacs_device_ms=round(whole_dev, 3),
                   host_encoder_ms=round(host_enc, 3), wav_fallback_ms=round(wav, 3), wav_on_tmpfs=tmpfs is not None)
        rows.append(row)
        print("%2d x %.0f s at %d Hz (%d frames, %.3f of s16): tables+headers %.3f, H2D %.3f, table upload %.3f, encode kernel %.3f, "
              "(one-lane CRC %.3f; 24-bit noise %.3f, one-lane CRC %.3f), scan+copy %.3f, D2H %.3f, encode_flacs %.3f (numpy) %.3f (device) ms; "
              "host encoder %.3f ms; WAV fallback %.3f ms" % (
                  n, args.seconds, args.rate, len(ftab), row["ratio"], tables, h2d, up, kern, kern_serial, kern24, kern24_serial, scan,
                  d2h, whole_np, whole_dev, host_enc, wav), flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
