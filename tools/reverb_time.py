"""Time the reverb (csrc/reverb.h) on the GPU, beside the compressor.

The device time of ONE gsv_reverb call -- the upload of the rows, parameters and powers and all seven launches, the "voice" preset out
of place -- with hipEvents around it: the median of --calls calls after a warm-up, with the lowest and highest beside it, for

    one 10 s clip at 32 kHz,    16 x 10 s packed,

and, in the same run on the same card, one gsv_compressor call with its "voice" preset over the same clips.  The first clip of the
device's output is compared with the host twin's, byte for byte, so that what is timed is known to be the call that is tested.  A
JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/reverb_time.py [--calls 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import compressor as CM  # noqa: E402
from gsv_tts_lite_amd import reverb as RV  # noqa: E402

RATE = 32000
CASES = [("1 x 10 s", 1, 10), ("16 x 10 s", 16, 10)]


def timed(call, calls, dev):
    for _ in range(10):
        call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2), high_us=round(1e3 * ms[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reverb_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    L = N.lib()
    voice = RV.Reverb.preset("voice").parameters(RATE)
    co = CM.Compressor.preset("voice").coefficients(RATE)
    delays = [int(v) for v in voice[0]]
    res = dict(calls=args.calls, rate=RATE, comb_delays=delays[:8], allpass_delays=delays[8:], cases={})
    for name, clips, seconds in CASES:
        n = seconds * RATE
        rng = np.random.default_rng(5)
        host = (rng.uniform(-1.0, 1.0, clips * n) * np.repeat(rng.uniform(0.5, 1.0, clips), n)).astype(np.float32)
        x0 = torch.from_numpy(host).to(dev)
        stream = N.current_stream_ptr(dev)
        offsets, lengths = [c * n for c in range(clips)], [n] * clips
        y = torch.empty_like(x0)

        tab, par = RV._tables(offsets, lengths, [0] * clips, [voice])
        need = L.gsv_reverb_work_bytes(tab, clips, par, 1)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        rec = torch.empty(clips * RV.RECORD_BYTES, dtype=torch.uint8, device=dev)

        def rvb_call():
            N.check(L.gsv_reverb(x0.data_ptr(), x0.numel(), tab, clips, par, 1, y.data_ptr(), rec.data_ptr(), work.data_ptr(), need, stream))
        r = timed(rvb_call, args.calls, dev)
        recs = RV.records(rec)
        first = torch.from_numpy(host[:n].copy())
        twin = torch.empty_like(first)
        twin_rec = RV.run_packed(first, [0], [n], [0], [voice], twin)
        same = y[:n].cpu().numpy().tobytes() == twin.numpy().tobytes() and rec[: RV.RECORD_BYTES].cpu().numpy().tobytes() == twin_rec.numpy().tobytes()
        r.update(workspace_bytes=int(need), comb_blocks_per_clip=[-(-n // d) for d in delays[:8]], allpass_steps_per_phase=[-(-n // d) for d in delays[8:]],
                 peak_in=float(recs[0].peak_in), peak_out=float(recs[0].peak_out), clips_reverbed=sum(int(v.reverbed) for v in recs),
                 first_clip_equals_host_twin=bool(same))

        ctab, cpar = CM._tables(offsets, lengths, [0] * clips, [co])
        cneed = L.gsv_compressor_work_bytes(ctab, clips, cpar, 1)
        cwork = torch.empty(cneed, dtype=torch.uint8, device=dev)
        crec = torch.empty(clips * CM.RECORD_BYTES, dtype=torch.uint8, device=dev)

        def cmp_call():
            N.check(L.gsv_compressor(x0.data_ptr(), x0.numel(), ctab, clips, cpar, 1, y.data_ptr(), crec.data_ptr(), cwork.data_ptr(), cneed, stream))
        r["compressor"] = timed(cmp_call, args.calls, dev)
        res["cases"][name] = r
        print("%-10s gsv_reverb %9.2f us [%9.2f, %9.2f]   gsv_compressor %9.2f us [%9.2f, %9.2f]   (peak %.3f -> %.3f, equals the host twin: %s)" % (
            name, r["median_us"], r["low_us"], r["high_us"], r["compressor"]["median_us"], r["compressor"]["low_us"], r["compressor"]["high_us"],
            r["peak_in"], r["peak_out"], same), flush=True)
    print(json.dumps(res))
    if not all(c["first_clip_equals_host_twin"] for c in res["cases"].values()):
        raise SystemExit("reverb_time: the device's output differs from the host twin's")


if __name__ == "__main__":
    main()
