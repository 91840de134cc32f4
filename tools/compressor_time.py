"""Time the compressor (csrc/compressor.h) on the GPU, beside the equaliser.

The device time of ONE gsv_compressor call -- the upload of the rows, parameters and powers and all launches, the "voice" preset out
of place -- with hipEvents around it: the median of --calls calls after a warm-up, with the lowest and highest beside it, for

    one 10 s clip at 32 kHz,    32 x 10 s packed,

and, in the same run on the same card, one gsv_eq call with its "voice" preset over the same clips: three sections, so three scans
of two values per pass where the compressor runs one of two values and one of one.  A JSON object with everything comes last.
There is no CPU path: without a GPU the tool fails.

    python tools/compressor_time.py [--calls 5]
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
from gsv_tts_lite_amd import eq as EQM  # noqa: E402

RATE = 32000
CASES = [("1 x 10 s", 1, 10), ("32 x 10 s", 32, 10)]


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
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compressor_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    L = N.lib()
    co = CM.Compressor.preset("voice").coefficients(RATE)
    eco = EQM.design(EQM.EQ.preset("voice", RATE), RATE)
    res = dict(calls=args.calls, rate=RATE, cases={})
    for name, clips, seconds in CASES:
        n = seconds * RATE
        rng = np.random.default_rng(5)
        # every clip well above the preset's threshold (0.126), so the gain's log2 and exp2 run for nearly every sample
        x0 = torch.from_numpy((rng.uniform(-1.0, 1.0, clips * n) * np.repeat(rng.uniform(0.5, 1.0, clips), n)).astype(np.float32)).to(dev)
        stream = N.current_stream_ptr(dev)
        offsets, lengths = [c * n for c in range(clips)], [n] * clips
        y = torch.empty_like(x0)

        tab, par = CM._tables(offsets, lengths, [0] * clips, [co])
        need = L.gsv_compressor_work_bytes(tab, clips, par, 1)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        rec = torch.empty(clips * CM.RECORD_BYTES, dtype=torch.uint8, device=dev)

        def cmp_call():
            N.check(L.gsv_compressor(x0.data_ptr(), x0.numel(), tab, clips, par, 1, y.data_ptr(), rec.data_ptr(), work.data_ptr(), need, stream))
        r = timed(cmp_call, args.calls, dev)
        recs = CM.records(rec)
        r.update(workspace_bytes=int(need), chunks_per_clip=-(-n // CM.CHUNK), peak_in=float(recs[0].peak_in), peak_out=float(recs[0].peak_out),
                 min_gain=float(recs[0].min_gain), clips_compressed=sum(int(v.compressed) for v in recs))

        etab, edes = EQM._tables(offsets, lengths, [0] * clips, [eco])
        eneed = L.gsv_eq_work_bytes(etab, clips, edes, 1)
        ework = torch.empty(eneed, dtype=torch.uint8, device=dev)
        erec = torch.empty(clips * EQM.RECORD_BYTES, dtype=torch.uint8, device=dev)

        def eq_call():
            N.check(L.gsv_eq(x0.data_ptr(), x0.numel(), etab, clips, edes, 1, y.data_ptr(), erec.data_ptr(), ework.data_ptr(), eneed, stream))
        r["eq"] = timed(eq_call, args.calls, dev)
        res["cases"][name] = r
        print("%-10s gsv_compressor %9.2f us [%9.2f, %9.2f]   gsv_eq %9.2f us [%9.2f, %9.2f]   (peak %.3f -> %.3f, min gain %.3f)" % (
            name, r["median_us"], r["low_us"], r["high_us"], r["eq"]["median_us"], r["eq"]["low_us"], r["eq"]["high_us"], r["peak_in"],
            r["peak_out"], r["min_gain"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
