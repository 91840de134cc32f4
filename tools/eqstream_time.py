"""Time the stream equaliser (csrc/eqstream.h) on the GPU.

The device time of ONE gsv_eqstream_push (its four launches, in place) of a 16 000-sample chunk at 32 kHz with hipEvents around it
-- the median of --calls calls after a warm-up, with the lowest and highest beside it -- in the middle of a stream whose state is
put back before every call, so every call does the same work: with the three sections of the "voice" preset and with six.  Beside
it, in the same process and on the same chunk: gsv_eq over the chunk as one clip (the work a push repeats, without the rerun of the
open chunk), gsv_level_push (in place) and gsv_track_push (32 -> 48 kHz), which sit next to it in a stream.

Then the chunk epilogue as TTS.infer_stream_batched issues it: stream.ChunkEmitter.push of a vocoded chunk of that length (emit,
level, limit, track and the asynchronous copy) with and without the equaliser in front, hipEvents around the push, the same way.

A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/eqstream_time.py [--calls 100] [--samples 16000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import eq as EQM  # noqa: E402
from gsv_tts_lite_amd import level as LV  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402
from gsv_tts_lite_amd.stream import ChunkEmitter  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402

RATE = 32000
SIX = EQM.EQ([EQM.Band("highpass", 20.0, q=0.5), EQM.Band("lowshelf", 120.0, q=0.7, gain_db=4.0), EQM.Band("peak", 300.0, q=1.0, gain_db=2.5),
              EQM.Band("peak", 2500.0, q=4.0, gain_db=-6.0), EQM.Band("highshelf", 6000.0, q=0.8, gain_db=3.0), EQM.Band("lowpass", 14400.0)])


def _timed(call, calls, dev, before=None, after=None):
    ms = []
    for k in range(10 + calls):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        e1.synchronize()
        if after:
            after(got)
        if k >= 10:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return dict(median_us=round(1e3 * ms[len(ms) // 2], 2), low_us=round(1e3 * ms[0], 2), high_us=round(1e3 * ms[-1], 2))


def _show(name, r):
    print("%-64s %9.2f us [%9.2f, %9.2f]" % (name, r["median_us"], r["low_us"], r["high_us"]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=16000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eqstream_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    n = args.samples
    sig = np.random.default_rng(3).standard_normal(2 * n).astype(np.float32) * 0.25
    x = torch.from_numpy(sig).to(dev)
    chunk = x[n:].clone()
    res = dict(calls=args.calls, samples=n, push={}, epilogue={})
    for name, e in (("voice, 3 sections", EQM.EQ.preset("voice", RATE)), ("6 sections", SIX)):
        st = EQM.StreamEQ(e, RATE, dev)
        st.push_tensor(x[:n])                                      # the first half: the timed push is in the middle of a stream
        start = st.state.clone()
        buf = chunk.clone()
        rec = torch.empty(4, dtype=torch.int64, device=dev)

        def put_back():
            st.state.copy_(start)
            buf.copy_(chunk)
        key = "eqstream push %d samples in place: %s" % (n, name)
        res["push"][key] = _show(key, _timed(lambda: st.enqueue(buf.data_ptr(), n, None, False, buf.data_ptr(), rec.data_ptr()),
                                             args.calls, dev, put_back))
        r = EQM.stream_record(rec.view(torch.uint8))
        print("    emitted %d, total %d, peak out %.4f" % (r.emitted, r.total, float(r.peak_out_run)), flush=True)
        out = torch.empty(n, device=dev)
        work = torch.empty(EQM.work_bytes([n], 1), dtype=torch.uint8, device=dev)
        crec = torch.empty(EQM.RECORD_BYTES, dtype=torch.uint8, device=dev)
        co = [EQM.design(e, RATE)]
        key = "gsv_eq over the same chunk as one clip: %s" % name
        res["push"][key] = _show(key, _timed(lambda: EQM.run_packed(chunk, [0], [n], [0], co, out, crec, work), args.calls, dev))
    lv = LV.StreamLeveller(-18.0, RATE, dev)
    lv.push_tensor(x[:n])
    lstart = lv.state.clone()
    y, lrec = torch.empty(n, device=dev), torch.empty(5, dtype=torch.int64, device=dev)
    key = "level push %d samples (same chunk)" % n
    res["push"][key] = _show(key, _timed(lambda: lv.enqueue(chunk.data_ptr(), n, None, False, y.data_ptr(), lrec.data_ptr()),
                                         args.calls, dev, lambda: lv.state.copy_(lstart)))
    rs = TrackResampler(TrackFormat(48000, 1, 20), RATE, dev)
    pcm, trec = torch.empty(rs.capacity(n), dtype=torch.int16, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    key = "track push %d samples, 32 -> 48 kHz (same chunk)" % n
    res["push"][key] = _show(key, _timed(lambda: rs.enqueue(chunk.data_ptr(), n, None, False, pcm.data_ptr(), trec.data_ptr()),
                                         args.calls, dev))
    # the chunk epilogue: every push is the first chunk of a segment (no splice search), the streams run on
    make = lambda **kw: ChunkEmitter(640, track=TrackResampler(TrackFormat(48000, 1, 20), RATE, dev), level=LV.StreamLeveller(-18.0, RATE, dev),
                                     limit=LM.StreamLimiter(-1.0, RATE, dev), **kw)
    for name, em in (("emit + level + limit + track", make()),
                     ("emit + eq (voice) + level + limit + track", make(eq=EQM.StreamEQ("voice", RATE, dev))),
                     ("emit alone", ChunkEmitter(640)), ("emit + eq (voice)", ChunkEmitter(640, eq=EQM.StreamEQ("voice", RATE, dev)))):
        key = "epilogue of a %d-sample chunk: %s" % (n, name)
        res["epilogue"][key] = _show(key, _timed(lambda: em.push(chunk, False), args.calls, dev, em.new_segment, lambda h: h.result()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
