"""Time the stream compressor (csrc/cmpstream.h) on the GPU.

The device time of ONE gsv_cmpstream_push (its six launches, in place) of a 16 000-sample chunk at 32 kHz with hipEvents around it
-- the median of --calls calls after a warm-up, with the lowest and highest beside it -- in the middle of a stream whose state is
put back before every call, so every call does the same work: with the "voice" preset over a signal that drives it.  The push
starts 16 000 samples into the stream, so it reruns the kept samples of the open chunk, completes that chunk (the three passes
and both chains) and leaves the next one open.  Beside it, in the same process and on the same chunk: gsv_eqstream_push with the
"voice" equaliser (the same plan, two passes), gsv_compressor over the chunk as one clip, and a compressor push that completes no
chunk (384 samples into a fresh chunk: the full pass alone does work).

Then the chunk epilogue as TTS.infer_stream_batched issues it: stream.ChunkEmitter.push of a vocoded chunk of that length with and
without the compressor, hipEvents around the push, the same way.

A JSON object with everything comes last.  There is no CPU path: without a GPU the tool fails.

    python tools/cmpstream_time.py [--calls 100] [--samples 16000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import compressor as CM  # noqa: E402
from gsv_tts_lite_amd import eq as EQM  # noqa: E402
from gsv_tts_lite_amd import level as LV  # noqa: E402
from gsv_tts_lite_amd import limiter as LM  # noqa: E402
from gsv_tts_lite_amd.stream import ChunkEmitter  # noqa: E402
from gsv_tts_lite_amd.track import TrackFormat, TrackResampler  # noqa: E402

RATE = 32000


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
    print("%-72s %9.2f us [%9.2f, %9.2f]" % (name, r["median_us"], r["low_us"], r["high_us"]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=16000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cmpstream_time: no GPU -- nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    n = args.samples
    sig = np.random.default_rng(3).standard_normal(2 * n).astype(np.float32) * 0.25        # about -12 dBFS: over the preset's threshold
    x = torch.from_numpy(sig).to(dev)
    chunk = x[n:].clone()
    res = dict(calls=args.calls, samples=n, push={}, epilogue={})

    def push_of(st, rec_words, head, name):
        """one in-place push of `chunk` behind `head` samples of the stream, the state put back before every call"""
        st.push_tensor(x[:head], flush=False)
        start = st.state.clone()
        buf = chunk.clone()
        rec = torch.empty(rec_words, dtype=torch.int64, device=dev)

        def put_back():
            st.state.copy_(start)
            buf.copy_(chunk)
        res["push"][name] = _show(name, _timed(lambda: st.enqueue(buf.data_ptr(), int(buf.numel()), None, False, buf.data_ptr(), rec.data_ptr()),
                                               args.calls, dev, put_back))
        return rec

    rec = push_of(CM.StreamCompressor("voice", RATE, dev), 5, n, "cmpstream push %d samples in place: voice" % n)
    r = CM.stream_record(rec.view(torch.uint8))
    print("    emitted %d, total %d, smallest gain %.4f" % (r.emitted, r.total, float(r.min_gain_run)), flush=True)
    push_of(EQM.StreamEQ("voice", RATE, dev), 4, n, "eqstream push %d samples in place: voice, 3 sections" % n)
    out = torch.empty(n, device=dev)
    co = [CM.Compressor.preset("voice").coefficients(RATE)]
    crec = torch.empty(CM.RECORD_BYTES, dtype=torch.uint8, device=dev)
    key = "gsv_compressor over the same chunk as one clip: voice"
    res["push"][key] = _show(key, _timed(lambda: CM.run_packed(chunk, [0], [n], [0], co, out, crec), args.calls, dev))
    small = CM.StreamCompressor("voice", RATE, dev)
    small.push_tensor(x[:384])
    sstart, sbuf, srec = small.state.clone(), chunk[:384].clone(), torch.empty(5, dtype=torch.int64, device=dev)

    def small_back():
        small.state.copy_(sstart)
        sbuf.copy_(chunk[:384])
    key = "cmpstream push 384 samples in place, no chunk completed: voice"
    res["push"][key] = _show(key, _timed(lambda: small.enqueue(sbuf.data_ptr(), 384, None, False, sbuf.data_ptr(), srec.data_ptr()),
                                         args.calls, dev, small_back))
    # the chunk epilogue: every push is the first chunk of a segment (no splice search), the streams run on
    make = lambda **kw: ChunkEmitter(640, track=TrackResampler(TrackFormat(48000, 1, 20), RATE, dev), level=LV.StreamLeveller(-18.0, RATE, dev),
                                     limit=LM.StreamLimiter(-1.0, RATE, dev), eq=EQM.StreamEQ("voice", RATE, dev), **kw)
    for name, em in (("emit + eq + level + limit + track", make()),
                     ("emit + eq + compress (voice) + level + limit + track", make(compress=CM.StreamCompressor("voice", RATE, dev))),
                     ("emit alone", ChunkEmitter(640)),
                     ("emit + compress (voice)", ChunkEmitter(640, compress=CM.StreamCompressor("voice", RATE, dev)))):
        key = "epilogue of a %d-sample chunk: %s" % (n, name)
        res["epilogue"][key] = _show(key, _timed(lambda: em.push(chunk, False), args.calls, dev, em.new_segment, lambda h: h.result()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
