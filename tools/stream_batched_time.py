"""Time TTS.infer_stream_batched against the only other way to stream S texts, S consecutive TTS.infer_stream calls, on the same
build: synthetic models (24-layer GPT, v2Pro vocoder; random weights, EOS gain 4), a toy front end, stream_chunk 25.  Tokens are
greedy by default (--top-k 1), so that both ways decode the same token sequences and hand out the same audio -- like for like; with
--top-k 15 they sample from different noise streams and the texts' lengths differ between the two ways.  --subtitles times the
return_subtitles=True mode (the frame -> phoneme path and the word timings per clip).  For S = 1, 4, 16, 32 texts it prints

  * seconds of audio handed out per second of wall time,
  * the time from the start of serving to each text's first clip (median and worst over the texts),
  * the share of the wall time the device spends in the vocoder passes and chunk epilogues (hipEvents around the calls),

for both ways, each as the median of --reps runs with the lowest and highest run beside it (the run's spread), and a JSON object
at the end.

    python tools/stream_batched_time.py [--reps 3] [--sizes 1,4,16,32] [--dtype bfloat16] [--stream-chunk 25] [--top-k 1] [--subtitles]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv_tts_lite_amd import stream as stream_mod  # noqa: E402
from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.tts import TTS  # noqa: E402

WORDS = ("alpha beta gamma delta river stone cloud ember quiet frost maple linen orbit pixel quartz tango umber violet willow "
         "xenon yonder zephyr").split()
REF = ("spk.wav", "prompt.wav", "prompt text.")


def _frontend(text):
    """words = latin runs or single marks; one phoneme per character; norm_text == text"""
    words = re.findall(r"[A-Za-z]+|[^\sA-Za-z]", text)
    ids = [1 + (ord(c) * 7) % 690 for w in words for c in w]
    return ids, {"word": words, "ph": [len(w) for w in words]}, None, text


def _texts(n):
    rng = np.random.default_rng(17)
    return [" ".join(rng.choice(WORDS, int(rng.integers(4, 9)))) + str(rng.choice(list(".!?"))) for _ in range(n)]


class _DeviceTime:
    """hipEvents around every call of the wrapped functions; total() once the stream has drained"""

    def __init__(self):
        self.pairs = []

    def wrap(self, fn):
        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.pairs.append((e0, e1))
            return out
        return timed

    def total(self):
        torch.cuda.synchronize()
        ms, self.pairs = sum(a.elapsed_time(b) for a, b in self.pairs), []
        return ms / 1e3


def _serve(clips_of, n, clock):
    """drain a generator of (text, clip): wall time, audio seconds, seconds to each text's first clip"""
    torch.cuda.synchronize()
    t0, first, audio = time.perf_counter(), [None] * n, 0.0
    for t, clip in clips_of():
        if first[t] is None:
            first[t] = time.perf_counter() - t0
        audio += len(clip.audio_data) / clip.samplerate
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, audio_s=audio, audio_per_wall=audio / wall, first_median_s=float(np.median(first)), first_worst_s=max(first),
                vocoder_share=clock.total() / wall)


def _spread(runs):
    out = {}
    for k in runs[0]:
        v = sorted(r[k] for r in runs)
        out[k] = dict(median=round(v[len(v) // 2], 4), low=round(v[0], 4), high=round(v[-1], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1,4,16,32")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--stream-chunk", type=int, default=25)
    ap.add_argument("--top-k", type=int, default=1)
    ap.add_argument("--subtitles", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    tts = TTS(gpt_cache=[(s, 512) for s in sorted(set(sizes) | {1})], sovits_cache=[50, 55], device="cuda:0", dtype=args.dtype)
    tts.load_gpt_model("synthetic://gpt?seed=1234&eos_gain=4.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    vq = next(iter(tts.sovits_models.values())).vq_model
    clock = _DeviceTime()
    vq.decode = clock.wrap(vq.decode)
    stream_mod.ChunkEmitter.push = clock.wrap(stream_mod.ChunkEmitter.push)
    stream_mod.ChunkSplicer.push = clock.wrap(stream_mod.ChunkSplicer.push)
    kw = dict(stream_chunk=args.stream_chunk, debug=False, top_k=args.top_k, return_subtitles=args.subtitles)
    res = dict(dtype=args.dtype, stream_chunk=args.stream_chunk, top_k=args.top_k, subtitles=args.subtitles, reps=args.reps, sizes={})
    for S in sizes:
        texts = _texts(S)
        seeds = list(range(100, 100 + S))

        def batched():
            return tts.infer_stream_batched(*REF, texts, slots=S, seed=seeds, **kw)

        def consecutive():
            for t, text in enumerate(texts):
                torch.manual_seed(seeds[t])
                for clip in tts.infer_stream(*REF, text, **kw):
                    yield t, clip
        row = {}
        for name, fn in (("infer_stream_batched", batched), ("consecutive_infer_stream", consecutive)):
            _serve(fn, S, clock)                                    # warm-up: graphs captured, buffers grown
            row[name] = _spread([_serve(fn, S, clock) for _ in range(args.reps)])
            r = row[name]
            print("S=%2d %-24s audio/wall %7.2f [%7.2f, %7.2f]  first clip median %.4f s [%.4f, %.4f] worst %.4f s  vocoder+epilogue %4.1f %% of "
                  "wall  (wall %.3f s, audio %.1f s)" % (S, name, r["audio_per_wall"]["median"], r["audio_per_wall"]["low"],
                                                          r["audio_per_wall"]["high"], r["first_median_s"]["median"], r["first_median_s"]["low"],
                                                          r["first_median_s"]["high"], r["first_worst_s"]["median"],
                                                          100 * r["vocoder_share"]["median"], r["wall_s"]["median"], r["audio_s"]["median"]), flush=True)
        res["sizes"][S] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
