"""cost of the per-slot repetition penalty / start suppression: python tools/slot_penalty_cost.py [B ...]

Per slot count B (default 8 32 64), bf16, 24 layers, graph replay, kv ~ 200: the raw decode step
  scalar   no table bound (the table-less kernels)
  zero     a table bound, every entry zero (greedy, no penalty, no suppression)
  pen      a table bound, every slot penalising (1.35) and suppressing (10), ctl[2] set: the steps keep `seen` up to date
each timed by hipEvents over GSV_STEPS steps (default 200), GSV_REPS times alternating (default 5; the median and the
range are printed), and gsv_t2s_seed_seen + gsv_t2s_put_slot_sampling for 1 .. B slots against the prompt pass they precede.
On a library without gsv_t2s_seed_seen (an older build through GSV_HIP_LIB) the `pen` case and the seeding are left out, so the
same script gives the `scalar` / `zero` figures of both builds."""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "gsv-tts-lite_amd"))
import torch
from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import slot_sampling as SS
from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.t2s import Text2SemanticDecoder

dev = torch.device("cuda:0")
NST = int(os.environ.get("GSV_STEPS", "200"))
REPS = int(os.environ.get("GSV_REPS", "5"))
HAVE = "gsv_t2s_seed_seen" in N.EXPORTS
cfg = synth.gpt_config(n_layer=int(os.environ.get("GSV_NLAYER", "24")))
w = synth.gpt_weights(cfg, seed=1, eos_gain=-8.0)


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


@torch.inference_mode()
def main(B):
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(w)
    m.initialize_runtime(torch.bfloat16, dev, [(B, 640)])
    rt = m._rt[B]
    rs = [synth.synth_request(i, 40, 60, 100, seed=1) for i in range(B)]
    X, Y, Bt = ([torch.from_numpy(r[k]).to(dev) for r in rs] for k in range(3))

    def start(case):
        """a fresh prompt pass of all slots under `case`; returns after a warm-up window"""
        m._samp = None
        if case == "pen":
            m._samp = SS.resolve(B, 1, 1.0, 1.0, repetition_penalty=[1.35] * B, initial_suppression_steps=[10] * B)
        m._set_ctl(rt, 0, 0, case == "pen", 1.0)
        rt["kv_len"].zero_(); rt["x_len"].zero_()
        if case != "scalar":
            rt["samp"].zero_()
        if case == "pen":
            m._put_request(B, range(B), range(B), m._seed_tokens(range(B), Y))
        xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
        m.prefill(B, 0, xy, xl, yl)
        m._decode(B, 10)
        torch.cuda.synchronize()

    cases = ["scalar", "zero"] + (["pen"] if HAVE else [])
    res = {c: [] for c in cases}
    for rep in range(REPS):
        for c in cases:
            if c == "scalar":
                m._unbind_sampling()
            elif not m._samp_bound:
                m._bind_sampling(rt)
            start(c)
            res[c].append(timed(lambda: m._decode(B, NST)) / NST)
    m._samp = None
    for c in cases:
        v = res[c]
        print("B=%d bf16 %-6s step %.4f ms  (median of %d; %.4f .. %.4f)%s" % (
            B, c, statistics.median(v), len(v), min(v), max(v),
            "" if c == "scalar" else "  %+.2f us vs scalar" % ((statistics.median(v) - statistics.median(res["scalar"])) * 1e3)))
    # the refill: seeding + entries against the prompt pass of the same rows
    if HAVE:
        if not m._samp_bound:
            m._bind_sampling(rt)
        m._samp = SS.resolve(B, 1, 1.0, 1.0, repetition_penalty=[1.35] * B, initial_suppression_steps=[10] * B)
        for n in sorted({1, 2, min(8, B), B}):
            rows = list(range(n))
            seed = m._seed_tokens(rows, Y)
            xy, xl, yl, _, _ = m.embed_prompt(X[:n], Y[:n], Bt[:n])
            put = lambda: m._put_request(B, rows, rows, seed)
            pas = lambda: m.prefill_slots(B, rows, xy.clone(), xl, yl)
            put(); pas(); torch.cuda.synchronize()
            t_put = statistics.median(timed(put, 20) for _ in range(REPS))
            t_pas = statistics.median(timed(pas) for _ in range(REPS))
            print("B=%d refill of %2d slots: seed_seen + put_slot_sampling %.1f us, prompt pass %.3f ms (%.2f %%)" % (
                B, n, t_put * 1e3, t_pas, 100 * t_put / t_pas))
        m._samp = None
    m._unbind_sampling()


for B in ([int(a) for a in sys.argv[1:]] or [8, 32, 64]):
    main(B)
