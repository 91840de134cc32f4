"""scratch: per-phase shader-clock breakdown of the last layer's decode kernels"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gsv-tts-lite_amd"))
import numpy as np, torch
from gsv_tts_lite_amd import synth, _native as N
from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
dev = torch.device("cuda:0")
cfg = synth.gpt_config(); w = synth.gpt_weights(cfg, eos_gain=0.0)
m = Text2SemanticDecoder(cfg); m.load_state_dict(w); m.initialize_runtime(torch.bfloat16, dev, [(1, 256), (1, 450)])
x, y, bert, _ = synth.synth_request(0)
T = lambda a: torch.from_numpy(a).to(dev)
dbg = torch.zeros(64, dtype=torch.int64, device=dev)      # slots 0-15 wave 0, 16-31 last wave, slot 16 + k at 32 + 2 k / 33 + 2 k
N.check(N.lib().gsv_t2s_set_debug(m._h, dbg.data_ptr()))
tok = m.infer(T(x)[None], T(y)[None], T(bert)[None], top_k=1)
torch.cuda.synchronize()
rows = []
for it in range(20):
    m._decode(1, 1); torch.cuda.synchronize()
    d = dbg.cpu().numpy().astype(np.int64)
    rows.append(d.copy())
r = np.array(rows)
a = r[:, 1:7] - r[:, 0:6]
f = r[:, 9:13] - r[:, 8:12]
w15 = r[:, 16:32]
a15 = w15[:, 1:7] - w15[:, 0:6]
# bf16 handles run the attention phase on waves 8-15 (wave 0 only waits at its barrier, then merges): the phase's length is the LAST wave's
# stamp 3 -> 4, and wave 0's "attention" / "combine" columns are its wait for that / the rest of the wait + the merge.  fp32 handles: every wave attends.
print("attn phases (cycles), wave 0:    entry->firstload, LN+xs, QKV, attention (bf16: waits), combine, panel:", np.median(a, axis=0), "total", np.median(r[:, 6] - r[:, 0]))
print("attn phases (cycles), last wave: entry->firstload, LN+xs, QKV, attention, barrier + merge wait, panel:  ", np.median(a15, axis=0), "total", np.median(w15[:, 6] - w15[:, 0]))
print("ffn phases entry->firstload, LN+xs, W1, panel:", np.median(f, axis=0), "total", np.median(r[:, 12] - r[:, 8]))
# (no 'attn end -> ffn start': the two kernels' blocks (0, 0) may sit on different XCDs, whose clocks are not comparable)
print("ffn LN detail: park", np.median(r[:,13]-r[:,9]), "barrier", np.median(r[:,14]-r[:,13]), "finish+ln", np.median(r[:,15]-r[:,14]), "xs+barrier", np.median(r[:,10]-r[:,15]))
print("last wave, relative to wave 0's entry stamp: attn stamps 0..6:", np.median(w15[:, 0:7] - r[:, 0:1], axis=0))
print("wave 0,    relative to its entry stamp:      attn stamps 0..6:", np.median(r[:, 0:7] - r[:, 0:1], axis=0))
# stamp 7 sits behind the last load instruction of the kernel's entry and in front of the pin's wait, stamp 1 behind that wait: a wave whose
# stamp 7 is late is still ISSUING its loads; one whose stamp 7 is early and stamp 1 late waits for data
print("attn stamp 7 (entry loads issued) / stamp 1 (first load landed), rel. to wave 0's entry: wave 0 %.0f / %.0f, last wave %.0f / %.0f"
      % tuple(np.median(c - r[:, 0]) for c in (r[:, 7], r[:, 1], w15[:, 7], w15[:, 1])))
print("last wave ffn stamps 8,9,13,14,15,10,11,12 rel. to wave 0's stamp 8:", np.median(w15[:, [8, 9, 13, 14, 15, 10, 11, 12]] - r[:, 8:9], axis=0))
print("wave 0    ffn stamps 8,9,13,14,15,10,11,12 rel. to its stamp 8:     ", np.median(r[:, [8, 9, 13, 14, 15, 10, 11, 12]] - r[:, 8:9], axis=0))
# stamp 16 sits behind park() and in front of the partial-sum barrier (MODE 1 attention kernel): a wave's wait at that barrier is read
# directly, and the barrier completes when the last wave's stamp 16 is taken.  The LayerNorm and the xs barrier follow: "behind" = stamp 2
p0, p15 = r[:, 32], r[:, 33]
print("attn park() done (stamp 16) rel. to wave 0's entry: wave 0 %.0f, last wave %.0f; from there to xs ready (stamp 2): wave 0 %.0f, last wave %.0f"
      % tuple(np.median(c) for c in (p0 - r[:, 0], p15 - r[:, 0], r[:, 2] - p0, w15[:, 2] - p15)))
print("attn: wave 0 ahead of the last wave at the partial-sum barrier by %.0f cycles" % np.median(p15 - p0))
