"""One decode step of more than 16 sequences against the oracle in the matching numerics, at every K/V chunk edge of the two
attention kernels that serve that range, on inputs whose edge rows carry weight.

Kernels under test: t2s_batch_attn2_kernel<NIT> inside the batched chain (csrc/t2s_small.h; bf16 handles, B >= batched_min, cache of at
most 1024 rows) and t2s_attn_multi_kernel<WT, 0, 2> with t2s_ffn_multi_kernel<WT, 2> behind it (csrc/t2s_decode_multi.h; fp32 handles
above 16 sequences, bf16 handles above 16 sequences with a cache of more than 1024 rows).  Before this file their hidden states were
compared at cache lengths below 60 only (test_hip_t2s_lowp.py::test_batched_step_hidden_vs_oracle_bf16_and_fp8); every path below gets
its first hidden-state comparison here.  The inputs are built by tests/decode_kv_edges_cases.py: designated rows either side of the last
chunk edge, the first and the last live row, and every dead row hold a key aligned with the query, so a skipped live row or an admitted
dead one moves the hidden state by at least 10 x the bound (tests/test_decode_kv_edges_cpu.py shows that on the oracle alone).

Regime -> path (n = cache length of a sequence before the step; nch = ceil(n / 64) live chunks):
  chain-1024       t2s_batch_attn2_kernel<16>: body 2 (n = 0 .. 128), 3 (129 .. 192), 4 (193 .. 256), 6 (257 .. 384), 8 (385 .. 512),
                   12 (513 .. 768), 16 (769 .. 1023): all seven, both sides of every switch (128/129, 192/193, 256/257, 384/385, 512/513,
                   768/769); a dead-chunk edge inside body 6 (320/321) and body 12 (640/641); the blind chunks 0 / 1 with 0, 1, 63 .. 65,
                   127 live rows; the last row of the cache (1023); two parked slots
  chain-512        t2s_batch_attn2_kernel<8>: bodies 2, 3, 4, 6, 8, body 8 up to the last row (510, 511); a parked slot between live ones
  chain-256        t2s_batch_attn2_kernel<4>: bodies 2, 3, 4, body 4 up to the last row (254, 255); B = 17, the first batch on the chain
  multi-fp32       t2s_attn_multi_kernel<float, 0, 2>: chunks of 256 rows (255/256/257, 511/512/513, 767/768/769), row iterations of 128
                   (127/128/129, 383/384/385), the clamp at the last row (1022, 1023); pairs: (long, short), (short, short), a parked
                   slot in either place of a pair, edge with edge; B = 21 is odd (decode_kv_edges_cases lists the pairs)
  multi-bf16-long  t2s_attn_multi_kernel<bf16_t, 0, 2>: chunks of 512 rows (511/512/513, 1023/1024/1025, 1535/1536/1537), row iterations
                   of 256 (255/256/257), the last rows (2046, 2047); (2047, parked) share a block; B = 17 is odd
Every regime has a control of the same handle, B and T whose lengths are 5 rows or more from every multiple of 64 and from T.

Per regime: one step of decode_hidden, eagerly, after a short prompt pass has primed the state; then
  * hidden states per live sequence: bf16 chain max < 3e-3 and mean < 3e-4 (("bf16", 1) of test_batched_step_hidden_vs_oracle_bf16_and_fp8),
    multi-fp32 max < 2e-5 (F32_TOL), multi-bf16-long max < 1e-3 (HID_TOL of test_hip_decode_park_order.py);
  * row n of K and V of every live sequence equals the oracle's: within 2e-5 (fp32 handle) or one bf16 ulp, |d| <= 2^-7 |value|;
  * every other row is bit-identical to what was copied in (a parked slot: every row but T - 1), kv_len is n + 1 / still -1;
  * parked rows of `hidden` are not compared (the oracle side holds NaN there).

Measured on MI355X (|hidden - oracle| over the live sequences: max, mean, the largest mean of one sequence; n of the worst sequence;
appended rows: max |d| / |value| on bf16 handles, max |d| on the fp32 one):
  regime             max        mean       seq. mean   worst n   appended rows      control: max   mean       seq. mean   appended rows
  chain-1024         7.36e-04   9.12e-06   1.92e-04    768       7.46e-03           6.13e-04       5.07e-06   1.42e-04    4.55e-03
  chain-512          2.29e-04   3.59e-06   6.28e-05    65        0 (bit-equal)      4.61e-05       9.47e-07   1.36e-05    4.93e-03
  chain-256          3.29e-04   4.78e-06   6.81e-05    191       6.80e-03           6.49e-04       1.40e-05   1.42e-04    0 (bit-equal)
  multi-fp32         1.19e-06   9.81e-08   1.92e-07    511       1.43e-06           1.91e-06       1.32e-07   3.03e-07    1.55e-06
  multi-bf16-long    6.86e-05   9.51e-07   1.63e-06    700       4.93e-03           5.42e-05       8.58e-07   1.66e-06    6.02e-03
Every hidden-state bound holds with a factor of 4 or more to spare, at the edges as in the controls: no kernel was changed.
With two wrong masks compiled into a scratch library (t2s_batch_attn2_kernel: `it * 64 + rsub < n - 1`, the last live row dropped;
t2s_attn_multi_kernel: `rr <= nr`, row n admitted) all ten tests failed on the hidden states: max 1.6e-01 .. 7.9e-01.

The appended row's bound is relative, so it is well posed only where an element is no cancellation residue: on a first set of inputs
(xin drawn once) one K element of control-chain-1024 was -6.3e-06, the device two bf16 ulps from the oracle (9.39e-03 |value|) and
ONE from the float64 value of the same dot, the fp32 oracle itself THREE.  decode_kv_edges_cases.build() therefore redraws xin until
every appended element is at least MIN_ROW_ABS = 4e-3, where an ulp is 7 x the oracle's own fp32 error; the bound is as it was.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_kv_edges_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5           # tests/test_hip_decode_park_order.py, tests/test_hip_t2s.py (ATOL)
HID_TOL = 1e-3           # tests/test_hip_decode_park_order.py, tests/test_hip_t2s_lowp.py
CHAIN_TOL = (3e-3, 3e-4)  # (max, mean): ("bf16", 1) of tests/test_hip_t2s_lowp.py::test_batched_step_hidden_vs_oracle_bf16_and_fp8
# regime -> (max, mean or None)
BOUND = {"chain-1024": CHAIN_TOL, "chain-512": CHAIN_TOL, "chain-256": CHAIN_TOL, "multi-fp32": (F32_TOL, None), "multi-bf16-long": (HID_TOL, None)}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # a copy: the cases' arrays are read-only


def _prime(m, B, dev, seed):
    """a short prompt pass per sequence: every piece of the bound state is what real use leaves there (test_hip_decode_park_order.py)"""
    from gsv_tts_lite_amd import synth
    rs = [synth.synth_request(800 + i, 3, 4 + i % 3, 5 + i % 4, seed=seed, bert="random") for i in range(B)]
    xy, xl, yl, _, _ = m.embed_prompt([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs])
    m.prefill(B, 0, xy, xl, yl)


def _step_vs_oracle(rid, dev):
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    case = C.build(rid)
    base = rid[len("control-"):] if rid.startswith("control-") else rid
    handle, B, T, lens = case["handle"], case["B"], case["T"], case["lens"]
    f32 = handle == "fp32"
    cfg, w = C.config_weights()
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(w)
    m.initialize_runtime(DTYPES[handle], dev, [(B, T)])
    # the path the regime is there for: the batched chain up to 1024 cache rows on a bf16 handle, else two sequences per block
    # (an fp32 handle has no batched chain: its batched_min is beyond every batch)
    assert B > 16 and base.startswith("chain") == (not f32 and B >= m.batched_min and T <= 1024)
    want, ko, vo = C.reference(rid, handle, m.batched_min, m.ffn_slices(B))
    _prime(m, B, dev, C.W_SEED)
    rt = m._rt[B]
    assert tuple(rt["k"].shape) == case["k"].shape
    with torch.inference_mode():
        rt["k"].copy_(_T(case["k"], dev).to(rt["k"].dtype))
        rt["v"].copy_(_T(case["v"], dev).to(rt["v"].dtype))
        rt["kv_len"].copy_(_T(case["kv_len"], dev))
        assert np.array_equal(rt["k"].float().cpu().numpy(), case["k"])          # the built values are bf16-representable
        got = m.decode_hidden(B, _T(case["xin"], dev)).cpu().numpy()
        torch.cuda.synchronize()
        k = rt["k"].float().cpu().numpy()
        v = rt["v"].float().cpu().numpy()
        kv = rt["kv_len"].cpu().numpy()
    del m
    bad = []                                     # every figure is printed before anything is asserted

    def expect(cond, *what):
        if not cond:
            bad.append(what)

    live = list(case["live"])
    assert np.isfinite(want[live]).all()
    expect(np.isfinite(got[live]).all(), "hidden states must be finite")
    err = np.abs(got[live] - want[live])                      # parked rows are left out: the oracle's are NaN
    smax, smean = err.max(axis=1), err.mean(axis=1)
    wb = int(np.argmax(smax))
    tol_max, tol_mean = BOUND[base]
    for i, b in enumerate(live):
        expect(smax[i] < tol_max, "hidden max", "sequence", b, "n", lens[b], float(smax[i]))
        if tol_mean is not None:
            expect(smean[i] < tol_mean, "hidden mean", "sequence", b, "n", lens[b], float(smean[i]))
    # the appended row, the rows nobody may write, the lengths
    row_rel = row_abs = 0.0
    for b, n in enumerate(lens):
        wrow = n if n >= 0 else T - 1
        for name, g, o_, src in (("k", k, ko, case["k"]), ("v", v, vo, case["v"])):
            keep = np.ones(T, bool)
            keep[wrow] = False
            expect(np.array_equal(g[0, b][:, keep], src[0, b][:, keep]), name, "sequence", b, "n", n, "a row other than %d was written" % wrow)
            if n < 0:
                continue
            d = np.abs(g[0, b, :, n] - o_[0, b, :, n])
            row_abs = max(row_abs, float(d.max()))
            if f32:
                expect(d.max() <= F32_TOL, name, "sequence", b, "n", n, "appended row", float(d.max()))
            else:
                ref = np.abs(o_[0, b, :, n])
                row_rel = max(row_rel, float((d / np.maximum(ref, 1e-30)).max()))
                for hh, e in zip(*np.nonzero(d > 2.0 ** -7 * ref)):
                    expect(False, name, "sequence", b, "n", n, "head", int(hh), "element", int(e), "appended row beyond one bf16 ulp: device",
                           float(g[0, b, hh, n, e]), "oracle", float(o_[0, b, hh, n, e]))
        expect(int(kv[b]) == (n + 1 if n >= 0 else -1), "kv_len", "sequence", b, "n", n, int(kv[b]))
    print("decode K/V edges %s (%s handle, B=%d, T=%d): hidden max %.2e mean %.2e (largest per-sequence mean %.2e), worst sequence n = %d; "
          "appended rows max |d| %.2e%s" % (rid, handle, B, T, smax.max(), err.mean(), smean.max(), lens[live[wb]], row_abs,
                                            "" if f32 else ", max |d| / |value| %.2e" % row_rel))
    assert not bad, "\n".join(" ".join(str(x) for x in what) for what in bad)


@pytest.mark.parametrize("rid", C.EDGE_IDS)
def test_decode_step_at_kv_chunk_edges(dev, rid):
    _step_vs_oracle(rid, dev)


@pytest.mark.parametrize("rid", C.CONTROL_IDS)
def test_decode_step_control_away_from_edges(dev, rid):
    _step_vs_oracle(rid, dev)
