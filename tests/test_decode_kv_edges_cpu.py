"""The bounds of tests/test_hip_decode_kv_edges.py discriminate -- shown on the oracle alone, no GPU.

That file holds one decode step of more than 16 sequences to the oracle in the matching numerics within BOUND[regime] (max |hidden -
oracle| per sequence).  Here the oracle itself computes what a kernel with a wrong row mask would: every designated row skipped in
turn, and the first stale row admitted (decode_kv_edges_cases.perturbations).  Each must move the hidden state of EVERY live sequence
it touches by at least 10 x BOUND, so such a kernel cannot pass.  The distance between the oracle in the handle's numerics and the
fp32 oracle is printed beside it: the construction does not inflate rounding noise.  The control regimes (lengths away from every
edge) are built the same way and must satisfy nothing but finiteness.

Measured (smallest shift over all live sequences and perturbations, where; its ratio to the bound; bf16-mode vs fp32 oracle, max / mean):
  chain-1024        7.84e-02  (b) n = 640     26 x 3e-3      2.84e-03 / 4.32e-04
  chain-512         8.04e-02  (b) n = 127     27 x 3e-3      2.96e-03 / 4.29e-04
  chain-256         8.17e-02  (b) n = 128     27 x 3e-3      2.76e-03 / 4.41e-04
  multi-fp32        7.52e-02  (b) n = 512   3758 x 2e-5      --
  multi-bf16-long   7.97e-02  (b) n = 2046    80 x 1e-3      2.17e-03 / 3.11e-04
The oracle's fp32 QKV dots against float64, over the ten cases: max 1.06e-06 .. 1.48e-06 (ORACLE_DOT_ERR = 2e-6); smallest appended
|element| 4.00e-03 .. 4.13e-03.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_kv_edges_cases as C  # noqa: E402

# max |hidden - oracle| the GPU file allows: ("bf16", 1) of test_hip_t2s_lowp.py::test_batched_step_hidden_vs_oracle_bf16_and_fp8 on the
# batched chain; F32_TOL and HID_TOL of test_hip_decode_park_order.py on the two-sequences-per-block kernels
BOUND = {"chain-1024": 3e-3, "chain-512": 3e-3, "chain-256": 3e-3, "multi-fp32": 2e-5, "multi-bf16-long": 1e-3}
FACTOR = 10


@pytest.mark.parametrize("rid", C.EDGE_IDS)
def test_every_wrong_row_mask_moves_every_live_sequence_beyond_the_bound(rid):
    case = C.build(rid)
    ref, _, _ = C.reference(rid)
    live = list(case["live"])
    parked = [b for b in range(case["B"]) if b not in live]
    assert np.isfinite(ref[live]).all()
    assert np.isnan(ref[parked]).all()            # a parked slot's row poisons whatever would compare it
    smallest = (np.inf, None, None)
    for name, k, kv, seqs in C.perturbations(case):
        hid, _, _ = C.run_oracle(case, case["handle"], k=k, kv_len=kv)
        assert np.isfinite(hid[live]).all()
        d = np.abs(hid - ref).max(axis=1)         # NaN on parked rows: never indexed below
        assert set(seqs) <= set(live)
        for b in seqs:
            if d[b] < smallest[0]:
                smallest = (float(d[b]), name, case["lens"][b])
        others = [b for b in live if b not in seqs]
        assert not others or d[others].max() == 0.0, (name, "a perturbation leaked into a sequence it does not touch")
        worst = min(seqs, key=lambda b: d[b])
        print("%s %s: %d sequences, smallest max |hidden - true| %.3e at n = %d" % (rid, name, len(seqs), d[worst], case["lens"][worst]))
        assert d[list(seqs)].min() >= FACTOR * BOUND[rid], (rid, name, case["lens"][worst], float(d[worst]))
    ratio = smallest[0] / BOUND[rid]
    print("%s: smallest shift %.3e (%s, n = %d) = %.0f x the bound %.0e" % (rid, smallest[0], smallest[1], smallest[2], ratio, BOUND[rid]))
    assert ratio >= FACTOR
    if case["handle"] != "fp32":
        d32 = np.abs(ref[live] - C.reference(rid, "fp32")[0][live])
        print("%s: %s-mode vs fp32 oracle: max %.2e mean %.2e" % (rid, case["handle"], d32.max(), d32.mean()))


@pytest.mark.parametrize("rid", C.CONTROL_IDS)
def test_control_regimes_are_away_from_every_edge_and_finite(rid):
    case = C.build(rid)
    edge = C.build(rid[len("control-"):])
    assert (case["handle"], case["B"], case["T"]) == (edge["handle"], edge["B"], edge["T"])
    assert [n < 0 for n in case["lens"]] == [n < 0 for n in edge["lens"]]
    for n in case["lens"]:
        if n >= 0:
            assert 5 <= n % 64 <= 59 and case["T"] - n >= 5, n
    ref, _, _ = C.reference(rid)
    live = list(case["live"])
    assert np.isfinite(ref[live]).all()
    assert np.isnan(np.delete(ref, live, axis=0)).all()


@pytest.mark.parametrize("rid", C.EDGE_IDS + C.CONTROL_IDS)
def test_appended_rows_stay_clear_of_cancellation_residues(rid):
    """the one-ulp bound of the GPU file on the appended K / V row is well posed on these inputs: no element (float64, the regime's
    operands) is below MIN_ROW_ABS, the oracle's own fp32 dots are within ORACLE_DOT_ERR of float64 (fp32 oracle against float64 on
    fp32 operands: its rows are stored unrounded), an ulp of the smallest element is 7 x that, and the oracle in the handle's numerics
    is itself within one bf16 ulp of the rounded float64 row"""
    case = C.build(rid)
    live = list(case["live"])
    exact = C.appended_rows_exact(case["handle"], case["T"], case["xin"])
    assert np.abs(exact).min() >= C.MIN_ROW_ABS
    _, k32, v32 = C.reference(rid, "fp32")
    e32 = C.appended_rows_exact(case["handle"], case["T"], case["xin"], fp32_weights=True)
    _, kh, vh = C.reference(rid)
    worst = 0.0
    for b in live:
        n = case["lens"][b]
        row32 = np.concatenate([k32[0, b, :, n].ravel(), v32[0, b, :, n].ravel()])
        worst = max(worst, float(np.abs(row32 - e32[b]).max()))
        if case["handle"] == "bf16":
            row = np.concatenate([kh[0, b, :, n].ravel(), vh[0, b, :, n].ravel()])
            want = C.round_bf16(exact[b].astype(np.float32))
            assert (np.abs(row - want) <= 2.0 ** -7 * np.abs(want)).all(), (rid, b)
    print("%s: oracle fp32 QKV dots vs float64: max %.2e; smallest appended |element| %.2e" % (rid, worst, np.abs(exact).min()))
    assert worst <= C.ORACLE_DOT_ERR
    assert 2.0 ** -8 * C.MIN_ROW_ABS >= 7 * C.ORACLE_DOT_ERR


def test_regimes_hold_the_lengths_their_paths_need():
    """the properties the GPU file's docstring maps to code paths"""
    R = C.REGIMES
    for rid, B in (("chain-1024", 31), ("chain-512", 19), ("chain-256", 17), ("multi-fp32", 21), ("multi-bf16-long", 17)):
        assert len(R[rid][2]) == B and B >= C.BATCHED_MIN
    # every straight-line body of t2s_batch_attn2_kernel (live 64-row chunks -> body), both sides of every switch, the dead-chunk edges
    body = lambda n: next(c for c in (2, 3, 4, 6, 8, 12, 16) if (n + 63) // 64 <= c)
    assert {body(n) for n in R["chain-1024"][2] if n >= 0} == {2, 3, 4, 6, 8, 12, 16}
    for lo in (128, 192, 256, 384, 512, 768):
        assert {lo, lo + 1} <= set(R["chain-1024"][2]) and body(lo) < body(lo + 1)
    assert {320, 321, 640, 641} <= set(R["chain-1024"][2]) and body(320) == body(321) and body(640) == body(641)
    assert max(R["chain-512"][2]) == 511 and max(R["chain-256"][2]) == 255 and max(R["chain-1024"][2]) == 1023
    # two sequences per block: a parked slot in either place of a pair, an odd B
    for rid in ("multi-fp32", "multi-bf16-long"):
        lens = R[rid][2]
        assert len(lens) % 2 == 1
        assert any(lens[i] >= 0 and lens[i + 1] < 0 for i in range(0, len(lens) - 1, 2))
    lens = R["multi-fp32"][2]
    assert any(lens[i] < 0 and lens[i + 1] >= 0 for i in range(0, len(lens) - 1, 2))
    assert {127, 128, 129, 255, 256, 257, 511, 512, 513} <= set(lens)
    assert {255, 256, 257, 511, 512, 513, 1023, 1024, 1025} <= set(R["multi-bf16-long"][2]) and R["multi-bf16-long"][1] > 1024
