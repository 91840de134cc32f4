"""The GPT prompt pass against the oracle in the matching numerics at every tile, mask and launch-shape edge.

Kernels under test: t2s_embed_kernel, t2s_prefill_attn_kernel (fp32 handles, behind tapgemm), t2s_prefill_attn_mfma_kernel
and the bgemm chain / bgemm_wide_kernel (bf16 and fp8 handles), t2s_prefill_finish_kernel and the first logits
(csrc/t2s_prefill.h, csrc/gsv_abi.hip: t2s_prefill_impl / t2s_gemm_chain).  The shapes, and the edge each one is there for,
are in tests/prefill_edges_cases.py; that the bounds below separate a correct mask from an off-by-one is shown on the oracle
alone in tests/test_prefill_edges_cpu.py (each mutant moves the hidden states by >= 5e-2).

Every pass runs into caches filled with a sentinel and a state holding junk lengths, and is compared on: the embedded
rows, the hidden states, every layer's K and V rows, the untouched cache rows and slots, kv_len / x_len / step / eos_at,
the last hidden row kept for the logits, and the greedy first sample wherever the oracle's decision margin allows.

Bounds (none of them new): fp32 handles ATOL = 2e-5 (test_hip_t2s.py); bf16 handles max < 1e-2 / mean < 1.5e-3 on the
hidden states, _kv_close on layer 0's K / V, mean < 5e-3 / max < 1e-1 on later layers' (test_hip_t2s_lowp.py).

Launch shapes of the bf16 GEMM chain reached (rtiles = ceil(M / 32), M = rows x l_max): M <= 48 (grid, 2..33 positions),
rtiles <= 20 (grid), 21..39 (PACK_4: 33; the 1056-position row: 33), 40..99 (PACK_7: 57), M >= 3072 = bgemm_wide_kernel
(PACK_13: M 3341, on a bf16 and on an fp8 handle).  `cpb = 8` (rtiles >= 100 on bgemm_kernel) is NOT reachable through an fp8
handle: the prompt pass hands the chain f8 = false on every handle (t2s_prefill_impl), so from M = 3072 = rtiles 96 on it runs
bgemm_wide_kernel there as well.  The branch is live only with the tuning aid GSV_WIDE_MIN_M set, which a process reads once:
PACK_13 runs once more in a child process that sets it (rtiles 105).

Measured on MI355X, the largest over all cases of a regime (every case prints its own):
  regime            embed      hidden max / mean      layer-0 K/V max   later layers' K/V max / mean   bound on hidden
  fp32, 1 layer     9.5e-07    2.6e-06 / 2.1e-07      3.3e-06 (every layer)                            2e-5
  fp32, 3 layers    9.5e-07    4.3e-06 / 2.7e-07      5.7e-06 (every layer)                            2e-5
  bf16, 1 layer     4.8e-07    2.2e-03 / 2.3e-04      3.1e-02 (one ulp)  --                            1e-2 / 1.5e-3
  bf16, 3 layers    4.8e-07    5.4e-03 / 7.4e-04      3.1e-02 (one ulp)  3.1e-02 / 1.9e-03             1e-2 / 1.5e-3
  fp8,  1 layer     4.8e-07    2.2e-03 / 2.3e-04      3.1e-02 (one ulp)  --                            1e-2 / 1.5e-3
One bf16 layer measures 4.5x (max) and 6.5x (mean) below the ceiling it shares with three; the ceiling is left where it is.
The oracle runs with the position table as the reference builds it (torch): its numpy restatement is up to 6e-5 away at the
positions these prompts reach, which alone put the 591-position fp32 case at 2.9e-5 (prefill_edges_cases.reference_sine_pe).
With two mask mutants compiled into a scratch library (MFMA kernel: an audio query misses its own key; fp32 kernel: text
queries see key lx) every test here that runs a pass failed, on the hidden states (max 5.4e-2 .. 1.4).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_edges_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

ATOL = 2e-5              # fp32 handles: hidden, K, V (test_hip_t2s.py)
HID_TOL = 1e-3           # bf16 handles: embedded rows (test_hip_t2s_lowp.py)
SENTINEL = 7.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()


def _model(numerics, n_layer, S, T, dev):
    """one handle per (numerics, layers, state shape), kept for the module"""
    key = (numerics, n_layer, S, T)
    if key not in _MODELS:
        from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
        cfg, w = C.config_weights(n_layer)
        m = Text2SemanticDecoder(cfg)
        m.load_state_dict(w)
        m.initialize_runtime(DTYPES[numerics], dev, [(S, T)])
        _MODELS[key] = m
    return _MODELS[key]


def _kv_close(got, want):
    """test_hip_t2s_lowp.py's, verbatim: bf16 cache rows of layer 0 (no upstream layers): a flipped bf16 operand of the QKV GEMM
    moves an output by ~1e-4, i.e. by a few ulps where the value is small -- so: nearly all elements within one ulp, none off by 2e-3"""
    d = np.abs(got - want)
    ulp = np.maximum(np.abs(want), 1e-2) * 2.0 ** -7
    assert not (d > np.maximum(ulp * 1.01, 2e-3)).any(), float(d.max())
    assert (d > ulp * 1.01).mean() < 2e-3 and d.mean() < 1e-4, ((d > ulp * 1.01).mean(), d.mean())


def _run_and_check(dev, numerics, n_layer, rows, S, T, slots=None, slot0=0):
    """one prompt pass of `rows` into a fresh-looking (S, T) state -- slots[b] of row b through prefill_slots, or slot0.. through
    prefill -- and every comparison of the module docstring.  Returns the pass's xy shape."""
    rows = tuple(rows)
    n = len(rows)
    ref = C.reference(numerics, n_layer, rows)
    m = _model(numerics, n_layer, S, T, dev)
    rt = m._rt[S]
    dst = list(slots) if slots is not None else list(range(slot0, slot0 + n))
    idle = [s for s in range(S) if s not in dst]
    assert len(set(dst)) == n and (idle or S == 1)
    reqs = [C.request(i, lx, ly) for i, (lx, ly) in enumerate(rows)]
    junk = {"kv_len": 3, "x_len": 2, "step": 9, "eos_at": 4}
    with torch.inference_mode():
        rt["k"].fill_(SENTINEL); rt["v"].fill_(SENTINEL)
        for key, val in junk.items():
            rt[key].fill_(val)
        rt["hidden"].fill_(-3.0); rt["pre_tokens"].fill_(-1); rt["seen"].zero_()
        m._set_ctl(rt, 0, 0, False, 1.0, suppress_first=True)       # greedy; the first sample never 280 / 486 / EOS (as infer sets it)
        xy, xl, yl, _, _ = m.embed_prompt([_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs])
        emb = xy.cpu().numpy()
        if slots is not None:
            m.prefill_slots(S, dst, xy, xl, yl)
        else:
            m.prefill(S, slot0, xy, xl, yl)
        torch.cuda.synchronize()
        state = {key: rt[key].cpu().numpy().copy() for key in junk}     # before the flush: its token kernel visits every slot
        m._flush(S)
        torch.cuda.synchronize()
    hid = xy.cpu().numpy()
    hlast = rt["hidden"].cpu().numpy()
    pre = rt["pre_tokens"].cpu().numpy()
    k = rt["k"].float().cpu().numpy(); v = rt["v"].float().cpu().numpy()          # [NL, S, H, T, Dh]
    lmax = max(lx + ly for lx, ly in rows)
    assert hid.shape == (n, lmax, 512)
    f32 = numerics == "fp32"
    bad = []                                     # every figure is printed before anything is asserted

    def expect(cond, *what):
        if not cond:
            bad.append(what)

    expect(np.isfinite(hid).all(), "hidden states (pad rows included) must be finite")
    worst = dict(emb=0.0, hmax=0.0, hmean=0.0, k0=0.0, kv=0.0, kvmean=0.0)
    for b, ((lx, ly), r, s) in enumerate(zip(rows, ref, dst)):
        L = lx + ly
        tag = (numerics, n_layer, "row", b, (lx, ly), "slot", s)
        # embedded rows; pad rows exactly zero
        e = float(np.abs(emb[b, :L] - r["embed"]).max())
        expect(e < (ATOL if f32 else HID_TOL), tag, "embed", e)
        expect(not emb[b, L:].any(), tag, "embedded pad rows must be exactly 0")
        # hidden states
        d = np.abs(hid[b, :L] - r["hidden"])
        worst["emb"] = max(worst["emb"], e); worst["hmax"] = max(worst["hmax"], float(d.max())); worst["hmean"] = max(worst["hmean"], float(d.mean()))
        if f32:
            expect(d.max() < ATOL, tag, "hidden", d.max())
        else:
            expect(d.max() < 1e-2 and d.mean() < 1.5e-3, tag, "hidden", d.max(), d.mean())
        # K / V rows of every layer, and the sentinel behind them
        for name, got, want in (("k", k, r["k"]), ("v", v, r["v"])):
            if f32:
                dk = float(np.abs(got[:, s, :, :L] - want).max())
                worst["kv"] = max(worst["kv"], dk)
                expect(dk < ATOL, tag, name, dk)
            else:
                worst["k0"] = max(worst["k0"], float(np.abs(got[0, s, :, :L] - want[0]).max()))
                try:
                    _kv_close(got[0, s, :, :L], want[0])
                except AssertionError as err:
                    expect(False, tag, name, "layer 0: _kv_close", str(err).splitlines()[0])
                for lay in range(1, n_layer):
                    dk = np.abs(got[lay, s, :, :L] - want[lay])
                    worst["kv"] = max(worst["kv"], float(dk.max())); worst["kvmean"] = max(worst["kvmean"], float(dk.mean()))
                    expect(dk.mean() < 5e-3 and dk.max() < 1e-1, tag, name, "layer", lay, dk.mean(), dk.max())
            expect((got[:, s, :, L:] == SENTINEL).all(), tag, name, "cache rows beyond the prompt were written")
        # bookkeeping of the slot
        st = tuple(int(state[q][s]) for q in ("kv_len", "x_len", "step", "eos_at"))
        expect(st == (L, lx, 0, -1), tag, "kv_len / x_len / step / eos_at", st)
        expect(np.array_equal(hlast[s], hid[b, L - 1]), tag, "hidden[slot] is not the last prompt row")
        # the first sample, where the oracle's decision is wider than the kernels' noise
        if r["gap"] >= (C.FP32_MARGIN if f32 else C.TOKEN_MARGIN):
            expect(pre[s, L] == r["token"], tag, "first sample", int(pre[s, L]), "oracle", r["token"], "gap", r["gap"])
    for s in idle:
        expect((k[:, s] == SENTINEL).all() and (v[:, s] == SENTINEL).all(), "slot", s, "the cache of a slot outside the pass was written")
        expect({q: int(a[s]) for q, a in state.items()} == junk, "slot", s, "the state of a slot outside the pass changed")
        expect((hlast[s] == -3.0).all(), "slot", s, "hidden of a slot outside the pass changed")
    print("prefill edges %s %d layer(s) rows %s -> slots %s: embed %.1e | hidden max %.2e mean %.2e | layer-0 K/V max %.1e | %s K/V max %.1e mean %.1e"
          % (numerics, n_layer, list(rows) if n <= 4 else "%d x l_max %d" % (n, lmax), dst if n <= 8 else "...", worst["emb"], worst["hmax"], worst["hmean"],
             worst["k0"], "every layer's" if f32 else "later layers'", worst["kv"], worst["kvmean"]))
    assert not bad, bad
    return tuple(hid.shape)


# ---- single rows ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_layer", [1, 3])
@pytest.mark.parametrize("numerics", ["bf16", "fp32"])
@pytest.mark.parametrize("lx,ly", C.GRID)
def test_single_row_grid(dev, lx, ly, numerics, n_layer):
    """every shape of prefill_edges_cases.GRID (the comment beside each names its edge) into slot 1 of a 2-slot state; M <= 48 and
    rtiles <= 20 of the bf16 GEMM chain; fp32: qsplit = 16"""
    _run_and_check(dev, numerics, n_layer, [(lx, ly)], 2, 260, slot0=1)


def test_bf16_lds_limit_1056_positions_and_the_refusal_beyond(dev):
    """33 key tiles, the most the MFMA attention stages (one layer: 1056 rows; rtiles = 33: QKV / W1 at four tiles); one position
    more is refused with a message naming the mode"""
    shape = _run_and_check(dev, "bf16", 1, [C.BF16_LDS_MAX], 1, 1057)
    assert shape[1] == 1056
    m = _model("bf16", 1, 1, 1057, dev)
    x, y, bert = C.request(0, 700, 357)
    with torch.inference_mode():
        xy, xl, yl, _, _ = m.embed_prompt([_T(x, dev)], [_T(y, dev)], [_T(bert, dev)])
        with pytest.raises(RuntimeError, match="bf16 mode"):
            m.prefill(1, 0, xy, xl, yl)


@pytest.mark.parametrize("n_layer", [1, 3])
def test_fp32_lds_limit_591_positions_and_the_refusal_beyond(dev, n_layer):
    """the most the fp32 attention stages (10 staging rounds, the last one clamped); one position more is refused"""
    shape = _run_and_check(dev, "fp32", n_layer, [C.FP32_LDS_MAX], 2, 592, slot0=1)
    assert shape[1] == 591
    m = _model("fp32", n_layer, 2, 592, dev)
    x, y, bert = C.request(0, 400, 192)
    with torch.inference_mode():
        xy, xl, yl, _, _ = m.embed_prompt([_T(x, dev)], [_T(y, dev)], [_T(bert, dev)])
        with pytest.raises(RuntimeError, match="fp32 mode"):
            m.prefill(2, 1, xy, xl, yl)


@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_cache_exactly_full(dev, numerics):
    """64 positions into slot 0 of a (2, 64) state: all 64 rows right (the `t < T` guards), slot 1 untouched"""
    _run_and_check(dev, numerics, 3, [C.FULL], 2, 64, slot0=0)


# ---- packed ragged passes into permuted slots -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_layer", [1, 3])
def test_bf16_pack_with_whole_blocks_and_waves_of_pad(dev, n_layer):
    """six rows of 2 .. 257 positions in a 7-slot state: the 2-position row's second and third block are all pad (qlast < 0, nkt = 0), three
    waves of its first block too (wkt = 0); rows are written by the block that owns the query, into the row's own slot"""
    rows, S, slots = C.PACK_PAD
    _run_and_check(dev, "bf16", n_layer, rows, S, 260, slots=slots)


@pytest.mark.parametrize("n_layer", [1, 3])
def test_bf16_pack_rtiles_21_to_39(dev, n_layer):
    """M = 4 x 257 = 1028 rows, rtiles = 33 (ragged last tile: 4 rows): QKV / W1 at four column tiles per block, out-proj / W2 at two"""
    rows, S, slots = C.PACK_4
    shape = _run_and_check(dev, "bf16", n_layer, rows, S, 260, slots=slots)
    assert 21 <= -(-shape[0] * shape[1] // 32) <= 39 and shape[0] * shape[1] % 32, shape


@pytest.mark.parametrize("n_layer", [1, 3])
def test_bf16_pack_rtiles_40_to_99(dev, n_layer):
    """M = 7 x 257 = 1799 rows, rtiles = 57 (ragged last tile: 7 rows): cpb = 4"""
    rows, S, slots = C.PACK_7
    shape = _run_and_check(dev, "bf16", n_layer, rows, S, 260, slots=slots)
    assert 40 <= -(-shape[0] * shape[1] // 32) <= 99 and shape[0] * shape[1] % 32, shape


@pytest.mark.parametrize("numerics", ["bf16", "fp8"])
def test_pack_of_3341_rows_runs_the_wide_gemm(dev, numerics):
    """M = 13 x 257 = 3341 >= 3072 rows (one layer): bgemm_wide_kernel, 26.1 groups of 128 rows.  On the fp8 handle too: its prompt path is
    the bf16 one (T2SOracle._prefill_rows), wide kernel included -- M >= 3200 there does NOT reach bgemm_kernel's cpb = 8 (module docstring)"""
    rows, S, slots = C.PACK_13
    shape = _run_and_check(dev, numerics, 1, rows, S, 260, slots=slots)
    assert shape[0] * shape[1] >= 3200 and shape[0] * shape[1] % 128, shape


def test_pack_of_3341_rows_on_bgemm_cpb8_with_the_wide_gemm_off():
    """rtiles = 105 >= 100 on bgemm_kernel: eight column tiles per block (cpb = 8).  bgemm_wide_kernel takes every such pass unless
    GSV_WIDE_MIN_M moves its threshold, and the library reads that once per process: so the case above runs again in a process of its own
    that has the threshold beyond every pass.  (This test is about that process: nothing else here starts one.)"""
    import subprocess
    env = dict(os.environ, GSV_WIDE_MIN_M="1000000")
    node = "%s::test_pack_of_3341_rows_runs_the_wide_gemm[bf16]" % os.path.abspath(__file__)
    p = subprocess.run([sys.executable, "-m", "pytest", node, "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       timeout=120)
    print("".join(ln + "\n" for ln in p.stdout.splitlines() if "prefill edges" in ln or "passed" in ln or "failed" in ln))
    assert p.returncode == 0 and "1 passed" in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]


@pytest.mark.parametrize("n_layer", [1, 3])
@pytest.mark.parametrize("nrows", [1, 2, 4, 8, 17])
def test_fp32_pack_every_query_split(dev, nrows, n_layer):
    """qsplit = 16 / 8 / 4 / 2 / 1 query slices per (head, row) at 1 / 2 / 4 / 8 / 17 rows (the cache is written by slice 0 only); row 0
    has 69 positions: a second, clamped staging round; every other row ends inside the first"""
    rows, S, slots = C.PACKS_F32[nrows]
    shape = _run_and_check(dev, "fp32", n_layer, rows, S, 72, slots=slots)
    assert shape[:2] == (nrows, 69)
    assert max(1, min(16, 256 // (16 * nrows))) == {1: 16, 2: 8, 4: 4, 8: 2, 17: 1}[nrows]


def test_first_sample_margin_share():
    """the first sample is asserted above wherever the oracle's gap clears the margin: that must be at least 90 % of the rows of either
    regime (a property of the seeds, on the oracle alone: tests/test_prefill_edges_cpu.py holds the same)"""
    for reg, (ok, n) in C.margin_share(C.all_cases()).items():
        assert n > 50 and ok >= C.MARGIN_SHARE * n, (reg, ok, n)
