"""The per-sequence decode kernels request their first GEMV's weight rows (QKV, W1) per wave role: the LayerNorm's owner waves
where nothing stands between a wave and its park(), the other eight behind the partial-sum barrier (csrc/t2s_decode.h, "Latency
discipline").  Each role then has its own counted `vmcnt` wait in front of its dots, and a wait that is one load short shows as
a wrong QKV or W1 row, not as a crash: so the hidden states are held against the oracle in the matching numerics, and two runs
against each other bit for bit.

Shapes: 3 layers (layer 0 takes its input directly, layers 1-2 and the logits kernel run the partial-sum prologue), cache length
1 024, batch 1 and 4 (64 FFN slices), 5 (32 slices, K/V rows loaded non-temporally) and 16; cache lengths per sequence around the
edges of the attention waves' deferred first chunk (512 positions on bf16 handles, 256 on fp32 ones) and of its row iterations
(128 / 256 rows): 127, 128, 129, 511, 512, and whatever three steps add to them.  The K/V rows are random bf16 values written into
the oracle's cache and copied into the library's (the step itself is what is compared, as in tests/test_hip_t2s_lowp.py).

Bounds: bf16 handles HID_TOL of tests/test_hip_t2s_lowp.py (1e-3, three layers, measured there against the bf16-mode oracle at one
sequence), except where the PARENT build (45c2236, the load order before this change) already exceeds it on these inputs: a
one-ulp bf16 operand flip behind a 1e-6 difference of the fp32 summation order (that file's docstring) is the more likely the more
sequences and steps there are.  Parent, max |hidden - oracle| over the three steps: B = 1 3.14e-05, B = 4 1.68e-03, B = 5 1.16e-03,
B = 16 9.22e-04 -- so B = 4 and 5 are held to twice the parent's maximum, 1 and 16 to HID_TOL.  (The new order gives the same
figures to the last digit: the arithmetic did not move.)  fp32 handles: ATOL of tests/test_hip_t2s.py (2e-5); parent 1.4e-06 / 2.2e-06.
"""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

HID_TOL = 1e-3           # tests/test_hip_t2s_lowp.py
# per batch shape: HID_TOL, or twice the parent build's measured maximum where that exceeds HID_TOL (module docstring)
BF16_TOL = {1: HID_TOL, 4: 2 * 1.68e-3, 5: 2 * 1.16e-3, 16: HID_TOL}
F32_TOL = 2e-5           # tests/test_hip_t2s.py (ATOL)
T_CACHE = 1024
N_LAYER = 3
# cache length of sequence i before the first step
LENS = [127, 128, 129, 511, 512, 33, 64, 255, 256, 257, 300, 383, 384, 385, 448, 509]
LENS_BY_B = {1: [127], 4: [127, 129, 511, 512], 5: LENS[:5], 8: LENS[:8], 16: LENS}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    cfg = synth.gpt_config(n_layer=N_LAYER)
    return cfg, synth.gpt_weights(cfg, seed=4321)


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(cfg, w, cache, dtype, dev):
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(w)
    m.initialize_runtime(dtype, dev, cache)
    return m


def _round_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _prime(m, B, dev, seed):
    """a short prompt pass per sequence: every piece of the bound state is what real use leaves there"""
    rs = [synth.synth_request(800 + i, 3, 4 + i % 3, 5 + i % 4, seed=seed, bert="random") for i in range(B)]
    xy, xl, yl, xlh, ylh = m.embed_prompt([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs])
    m.prefill(B, 0, xy, xl, yl)
    return (xlh + ylh).numpy()


def _hidden_vs_oracle(cfg, w, B, dtype, numerics, dev):
    from oracle import oracle as orc
    cache = [(B, T_CACHE)]
    lens = np.array(LENS_BY_B[B], np.int64)
    m = _model(cfg, w, cache, dtype, dev)
    o = orc.T2SOracle(cfg, w, cache, numerics=numerics, batched_min=m.batched_min, ffn_slices=m.ffn_slices)
    _prime(m, B, dev, 4321)
    rng = np.random.default_rng(100 + B)
    kc, vc = o.cache[B]
    for b in range(B):       # rows beyond a sequence's length stay zero on both sides
        kc[:, b, :, :lens[b]] = _round_bf16(rng.normal(size=(N_LAYER, 16, lens[b], 32)).astype(np.float32))
        vc[:, b, :, :lens[b]] = _round_bf16(rng.normal(size=(N_LAYER, 16, lens[b], 32)).astype(np.float32))
    rt = m._rt[B]
    with torch.inference_mode():
        rt["k"].copy_(torch.from_numpy(kc).to(dev).to(rt["k"].dtype))
        rt["v"].copy_(torch.from_numpy(vc).to(dev).to(rt["v"].dtype))
        rt["kv_len"].copy_(torch.from_numpy(lens).to(dev))
    kv = lens.copy()
    errs = []
    for _ in range(3):
        xin = rng.normal(size=(B, 512)).astype(np.float32)
        want = o.decode(xin, B, kv)
        got = m.decode_hidden(B, _T(xin, dev)).cpu().numpy()
        kv += 1
        assert np.array_equal(rt["kv_len"].cpu().numpy(), kv)
        errs.append(float(np.abs(got - want).max()))
    # the rows the three steps appended in the layers behind layer 0 (the ones whose QKV rows were requested per role)
    d = np.concatenate([np.abs(t[1:, b, :, lens[b]:lens[b] + 3].float().cpu().numpy() - oc[1:, b, :, lens[b]:lens[b] + 3]).ravel()
                        for b in range(B) for t, oc in ((rt["k"], kc), (rt["v"], vc))])
    del m
    return errs, float(d.max()), float(d.mean())


@pytest.mark.parametrize("B", [1, 4, 5, 16])
def test_bf16_decode_hidden_vs_bf16_oracle(dev, weights, B):
    cfg, w = weights
    errs, kv_max, kv_mean = _hidden_vs_oracle(cfg, w, B, torch.bfloat16, "bf16", dev)
    print("decode hidden vs bf16 oracle, B=%d, cache %d: max per step %s; appended K/V rows max %.2e mean %.2e"
          % (B, T_CACHE, ["%.2e" % e for e in errs], kv_max, kv_mean))
    assert max(errs) < BF16_TOL[B], errs
    # bf16 rows behind upstream one-ulp flips: the bounds tests/test_hip_t2s_lowp.py holds the prompt pass's later layers to
    assert kv_max < 1e-1 and kv_mean < 5e-3, (kv_max, kv_mean)


@pytest.mark.parametrize("B", [1, 8])
def test_fp32_decode_hidden_vs_fp32_oracle(dev, weights, B):
    cfg, w = weights
    errs, kv_max, _ = _hidden_vs_oracle(cfg, w, B, torch.float32, "fp32", dev)
    print("decode hidden vs fp32 oracle, B=%d, cache %d: max per step %s; appended K/V rows max %.2e"
          % (B, T_CACHE, ["%.2e" % e for e in errs], kv_max))
    assert max(errs) < F32_TOL, errs
    assert kv_max < F32_TOL, kv_max


@pytest.mark.parametrize("B", [1, 5])
def test_decode_hidden_run_to_run_and_graph_replay_bit_equal(dev, weights, B):
    """two fresh models, the same weights and inputs, eight decode_hidden steps: bit-equal between the two, and between eager
    launches and the replay of one captured step (the kernels read every position from the state; the first step is launched
    eagerly in every run, so nothing is loaded or allocated for the first time inside the capture)"""
    cfg, w = weights
    cache = [(B, T_CACHE)]
    rng = np.random.default_rng(7 + B)
    xs = [rng.normal(size=(B, 512)).astype(np.float32) for _ in range(8)]
    outs = []
    for mode in ("eager", "eager", "graph"):
        m = _model(cfg, w, cache, torch.bfloat16, dev)
        _prime(m, B, dev, 99)
        xin = torch.zeros(B, 512, dtype=torch.float32, device=dev)
        res = []
        with torch.inference_mode():
            g = None
            for i, x in enumerate(xs):
                xin.copy_(_T(x, dev))
                if mode == "graph" and i == 1:
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        m.decode_hidden(B, xin)
                if g is None:
                    m.decode_hidden(B, xin)
                else:
                    g.replay()
                res.append(m._rt[B]["hidden"].cpu().numpy().copy())
        outs.append(np.stack(res))
        del m, g
    assert np.isfinite(outs[0]).all() and np.abs(outs[0][-1] - outs[0][0]).max() > 1e-3
    assert np.array_equal(outs[0], outs[1]), "two eager runs differ"
    assert np.array_equal(outs[0], outs[2]), "graph replay differs from eager launches"
