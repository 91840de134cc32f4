"""The decode step's STAGED loads (csrc/t2s_decode.h, "Latency discipline"): the attention kernel requests the first chunk's K/V
rows behind the partial-sum barrier, on the eight waves that own no LayerNorm element (bf16), and its out-proj panel behind the
QKV dots; the FFN kernel requests its W2 panel behind the partial-sum barrier.  Only the position of load instructions moved, so
every token must be what it was.  These cases sit where a moved load could show:

  * the chunk edge -- kv crossing the number of positions one register chunk holds (256 fp32, 512 bf16), where the first
    chunk's deferred registers and the loop's own loads meet;
  * the other launch shapes of the same kernels -- 64 FFN slices (<= 4 sequences), 32 slices with non-temporal K/V (5);
  * graph replay against eager launches -- a deferred load that raced the step's own K/V append would show under one timing only.

Three layers, seeded weights with eos_gain = 0 (fixed-length runs).  Every seed was chosen with the CPU oracle ALONE so that
the oracle's smallest top-1 / top-2 logit gap over the compared steps clears the bound the test states; the tests assert that
gap, they do not skip on it."""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

FP32_MARGIN = 1e-3       # two hundred times the fp32 summation-order noise (tests/test_hip_bench_size.py)
TOKEN_MARGIN = 5e-2      # the bf16 gate: tests/test_hip_t2s_lowp.py TOKEN_MARGIN (its docstring derives it), used by the bench-shape
                         # bf16 test there (test_bf16_greedy_tokens_bench_shape_vs_bf16_oracle)
N_NEW = 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cfg():
    return synth.gpt_config(n_layer=3)


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(cfg, w, cache, dtype, dev):
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(w)
    m.initialize_runtime(dtype, dev, cache)
    return m


def _first_mismatch(tok, ref):
    nm = min(len(tok), len(ref))
    neq = np.nonzero(np.asarray(tok[:nm]) != np.asarray(ref[:nm]))[0]
    return int(neq[0]) if neq.size else None


def _single(cfg, dev, seed, dtype, numerics, n_prompt_tok, T):
    """prompt of 100 phonemes + n_prompt_tok tokens, N_NEW greedy tokens: (tokens, oracle tokens, oracle margins)"""
    from oracle import oracle as orc
    w = synth.gpt_weights(cfg, seed=seed, eos_gain=0.0)
    x, y, bert, _ = synth.synth_request(0, 40, 60, n_prompt_tok, seed=seed, bert="random")
    L = len(x) + len(y)
    o = orc.T2SOracle(cfg, w, [(1, L + N_NEW)], numerics=numerics)     # the oracle stops when its cache is full: N_NEW tokens
    ref = o.infer(x, y, bert, top_k=1)
    m = _model(cfg, w, [(1, T)], dtype, dev)
    tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, max_new_tokens=N_NEW)[0, 0].cpu().numpy()
    assert len(ref) == N_NEW and len(tok) == N_NEW, (len(ref), len(tok))
    return L, tok, ref, np.asarray(o.margins)


def test_fp32_tokens_bit_exact_across_the_chunk_edge(cfg, dev):
    """kv 250 -> 262 crosses 256, the positions of one fp32 register chunk: the deferred first-chunk loads and the loop's."""
    L, tok, ref, mm = _single(cfg, dev, 12, torch.float32, "fp32", 150, 512)
    assert L == 250
    print("fp32 chunk edge: oracle min margin %.3e" % mm.min())
    assert mm.min() >= FP32_MARGIN, mm.min()          # seed 12: 1.4e-1 (chosen on the CPU with the oracle alone)
    assert np.array_equal(tok, ref), (tok, ref)


def test_bf16_tokens_match_the_bf16_oracle_across_the_chunk_edge(cfg, dev):
    """kv 506 -> 518 crosses 512, the positions of one bf16 register chunk."""
    L, tok, ref, mm = _single(cfg, dev, 14, torch.bfloat16, "bf16", 406, 1024)
    assert L == 506
    print("bf16 chunk edge: oracle min margin %.3e" % mm.min())
    assert mm.min() >= TOKEN_MARGIN, mm.min()         # seed 14: 3.0e-1: no step of the window is below the gate
    first = _first_mismatch(tok, ref)
    assert first is None, (first, mm[first + 1], tok, ref)


# B = 3: 64 FFN slices (NJ = 64 attention / FFN instantiations); B = 5: 32 slices and non-temporal K/V rows
@pytest.mark.parametrize("B,seed", [(3, 12), (5, 21)])
def test_bf16_batched_launch_shapes_match_the_bf16_oracle(cfg, dev, B, seed):
    from oracle import oracle as orc
    n_new = 10
    w = synth.gpt_weights(cfg, seed=seed, eos_gain=0.0)
    rng = np.random.default_rng(seed)
    shapes = []
    for _ in range(B):                                 # ragged prompts of 20-60 positions
        tot = int(rng.integers(20, 61)); p = int(rng.integers(2, 8)); n = int(rng.integers(4, tot - 8))
        shapes.append((p, tot - p - n, n))
    rs = [synth.synth_request(100 + i, p, t, n, seed=seed, bert="random") for i, (p, t, n) in enumerate(shapes)]
    cache = [(B, 96)]
    m = _model(cfg, w, cache, torch.bfloat16, dev)
    assert m.ffn_slices(B) == (64 if B <= 4 else 32) and B < m.batched_min
    o = orc.T2SOracle(cfg, w, cache, numerics="bf16", batched_min=m.batched_min, ffn_slices=m.ffn_slices)
    ref, ref_idx = o.infer_batched([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], top_k=1)   # runs on to a full cache
    ref_by_req = {int(i): t for i, t in zip(ref_idx, ref)}
    pred, idx = m.infer_batched([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs], top_k=1,
                                max_new_tokens=[n_new] * B)
    assert sorted(idx.tolist()) == list(range(B))
    gap = min(min(o.req_margins[i][:n_new + 1]) for i in range(B))
    print("B = %d: oracle min margin over the compared steps %.3e" % (B, gap))
    assert gap >= TOKEN_MARGIN, gap                    # seeds 12 / 21: 1.2e-1 / 1.7e-1
    for req, tok in zip(idx.tolist(), pred):
        tok = tok.cpu().numpy()
        want = ref_by_req[req][:n_new]
        assert len(tok) == n_new and len(want) == n_new, (req, len(tok), len(want))
        assert np.array_equal(tok, want), (req, tok, want)


def test_bf16_graph_replay_equals_eager_launches(cfg, dev):
    """five-step window graphs against one launch at a time: the same kernels under two timings"""
    w = synth.gpt_weights(cfg, seed=14, eos_gain=0.0)
    x, y, bert, _ = synth.synth_request(1, 40, 60, 100, seed=14, bert="random")
    out = []
    for graph in (True, False):
        m = _model(cfg, w, [(1, 256)], torch.bfloat16, dev)
        m.use_graph = graph
        out.append(m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, max_new_tokens=20)[0, 0].cpu().numpy())
        del m
    assert len(out[0]) == 20 and np.array_equal(out[0], out[1]), out
