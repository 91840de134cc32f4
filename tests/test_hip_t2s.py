"""GPU parity tests of the GPT path: HIP kernels (through the C ABI) vs the CPU oracle and vs the
golden vectors produced by the imported reference.

fp32 mode is the parity mode: float tensors within 2e-5 abs, greedy token ids BIT-EXACT
(north_star: "bit-exact token ids from greedy AR decode").  bf16 mode (the production dtype,
as the reference on GPU) is checked for bounded error and margin-gated token agreement."""
import os

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu
ATOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(cfg, w, cache, dtype, dev):
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(w)
    m.initialize_runtime(dtype, dev, cache)
    return m


def test_layers_fp32_match_reference_golden(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, "t2s_layers.npz"))
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=int(g["seed"])), [(1, 96), (2, 96)], torch.float32, dev)
    x, y, bert = g["s_x"], g["s_y"], g["s_bert"]
    L = len(x) + len(y)
    xy, xl, yl, _, _ = m.embed_prompt([_T(x, dev)], [_T(y, dev)], [_T(bert, dev)])
    np.testing.assert_allclose(xy.cpu().numpy(), g["s_xy"], atol=ATOL)
    m.prefill(1, 0, xy, xl, yl)
    np.testing.assert_allclose(xy.cpu().numpy(), g["s_hidden"], atol=ATOL)      # xy now holds the hidden states
    np.testing.assert_allclose(m._rt[1]["hidden"].cpu().numpy()[0], g["s_hidden"][0, -1], atol=ATOL)
    np.testing.assert_allclose(m._rt[1]["k"].cpu().numpy()[:, 0, :, :L], g["s_k"], atol=ATOL)
    np.testing.assert_allclose(m._rt[1]["v"].cpu().numpy()[:, 0, :, :L], g["s_v"], atol=ATOL)
    assert m._rt[1]["kv_len"].tolist() == [L] and m._rt[1]["x_len"].tolist() == [len(x)]
    hd = m.decode_hidden(1, _T(g["d_x"][0], dev))
    np.testing.assert_allclose(hd.cpu().numpy(), g["d_hidden"][0], atol=ATOL)
    np.testing.assert_allclose(m._rt[1]["k"].cpu().numpy()[:, 0, :, L], g["d_k_new"], atol=ATOL)
    assert m._rt[1]["kv_len"].tolist() == [L + 1]
    # packed batch [x_b | y_b | pad]
    xs = [g["b0_x"], g["b1_x"]]; ys = [g["b0_y"], g["b1_y"]]; bs = [g["b0_bert"], g["b1_bert"]]
    xy, xl, yl, _, _ = m.embed_prompt([_T(a, dev) for a in xs], [_T(a, dev) for a in ys], [_T(a, dev) for a in bs])
    np.testing.assert_allclose(xy.cpu().numpy(), g["b_xy"], atol=ATOL)
    m.prefill(2, 0, xy, xl, yl)
    h = xy.cpu().numpy()
    assert np.isfinite(h).all()
    for b in range(2):
        n = len(xs[b]) + len(ys[b])
        np.testing.assert_allclose(h[b, :n], g["b_hidden"][b, :n], atol=ATOL)


@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("graph", [True, False])
def test_greedy_infer_fp32_bit_exact(golden_dir, dev, name, graph):
    """the 2-kernels-per-layer decode step, replayed from a hipGraph or launched eagerly"""
    g = np.load(os.path.join(golden_dir, "t2s_infer.npz"))
    seed, p, t, n = (int(v) for v in g[name + "_cfg"])
    cfg = synth.gpt_config()
    w = synth.gpt_weights(cfg, seed=seed, eos_gain=float(g[name + "_eos_gain"]))
    m = _model(cfg, w, [tuple(int(v) for v in c) for c in g[name + "_cache"]], torch.float32, dev)
    m.use_graph = graph
    x, y = g[name + "_x"], g[name + "_y"]
    tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], torch.zeros(1, len(x), 1024, device=dev), top_k=1)
    assert tok.shape[:2] == (1, 1) and tok.dtype == torch.int64
    assert np.array_equal(tok[0, 0].cpu().numpy(), g[name + "_tokens"])


@pytest.mark.parametrize("name", ["r", "s"])
def test_greedy_infer_batched_fp32_bit_exact(golden_dir, dev, name):
    """continuous batching with slot refill: tokens, completion order and semantic_orig_idx."""
    g = np.load(os.path.join(golden_dir, "t2s_batched.npz"))
    seed = int(g[name + "_seed"])
    cfg = synth.gpt_config()
    w = synth.gpt_weights(cfg, seed=seed, eos_gain=float(g[name + "_eos_gain"]))
    m = _model(cfg, w, [tuple(int(v) for v in c) for c in g[name + "_cache"]], torch.float32, dev)
    rs = [synth.synth_request(200 + i, int(p), int(t), int(n), seed=seed) for i, (p, t, n) in enumerate(g[name + "_reqs"])]
    pred, orig = m.infer_batched([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs], top_k=1)
    assert orig.tolist() == g[name + "_orig"].tolist()
    assert len(pred) == int(g[name + "_n"])
    for i, pt in enumerate(pred):
        assert np.array_equal(pt.cpu().numpy(), g["%s_tok%d" % (name, i)]), i


def test_greedy_infer_matches_oracle_on_fresh_inputs(dev):
    """not only the committed fixtures: a fresh seeded case against the oracle run on this box,
    including an EOS stop (negative eos_gain makes EOS win right after the suppression window)."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=6)
    for seed, eg, cache in [(77, 1.0, [(1, 64), (1, 100)]), (78, -8.0, [(1, 128)])]:
        w = synth.gpt_weights(cfg, seed=seed, eos_gain=eg)
        x, y, bert, _ = synth.synth_request(5, 7, 13, 17, seed=seed, bert="random")
        o = orc.T2SOracle(cfg, w, cache)
        ref = o.infer(x, y, bert, top_k=1)
        if min(o.margins) < 1e-3:
            pytest.skip("oracle margin too small for a bit-exact claim")
        m = _model(cfg, w, cache, torch.float32, dev)
        tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1)[0, 0].cpu().numpy()
        assert np.array_equal(tok, ref), (seed, tok, ref)
        if eg < 0:
            assert len(ref) < 128 - len(x) - len(y), "EOS case did not stop early"


def test_bf16_bounded_error_and_margin_gated_tokens(golden_dir, dev):
    """production dtype: bf16 weights + KV cache, fp32 accumulate.  Tokens must equal the fp32
    oracle up to the first step whose oracle decision margin is below the bf16 noise bound."""
    from oracle import oracle as orc
    g = np.load(os.path.join(golden_dir, "t2s_layers.npz"))
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=int(g["seed"])), [(1, 96), (2, 96)], torch.bfloat16, dev)
    x, y, bert = g["s_x"], g["s_y"], g["s_bert"]
    xy, xl, yl, _, _ = m.embed_prompt([_T(x, dev)], [_T(y, dev)], [_T(bert, dev)])
    m.prefill(1, 0, xy, xl, yl)
    assert np.abs(xy.cpu().numpy() - g["s_hidden"]).max() < 5e-2
    gi = np.load(os.path.join(golden_dir, "t2s_infer.npz"))
    cfg = synth.gpt_config()
    BF16_MARGIN = 0.35   # logits std ~6, bf16 weight rounding ~2^-9 relative => ~1e-1 logit noise
    for name in "abc":
        seed, p, t, n = (int(v) for v in gi[name + "_cfg"])
        w = synth.gpt_weights(cfg, seed=seed, eos_gain=float(gi[name + "_eos_gain"]))
        cache = [tuple(int(v) for v in c) for c in gi[name + "_cache"]]
        o = orc.T2SOracle(cfg, w, cache)
        xx, yy = gi[name + "_x"], gi[name + "_y"]
        ref = o.infer(xx, yy, np.zeros((len(xx), 1024), np.float32), top_k=1)
        mm = _model(cfg, w, cache, torch.bfloat16, dev)
        tok = mm.infer(_T(xx, dev)[None], _T(yy, dev)[None], torch.zeros(1, len(xx), 1024, device=dev), top_k=1)[0, 0].cpu().numpy()
        nm = min(len(tok), len(ref))
        neq = np.nonzero(tok[:nm] != ref[:nm])[0]
        if neq.size:
            first = int(neq[0])
            # output token i is sample s_{i+1}; margins[0] belongs to the prefill sample
            assert o.margins[first + 1] < BF16_MARGIN, (name, first, o.margins[first + 1])
            assert first >= 8, "bf16 diverged suspiciously early"


def test_stochastic_sampling_runs_and_respects_rules(dev):
    """top_k=15 host-sampled path (tok_override): tokens in range, no suppressed token in the first
    steps, deterministic under a seeded generator."""
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=3)
    m = _model(cfg, w, [(1, 96)], torch.float32, dev)
    x, y, bert, _ = synth.synth_request(9, 6, 10, 14, seed=3)
    outs = []
    for _ in range(2):
        gen = torch.Generator(device=dev); gen.manual_seed(1234)
        tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=15, generator=gen)[0, 0].cpu().numpy()
        outs.append(tok)
        assert tok.min() >= 0 and tok.max() < 1025 and len(tok) > 0
        assert not set(tok[:8].tolist()) & {280, 486, 1024}
    assert np.array_equal(outs[0], outs[1])


def test_bucket_hop_and_full_cache_fp32(dev):
    """the last sample is taken when the KV cache is exactly full (pre_tokens column T) and a hop
    between nested buckets changes nothing: [(1,72),(1,100)] must equal [(1,100)] token for token."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=91, eos_gain=0.0)
    x, y, bert, _ = synth.synth_request(3, 6, 9, 11, seed=91)
    outs = []
    for cache in ([(1, 72), (1, 100)], [(1, 100)]):
        m = _model(cfg, w, cache, torch.float32, dev)
        outs.append(m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1)[0, 0].cpu().numpy())
    assert len(outs[0]) == 100 - (len(x) + len(y))          # ran to capacity: max_kv - L tokens
    assert np.array_equal(outs[0], outs[1])
    ref = orc.T2SOracle(cfg, w, [(1, 100)]).infer(x, y, bert, top_k=1)
    assert np.array_equal(outs[0], ref)


def test_prompt_too_long_and_bad_args_raise(dev):
    cfg = synth.gpt_config(n_layer=2)
    m = _model(cfg, synth.gpt_weights(cfg, seed=1), [(1, 48)], torch.float32, dev)
    x, y, bert, _ = synth.synth_request(0, 20, 20, 20, seed=1)        # 60 positions > 48
    with pytest.raises(ValueError):
        m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1)
    from gsv_tts_lite_amd import _native as N
    import ctypes
    with pytest.raises(RuntimeError):                                 # unknown batch size: no state bound
        N.check(N.lib().gsv_t2s_decode(m._h, 7, 1, 0, N.current_stream_ptr(dev)))
    bad = N.T2SConfig(2, 256, 8, 1025, 1024, 4000, 732, 0)            # unsupported hidden size
    h = ctypes.c_void_p()
    assert N.lib().gsv_t2s_create(ctypes.byref(bad), ctypes.byref(h)) == 1
    assert b"unsupported" in N.lib().gsv_last_error()


def test_batched_ragged_lengths_vs_oracle_fresh(dev):
    """ragged batch (lengths 1..) with more requests than slots, oracle computed on this box"""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=5)
    w = synth.gpt_weights(cfg, seed=17, eos_gain=2.5)
    cache = [(4, 96), (4, 120)]
    shapes = [(1, 1, 1), (3, 9, 20), (8, 20, 5), (2, 2, 31), (5, 14, 9), (4, 4, 4), (9, 11, 17)]
    rs = [synth.synth_request(40 + i, p, t, n, seed=17, bert="random") for i, (p, t, n) in enumerate(shapes)]
    o = orc.T2SOracle(cfg, w, cache)
    ref, ref_idx = o.infer_batched([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], top_k=1)
    m = _model(cfg, w, cache, torch.float32, dev)
    pred, idx = m.infer_batched([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs], top_k=1)
    assert idx.tolist() == ref_idx.tolist()
    for a, b in zip(pred, ref):
        assert np.array_equal(a.cpu().numpy(), b)


def test_top_p_and_temperature_path_runs(dev):
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=2), [(1, 80), (2, 80)], torch.float32, dev)
    x, y, bert, _ = synth.synth_request(1, 5, 9, 12, seed=2)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=8, top_p=0.7, temperature=0.8, generator=gen)
    assert tok.shape[-1] > 0 and int(tok.max()) <= 1024
    pred, idx = m.infer_batched([_T(x, dev)] * 3, [_T(y, dev)] * 3, [_T(bert, dev)] * 3, top_k=5, generator=gen)
    assert sorted(idx.tolist()) == [0, 1, 2] and all(len(p) > 0 for p in pred)


def test_prefill_bf16_mfma_attention_packed_batch_and_cache(golden_dir, dev):
    """bf16 mode runs the prompt attention on the matrix cores (t2s_prefill_attn_mfma_kernel): packed ragged
    batch [x_b | y_b | pad] against the reference's golden hidden states, K/V cache rows written for every
    prompt position (and only those), finite everywhere incl. the padded rows.  Lengths of the fixture
    are not multiples of the 32-key / 128-query tiles."""
    g = np.load(os.path.join(golden_dir, "t2s_layers.npz"))
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=int(g["seed"])), [(1, 96), (2, 96)], torch.bfloat16, dev)
    x, y, bert = g["s_x"], g["s_y"], g["s_bert"]
    L = len(x) + len(y)
    with torch.inference_mode():
        m._rt[1]["k"].fill_(7.0); m._rt[1]["v"].fill_(7.0)
    xy, xl, yl, _, _ = m.embed_prompt([_T(x, dev)], [_T(y, dev)], [_T(bert, dev)])
    m.prefill(1, 0, xy, xl, yl)
    assert np.abs(xy.cpu().numpy() - g["s_hidden"]).max() < 5e-2
    k = m._rt[1]["k"].float().cpu().numpy(); v = m._rt[1]["v"].float().cpu().numpy()
    assert np.abs(k[:, 0, :, :L] - g["s_k"]).max() < 5e-2 and np.abs(v[:, 0, :, :L] - g["s_v"]).max() < 5e-2
    assert (k[:, 0, :, L:] == 7.0).all() and (v[:, 0, :, L:] == 7.0).all(), "cache rows beyond the prompt were touched"
    xs = [g["b0_x"], g["b1_x"]]; ys = [g["b0_y"], g["b1_y"]]; bs = [g["b0_bert"], g["b1_bert"]]
    xy, xl, yl, _, _ = m.embed_prompt([_T(a, dev) for a in xs], [_T(a, dev) for a in ys], [_T(a, dev) for a in bs])
    m.prefill(2, 0, xy, xl, yl)
    h = xy.cpu().numpy()
    assert np.isfinite(h).all()
    for b in range(2):
        n = len(xs[b]) + len(ys[b])
        assert np.abs(h[b, :n] - g["b_hidden"][b, :n]).max() < 5e-2, b


def test_device_sampler_matches_its_restatement_and_the_reference_distribution(dev):
    """The token kernel's sampler (ctl[0] == 2): (i) draw by draw against the numpy restatement of the same
    counter-based noise stream (oracle.device_sample), mismatches allowed only where the top-2 scores are
    closer than float noise; (ii) the empirical distribution over 6000 draws against the reference's
    logits_to_probs semantics (temperature, top-k pivot that keeps ties, -inf never drawn) by chi-square."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=1)
    m = _model(cfg, synth.gpt_weights(cfg, seed=5), [(1, 64)], torch.float32, dev)
    rt = m._rt[1]
    V = 1025
    rng = np.random.default_rng(0)
    logits = (rng.standard_normal(V) * 2.5).astype(np.float32)
    logits[[280, 486, 1024]] = -np.inf                    # suppressed entries arrive as -inf
    logits[7] = logits[11] = np.sort(logits)[::-1][14]    # a tie exactly at the top-15 pivot: both must stay
    top_k, temp = 15, 0.8
    ref_p = orc.device_sample_probs(logits, top_k, temp)
    assert (ref_p > 0).sum() >= 16                        # the tie widened the kept set
    n, bad = 6000, 0
    counts = np.zeros(V)
    with torch.inference_mode():
        rt["logits"][0].copy_(torch.from_numpy(logits))
        rt["kv_len"].fill_(3); rt["x_len"].fill_(1); rt["step"].fill_(2)
        for s in range(n):
            seed = 1000003 * s + 17
            m._set_ctl(rt, 2, 0, False, 1.0, top_k, temp, seed)
            m._flush(1)
            tok = int(rt["pre_tokens"][0, 3].item())
            counts[tok] += 1
            want, margin = orc.device_sample(logits, top_k, temp, seed, 0, 3, 2)
            if tok != want:
                assert margin < 1e-4, (s, tok, want, margin)
                bad += 1
    assert bad <= 3
    assert counts[ref_p == 0].sum() == 0, "drew a token outside the kept set"
    exp = ref_p[ref_p > 0] * n
    chi2 = (((counts[ref_p > 0] - exp) ** 2) / exp).sum()
    assert chi2 < 60.0, chi2                              # 15 dof: p ~ 2e-7 at 60
    # top_k >= V and top_k <= 0 keep everything finite; k = 1 is the argmax
    with torch.inference_mode():
        m._set_ctl(rt, 2, 0, False, 1.0, 1, 1.0, 99); m._flush(1)
        assert int(rt["pre_tokens"][0, 3].item()) == int(np.argmax(logits))
        m._set_ctl(rt, 2, 0, False, 1.0, 0, 1.0, 99); m._flush(1)
        assert int(rt["pre_tokens"][0, 3].item()) == orc.device_sample(logits, 0, 1.0, 99, 0, 3, 2)[0]


@pytest.mark.parametrize("top_k", [64, 65, 300, 1024, 1025])
def test_device_sampler_with_many_kept_entries(golden_dir, dev, top_k):
    """top_k beyond 64 up to the whole vocabulary stays on the device (from 65 on the k-th largest entry is found by bisection
    over the floats' order-preserving bit pattern instead of k arg-max rounds; there is no host sampling path): on the logits of
    the reference's own top_k = 300 / 1025 cases (sample.npz c4 / c5, whose probabilities pin oracle.logits_to_probs) and on
    logits with ties AT the pivot and fewer finite entries than k, draw by draw against oracle.device_sample, and never a token
    outside the kept set."""
    from oracle import oracle as orc
    g = np.load(os.path.join(golden_dir, "sample.npz"))
    cfg = synth.gpt_config(n_layer=1)
    m = _model(cfg, synth.gpt_weights(cfg, seed=5), [(1, 64)], torch.float32, dev)
    rt = m._rt[1]
    V = 1025
    rng = np.random.default_rng(top_k)
    tie = (rng.standard_normal(V) * 2.0).astype(np.float32)
    if top_k < V:
        piv = np.sort(tie)[::-1][top_k - 1]
        tie[[3, 900]] = piv                                # two more entries exactly at the pivot: all of them stay
    few = np.full(V, -np.inf, np.float32)
    few[rng.choice(V, 40, replace=False)] = (rng.standard_normal(40) * 3).astype(np.float32)   # 40 finite entries < k
    cases = [g["c4_logits"][0], g["c5_logits"][1], tie, few]
    temp = 0.9
    with torch.inference_mode():
        for ci, logits in enumerate(cases):
            logits = logits.astype(np.float32)
            ref_p = orc.device_sample_probs(logits, top_k, temp)
            rt["logits"][0].copy_(torch.from_numpy(logits))
            rt["kv_len"].fill_(3); rt["x_len"].fill_(1); rt["step"].fill_(2)
            bad = 0
            for s_ in range(300):
                seed = 7919 * s_ + 31 * ci + 5
                m._set_ctl(rt, 2, 0, False, 1.0, top_k, temp, seed)
                m._flush(1)
                tok = int(rt["pre_tokens"][0, 3].item())
                assert ref_p[tok] > 0, (ci, s_, tok)
                want, margin = orc.device_sample(logits, top_k, temp, seed, 0, 3, 2)
                if tok != want:
                    assert margin < 1e-4, (ci, s_, tok, want, margin)
                    bad += 1
            assert bad <= 2, (ci, bad)


def test_device_and_host_sampling_paths_agree_on_rules(dev):
    """default-parameter inference (top_k=15, repetition penalty) and a wide top_k = 400 through the device sampler (the only
    sampling path): deterministic under a seeded generator, tokens in range, no suppressed token in the first steps;
    infer_batched with slot refill runs on it too."""
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=3)
    m = _model(cfg, w, [(1, 96), (2, 96)], torch.float32, dev)
    x, y, bert, _ = synth.synth_request(9, 6, 10, 14, seed=3)
    assert not hasattr(m, "device_sampling")
    for top_k in (15, 400):
        outs = []
        for _ in range(2):
            gen = torch.Generator(device=dev); gen.manual_seed(4321)
            tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=top_k, generator=gen)[0, 0].cpu().numpy()
            outs.append(tok)
            assert tok.min() >= 0 and tok.max() < 1025 and len(tok) > 0
            assert not set(tok[:8].tolist()) & {280, 486, 1024}
        assert np.array_equal(outs[0], outs[1]), top_k
    gen = torch.Generator(device="cpu"); gen.manual_seed(1)
    pred, idx = m.infer_batched([_T(x, dev)] * 5, [_T(y, dev)] * 5, [_T(bert, dev)] * 5, top_k=15, generator=gen)
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4] and all(len(p) > 0 and int(p.max()) < 1025 for p in pred)


@pytest.mark.parametrize("name", ["e", "f"])
def test_greedy_infer_stream_fp32_matches_reference_golden(golden_dir, dev, name):
    """every (cumulative chunk, is_final) of t2s_model.infer_stream, bit-exact in fp32 mode (the final chunk
    after an EOS still starts with the first sample; chunks lag one behind unless boosted)."""
    g = np.load(os.path.join(golden_dir, "t2s_stream.npz"))
    seed, p, t, n, chunk, boost = (int(v) for v in g[name + "_cfg"])
    cfg = synth.gpt_config()
    w = synth.gpt_weights(cfg, seed=seed, eos_gain=float(g[name + "_eos_gain"]))
    m = _model(cfg, w, [tuple(int(v) for v in c) for c in g[name + "_cache"]], torch.float32, dev)
    x, y = g[name + "_x"], g[name + "_y"]
    got = list(m.infer_stream(_T(x, dev)[None], _T(y, dev)[None], torch.zeros(1, len(x), 1024, device=dev), top_k=1,
                              stream_chunk=chunk, boost_first_chunk=bool(boost)))
    assert len(got) == int(g[name + "_n"])
    for i, (c, fin) in enumerate(got):
        assert c.dim() == 3 and c.shape[:2] == (1, 1)
        assert np.array_equal(c[0, 0].cpu().numpy(), g["%s_chunk%d" % (name, i)]) and int(fin) == int(g["%s_final%d" % (name, i)]), (name, i)


def test_batched_step_bf16_mfma_path_margin_gated(dev):
    """bf16 with >= 36 slots runs the batched step (rowgemm GEMM chain on B rows + t2s_batch_attn2_kernel; weights
    streamed once per step).  43 ragged requests through 40 slots (three refills), greedy: tokens must equal the
    fp32 oracle's continuous-batching output up to the first step whose oracle top-1/top-2 margin is below the
    bf16 noise bound; completion order bookkeeping must be a permutation."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=23, eos_gain=2.0)
    cache = [(40, 128)]
    rng = np.random.default_rng(1)
    shapes = [(int(rng.integers(1, 9)), int(rng.integers(2, 20)), int(rng.integers(1, 30))) for _ in range(43)]
    rs = [synth.synth_request(70 + i, p, t, n, seed=23, bert="random") for i, (p, t, n) in enumerate(shapes)]
    o = orc.T2SOracle(cfg, w, cache)
    ref, ref_idx = o.infer_batched([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], top_k=1)
    ref_by_req = {int(i): t for i, t in zip(ref_idx, ref)}
    m = _model(cfg, w, cache, torch.bfloat16, dev)
    pred, idx = m.infer_batched([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs], top_k=1)
    assert sorted(idx.tolist()) == list(range(43))
    BF16_MARGIN = 0.35
    exact = 0
    for req, tok in zip(idx.tolist(), pred):
        tok = tok.cpu().numpy()
        want = ref_by_req[req]
        nm = min(len(tok), len(want))
        neq = np.nonzero(tok[:nm] != want[:nm])[0]
        if neq.size == 0 and len(tok) == len(want):
            exact += 1
            continue
        first = int(neq[0]) if neq.size else nm
        # the oracle's decision margins for this request (single-sequence run with the batched path's rules)
        o1 = orc.T2SOracle(cfg, w, [(1, 128)])
        single = o1.infer(rs[req][0], rs[req][1], rs[req][2], top_k=1, repetition_penalty=1.0, initial_suppression_steps=0)
        if len(single) >= first and np.array_equal(single[:first], want[:first]) and first + 1 < len(o1.margins):
            assert o1.margins[first + 1] < BF16_MARGIN, (req, first, o1.margins[first + 1])
    assert exact >= 30, exact


@pytest.mark.parametrize("top_k,top_p,temp", [(15, 0.6, 1.0), (0, 0.85, 0.7)])
def test_device_sampler_top_p(dev, top_k, top_p, temp):
    """top-p on device (bisection for the {p >= tau} set instead of sort + cumsum): the kept set must be the
    reference's (oracle.logits_to_probs is pinned to GPT/utils.py by sample.npz), draws must agree with the
    restated noise stream, and the empirical distribution must pass chi-square."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=1)
    m = _model(cfg, synth.gpt_weights(cfg, seed=5), [(1, 64)], torch.float32, dev)
    rt = m._rt[1]
    V = 1025
    logits = (np.random.default_rng(3).standard_normal(V) * 3.0).astype(np.float32)
    logits[[280, 486, 1024]] = -np.inf
    ref_p = orc.logits_to_probs(logits[None].copy(), None, temperature=temp, top_k=(top_k or None), top_p=top_p)[0]
    mine = orc.device_sample_probs(logits, top_k, temp, top_p)
    assert np.array_equal(ref_p > 0, mine > 0) and np.abs(ref_p - mine).max() < 1e-6
    n, bad = 3000, 0
    counts = np.zeros(V)
    with torch.inference_mode():
        rt["logits"][0].copy_(torch.from_numpy(logits))
        rt["kv_len"].fill_(5); rt["x_len"].fill_(2); rt["step"].fill_(4)
        for s in range(n):
            seed = 7919 * s + 3
            m._set_ctl(rt, 2, 0, False, 1.0, top_k, temp, seed, top_p)
            m._flush(1)
            tok = int(rt["pre_tokens"][0, 5].item())
            counts[tok] += 1
            want, margin = orc.device_sample(logits, top_k, temp, seed, 0, 5, 4, top_p)
            if tok != want:
                assert margin < 1e-4, (s, tok, want, margin)
                bad += 1
    assert bad <= 3
    assert counts[ref_p == 0].sum() == 0, "drew a token outside the top-p / top-k set"
    kept = ref_p > 0
    exp = ref_p[kept] * n
    big = exp >= 5                                       # chi-square needs expected counts that are not tiny
    chi2 = (((counts[kept][big] - exp[big]) ** 2) / exp[big]).sum()
    assert chi2 < 30.0 + 3.0 * big.sum(), (chi2, int(big.sum()))


def test_batched_sampling_with_refills_is_reproducible(dev):
    """infer_batched with the production sampling parameters (top_k 15, top_p 0.9, temperature 0.8; no repetition
    penalty in the batched path, t2s_model.py:555-734) over more requests than slots -- the per-sequence kernels at
    4 slots, the batched MFMA step at 40 -- completes every request once, keeps tokens in range and repeats exactly
    for the same generator seed (the device sampler's stream is a counter-based function of seed / slot / position)."""
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    cfg = synth.gpt_config(n_layer=6)
    m = Text2SemanticDecoder(cfg)
    m.load_state_dict(synth.gpt_weights(cfg, seed=3, eos_gain=3.0))
    m.initialize_runtime(torch.bfloat16, dev, [(4, 256), (40, 256)])
    reqs = [synth.synth_request(i, 10, 12 + i % 5, 20 + i % 7, seed=3) for i in range(50)]
    xs = [torch.from_numpy(r[0]).to(dev) for r in reqs]
    ys = [torch.from_numpy(r[1]).to(dev) for r in reqs]
    bs = [torch.from_numpy(r[2]).to(dev) for r in reqs]
    for n in (11, 50):
        outs = []
        for _ in range(2):
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            pred, orig = m.infer_batched(xs[:n], ys[:n], bs[:n], top_k=15, top_p=0.9, temperature=0.8, generator=g)
            outs.append(([p.cpu().numpy() for p in pred], orig.cpu().numpy()))
        assert sorted(outs[0][1].tolist()) == list(range(n))
        assert np.array_equal(outs[0][1], outs[1][1])
        for a, b in zip(outs[0][0], outs[1][0]):
            assert np.array_equal(a, b) and ((a >= 0) & (a < 1024)).all()
        assert max(len(p) for p in outs[0][0]) > 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefill_into_scattered_slots_equals_one_by_one(dev, dtype):
    """gsv_t2s_prefill_slots (the packed refill of a check window): rows of different lengths sent to slots [5, 0, 3]
    in one call leave exactly the state that three single-row prefills leave -- K/V cache rows, kv_len / x_len, the
    first logits and the recorded prompt tokens, bit for bit (rows are independent through every prefill kernel)."""
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=21)
    shapes = [(6, 11, 14), (3, 4, 30), (9, 20, 7)]
    rs = [synth.synth_request(70 + i, p, t, n, seed=21, bert="random") for i, (p, t, n) in enumerate(shapes)]
    slots = [5, 0, 3]
    xs, ys, bs = ([_T(r[k], dev) for r in rs] for k in range(3))
    states = []
    for packed in (False, True):
        with torch.inference_mode():
            m = _model(cfg, w, [(6, 96)], dtype, dev)
            rt = m._rt[6]
            for t in (rt["kv_len"], rt["x_len"], rt["logits"], rt["pre_tokens"]):
                t.zero_()
            m.k_cache_root.zero_()
            m.v_cache_root.zero_()
            if packed:
                xy, xl, yl, _, _ = m.embed_prompt(xs, ys, bs)
                m.prefill_slots(6, slots, xy, xl, yl)
            else:
                for s_, x, y, b in zip(slots, xs, ys, bs):
                    xy, xl, yl, _, _ = m.embed_prompt([x], [y], [b])
                    m.prefill(6, s_, xy, xl, yl)
            m._flush(6)
            torch.cuda.synchronize()
            st = {k: rt[k].clone() for k in ("kv_len", "x_len", "logits", "pre_tokens")}
            st.update({"k": m.k_cache_root.clone(), "v": m.v_cache_root.clone()})
            states.append(st)
    a, b = states
    assert a["kv_len"].tolist() == b["kv_len"].tolist() and a["kv_len"][5] == 6 + 11 + 14 and a["kv_len"][1] == 0
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("nreq,plen,dtype", [(6, 130, torch.bfloat16), (26, 190, torch.bfloat16), (26, 190, torch.float32)])
def test_packed_prompt_pass_of_many_rows_equals_one_by_one_bf16(dev, nreq, plen, dtype):
    """A request's K/V rows, first logits and recorded tokens must not depend on how many prompts shared its prompt pass (the slot
    loop's refills and the engine's ranks pack different sets): a packed pass of ~800 rows and one of ~5 000 rows against the same
    prompts one by one, bit for bit.  The second size is the one that FAILED in round 4: from ~2 000 phoneme rows on the BERT
    projection (a tapgemm launch) switched from its split-K tile to a wide tile that sums K in another order, the embedded rows
    moved by an fp32 ulp and the bf16 K/V rows behind them by a bf16 ulp (csrc/abi_common.h: Epi::fixed_order pins the tile)."""
    cfg = synth.gpt_config(n_layer=3)
    w = synth.gpt_weights(cfg, seed=33)
    rng = np.random.default_rng(nreq)
    shapes = [(int(rng.integers(20, 40)), int(rng.integers(plen // 2 - 20, plen // 2)), int(rng.integers(plen // 3, plen // 2))) for _ in range(nreq)]
    rs = [synth.synth_request(170 + i, p, t, n, seed=33, bert="random") for i, (p, t, n) in enumerate(shapes)]
    xs, ys, bs = ([_T(r[k], dev) for r in rs] for k in range(3))
    B = nreq
    slots = list(rng.permutation(B))
    states = []
    for packed in (False, True):
        with torch.inference_mode():
            m = _model(cfg, w, [(B, 256)], dtype, dev)
            rt = m._rt[B]
            for t in (rt["kv_len"], rt["x_len"], rt["logits"], rt["pre_tokens"]):
                t.zero_()
            m.k_cache_root.zero_()
            m.v_cache_root.zero_()
            if packed:
                xy, xl, yl, _, _ = m.embed_prompt(xs, ys, bs)
                assert xy.shape[0] * xy.shape[1] >= (4096 if nreq > 20 else 512), xy.shape     # rows of the packed pass
                m.prefill_slots(B, [int(v) for v in slots], xy, xl, yl)
            else:
                for s_, x, y, b in zip(slots, xs, ys, bs):
                    xy, xl, yl, _, _ = m.embed_prompt([x], [y], [b])
                    m.prefill(B, int(s_), xy, xl, yl)
            m._flush(B)
            torch.cuda.synchronize()
            st = {k: rt[k].clone() for k in ("kv_len", "x_len", "logits", "pre_tokens")}
            st.update({"k": m.k_cache_root.clone(), "v": m.v_cache_root.clone()})
            states.append(st)
            del m
    a, b = states
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_bf16_long_prompt_uses_the_mfma_attention_limit(dev):
    """the bf16 prompt pass is gated by ITS kernel's LDS footprint (prompts up to 1056 positions), not by
    the fp32 parity kernel's (591): a 900-position prompt -- inside the reference's default 1024 bucket -- must run
    in bf16 and still be refused, with a message naming the mode, in fp32."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=2)
    w = synth.gpt_weights(cfg, seed=21, eos_gain=0.0)
    x, y, bert, _ = synth.synth_request(9, 300, 400, 200, seed=21)      # 700 phonemes + 200 prompt tokens = 900 positions
    cache = [(1, 1024)]
    m = _model(cfg, w, cache, torch.bfloat16, dev)
    tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, max_new_tokens=12)[0, 0].cpu().numpy()
    assert len(tok) == 12
    o = orc.T2SOracle(cfg, w, [(1, 912)], numerics="bf16")
    ref = o.infer(x, y, bert, top_k=1)
    first = next((i for i in range(12) if tok[i] != ref[i]), None)
    assert first is None or o.margins[first + 1] < 2e-2, (first, tok, ref[:12])
    m32 = _model(cfg, w, cache, torch.float32, dev)
    with pytest.raises(RuntimeError, match="fp32 mode"):
        m32.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, max_new_tokens=2)


def test_first_sample_is_suppressed_even_without_suppression_steps(dev):
    """infer() / infer_stream() never let the PREFILL's sample be 280 / 486 / EOS (t2s_model.py:415-416),
    whatever initial_suppression_steps is; the loop's samples are only suppressed while idx < that (:444-445).  A
    predict layer whose row 280 dominates makes the difference observable; the oracle restates the reference."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=2)
    w = synth.gpt_weights(cfg, seed=33, eos_gain=0.0)
    pw = np.array(w["ar_predict_layer.weight"], copy=True)
    pw[280] = pw[280] * 0 + 0.05 * np.sign(np.random.default_rng(0).normal(size=512)).astype(np.float32)
    w["ar_predict_layer.weight"] = pw
    x, y, bert, _ = synth.synth_request(2, 6, 9, 11, seed=33)
    cache = [(1, 64)]
    m = _model(cfg, w, cache, torch.float32, dev)
    o = orc.T2SOracle(cfg, w, cache)
    for steps in (0, 10):
        ref = o.infer(x, y, bert, top_k=1, initial_suppression_steps=steps)
        tok = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, initial_suppression_steps=steps)[0, 0].cpu().numpy()
        assert np.array_equal(tok, ref), (steps, tok[:8], ref[:8])
    # the prefill sample itself (kept at kv position Lp): never a suppressed id, also with steps = 0
    m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1, initial_suppression_steps=0, max_new_tokens=2)
    s0 = int(m._rt[1]["pre_tokens"][0, len(x) + len(y)].item())
    assert s0 not in (280, 486, 1024)


@pytest.mark.parametrize("dtype,slots,n_layer", [(torch.float32, 4, 5), (torch.bfloat16, 4, 5), (torch.bfloat16, 40, 4)])
def test_staged_refill_returns_the_same_tokens_per_request(dev, dtype, slots, n_layer):
    """async_refill: a finished slot is parked (kv_len = -1), its prompt pass runs on a side stream into the live K/V
    rows and the library's staging while the other slots keep stepping, and gsv_t2s_commit_slots joins it later.  Which
    window it joins at depends on timing; the tokens of every request must not: they equal the reference-order run's
    (fp32: also the oracle's), request by request, on the per-sequence kernels (4 slots) and the batched chain (40)."""
    cfg = synth.gpt_config(n_layer=n_layer)
    w = synth.gpt_weights(cfg, seed=29, eos_gain=2.5)
    cache = [(slots, 160)]
    rng = np.random.default_rng(29)
    n_req = 6 * slots + 3
    shapes = [(int(rng.integers(2, 9)), int(rng.integers(3, 30)), int(rng.integers(4, 40))) for _ in range(n_req)]
    rs = [synth.synth_request(300 + i, p, t, n, seed=29, bert="random") for i, (p, t, n) in enumerate(shapes)]
    # fp32: requests end at their EOS, as in the oracle; bf16: a token budget per request as well (bench.py's workload)
    budget = None if dtype == torch.float32 else [int(rng.integers(3, 60)) for _ in range(n_req)]
    m = _model(cfg, w, cache, dtype, dev)
    if dtype != torch.float32:
        # bf16: the batched chain (>= 17 slots) and the per-sequence kernels round differently, so a request that continues on a tail
        # state is not bit-identical to one that stays in the 40-slot chain; what compaction does to bf16 tokens has its own test below
        m.tail_levels = []
    X, Y, Bt = [_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs]

    def run(**kw):
        pred, idx = m.infer_batched(X, Y, Bt, top_k=1, max_new_tokens=budget, **kw)
        assert sorted(idx.tolist()) == list(range(n_req))
        return {int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)}, dict(m.last_stats)

    ref, st0 = run()
    # refill_ahead > 0 (the default): the NEXT requests' prompt passes run ahead into a second bound state, several per pass, and a
    # finished slot adopts one (gsv_t2s_adopt_slots); 0: park -> prompt pass into the live rows -> commit.  3: fewer ahead slots than finishers
    for ahead in (m.refill_ahead, 3, 0):
        m.refill_ahead = ahead
        for rep in range(2):        # twice: the staging / parked state of one run must not leak into the next
            got, st1 = run(async_refill=True)
            assert st1["refills"] == st0["refills"] == n_req - slots
            for i in range(n_req):
                assert np.array_equal(got[i], ref[i]), (ahead, rep, i)
        if ahead > 3:
            assert st1["passes"] <= st1["refills"] // 2 + 2, st1    # at least two requests per prompt pass (half the ahead slots)
    again, _ = run()
    for i in range(n_req):
        assert np.array_equal(again[i], ref[i])
    if dtype == torch.float32:
        from oracle import oracle as orc
        o = orc.T2SOracle(cfg, w, cache)
        op, oi = o.infer_batched([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], top_k=1)
        for i, p in zip(oi.tolist(), op):
            assert np.array_equal(ref[int(i)], p)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@torch.inference_mode()
def test_move_slots_continues_live_requests_where_they_were(dev, dtype):
    """gsv_t2s_move_slots: three live slots of a 6-slot state, a few windows into their decode, move into slots of a 4-slot state
    with its own K/V cache (one of the moves lands on a slot index that is another move's source: the pending tokens live in ONE
    array per handle) and decode on: the tokens they produce equal those of a run that never moved (fp32 and bf16 alike: both
    sizes run the per-sequence kernels... 6 and 4 slots differ in the FFN slice count on bf16 handles, so bf16 compares 6 -> 5)."""
    from gsv_tts_lite_amd import _native as N
    cfg = synth.gpt_config(n_layer=3)
    nb = 4 if dtype == torch.float32 else 5
    m = _model(cfg, synth.gpt_weights(cfg, seed=41, eos_gain=0.0), [(6, 96)], dtype, dev)
    rt = m._rt[6]
    reqs = [synth.synth_request(60 + i, 4 + i, 6 + 3 * i, 8 + 4 * i, seed=41, bert="random") for i in range(6)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    L = [len(r[0]) + len(r[1]) for r in reqs]

    def start():
        m._set_ctl(rt, 0, 0, False, 1.0)
        rt["kv_len"].zero_(); rt["x_len"].zero_()
        xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
        m.prefill(6, 0, xy, xl, yl)
        m._decode(6, 6); m._flush(6)

    start()
    m._decode(6, 9); m._flush(6)
    torch.cuda.synchronize()
    want = {s_: rt["pre_tokens"][s_, L[s_] + 1: L[s_] + 15].clone() for s_ in (1, 2, 5)}
    start()
    tail = m._tail_state(nb, 96)
    assert tail is not None and tail["batch"] == nb
    for k in ("ctl", "fctl"):
        tail[k].copy_(rt[k])
    tail["fused_ok"] = rt.get("fused_ok", False)
    tail["kv_len"].fill_(-1)
    m.move_slots(nb, [0, 1, 2], 6, [1, 2, 5])        # slot 1 -> 0, 2 -> 1 (1 is also a source), 5 -> 2
    m._decode(nb, 9); m._flush(nb)
    torch.cuda.synchronize()
    for j, s_ in enumerate((1, 2, 5)):
        got = tail["pre_tokens"][j, L[s_] + 1: L[s_] + 15]
        assert torch.equal(got, want[s_]), (s_, got.tolist(), want[s_].tolist())
        assert int(tail["kv_len"][j]) == int(rt["kv_len"][s_]) + 9
    assert int(tail["kv_len"][3]) == -1
    # refused: same state twice, a slot listed twice, a longer source cache
    bad = lambda *a_: N.lib().gsv_t2s_move_slots(m._h, *a_, N.current_stream_ptr(dev))
    import ctypes
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    assert bad(6, i32([0]), 6, i32([1]), 1) != 0
    assert bad(nb, i32([0, 0]), 6, i32([1, 2]), 2) != 0
    assert bad(nb, i32([0, 1]), 6, i32([2, 2]), 2) != 0


@pytest.mark.parametrize("dtype,slots,n_layer", [(torch.float32, 20, 4), (torch.bfloat16, 40, 4)])
def test_tail_compaction_keeps_every_requests_tokens(dev, dtype, slots, n_layer):
    """queue empty, nothing prefilled ahead: the live requests continue on a smaller bound state (t2s.py `compact`, gsv_t2s_move_slots)
    instead of paying the step of the full batch (t2s_model.py:684-694).  fp32: every request's tokens equal the run without
    compaction and the oracle's, bit for bit.  bf16: the tail runs on the per-sequence kernels, whose rounding differs from the
    batched chain's -- tokens equal the uncompacted run's up to the first step whose fp32 decision margin is below the bf16 gate."""
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=n_layer)
    w = synth.gpt_weights(cfg, seed=31, eos_gain=0.0 if dtype != torch.float32 else 2.0)
    cache = [(slots, 160)]
    rng = np.random.default_rng(31)
    n_req = 2 * slots + 5
    shapes = [(int(rng.integers(2, 9)), int(rng.integers(3, 30)), int(rng.integers(4, 40))) for _ in range(n_req)]
    rs = [synth.synth_request(700 + i, p, t, n, seed=31, bert="random") for i, (p, t, n) in enumerate(shapes)]
    budget = None if dtype == torch.float32 else [int(rng.integers(5, 90)) for _ in range(n_req)]
    m = _model(cfg, w, cache, dtype, dev)
    X, Y, Bt = [_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs]

    def run(levels):
        m.tail_levels = levels
        pred, idx = m.infer_batched(X, Y, Bt, top_k=1, max_new_tokens=budget, async_refill=True)
        assert sorted(idx.tolist()) == list(range(n_req))
        return {int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)}, dict(m.last_stats)

    ref, st0 = run([])
    assert not st0["compactions"] and st0["slot_steps"] == st0["steps"] * slots
    for rep in range(2):
        got, st1 = run([16, 8, 4])
        assert st1["compactions"], st1
        assert st1["slot_steps"] < st1["steps"] * slots
        assert all(b1 < b0 and live <= b1 for _, b0, b1, live in st1["compactions"]), st1["compactions"]
        for i in range(n_req):
            if dtype == torch.float32:
                assert np.array_equal(got[i], ref[i]), (rep, i)
                continue
            assert len(got[i]) == len(ref[i]) == budget[i]
            neq = np.nonzero(got[i] != ref[i])[0]
            if neq.size:
                first = int(neq[0])
                o1 = orc.T2SOracle(cfg, w, [(1, 160)])
                single = o1.infer(rs[i][0], rs[i][1], rs[i][2], top_k=1, repetition_penalty=1.0, initial_suppression_steps=0)
                if len(single) > first and np.array_equal(single[:first], ref[i][:first]):
                    assert o1.margins[first + 1] < 0.35, (i, first, o1.margins[first + 1])
    if dtype == torch.float32:
        o = orc.T2SOracle(cfg, w, cache)
        op, oi = o.infer_batched([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], top_k=1)
        for i, p in zip(oi.tolist(), op):
            assert np.array_equal(ref[int(i)], p)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@torch.inference_mode()
def test_adopt_slots_equals_a_prompt_pass_into_the_slots(dev, dtype):
    """gsv_t2s_adopt_slots: a prompt pass run AHEAD into a second bound state (its own K/V cache, the library's staging), then
    adopted by slots of the stepped state, leaves those slots exactly as gsv_t2s_prefill_slots into them does -- K/V rows, kv_len,
    x_len, step, eos_at, first logits / hidden -- and the steps that follow produce the same tokens; bad arguments are refused."""
    from gsv_tts_lite_amd import _native as N
    import ctypes
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=5, eos_gain=0.0), [(4, 96)], dtype, dev)
    rt = m._rt[4]
    reqs = [synth.synth_request(40 + i, 5, 9 + 4 * i, 12 + 5 * i, seed=5, bert="random") for i in range(2)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    L = [len(r[0]) + len(r[1]) for r in reqs]
    slots = [3, 1]

    def snapshot():
        m._decode(4, 4); m._flush(4)
        torch.cuda.synchronize()
        out = {k: rt[k][slots].clone() for k in ("kv_len", "x_len", "step", "eos_at", "logits", "hidden")}
        out["tok"] = torch.stack([rt["pre_tokens"][s, L[j]: L[j] + 5] for j, s in enumerate(slots)])
        out["k"] = [rt["k"][:, s, :, : L[j] + 4].clone() for j, s in enumerate(slots)]
        out["v"] = [rt["v"][:, s, :, : L[j] + 4].clone() for j, s in enumerate(slots)]
        return out

    def reset():
        m._set_ctl(rt, 0, 0, False, 1.0)
        rt["kv_len"].fill_(-1); rt["x_len"].zero_(); rt["k"].zero_(); rt["v"].zero_(); rt["pre_tokens"].zero_()

    reset()
    xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
    m.prefill_slots(4, slots, xy, xl, yl)
    want = snapshot()

    reset()
    sh = m._ahead_state(2, 96)
    assert sh["batch"] != 4 and sh["k"].data_ptr() != rt["k"].data_ptr()
    for k in ("ctl", "fctl"):
        sh[k].copy_(rt[k])
    xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
    src = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    m.prefill_slots_staged(sh["batch"], src, xy, xl, yl, N.current_stream_ptr(dev))
    assert int(rt["kv_len"][3]) == -1                       # nothing of the stepped state was touched by the pass
    m.adopt_slots(4, slots, sh["batch"], [1, 0])
    got = snapshot()
    for k in ("kv_len", "x_len", "step", "eos_at", "tok"):
        assert torch.equal(got[k], want[k]), k
    for k in ("logits", "hidden"):
        assert torch.equal(got[k], want[k]), k
    for j in range(2):
        assert torch.equal(got["k"][j], want["k"][j]) and torch.equal(got["v"][j], want["v"][j]), j

    lib, h = N.lib(), m._h
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    st = N.current_stream_ptr(dev)
    assert lib.gsv_t2s_adopt_slots(h, 4, i32(0), 4, i32(0), None, 1, st) != 0                   # the same state
    assert lib.gsv_t2s_adopt_slots(h, 4, i32(4), sh["batch"], i32(0), None, 1, st) != 0         # destination out of range
    assert lib.gsv_t2s_adopt_slots(h, 4, i32(0), sh["batch"], i32(sh["batch"]), None, 1, st) != 0
    assert lib.gsv_t2s_adopt_slots(h, 4, i32(1, 1), sh["batch"], i32(0, 1), None, 2, st) != 0   # one slot twice
    assert lib.gsv_t2s_adopt_slots(h, 4, i32(0), 77, i32(0), None, 1, st) != 0                  # no such state
    # a source slot no prompt pass has filled since the bind holds kv_len 0: adopting it copies no row and leaves an empty slot
    sh3 = m._ahead_state(3, 96)
    rt["kv_len"].fill_(7)
    m.adopt_slots(4, [2], sh3["batch"], [2])
    torch.cuda.synchronize()
    assert int(rt["kv_len"][2]) == 0 and int(rt["eos_at"][2]) == -1 and int(rt["kv_len"][0]) == 7


@pytest.mark.parametrize("slots,n_req", [(1, 4), (3, 2), (3, 3), (2, 9)])
def test_ahead_refill_edge_cases(dev, slots, n_req):
    """the slot loop with prompt passes run ahead, at its edges: one slot (the ahead state then needs another batch size than the stepped
    one), fewer requests than slots (nothing to prefill ahead), exactly as many, and more ahead slots than requests left -- every
    request's tokens equal the reference-order loop's, with a token budget and with EOS ends"""
    cfg = synth.gpt_config(n_layer=2)
    w = synth.gpt_weights(cfg, seed=77, eos_gain=2.0)
    m = _model(cfg, w, [(slots, 128)], torch.float32, dev)
    rng = np.random.default_rng(slots * 100 + n_req)
    rs = [synth.synth_request(500 + i, int(rng.integers(2, 6)), int(rng.integers(3, 20)), int(rng.integers(4, 30)), seed=77, bert="random")
          for i in range(n_req)]
    X, Y, Bt = [_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs]
    for budget in (None, [int(rng.integers(1, 25)) for _ in range(n_req)]):
        ref, ridx = m.infer_batched(X, Y, Bt, top_k=1, max_new_tokens=budget)
        want = {int(i): p.cpu().numpy() for i, p in zip(ridx.tolist(), ref)}
        for ahead in (8, 1):
            m.refill_ahead = ahead
            got, gidx = m.infer_batched(X, Y, Bt, top_k=1, max_new_tokens=budget, async_refill=True)
            assert sorted(gidx.tolist()) == list(range(n_req))
            assert m.last_stats["refills"] == max(0, n_req - slots)
            for i, p in zip(gidx.tolist(), got):
                assert np.array_equal(p.cpu().numpy(), want[int(i)]), (budget is not None, ahead, i)


def test_staged_refill_cuts_a_full_cache_like_the_reference_order_loop(dev):
    """requests that never sample EOS end when kv + check_interval reaches the cache size at a 5-step window boundary
    (t2s_model.py:655-657); where that boundary falls depends on the window a slot was filled at, so the staged loop may cut
    up to one window earlier or later than the reference-order loop -- the tokens themselves are the same sequence."""
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=13, eos_gain=0.0), [(4, 96)], torch.float32, dev)   # EOS (almost) never wins
    reqs = [synth.synth_request(900 + i, 5, 8 + 2 * i, 10 + 3 * i, seed=13, bert="random") for i in range(11)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    out = {}
    for mode in (False, True):
        pred, idx = m.infer_batched(X, Y, Bt, top_k=1, async_refill=mode)
        assert sorted(idx.tolist()) == list(range(11))
        out[mode] = {int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)}
    for i in range(11):
        a, b = out[False][i], out[True][i]
        L = len(reqs[i][0]) + len(reqs[i][1])
        n = min(len(a), len(b))
        assert n > 0 and np.array_equal(a[:n], b[:n]), i
        assert abs(len(a) - len(b)) <= 5 and L + max(len(a), len(b)) < 96, (i, len(a), len(b), L)
        assert L + min(len(a), len(b)) >= 96 - 12, (i, len(a), len(b), L)      # both ran the cache (nearly) full


def test_staged_refill_raises_on_a_prompt_that_does_not_fit_and_recovers(dev):
    """a queued request whose prompt exceeds the cache raises (as the reference-order loop does) also when the slot loop is
    the staged one; nothing of the aborted run (parked slots, a prompt pass in flight) leaks into the next call"""
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=21, eos_gain=2.5), [(2, 64)], torch.float32, dev)
    ok = [synth.synth_request(700 + i, 4, 6 + i, 8 + i, seed=21, bert="random") for i in range(6)]
    bad = synth.synth_request(799, 4, 40, 40, seed=21, bert="random")           # 80 positions > 64
    X = lambda rs: ([_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs])
    ref, ridx = m.infer_batched(*X(ok), top_k=1)
    want = {int(i): p.cpu().numpy() for i, p in zip(ridx.tolist(), ref)}
    with pytest.raises(ValueError):
        m.infer_batched(*X(ok[:4] + [bad] + ok[4:]), top_k=1, async_refill=True)
    got, gidx = m.infer_batched(*X(ok), top_k=1, async_refill=True)
    for i, p in zip(gidx.tolist(), got):
        assert np.array_equal(p.cpu().numpy(), want[int(i)]), i


def test_device_sampling_is_keyed_by_request_not_by_slot(dev):
    """continuous batching draws each request's noise from ITS stream (tok_override carries request index + 1 in device-
    sampling mode): the sampled tokens of a request are the same with 4 or 6 slots, with the reference-order or the staged
    refill -- i.e. independent of the slot, the refill order and (engine tests) the rank it lands on"""
    cfg = synth.gpt_config(n_layer=4)
    m = _model(cfg, synth.gpt_weights(cfg, seed=9, eos_gain=3.0), [(4, 200), (6, 200)], torch.bfloat16, dev)
    reqs = [synth.synth_request(i, 8, 10 + i % 7, 15 + i % 9, seed=9) for i in range(30)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    runs = []
    for slots, mode in ((4, False), (6, False), (4, True), (6, True)):
        g = torch.Generator(device=dev); g.manual_seed(11)
        pred, idx = m.infer_batched(X, Y, Bt, top_k=15, top_p=0.9, temperature=0.8, generator=g, slots=slots, async_refill=mode)
        runs.append({int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)})
    assert max(len(v) for v in runs[0].values()) > 5 and len({tuple(v) for v in runs[0].values()}) > 20   # real sampling, not one answer
    for r in runs[1:]:
        for i in range(30):
            assert np.array_equal(r[i], runs[0][i]), i
    # a single-sequence run after a batched one draws from slot 0's stream again (the batched run's ids are cleared)
    m2 = _model(cfg, synth.gpt_weights(cfg, seed=9, eos_gain=3.0), [(1, 200)], torch.bfloat16, dev)
    outs = []
    for pre in (False, True):
        if pre:
            g = torch.Generator(device=dev); g.manual_seed(5)
            m2.infer_batched(X[:3], Y[:3], Bt[:3], top_k=15, generator=g)          # 3 requests through the 1-slot family
        g = torch.Generator(device=dev); g.manual_seed(11)
        outs.append(m2.infer(X[7][None], Y[7][None], Bt[7][None], top_k=15, top_p=0.9, temperature=0.8, generator=g).cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


def test_staged_refill_with_device_sampling_and_callbacks(dev):
    """the staged slot loop under the production sampling parameters (device sampler, noise keyed by slot: which slot a
    request gets is decided when the slot is parked, so a run is as reproducible as the reference-order one) and with an
    on_finish callback (the engine's overlapped vocoder hook): every request served once, callback per request, tokens in range"""
    cfg = synth.gpt_config(n_layer=4)
    m = _model(cfg, synth.gpt_weights(cfg, seed=9, eos_gain=3.0), [(6, 200)], torch.bfloat16, dev)
    reqs = [synth.synth_request(i, 8, 10 + i % 7, 15 + i % 9, seed=9) for i in range(40)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    seen = []
    g = torch.Generator(device=dev); g.manual_seed(3)
    pred, idx = m.infer_batched(X, Y, Bt, top_k=15, top_p=0.9, temperature=0.8, generator=g, async_refill=True,
                                on_finish=lambda i, t: seen.append((int(i), int(t.numel()))))
    assert sorted(idx.tolist()) == list(range(40)) and sorted(i for i, _ in seen) == list(range(40))
    assert [n for _, n in seen] == [int(p.numel()) for p in pred]
    for p in pred:
        a = p.cpu().numpy()
        assert ((a >= 0) & (a < 1024)).all()
    assert max(int(p.numel()) for p in pred) > 3 and m.last_stats["refills"] == 34


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_token_step_fused_into_layer0_equals_the_token_kernel(dev, dtype):
    """GSV_STEP_FUSED_TOKEN: with greedy / host-chosen tokens the first layer's attention kernel derives the pending token,
    its embedding + position row and keeps the books (pre_tokens, seen, eos_at, step) itself.  Same tokens and the same
    state as the step that starts with t2s_token_kernel: single sequence with repetition penalty and suppression
    (infer), 4 slots (one sequence per block) and 19 slots (two per block, the odd last block half empty) with refills
    (infer_batched), graph replay and eager launches."""
    cfg = synth.gpt_config(n_layer=4)
    w = synth.gpt_weights(cfg, seed=41, eos_gain=2.0)
    m = _model(cfg, w, [(1, 200), (4, 200), (19, 200)], dtype, dev)
    rs = [synth.synth_request(500 + i, 6, 10 + (3 * i) % 40, 12 + (5 * i) % 60, seed=41, bert="random") for i in range(45)]
    X, Y, Bt = [_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs]
    res = {}
    for graph in (True, False):
        for fused in (False, True):
            m.use_graph, m.fuse_token_step = graph, fused
            one = m.infer(X[0][None], Y[0][None], Bt[0][None], top_k=1, repetition_penalty=1.35).cpu().numpy()
            st = {k: m._rt[1][k].clone() for k in ("pre_tokens", "seen", "step", "eos_at", "kv_len")}
            many = {}
            for slots, n in ((4, 9), (19, 45)):
                pred, idx = m.infer_batched(X[:n], Y[:n], Bt[:n], top_k=1, slots=slots)
                many.update({(slots, int(i)): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)})
            res[(graph, fused)] = (one, st, many)
    m.use_graph, m.fuse_token_step = True, True
    ref = res[(True, False)]
    assert ref[0].size > 3
    for key, (one, st, many) in res.items():
        assert np.array_equal(one, ref[0]), key
        for k in st:
            assert torch.equal(st[k], ref[1][k]), (key, k)
        assert set(many) == set(ref[2]) and len(many) == 9 + 45
        for i in many:
            assert np.array_equal(many[i], ref[2][i]), (key, i)


def test_rebinding_state_and_reloading_weights_do_not_grow_the_handle(dev):
    """the handle's arena hands given-back pieces out again by size (gsv_t2s_device_bytes): a C-ABI user who re-binds a
    state per request or hot-swaps weights of the same architecture must not leak device memory until destroy"""
    import ctypes
    from gsv_tts_lite_amd import _native as N
    cfg = synth.gpt_config(n_layer=2)
    w = synth.gpt_weights(cfg, seed=3)
    m = _model(cfg, w, [(1, 64), (4, 64)], torch.bfloat16, dev)
    L = N.lib()
    x, y, bert, _ = synth.synth_request(1, 5, 9, 11, seed=3)
    tok0 = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1)[0, 0].cpu().numpy()
    before = L.gsv_t2s_device_bytes(m._h)
    assert before > 0
    for b, rt in m._rt.items():
        st = N.T2SState(b, rt["T"], *[rt[k].data_ptr() for k in (
            "k", "v", "kv_len", "x_len", "pre_tokens", "seen", "step", "eos_at", "logits", "hidden", "tok_override", "ctl", "fctl")])
        for _ in range(40):
            N.check(L.gsv_t2s_bind_state(m._h, ctypes.byref(st)))
        if b == 1:
            N.check(L.gsv_t2s_set_eos_mirror(m._h, b, rt["eos_host"].data_ptr()))
    stream = N.current_stream_ptr(dev)
    for _ in range(6):     # the same tensors again: fragments and panels are re-packed
        for name, t in m._weights.items():
            if name.endswith("position.alpha"):
                continue
            d = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            N.check(L.gsv_t2s_load_tensor(m._h, name.encode(), d.data_ptr(), d.numel(), stream))
        N.check(L.gsv_t2s_finalize(m._h, stream))
    torch.cuda.synchronize(dev)
    assert L.gsv_t2s_device_bytes(m._h) == before, (before, L.gsv_t2s_device_bytes(m._h))
    tok1 = m.infer(_T(x, dev)[None], _T(y, dev)[None], _T(bert, dev)[None], top_k=1)[0, 0].cpu().numpy()
    assert np.array_equal(tok0, tok1)
