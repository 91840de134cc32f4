"""GPU tests of per-request sampling parameters in the continuous-batching step (the per-slot sampling table,
gsv_t2s_set_slot_sampling): the sampler per slot against the oracle, a mixed call against the scalar calls it replaces,
request-keyed seeds, the untouched scalar path, and the table entries through move / adopt."""
import ctypes

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import slot_sampling as SS
from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

# (top_k, temperature, top_p): greedy; top-k 5 at 0.8; top-k 15, top-p 0.9 at 1.2; top-k off, top-p 0.5; top-k 50 at 0.6
SETS = [(1, 1.0, 1.0), (5, 0.8, 1.0), (15, 1.2, 0.9), (0, 1.0, 0.5), (50, 0.6, 1.0)]


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


def _requests(n, seed, dev, base=0):
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(2, 9)), int(rng.integers(3, 30)), int(rng.integers(4, 40))) for _ in range(n)]
    rs = [synth.synth_request(base + i, p, t, k, seed=seed, bert="random") for i, (p, t, k) in enumerate(shapes)]
    return rs, [_T(r[0], dev) for r in rs], [_T(r[1], dev) for r in rs], [_T(r[2], dev) for r in rs]


def _by_request(pred, idx, n):
    assert sorted(idx.tolist()) == list(range(n))
    return {int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)}


@pytest.mark.parametrize("dtype,B", [(torch.float32, 4), (torch.float32, 20), (torch.bfloat16, 4), (torch.bfloat16, 20)])
@torch.inference_mode()
def test_sampler_per_slot_matches_the_oracle(dev, dtype, B):
    """B slots, each with its own table entry, one _flush, every slot's token against oracle.device_sample with THAT slot's
    parameters.  4 slots: the per-sequence step; 20: the batched chain on the bf16 handle (>= gsv_t2s_batched_min), the
    multi-sequence kernels on the fp32 one.  The slots hold a real prompt pass (a greedy slot takes the arg-max the logits
    kernel left, not the `logits` rows); sampled slots get known logits.  Cases whose top-1 / top-2 score margin in the
    oracle is below 1e-4 are dropped BEFORE the GPU runs (at most 1 % of the cases drawn); all others must be equal."""
    from gsv_tts_lite_amd import _native as N
    from oracle import oracle as orc
    cfg = synth.gpt_config(n_layer=2)
    m = _model(cfg, synth.gpt_weights(cfg, seed=5, eos_gain=0.0), [(B, 96)], dtype, dev)
    if dtype == torch.bfloat16 and B >= 17:
        assert B >= N.lib().gsv_t2s_batched_min(m._h)
    rt = m._rt[B]
    V = m.vocab_size
    _, X, Y, Bt = _requests(B, 3, dev)
    m._set_ctl(rt, 2, 0, False, 1.0)
    rt["kv_len"].zero_(); rt["x_len"].zero_()
    xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
    m.prefill(B, 0, xy, xl, yl)
    torch.cuda.synchronize()
    pos = rt["kv_len"].tolist()
    pre = rt["logits"].cpu().numpy().copy()                # the prompt pass's logits: what a greedy slot decides on
    rng = np.random.default_rng(B)
    rounds = 100 if B == 4 else 25
    drawn = dropped = checked = 0
    m._bind_sampling(rt)
    try:
        for r in range(rounds):
            sets = [SETS[(b + r) % len(SETS)] for b in range(B)]
            seeds = [int(rng.integers(0, 2 ** 62)) for _ in range(B)]
            logits = (rng.standard_normal((B, V)) * 3.0).astype(np.float32)
            m._samp = SS.resolve(B, [s[0] for s in sets], [s[2] for s in sets], [s[1] for s in sets], seeds)
            want = []
            for b in range(B):
                k, temp, p = sets[b]
                if k == 1:
                    logits[b] = pre[b]
                    top2 = np.sort(pre[b])[::-1][:2]
                    tok, margin = int(np.argmax(pre[b])), float(top2[0] - top2[1])
                else:
                    tok, margin = orc.device_sample(logits[b], k, temp, seeds[b], 0, pos[b], 0, p)
                drawn += 1
                if margin < 1e-4:
                    dropped += 1
                    tok = None
                want.append(tok)
            rt["logits"].copy_(torch.from_numpy(logits))
            rt["tok_override"].copy_(torch.tensor([m._stream_id(b) for b in range(B)], dtype=torch.int64))
            m._put_sampling(B, range(B), range(B))
            m._flush(B)
            got = rt["pre_tokens"][torch.arange(B, device=dev), rt["kv_len"]].tolist()
            for b in range(B):
                if want[b] is not None:
                    checked += 1
                    assert got[b] == want[b], (r, b, sets[b], got[b], want[b])
    finally:
        m._samp = None
        m._unbind_sampling()
    print("cases drawn %d, dropped below the 1e-4 margin %d, compared %d" % (drawn, dropped, checked))
    assert dropped <= 0.01 * drawn, (dropped, drawn)
    assert checked >= 0.99 * drawn


def _mixed_vs_uniform(m, X, Y, Bt, n_req, budget, sets, **kw):
    def gen():
        g = torch.Generator(device=m.device)
        g.manual_seed(11)
        return g

    deal = [sets[i % len(sets)] for i in range(n_req)]
    binds = getattr(m, "sampling_binds", 0)
    pred, idx = m.infer_batched(X, Y, Bt, top_k=[s[0] for s in deal], temperature=[s[1] for s in deal],
                                top_p=[s[2] for s in deal], generator=gen(), max_new_tokens=budget, **kw)
    assert m.sampling_binds > binds
    mixed, stats = _by_request(pred, idx, n_req), dict(m.last_stats)
    binds = m.sampling_binds
    for g_, (k, temp, p) in enumerate(sets):
        pred, idx = m.infer_batched(X, Y, Bt, top_k=k, temperature=temp, top_p=p, generator=gen(), max_new_tokens=budget, **kw)
        uni = _by_request(pred, idx, n_req)
        for i in range(g_, n_req, len(sets)):
            assert np.array_equal(mixed[i], uni[i]), (kw, g_, i, mixed[i].tolist(), uni[i].tolist())
    assert m.sampling_binds == binds                       # the scalar calls bound no table
    return mixed, stats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mixed_call_equals_the_uniform_calls_request_by_request(dev, dtype):
    """43 mixed-length requests through 8 slots, four parameter sets (greedy among them) dealt round-robin: request i of the
    mixed call returns exactly the tokens it returns in the SCALAR call with its set (same generator seed: same call seed,
    the noise stream is the request's).  Reference-order loop, staged refill, refill ahead; fp32 with tail compaction to the
    4-slot level.  bf16: 4 slots and fewer sum 64 FFN slices against 32 above, so a request that moves to the 4-slot level
    is not bit-identical; its exact comparison runs without compaction and with a 5-slot level (the same kernels)."""
    cfg = synth.gpt_config(n_layer=3)
    w = synth.gpt_weights(cfg, seed=29, eos_gain=2.5)
    n_req = 43
    m = _model(cfg, w, [(8, 160)], dtype, dev)
    rng = np.random.default_rng(29)
    _, X, Y, Bt = _requests(n_req, 29, dev, base=300)
    budget = [int(rng.integers(3, 60)) for _ in range(n_req)]
    sets = SETS[:4]
    levels = [[4]] if dtype == torch.float32 else [[], [5]]
    ref = None
    for lv in levels:
        m.tail_levels = lv
        for kw in (dict(), dict(async_refill=True, _ahead=0), dict(async_refill=True, _ahead=32)):
            kw = dict(kw)
            m.refill_ahead = kw.pop("_ahead", m.refill_ahead)
            mixed, stats = _mixed_vs_uniform(m, X, Y, Bt, n_req, budget, sets, **kw)
            assert stats["refills"] == n_req - 8
            if kw and m.refill_ahead > 0 and lv:
                assert stats["compactions"], stats
            if ref is None:
                ref = mixed
            for i in range(n_req):
                assert np.array_equal(mixed[i], ref[i]), (lv, kw, i)
    sampled = [i for i in range(n_req) if i % 4 != 0]
    assert len({tuple(ref[i]) for i in sampled}) > len(sampled) // 2      # real sampling, not one answer


def test_own_seeds_make_a_request_independent_of_the_call(dev):
    """seed=[...]: request i draws from (seed[i], stream 0): the same tokens alone, among all requests and in the reversed
    list (fp32, the 4-slot family each time); another seed gives other tokens at top_k 15."""
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=9, eos_gain=2.0), [(4, 160)], torch.float32, dev)
    n_req = 11
    _, X, Y, Bt = _requests(n_req, 9, dev, base=100)
    deal = [SETS[1 + i % 4] for i in range(n_req)]
    seeds = [1000003 * i + 17 for i in range(n_req)]
    arg = lambda order: dict(top_k=[deal[i][0] for i in order], temperature=[deal[i][1] for i in order],
                             top_p=[deal[i][2] for i in order], seed=[seeds[i] for i in order], slots=4, async_refill=True,
                             max_new_tokens=[30] * len(order))
    sel = lambda L, order: [L[i] for i in order]
    order = list(range(n_req))
    full = _by_request(*m.infer_batched(X, Y, Bt, **arg(order)), n_req)
    rev = order[::-1]
    back = _by_request(*m.infer_batched(sel(X, rev), sel(Y, rev), sel(Bt, rev), **arg(rev)), n_req)
    for j, i in enumerate(rev):
        assert np.array_equal(back[j], full[i]), i
    for i in (0, 3, 7, 10):
        alone = _by_request(*m.infer_batched([X[i]], [Y[i]], [Bt[i]], **arg([i])), 1)
        assert np.array_equal(alone[0], full[i]), i
    a = m.infer_batched([X[2]], [Y[2]], [Bt[2]], top_k=[15], seed=[12345], slots=4, max_new_tokens=[30])[0][0]
    b = m.infer_batched([X[2]], [Y[2]], [Bt[2]], top_k=[15], seed=[54321], slots=4, max_new_tokens=[30])[0][0]
    assert a.numel() > 5 and not torch.equal(a, b)


def test_scalar_call_binds_no_table_and_equals_repeated_lists(dev):
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=9, eos_gain=2.0), [(4, 160)], torch.bfloat16, dev)
    n_req = 13
    _, X, Y, Bt = _requests(n_req, 4, dev, base=700)
    outs = []
    for lists in (False, True):
        g = torch.Generator(device=dev); g.manual_seed(5)
        binds = getattr(m, "sampling_binds", 0)
        rep = (lambda v: [v] * n_req) if lists else (lambda v: v)
        pred, idx = m.infer_batched(X, Y, Bt, top_k=rep(15), top_p=rep(0.9), temperature=rep(0.8), generator=g, async_refill=True,
                                    max_new_tokens=[25] * n_req)
        outs.append(_by_request(pred, idx, n_req))
        assert (getattr(m, "sampling_binds", 0) > binds) == lists
        assert m._samp is None and m._samp_bound == []      # nothing stays bound behind a call
    for i in range(n_req):
        assert np.array_equal(outs[0][i], outs[1][i]), i
    with pytest.raises(ValueError, match="temperature.*12.*13"):
        m.infer_batched(X, Y, Bt, temperature=[1.0] * 12)


@torch.inference_mode()
def test_move_and_adopt_carry_the_slots_entries(dev):
    """In the form of test_move_slots_continues_live_requests_where_they_were: six live slots with six different table entries,
    three of them moved into a 5-slot state (the same kernels and FFN slice count as six slots) (one destination index is another move's source) decode on with the tokens they
    produce unmoved; a prompt pass adopted from the ahead state draws its first and later tokens with the entry put for it.
    Moving into a state without a table is refused."""
    from gsv_tts_lite_amd import _native as N
    cfg = synth.gpt_config(n_layer=3)
    m = _model(cfg, synth.gpt_weights(cfg, seed=41, eos_gain=0.0), [(6, 96)], torch.float32, dev)
    rt = m._rt[6]
    reqs = [synth.synth_request(60 + i, 4 + i, 6 + 3 * i, 8 + 4 * i, seed=41, bert="random") for i in range(6)]
    X, Y, Bt = [_T(r[0], dev) for r in reqs], [_T(r[1], dev) for r in reqs], [_T(r[2], dev) for r in reqs]
    L = [len(r[0]) + len(r[1]) for r in reqs]
    deal = [SETS[(i + 1) % 5] for i in range(6)]             # slot 4 greedy, the others sampled, all different from their neighbours
    m._samp = SS.resolve(6, [s[0] for s in deal], [s[2] for s in deal], [s[1] for s in deal], [77 + i for i in range(6)])
    try:
        m._bind_sampling(rt)
        tail = m._tail_state(5, 96)
        assert tail is not None and tail["batch"] == 5
        sh = m._ahead_state(2, 96)

        def start(live=range(6)):
            m._set_ctl(rt, 2, 0, False, 1.0)
            rt["kv_len"].fill_(-1); rt["x_len"].zero_(); rt["samp"].zero_()
            xy, xl, yl, _, _ = m.embed_prompt([X[i] for i in live], [Y[i] for i in live], [Bt[i] for i in live])
            m.prefill_slots(6, list(live), xy, xl, yl)
            rt["tok_override"].fill_(1)
            m._put_sampling(6, list(live), list(live))

        start()
        m._decode(6, 15); m._flush(6)
        torch.cuda.synchronize()
        want = {s_: rt["pre_tokens"][s_, L[s_]: L[s_] + 15].clone() for s_ in range(6)}
        assert len({tuple(v.tolist()) for v in want.values()}) == 6

        # ---- move: 1 -> 0, 2 -> 1 (1 is also a source), 5 -> 2
        start()
        m._decode(6, 6); m._flush(6)
        m._bind_sampling(tail)
        for k in ("ctl", "fctl"):
            tail[k].copy_(rt[k])
        tail["fused_ok"] = False
        tail["kv_len"].fill_(-1)
        m.move_slots(5, [0, 1, 2], 6, [1, 2, 5])
        m._decode(5, 9); m._flush(5)
        torch.cuda.synchronize()
        for j, s_ in enumerate((1, 2, 5)):
            assert torch.equal(tail["samp"][j], rt["samp"][s_]) and int(tail["samp"][j, 0]) == 2
            got = tail["pre_tokens"][j, L[s_]: L[s_] + 15]
            assert torch.equal(got, want[s_]), (s_, got.tolist(), want[s_].tolist())
        i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
        N.check(N.lib().gsv_t2s_set_slot_sampling(m._h, 5, None))
        assert N.lib().gsv_t2s_move_slots(m._h, 5, i32([3]), 6, i32([0]), 1, N.current_stream_ptr(dev)) != 0
        assert b"sampling table" in N.lib().gsv_last_error()
        # put: refused without a table, for a slot out of range and for a mode that is not 0 / 2
        put = lambda batch, slot, mode: N.lib().gsv_t2s_put_slot_sampling(
            m._h, batch, i32([slot]), (N.SlotSampling * 1)(N.SlotSampling(mode, 5, 1.0, 1.0, 1, 0)), 1, N.current_stream_ptr(dev))
        assert put(5, 0, 2) != 0 and put(6, 6, 2) != 0 and put(6, 0, 1) != 0 and put(6, 0, 2) == 0

        # ---- adopt: requests 4 (greedy) and 3 prefilled ahead into source slots 1, 0; adopted by slots 0, 1 (overlapping indices)
        start(live=[1, 2])
        for k in ("ctl", "fctl"):
            sh[k].copy_(rt[k])
        xy, xl, yl, _, _ = m.embed_prompt([X[4], X[3]], [Y[4], Y[3]], [Bt[4], Bt[3]])
        src = torch.tensor([1, 0], dtype=torch.int32, device=dev)
        m.prefill_slots_staged(sh["batch"], src, xy, xl, yl, N.current_stream_ptr(dev))
        m.adopt_slots(6, [0, 4], sh["batch"], [1, 0], [1, 1])
        m._put_sampling(6, [0, 4], [4, 3])
        m._decode(6, 15); m._flush(6)
        torch.cuda.synchronize()
        for slot, r in ((0, 4), (4, 3), (1, 1), (2, 2)):
            got = rt["pre_tokens"][slot, L[r]: L[r] + 15]
            assert torch.equal(got, want[r]), (slot, r, got.tolist(), want[r].tolist())
    finally:
        m._samp = None
        m._unbind_sampling()


def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def test_facade_per_text_values_reach_every_segment(dev, monkeypatch):
    """TTS.infer_batched(top_k=[...], temperature=[...]): the segments cut_text makes of a text are decoded with the text's
    values -- their tokens equal those of the scalar call with these values; a per-text list of the wrong length raises."""
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 128), (1, 160), (4, 160)], sovits_cache=[50, 55], device=str(dev), dtype="float32")
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=4&eos_gain=1.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_toy_frontend)
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    texts = ["First sentence is here. Second one follows! And a third, longer one.", "Another text", "Third, with a comma. Then more."]
    t2s = next(iter(tts.gpt_models.values())).t2s_model
    seen = []
    inner = t2s.infer_batched

    def spy(ids, prompts, berts, **kw):
        pred, idx = inner(ids, prompts, berts, **kw)
        seen.append(({int(i): p.cpu().numpy() for i, p in zip(idx.tolist(), pred)}, kw))
        return pred, idx

    monkeypatch.setattr(t2s, "infer_batched", spy)
    top_k, temp = [15, 1, 5], [1.2, 1.0, 0.8]

    def run(**kw):
        torch.manual_seed(3)        # the facade passes no generator: the call's seed comes from the global one
        clips = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", texts, noise_scale=0.0, cut_minlen=8, **kw)
        assert len(clips) == 3 and all(np.isfinite(c.audio_data).all() for c in clips)
        return seen[-1]

    mixed, kw = run(top_k=top_k, temperature=temp)
    n_seg = len(mixed)
    assert n_seg > 3 and len(kw["top_k"]) == n_seg and kw["top_k"][:2] == [15, 15] and kw["top_k"][-1] == 5
    seg_text = [top_k.index(k) for k in kw["top_k"]]        # the three values are distinct: a segment's value names its text
    assert sorted(set(seg_text)) == [0, 1, 2] and seg_text.count(0) >= 2
    for t in range(3):
        uni, _ = run(top_k=top_k[t], temperature=temp[t])
        assert len(uni) == n_seg
        for s_ in range(n_seg):
            if seg_text[s_] == t:
                assert np.array_equal(mixed[s_], uni[s_]), (t, s_)
    with pytest.raises(ValueError, match="top_k.*2.*3"):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", texts, top_k=[15, 1], noise_scale=0.0, cut_minlen=8)
