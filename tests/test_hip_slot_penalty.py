"""GPU tests of the per-request repetition penalty and start suppression of infer_batched (the two anti-loop words of the
per-slot sampling table, gsv_t2s_seed_seen): a request's tokens against the oracle's `infer`, the logits kernel's table
instantiation element by element, what a slot keeps of its previous tenant through the three refill loops, and the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import slot_sampling as SS
from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu

# (repetition_penalty, initial_suppression_steps), dealt round-robin: `infer`'s defaults; nothing; a mild pair; a strong penalty
SETS = [(1.35, 10), (1.0, 0), (1.1, 3), (2.0, 10)]
BARRED = (280, 486)
GSV_ERR_ARG = 1     # include/gsv_tts_hip.h
# reference order; park / staged prompt pass / commit; prompt passes ahead (+ tail compaction at its default levels)
LOOPS = [dict(), dict(async_refill=True, _ahead=0), dict(async_refill=True, _ahead=32)]


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


def _run(m, X, Y, Bt, loop, **kw):
    loop = dict(loop)
    m.refill_ahead = loop.pop("_ahead", m.refill_ahead)
    return _by_request(*m.infer_batched(X, Y, Bt, top_k=1, **loop, **kw), len(X))


@pytest.fixture(scope="module")
def world():
    cfg = synth.gpt_config(n_layer=2)
    return cfg, synth.gpt_weights(cfg, seed=5, eos_gain=0.0)


@pytest.fixture(scope="module")
def infer_reference(world):
    """`infer` of the CPU oracle for the 18 of the 24 requests that suppress, once for the three loops: (tokens[:24], margin)"""
    from oracle import oracle as orc
    cfg, w = world
    rng = np.random.default_rng(3)
    shapes = [(int(rng.integers(2, 9)), int(rng.integers(3, 30)), int(rng.integers(4, 40))) for _ in range(24)]
    o = orc.T2SOracle(cfg, w, [(1, 96)])
    ref = {}
    for i, (p, t, k) in enumerate(shapes):
        rp, n = SETS[i % 4]
        if n > 0:
            x, y, bert, _ = synth.synth_request(i, p, t, k, seed=3, bert="random")
            tok = o.infer(x, y, bert, top_k=1, repetition_penalty=rp, initial_suppression_steps=n)[:24]
            ref[i] = (tok, min(o.margins[:25]))
    return ref


@pytest.mark.parametrize("loop", LOOPS, ids=["reference_order", "staged", "ahead"])
def test_tokens_equal_infer(dev, world, infer_reference, loop):
    """24 requests through 8 slots, fp32, greedy, 24 new tokens each, four (penalty, steps) sets dealt round-robin.  A request
    with steps > 0 is decoded under the rules of `infer` and must return the oracle's `infer` tokens, whichever slot it lands
    in and however that slot was refilled (tail compaction at its default levels).  A request is left out only if the
    oracle's smallest decision margin over its 25 samples is below 1e-4 (at most 2 of 24).  A prompt near the end of the
    96-position cache ends at the loop's cache limit (at least 86 - prompt length tokens): what it returned is compared.
    The (1.0, 0) requests equal the scalar call's tokens array for array."""
    cfg, w = world
    n_req = 24
    m = _model(cfg, w, [(8, 96)], torch.float32, dev)
    rs, X, Y, Bt = _requests(n_req, 3, dev)
    deal = [SETS[i % 4] for i in range(n_req)]
    budget = [24] * n_req
    got = _run(m, X, Y, Bt, loop, repetition_penalty=[d[0] for d in deal], initial_suppression_steps=[d[1] for d in deal],
               max_new_tokens=budget)
    assert m.last_stats["refills"] == n_req - 8
    assert m._samp is None and m._samp_bound == []
    left_out = compared = tokens = 0
    for i, (want, margin) in sorted(infer_reference.items()):
        print("request %d %s: oracle margin %.3g, %d tokens" % (i, deal[i], margin, len(got[i])))
        if margin < 1e-4:
            left_out += 1
            continue
        L = len(rs[i][0]) + len(rs[i][1])
        assert len(got[i]) >= min(len(want), 86 - L) and len(got[i]) <= len(want), (i, len(got[i]), len(want), L)
        assert np.array_equal(got[i], want[: len(got[i])]), (loop, i, deal[i], got[i].tolist(), want.tolist())
        compared += 1
        tokens += len(got[i])
    print("compared %d requests (%d tokens), left out below the 1e-4 margin: %d" % (compared, tokens, left_out))
    assert left_out <= 2 and compared >= 16 and tokens >= 10 * compared
    scalar = _run(m, X, Y, Bt, loop, max_new_tokens=budget)
    for i in range(1, n_req, 4):
        assert np.array_equal(got[i], scalar[i]), (loop, i, got[i].tolist(), scalar[i].tolist())


def _expected(raw, seen_ids, rp, suppressed, eos):
    """the logits the table instantiation must produce from the zero-table ones: suppression, then the penalty over `seen_ids`"""
    want = raw.copy()
    if suppressed:
        want[[*BARRED, eos]] = -np.inf
    scaled = np.zeros(raw.shape, bool)
    if rp not in (0.0, 1.0):
        ids = np.unique(seen_ids)
        r = np.float32(rp)
        with np.errstate(invalid="ignore"):
            want[ids] = np.where(want[ids] < 0, want[ids] * r, want[ids] / r).astype(np.float32)
        scaled[ids] = True
    return want, scaled


@pytest.mark.parametrize("dtype,B", [(torch.float32, 4), (torch.float32, 20), (torch.bfloat16, 4), (torch.bfloat16, 20)])
@torch.inference_mode()
def test_logits_are_the_zero_table_logits_penalised_and_suppressed(dev, world, dtype, B):
    """A real prompt pass into B slots with entries and seeded `seen` in place against the same pass with an all-zero table,
    rt["logits"] element by element: EOS is -inf in both; 280 / 486 are -inf iff the slot suppresses; a prompt token's logit
    is raw * r (raw < 0) or raw / r; every other element is bit-equal.  Then decode steps from a re-run pass, with the tokens
    given by the host (ctl[0] = 1 overrides the table, so both runs feed the same tokens): `seen` has grown by the sample, and
    280 / 486 / EOS are -inf while the step counter is below the slot's count -- at step 1 for counts 3 and 10, at step 3 for
    10 only.  4 slots: the per-sequence step; 20: the multi-sequence kernels (fp32) and the batched chain (bf16).
    The scaled elements are one fp32 multiplication or division of the same operands: rtol 1e-6 (fp32 epsilon is 1.2e-7)."""
    from gsv_tts_lite_amd import _native as N
    cfg, w = world
    m = _model(cfg, w, [(B, 96)], dtype, dev)
    if dtype == torch.bfloat16 and B >= 17:
        assert B >= N.lib().gsv_t2s_batched_min(m._h)
    rt = m._rt[B]
    V, eos = m.vocab_size, m.EOS
    rs, X, Y, Bt = _requests(B, 3, dev)
    deal = [SETS[b % 4] for b in range(B)]
    forced = [int(rs[b][1][0]) if b % 3 == 0 else 7 + 11 * b for b in range(B)]      # a prompt token again, or a new one
    steps_at = (0, 1, 3)

    def run(table):
        """logits after the prompt pass and after 1 and 3 decode steps"""
        m._samp = SS.resolve(B, 1, 1.0, 1.0, repetition_penalty=[d[0] for d in deal],
                             initial_suppression_steps=[d[1] for d in deal]) if table else None
        m._set_ctl(rt, 1, 0, True, 1.0)         # host tokens; the steps keep `seen` up to date
        rt["tok_override"].copy_(torch.tensor(forced, dtype=torch.int64))
        rt["kv_len"].zero_(); rt["x_len"].zero_(); rt["samp"].zero_()
        rt["seen"].fill_(1)                     # a previous tenant's set: the seeding has to clear it
        if table:
            m._put_request(B, range(B), range(B), m._seed_tokens(range(B), Y))
        xy, xl, yl, _, _ = m.embed_prompt(X, Y, Bt)
        m.prefill(B, 0, xy, xl, yl)
        out = [rt["logits"].cpu().numpy().copy()]
        for k in (1, 2):
            m._decode(B, k)
            out.append(rt["logits"].cpu().numpy().copy())
        return out, rt["seen"].cpu().numpy().copy()

    m._bind_sampling(rt)
    try:
        raws, _ = run(False)
        gots, seen = run(True)
    finally:
        m._samp = None
        m._unbind_sampling()
    worst = 0.0
    for k, raw, got in zip(steps_at, raws, gots):
        for b in range(B):
            rp, n = deal[b]
            assert np.isneginf(raw[b, eos]) == (k == 0)                       # the prompt pass drops the EOS column
            ids = rs[b][1] if k == 0 else np.concatenate([rs[b][1], [forced[b]]])
            want, scaled = _expected(raw[b], ids, rp, n > k, eos)
            for v in (*BARRED, eos):
                assert np.isneginf(got[b, v]) == (n > k or np.isneginf(raw[b, v])), (k, b, v, deal[b])
            assert np.array_equal(got[b][~scaled], want[~scaled]), (k, b, deal[b])     # bit-equal (-inf == -inf)
            fin = scaled & np.isfinite(want)
            if fin.any():
                rel = np.abs(got[b][fin] - want[fin]) / np.abs(want[fin])
                worst = max(worst, float(rel.max()))
                assert rel.max() <= 1e-6, (k, b, deal[b], float(rel.max()))
                assert not np.array_equal(got[b][fin], raw[b][fin])
            assert np.array_equal(np.isneginf(got[b][scaled]), np.isneginf(want[scaled]))
    print("largest relative error of a scaled logit: %.3g" % worst)
    # `seen` after the steps: exactly the prompt's and the given tokens for a penalising slot; the prompt's never entered the others'
    for b in range(B):
        row = np.zeros(V, np.uint8)
        if deal[b][0] != 1.0:
            row[rs[b][1]] = 1
        row[forced[b]] = 1
        assert np.array_equal(seen[b], row), b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_refilled_slot_keeps_nothing_of_its_previous_tenant(dev, world, dtype):
    """6 requests through a slot family of 2: odd requests penalise and suppress (1.35, 10), even ones do not, so every slot
    changes hands between the two kinds.  In each of the three loops every even request returns the scalar call's tokens (no
    `seen` row and no entry leaks into it), and the same call twice returns the same tokens.  bf16 without tail compaction, as
    test_mixed_call_equals_the_uniform_calls_request_by_request (the 1-slot level sums other FFN slices)."""
    cfg, w = world
    n_req = 6
    m = _model(cfg, w, [(2, 96)], dtype, dev)
    if dtype == torch.bfloat16:
        m.tail_levels = []
    _, X, Y, Bt = _requests(n_req, 3, dev)
    rp = [1.35 if i % 2 else 1.0 for i in range(n_req)]
    ns = [10 if i % 2 else 0 for i in range(n_req)]
    budget = [24] * n_req
    first = None
    for loop in LOOPS:
        scalar = _run(m, X, Y, Bt, loop, max_new_tokens=budget)
        a = _run(m, X, Y, Bt, loop, repetition_penalty=rp, initial_suppression_steps=ns, max_new_tokens=budget)
        b = _run(m, X, Y, Bt, loop, repetition_penalty=rp, initial_suppression_steps=ns, max_new_tokens=budget)
        assert m.last_stats["refills"] == n_req - 2
        for i in range(n_req):
            assert np.array_equal(a[i], b[i]), (loop, i)
            if i % 2 == 0:
                assert np.array_equal(a[i], scalar[i]), (loop, i, a[i].tolist(), scalar[i].tolist())
            else:
                assert not np.isin(a[i][:10], [*BARRED, m.EOS]).any(), (loop, i, a[i].tolist())
        if first is None:
            first = a
        for i in range(n_req):
            assert np.array_equal(a[i], first[i]), (loop, i)        # the same tokens in every loop


@torch.inference_mode()
def test_seed_seen_adopt_move_and_put_at_the_abi(dev, world):
    """gsv_t2s_seed_seen on rows of zero, one and 40 tokens with duplicates and ids outside the vocabulary: the rows equal a
    numpy scatter, other slots keep theirs.  gsv_t2s_adopt_slots and gsv_t2s_move_slots carry a slot's row.
    gsv_t2s_put_slot_sampling refuses a negative or NaN penalty and negative steps with GSV_ERR_ARG."""
    from gsv_tts_lite_amd import _native as N
    cfg, w = world
    m = _model(cfg, w, [(6, 96)], torch.float32, dev)
    rt = m._rt[6]
    V = m.vocab_size
    L = N.lib()
    st = N.current_stream_ptr(dev)
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    rng = np.random.default_rng(7)
    rows = [np.zeros(0, np.int64), np.array([V - 1], np.int64),
            np.concatenate([rng.integers(0, V, 30), [5, 5, 5, 0, -1, V, V + 7, 2 ** 40, -2 ** 33, 17]]).astype(np.int64)]
    assert len(rows[2]) == 40
    slots = [4, 0, 2]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    tok = _T(np.concatenate(rows), dev)
    before = (rng.random((6, V)) < 0.5).astype(np.uint8)
    rt["seen"].copy_(torch.from_numpy(before))
    N.check(L.gsv_t2s_seed_seen(m._h, 6, i32(slots), tok.data_ptr(), i32(off), 3, st))
    want = before.copy()
    for s_, r in zip(slots, rows):
        want[s_] = 0
        want[s_, r[(r >= 0) & (r < V)]] = 1
    assert np.array_equal(rt["seen"].cpu().numpy(), want)
    N.check(L.gsv_t2s_seed_seen(m._h, 6, i32([1]), None, i32([0, 0]), 1, st))         # no tokens at all: only clears
    want[1] = 0
    assert np.array_equal(rt["seen"].cpu().numpy(), want)
    assert L.gsv_t2s_seed_seen(m._h, 6, i32([6]), tok.data_ptr(), i32([0, 1]), 1, st) == GSV_ERR_ARG
    assert L.gsv_t2s_seed_seen(m._h, 6, i32([1, 1]), tok.data_ptr(), i32([0, 1, 2]), 2, st) == GSV_ERR_ARG
    assert L.gsv_t2s_seed_seen(m._h, 6, i32([1]), tok.data_ptr(), i32([3, 1]), 1, st) == GSV_ERR_ARG
    assert np.array_equal(rt["seen"].cpu().numpy(), want)

    # adopt: rows of the ahead state's slots 1, 0 go to slots 3, 5 (no prompt pass has run there: no K/V rows to copy)
    sh = m._ahead_state(2, 96)
    src = (rng.random((sh["batch"], V)) < 0.3).astype(np.uint8)
    sh["seen"].copy_(torch.from_numpy(src))
    m.adopt_slots(6, [3, 5], sh["batch"], [1, 0])
    want[3], want[5] = src[1], src[0]
    assert np.array_equal(rt["seen"].cpu().numpy(), want)
    # move: slots 0, 2 -> slots 1, 0 of a 5-slot state
    tail = m._tail_state(5, 96)
    tail["seen"].fill_(1)
    m.move_slots(5, [1, 0], 6, [0, 2])
    got = tail["seen"].cpu().numpy()
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[0], want[2]) and got[2:].all()

    m._bind_sampling(rt)
    try:
        def put(rp, n):
            e = N.SlotSampling(0, 1, 1.0, 1.0, 0, 0, rp, n)
            return L.gsv_t2s_put_slot_sampling(m._h, 6, i32([2]), (N.SlotSampling * 1)(e), 1, st)
        assert put(-0.5, 0) == GSV_ERR_ARG and b"rep_penalty" in L.gsv_last_error()
        assert put(float("nan"), 0) == GSV_ERR_ARG
        assert put(float("inf"), 0) == GSV_ERR_ARG
        assert put(1.35, -1) == GSV_ERR_ARG and b"suppress_steps" in L.gsv_last_error()
        torch.cuda.synchronize()
        assert not rt["samp"].any()                                            # a refused put writes nothing
        assert put(1.35, 10) == 0 and put(0.0, 0) == 0
    finally:
        m._unbind_sampling()
