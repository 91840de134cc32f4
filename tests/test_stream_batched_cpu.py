"""CPU check of the chunk protocol of Text2SemanticDecoder.infer_stream_batched (gsv_tts_lite_amd.slot_loop: the `on_chunks` hook of
SlotLoop and `stream_chunks` over its windows) on a simulated stepped state, in the manner of tests/test_slot_loop_cpu.py: per
request the (token rows, is_final) it yields are those of a plain restatement of `infer_stream`'s loop, whichever slot and window
the request lands in.  A token is its row of pre_tokens: request r's row a reads 1000 r + a."""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import slot_loop as SL

CAP, CHECK = 400, 5


class _Device:
    """slot i decodes request req[i] from `load` to `park`; sample s of a request is the EOS when s == eos[request]"""

    def __init__(self, B, eos):
        self.eos_of, self.req, self.steps, self.parked = eos, [None] * B, [0] * B, [True] * B
        self.buf, self.issued, self.reads = [None, None], 0, 0

    def load(self, i, r):
        assert self.parked[i]
        self.req[i], self.steps[i], self.parked[i] = r, 0, False

    def window(self, n, buf):
        for i in range(len(self.req)):
            if not self.parked[i]:
                self.steps[i] += n
        eos_at = [-1 if r is None or self.eos_of[r] is None or self.eos_of[r] > s else self.eos_of[r]
                  for r, s in zip(self.req, self.steps)]
        self.issued += 1
        self.buf[buf] = (self.issued, eos_at)
        return self.issued

    def eos(self, buf, ev):
        assert self.buf[buf][0] == ev, "the buffer was overwritten before its window was examined"
        return self.buf[buf][1]

    def tokens(self, i, a0, n):
        assert not self.parked[i], "a slot's rows are read after it was given up"
        self.reads += 1
        return 1000 * self.req[i] + torch.arange(a0, a0 + max(0, n))

    def park(self, i):
        self.parked[i] = True


class _Loop(SL.SlotLoop):
    """an emptied slot takes the next request zero to two windows later"""

    def __init__(self, rng, *args):
        super().__init__(*args)
        self.rng, self.free = rng, {}

    def ended(self, i):
        self.stepped.park(i)
        self.state[i] = SL.EMPTY
        self.free[i] = self.window + 1 + int(self.rng.integers(0, 3))

    def before_window(self, block):
        for i in [i for i, w in sorted(self.free.items()) if block or w <= self.window]:
            del self.free[i]
            nr = self.next_request()
            if nr is not None:
                self.stepped.load(i, nr[0])
                self.admit(i, *nr)

    def after_window(self):
        pass

    def idle(self):
        return False


def _infer_stream(r, start, e, chunk, boost):
    """Text2SemanticDecoder.infer_stream's loop (t2s.py) for a request of prompt length `start` whose sample `e` is the EOS:
    windows of at most 5 steps that stop at the chunk boundaries, the EOS tested behind each"""
    rows = lambda a, n: [1000 * r + k for k in range(a, a + n)]
    out, done, first, pre = [], 0, True, None
    while True:
        done += min(5, chunk - done % chunk)
        if e <= done:
            return out + [(rows(start, e), True)]           # pre_tokens[Lp: Lp + eos_at]: starts with sample 0
        if done % chunk == 0:
            if pre is not None:
                out.append((pre, False))
            pre = rows(start + 1, done)
            if boost and first:
                first = False
                out.append((pre, False))
                pre = None


def _requests(rng, n_req):
    prompt = [int(rng.integers(4, 60)) for _ in range(n_req)]
    eos = [int(rng.integers(1, 90)) for _ in range(n_req)]
    # an EOS in the first window (sample 1: the one-step window that opens a cycle; sample 3: inside a later request's first
    # five steps), on a chunk boundary and one beside it for every chunk size of the grid
    for r, e in zip(rng.permutation(n_req).tolist(), [1, 3, 2, 5, 6, 8, 9, 24, 25, 26, 50, 51, 16]):
        eos[r] = e
    return prompt, eos


def _run(seed, B, chunk, boost, prompt, eos, stream=True):
    rng = np.random.default_rng(seed)
    n_req = len(prompt)
    dev = _Device(B, eos)
    for i in range(B):
        dev.load(i, i)
    queue = iter(range(B, n_req))
    loop = _Loop(rng, dev, B, list(range(B)), prompt[:B], CAP, CHECK, None, lambda: next(queue, None), False,
                 lambda r: prompt[r], None)
    if not stream:
        return loop, loop.run()
    got = {}
    for r, rows, is_final in SL.stream_chunks(loop, chunk, boost):
        assert not got.get(r) or not got[r][-1][1], "a chunk behind the final one"
        got.setdefault(r, []).append((rows.tolist(), is_final))
    return loop, got


@pytest.mark.parametrize("boost", [True, False])
@pytest.mark.parametrize("chunk", [3, 5, 8, 25])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_every_request_streams_what_infer_stream_streams(B, chunk, boost):
    n_req = 14                  # more requests than slots
    prompt, eos = _requests(np.random.default_rng(100 + B), n_req)
    flags = [boost] * n_req
    flags[3] = not boost        # one bool per request
    loop, got = _run(7, B, chunk, flags, prompt, eos)
    assert sorted(got) == list(range(n_req))
    for r in range(n_req):
        want = _infer_stream(r, prompt[r], eos[r], chunk, flags[r])
        assert got[r] == want, (r, prompt[r], eos[r], got[r], want)
        assert got[r][-1][1] and not any(f for _, f in got[r][:-1])
        assert got[r][-1][0][0] == 1000 * r + prompt[r]                                # the final chunk starts with sample 0
        assert all(t < 1000 * r + prompt[r] + eos[r] for rows, _ in got[r] for t in rows)   # nothing at or behind the EOS
    # what run() returns is what it returned: the same requests through a loop that does not stream
    plain, (pred, orig) = _run(7, B, chunk, flags, prompt, eos, stream=False)
    assert orig == loop.orig and [p.tolist() for p in pred] == [p.tolist() for p in loop.pred]
    for r, seg in zip(orig, pred):
        assert seg.tolist() == [1000 * r + prompt[r] + 1 + k for k in range(eos[r] - 1)]
    assert plain.last_stats == loop.last_stats and not loop.handed


@pytest.mark.parametrize("chunk", [3, 8])
def test_a_request_the_host_ends_streams_from_its_saved_rows(chunk):
    """a full cache ends a request with no lag and its slot is given up at once: its chunks and its final rows come from the copy
    taken then (the simulated state refuses a read of a parked slot).  Without an EOS the final rows are what run() collects; with
    an EOS inside the last window they are infer_stream's."""
    cap = 60
    prompt, eos = [20, 30, 10, 28], [None, 12, None, 27]
    dev = _Device(2, eos)
    for i in range(2):
        dev.load(i, i)
    queue = iter(range(2, 4))
    loop = _Loop(np.random.default_rng(3), dev, 2, [0, 1], prompt[:2], cap, CHECK, None, lambda: next(queue, None), False,
                 lambda r: prompt[r], None)
    got = {}
    for r, rows, is_final in SL.stream_chunks(loop, chunk, [True] * 4):
        got.setdefault(r, []).append((rows.tolist(), is_final))
    kept = dict(zip(loop.orig, loop.pred))
    for r in range(4):
        if eos[r] is not None and len(kept[r]) == eos[r] - 1:       # ended by its EOS, seen by the host or not
            assert got[r] == _infer_stream(r, prompt[r], eos[r], chunk, True), r
            continue
        v = len(kept[r])
        assert got[r][-1] == (kept[r].tolist(), True) and v > 0
        sent = [rows for rows, f in got[r][:-1]]
        bounds = [k * chunk for k in range(1, v // chunk + 1)]
        lagged = [bounds[0]] + bounds[1:-1] if bounds else []       # boosted: the first at once, the others one behind
        assert [len(s) for s in sent] == lagged, (r, v, [len(s) for s in sent])
        assert all(s == kept[r].tolist()[: len(s)] for s in sent)
    assert eos[3] is not None and len(kept[3]) == eos[3] - 1 and 28 + 27 + CHECK >= cap     # request 3: an EOS the host end hides
