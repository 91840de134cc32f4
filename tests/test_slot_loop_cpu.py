"""CPU checks of the host rules of continuous batching (gsv_tts_lite_amd.slot_loop) and of the decode state's description
(gsv_tts_lite_amd.t2s): the window cadence, which tokens a request keeps when a budget, a full cache or an EOS ends it, and
that a bound state's pointers reach the C ABI's fields by name.  Host functions only."""
import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import slot_loop as SL
from gsv_tts_lite_amd import t2s


@pytest.mark.parametrize("check_interval", [1, 2, 5, 7])
def test_windows_partition_the_steps_at_the_references_tests(check_interval):
    """the plain loop is `for idx in range(1000): step; if idx % check_interval == 0: test`, repeated"""
    total, idx, done, untested = 2100 + check_interval, 0, 0, []
    while done < total:
        n, nxt = SL.next_window(idx, check_interval)
        assert n >= 1 and idx + n <= 1000
        last = idx + n - 1                                  # index of the window's last step in the plain loop
        assert not any(i % check_interval == 0 for i in range(idx, last)), "a test of the plain loop inside a window"
        closes = last == 999
        assert last % check_interval == 0 or closes         # a boundary falls behind a tested index, or closes the cycle
        assert SL.reference_tests(idx, n, check_interval) == (last % check_interval == 0)
        if not SL.reference_tests(idx, n, check_interval):
            untested.append(done + n)
        assert nxt == (0 if closes else last + 1)           # the windows partition the steps: the next starts where this ends
        idx, done = nxt, done + n
    # untested: exactly the windows that close a cycle behind an index the plain loop does not test
    assert untested == [c for c in (1000, 2000) if 999 % check_interval != 0]


class _Device:
    """the stepped state, simulated: slot i decodes request `req[i]` from `load` to `park`; sample s of a request is the EOS when
    s == eos[request].  The read-back of a window is what eos_at held behind its steps, in one of two buffers."""

    def __init__(self, B, eos):
        self.eos_of, self.req, self.steps, self.parked = eos, [None] * B, [0] * B, [True] * B
        self.windows = {}               # request -> the windows it was live in
        self.buf, self.issued = [None, None], 0

    def load(self, i, r):
        assert self.parked[i]
        self.req[i], self.steps[i], self.parked[i], self.windows[r] = r, 0, False, []

    def window(self, n, buf):
        for i in range(len(self.req)):
            if not self.parked[i]:
                self.steps[i] += n
                self.windows[self.req[i]].append(n)
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
        return 1000 * self.req[i] + torch.arange(a0, a0 + max(0, n))

    def park(self, i):
        self.parked[i] = True


class _Loop(SL.SlotLoop):
    """the policy of the simulation: an emptied slot takes the next request a few windows later"""

    def __init__(self, rng, *args):
        super().__init__(*args)
        self.rng, self.free = rng, {}       # slot -> window from which it takes the next request

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


def _expected(start, windows, eos, budget, check_interval, cap):
    """(tokens kept, windows the request is live in), restated per request: behind each window a budget or a full cache ends it
    at once; an EOS ends it one window after the read-back that shows it"""
    steps = 0
    for j, n in enumerate(windows):
        seen_before = j > 0 and eos is not None and eos <= steps    # shown by the read-back of the window before
        steps += n
        full = start + steps + check_interval >= cap
        over = budget is not None and steps - 1 >= budget
        if full or over:
            n_max = budget if over else steps - 1
            e = eos if eos is not None and eos <= steps else -1
            return (n_max if e < 1 else min(n_max, e - 1)), j + 1
        if seen_before:
            return max(0, eos - 1), j + 1
    raise AssertionError("the request never ended")


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_every_request_is_collected_once_with_the_tokens_its_end_rule_keeps(seed):
    B, cap, check_interval, n_req = 4, 160, 5, 40
    rng = np.random.default_rng(seed)
    prompt = [int(rng.integers(4, 60)) for _ in range(n_req)]
    eos = [None if rng.random() < 0.25 else int(rng.integers(0, 70)) for _ in range(n_req)]
    budget = [None if rng.random() < 0.4 else int(rng.integers(0, 50)) for _ in range(n_req)]
    # EOS at sample 0 and 1; a budget of 0; an EOS inside the window that also reaches the budget; requests that fill the cache
    # (no EOS: from a short and from a long prompt, with and without a budget beyond the cache)
    fixed = [(10, 0, None), (11, 1, None), (12, 9, 0), (13, 0, 0), (14, 8, 7), (15, 5, 7), (16, 7, 7), (9, None, None),
             (150, None, None), (154, 30, None), (100, None, 400), (20, 1, 1), (21, 12, 11)]
    for r, (p, e, b) in zip(rng.permutation(n_req)[: len(fixed)].tolist(), fixed):
        prompt[r], eos[r], budget[r] = p, e, b
    if seed >= 2:       # a call without budgets; otherwise max_new_tokens holds a number per request: "none" is one never reached
        budget = [None] * n_req
    given = None if seed >= 2 else [10 ** 9 if b is None else b for b in budget]
    dev = _Device(B, eos)
    for i in range(B):
        dev.load(i, i)
    queue = iter(range(B, n_req))
    finished = []
    loop = _Loop(rng, dev, B, list(range(B)), prompt[:B], cap, check_interval, given, lambda: next(queue, None), False,
                 lambda r: prompt[r], lambda r, seg: finished.append(r))
    pred, orig = loop.run()
    assert sorted(orig) == list(range(n_req)) and finished == orig         # every request once, on_finish for each
    for r, seg in zip(orig, pred):
        keep, live = _expected(prompt[r], dev.windows[r], eos[r], budget[r], check_interval, cap)
        assert len(dev.windows[r]) == live, (r, dev.windows[r], live)
        assert seg.tolist() == [1000 * r + prompt[r] + 1 + k for k in range(keep)], (r, prompt[r], eos[r], budget[r], seg.tolist())
    st = loop.last_stats
    assert sum(_windows(st["steps"], check_interval)) == st["steps"]        # whole windows of the cadence
    assert st["live_slot_steps"] == sum(sum(w) for w in dev.windows.values()) <= st["slot_steps"] == B * st["steps"]


def _windows(total, check_interval):
    idx, done = 0, 0
    while done < total:
        n, idx = SL.next_window(idx, check_interval)
        done += n
        yield n


def test_the_end_rules():
    assert SL.host_end(10, 6, 5, 160, None) is None
    assert SL.host_end(10, 144, 5, 160, None) is None and SL.host_end(10, 145, 5, 160, None) == 144      # full: 10 + 145 + 5 >= 160
    assert SL.host_end(10, 6, 5, 160, 6) is None and SL.host_end(10, 6, 5, 160, 5) == 5
    assert SL.host_end(10, 11, 5, 160, 7) == 7 and SL.host_end(10, 1, 5, 160, 0) == 0
    assert SL.host_end(150, 6, 5, 160, 40) == 5                                                          # full before the budget
    assert [SL.kept(7, e) for e in (-1, 0, 1, 2, 8, 9)] == [7, 7, 0, 1, 7, 7]


def test_state_description_names_the_abi_fields():
    keys = [key for key, _, _ in t2s.state_spec(3, 16, 1025, 512)]
    fields = [f for f, _ in N.T2SState._fields_]
    assert fields[:2] == ["batch", "max_kv"]
    assert sorted(t2s.STATE_FIELD[k] for k in keys) == sorted(set(fields[2:]) - {"k_cache", "v_cache"}) and len(keys) == 11
    assert t2s.STATE_FIELD["k"] == "k_cache" and t2s.STATE_FIELD["v"] == "v_cache" and set(t2s.STATE_FIELD) == set(keys) | {"k", "v"}
    assert set(t2s.STATE_INIT) <= set(keys)
    shapes = {key: (shp, dt) for key, shp, dt in t2s.state_spec(3, 16, 1025, 512)}
    assert shapes["pre_tokens"] == ((3, 17), torch.int64) and shapes["seen"] == ((3, 1025), torch.uint8)
    assert shapes["hidden"] == ((3, 512), torch.float32) and shapes["ctl"] == ((8,), torch.int32)
    # by name, not by position: each dummy pointer lands in the field of its key, whatever order the keys come in
    ptrs = {key: 0x1000 * (n + 1) for n, key in enumerate(reversed(sorted(t2s.STATE_FIELD)))}
    st = t2s.state_struct(3, 16, ptrs)
    assert (st.batch, st.max_kv) == (3, 16)
    for key, p in ptrs.items():
        assert getattr(st, t2s.STATE_FIELD[key]) == p
    with pytest.raises(KeyError):
        t2s.state_struct(3, 16, {k: p for k, p in ptrs.items() if k != "fctl"})
