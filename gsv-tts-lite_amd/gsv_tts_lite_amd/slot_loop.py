"""The slot loops of continuous batching (t2s_model.py:555-734) behind `Text2SemanticDecoder.infer_batched`'s first prompt pass.

Three loops decode the same requests to the same tokens per request:

  * `reference_order` waits for every window and refills in the reference's order (completion order is the reference's);
  * `StagedLoop` (async_refill, GSV_REFILL_AHEAD=0): a finished slot is parked, its prompt pass runs on a side stream into the
    live rows, and it joins at a later window boundary;
  * `AheadLoop` (async_refill, the default): the next requests' prompt passes run ahead into a second bound state, a finished
    slot adopts one before the next window, and the last live requests move to a smaller state once the queue is empty.

What the two asynchronous loops share is written once: the host rules that decide which tokens a request returns (`next_window`,
`host_end`, `kept`: plain arithmetic) and `SlotLoop`, the bookkeeping around them.  A loop supplies only its refill policy.
"""
import numpy as np
import torch

CYCLE = 1000    # the reference's inner loop: `for idx in range(1000)`, EOS tested when idx % check_interval == 0


def next_window(idx, check_interval):
    """(steps of the window that starts at index `idx` of the reference's inner loop, index the next one starts at): the
    reference tests after steps 1, 6, 11, ... of each 1000-iteration inner loop, and a window is the steps between two tests"""
    n = 1 if idx == 0 else min(check_interval, CYCLE - idx)
    return n, (0 if idx + n >= CYCLE else idx + n)


def reference_tests(idx, n, check_interval):
    """does the reference test for EOS behind the window of `n` steps from `idx`?  Not behind the one that closes a cycle short"""
    return (idx + n - 1) % check_interval == 0


def host_end(start, steps, check_interval, cap, budget):
    """the most tokens a slot returns if it ends behind this window by a rule the host can evaluate, else None.  `start`: the
    kv_len it joined with, `steps`: issued since.  Full cache: the reference's last bucket (kv + check_interval >= max_kv);
    budget: the request has produced that many tokens (sample 0, the prompt pass's, is never returned)."""
    full = start + steps + check_interval >= cap
    if full or (budget is not None and steps - 1 >= budget):
        return steps - 1 if budget is None else min(steps - 1, budget)
    return None


def kept(n_max, e):
    """tokens kept of `n_max`, given the device's eos_at `e`: the index of the first EOS among the slot's samples, or -1"""
    return n_max if e < 1 else min(n_max, e - 1)


LIVE, EMPTY = 0, 1


class SlotLoop:
    """Bookkeeping of a slot loop in which the host never waits for the window it has just issued: the read-back of a window
    (kv_len, eos_at) is an asynchronous copy examined one window later, while the next window runs.  Ends the host can
    predict (`host_end`) free the slot with no lag, its tokens saved behind that window's steps; an EOS is seen one window
    (<= check_interval garbage steps of that slot) late.  Tokens are cut at the first EOS from the device's eos_at, so the
    lag never shows.

    `stepped` is the state the windows run on: window(n, buf) -> event, eos(buf, event) -> eos_at per slot as that window
    left it, tokens(slot, first row, count) -> a copy, park(slot).  A policy (subclass) supplies `ended(slot)`: what becomes of
    a slot that ended; `before_window(block)`: slots take requests (block: no slot is live, nothing to overlap a wait with);
    `after_window()`: host work behind the steps the GPU is busy with; `idle()`: no slot is live and every read-back has been
    examined -- True if slots may still take requests.

    Streaming (`stream_chunk` set by the driver, Text2SemanticDecoder.infer_stream_batched): when a window's read-back is examined,
    `on_chunks` receives [(request, cumulative token rows -- a copy --, is_final)] for the slots whose count of certainly valid
    tokens has passed a multiple of `stream_chunk` (no EOS among samples 0 .. steps: `steps` tokens are valid), in order, and for
    the requests that ended.  The rows are copied while the slot still holds them: from the live slot, or from what was saved when
    the host ended it.  An end is seen one window late, so a chunk lags by up to `check_interval` steps; it never holds a token at
    or behind the EOS.  After an EOS at sample e the final rows are samples 0 .. e - 1 (`infer_stream`'s final chunk, which
    starts with the sample `collect` drops); after a host end they are what `collect` gets."""

    def __init__(self, stepped, B, first, first_len, cap, check_interval, budgets, nxt, exhausted, prompt_len, on_finish):
        self.stepped, self.B, self.cap, self.check_interval, self.budgets = stepped, B, cap, check_interval, budgets
        self.nxt, self.exhausted, self.prompt_len, self.on_finish = nxt, exhausted, prompt_len, on_finish
        pad = B - len(first)
        self.state = [LIVE] * len(first) + [EMPTY] * pad
        self.req = list(first) + [-1] * pad
        self.start = list(first_len) + [0] * pad        # kv_len the slot joined with (its prompt length)
        self.steps = [0] * B                            # steps issued since the slot joined
        self.joined = [0] * B                           # first window whose read-back shows the slot's current request
        self.window, self.idx = 0, 0
        self.to_cut = []        # (window, slot, request, saved tokens, most tokens, the saved rows: with sample 0 in front when streaming): ended by the host, tokens not cut yet
        self.snaps = []         # (window, buffer, event): read-backs not examined yet, two buffers in turn
        self.pred, self.orig = [], []
        self.stream_chunk, self.on_chunks = None, None
        self.handed = {}        # request -> chunk boundaries handed to on_chunks so far
        self.last_stats = {"slots": B, "steps": 0, "kv_rows": 0, "prefill_rows": len(first), "refills": 0,
                           "slot_steps": 0, "live_slot_steps": 0}

    def next_request(self):
        """(request, prompt length) from the queue, or None once it is empty"""
        cur = None if self.exhausted else self.nxt()
        if cur is None:
            self.exhausted = True
            return None
        n_new = self.prompt_len(cur)
        if n_new > self.cap - 1:
            raise ValueError("prompt longer than the largest KV bucket")
        return cur, n_new

    def admit(self, i, cur, n_new):
        self.state[i], self.req[i], self.steps[i], self.start[i], self.joined[i] = LIVE, cur, 0, n_new, self.window

    def collect(self, r, seg):
        self.pred.append(seg)
        self.orig.append(r)
        if self.on_finish is not None:
            self.on_finish(r, seg)

    def issue_window(self):
        n, self.idx = next_window(self.idx, self.check_interval)
        buf = self.window & 1
        ev = self.stepped.window(n, buf)
        for key, count in (("steps", 1), ("slot_steps", self.B), ("live_slot_steps", self.state.count(LIVE))):
            self.last_stats[key] += count * n
        for i in range(self.B):
            if self.state[i] != LIVE:
                continue
            self.steps[i] += n
            self.last_stats["kv_rows"] += (self.start[i] + self.steps[i]) * n
            budget = None if self.budgets is None else int(self.budgets[self.req[i]])
            n_max = host_end(self.start[i], self.steps[i], self.check_interval, self.cap, budget)
            if n_max is not None:
                # the slot may decode another request from the next window on: its tokens are saved now (behind this
                # window's steps on the stream), cut at the first EOS when the window's read-back is in
                lead = 1 if self.stream_chunk else 0        # a stream's final chunk behind an EOS starts with sample 0
                rows = self.stepped.tokens(i, self.start[i] + 1 - lead, n_max + lead)
                self.to_cut.append((self.window, i, self.req[i], rows[lead:], n_max, rows))
                self.ended(i)
        self.snaps.append((self.window, buf, ev, list(self.steps) if self.stream_chunk else None))

    def boundaries(self, out, r, valid, rows):
        """the chunk boundaries of request `r` that `valid` tokens pass; rows(n) -> a copy of its first n tokens"""
        k = self.handed.get(r, 0)
        while (k + 1) * self.stream_chunk <= valid:
            k += 1
            out.append((r, rows(k * self.stream_chunk), False))
        self.handed[r] = k

    def examine(self, window, buf, ev, steps=None):
        """read-back of `window` (taken after its steps; `steps`: per slot, issued up to it): cut what the host ended at that
        boundary, find EOS ends, hand out the chunks of a stream"""
        eos = self.stepped.eos(buf, ev)
        out = []
        for rec in [c for c in self.to_cut if c[0] == window]:
            _, i, r, saved, n_max, rows = rec
            keep = max(0, kept(n_max, eos[i]))
            self.collect(r, saved[:keep].clone())
            self.to_cut.remove(rec)
            if self.stream_chunk:
                self.boundaries(out, r, keep, lambda n: saved[:n].clone())
                self.handed.pop(r)
                out.append((r, rows[: eos[i]].clone() if 1 <= eos[i] <= n_max + 1 else saved[:keep].clone(), True))
        for i in range(self.B):
            if self.state[i] != LIVE or self.joined[i] > window:
                continue
            r, e = self.req[i], eos[i]
            if e >= 0 and not self.stream_chunk:
                self.collect(r, self.stepped.tokens(i, self.start[i] + 1, e - 1))
                self.ended(i)
            elif e >= 0:
                rows = self.stepped.tokens(i, self.start[i], e)         # samples 0 .. e - 1
                self.collect(r, rows[1:])
                self.boundaries(out, r, max(0, e - 1), lambda n: rows[1: 1 + n].clone())
                self.handed.pop(r)
                out.append((r, rows, True))
                self.ended(i)
            elif self.stream_chunk:
                self.boundaries(out, r, steps[i], lambda n: self.stepped.tokens(i, self.start[i] + 1, n))
        if out:
            self.on_chunks(out)

    def drain(self):
        while self.snaps:
            self.examine(*self.snaps.pop(0))

    def run(self):
        """-> (tokens per request in completion order, their request indices); ends when `idle` says nothing is left"""
        for _ in self.windows():
            pass
        return self.pred, self.orig

    def windows(self):
        """`run` as a generator: yields wherever read-backs have been examined (a stream's chunks are with `on_chunks` by then)"""
        while True:
            live = LIVE in self.state
            if not live:
                self.drain()                        # nothing is running that the read-backs could hide behind
                yield
            self.before_window(block=not live)
            if LIVE not in self.state:
                if self.idle():
                    continue
                break
            self.issue_window()
            self.after_window()
            while len(self.snaps) > 1:              # the PREVIOUS window's read-back: on the host by now
                self.examine(*self.snaps.pop(0))
            self.window += 1
            yield
        self.drain()
        assert not self.to_cut


def stream_chunks(loop, stream_chunk, boost, ticks=False):
    """`infer_stream`'s chunk protocol (t2s_model.py:466-553) over the windows of a slot loop: a generator of (request, cumulative
    token rows, is_final).  The loop reports when a request's valid tokens pass a multiple of `stream_chunk` (`on_chunks`); a
    request's chunk is sent when its NEXT one is known -- the first at once if boost[request] -- and the final rows end it.  The
    windows are issued inside torch.inference_mode; the consumer runs outside it, between two windows.  `ticks`: (None, None,
    False) behind every window as well, for a consumer with work of its own to poll while the slots decode."""
    chunks, state = [], {}          # state: request -> (no chunk sent yet, the chunk held back)
    loop.stream_chunk, loop.on_chunks = stream_chunk, chunks.extend
    windows, running = loop.windows(), True
    while running:
        with torch.inference_mode():
            running = next(windows, False) is None
        for r, rows, is_final in chunks[:]:
            first, held = state.pop(r, (True, None))
            if is_final:
                yield r, rows, True
                continue
            if held is not None:
                yield r, held, False
            held = rows
            if boost[r] and first:
                first, held = False, None
                yield r, rows, False
            state[r] = (first, held)
        del chunks[:]
        if ticks and running:
            yield None, None, False


class _Stepped:
    """a bound state of the decoder as `SlotLoop` steps it, with the pinned two-buffer read-back of (kv_len, eos_at)"""

    def __init__(self, dec, B):
        self.dec, self.B, self.rt = dec, B, dec._rt[B]
        self.main = torch.cuda.current_stream(dec.device)
        self.host = torch.empty((2, 2, B), dtype=torch.int64).pin_memory()

    def window(self, n, buf):
        self.dec._decode(self.B, n)
        self.dec._flush(self.B)
        self.host[buf].copy_(torch.stack([self.rt["kv_len"], self.rt["eos_at"].to(torch.int64)]), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(self.main)
        return ev

    def eos(self, buf, ev):
        ev.synchronize()
        return self.host[buf].tolist()[1]

    def tokens(self, i, a0, n):
        return self.rt["pre_tokens"][i, a0: a0 + max(0, n)].clone()

    def park(self, i):
        self.rt["kv_len"][i] = -1       # the step leaves the slot's rows and state alone and attends over one row


class _RefillLoop(SlotLoop):
    """what the two policies share: the decoder, the requests, and a prompt pass on the side stream.  The prefill of `first`
    into slots 0.. has already run on the current stream."""

    def __init__(self, dec, x, y, bert_feature, B, first, nxt, exhausted, first_len, check_interval, on_finish,
                 max_new_tokens, stream_by_request=False):
        cap = max(b.max_kv_cache for b in dec.cuda_graph_buckets[B])
        super().__init__(_Stepped(dec, B), B, first, first_len, cap, check_interval, max_new_tokens, nxt, exhausted,
                         lambda c: int(x[c].shape[0]) + int(y[c].shape[0]), on_finish)
        self.dec, self.x, self.y, self.bert_feature, self.stream_by_request = dec, x, y, bert_feature, stream_by_request
        dec.last_stats = self.last_stats
        if dec._refill_stream is None:
            dec._refill_stream = torch.cuda.Stream(device=dec.device, priority=dec.refill_priority)
        self.side, self.main = dec._refill_stream, self.stepped.main
        # the requests' inputs (phoneme ids, prompt tokens, BERT rows) were produced on the caller's stream; the side stream
        # reads them in embed_prompt BEFORE it waits on any step.  One event orders the inputs, not the steps.
        inputs_ready = torch.cuda.Event()
        inputs_ready.record(self.main)
        self.side.wait_event(inputs_ready)
        if len(first) < B:
            self.stepped.rt["kv_len"][len(first):] = -1

    def prompt_pass(self, batch, group, after, with_ids=False):
        """one packed prompt pass on the side stream for `group` [(slot of state `batch`, request, prompt length)], behind the
        event `after` -> (completion event, tensors to keep alive until it has fired)"""
        dec, dev = self.dec, self.dec.device
        rq = [c for _, c, _ in group]
        with torch.cuda.stream(self.side):
            # the embedding and its host->device copies first: they depend on nothing the steps do, and a pageable
            # copy blocks the host until its stream gets there -- it must not sit behind the wait on the steps
            xy, xl, yl, _, _ = dec.embed_prompt([self.x[c] for c in rq], [self.y[c] for c in rq], [self.bert_feature[c] for c in rq])
            sl = torch.tensor([i for i, _, _ in group], dtype=torch.int32, device=dev)
            ids = torch.tensor([dec._stream_id(c) for c in rq], dtype=torch.int64, device=dev) if with_ids else None
            seed = dec._seed_tokens(rq, self.y)
            if after is not None:
                self.side.wait_event(after)
            # the slots' penalty sets and table entries, behind the last step that recorded their previous tenants' tokens
            dec._put_request(batch, [i for i, _, _ in group], rq, seed)
            dec.prefill_slots_staged(batch, sl, xy, xl, yl, self.side.cuda_stream)
            done = torch.cuda.Event()
            done.record(self.side)
        self.last_stats["refills"] += len(group)
        self.last_stats["prefill_rows"] += len(group)
        return done, (xy, xl, yl, sl, ids)


class StagedLoop(_RefillLoop):
    """A finished slot is PARKED (kv_len = -1) and given the next request at once; the prompt pass of the parked slots runs on
    a side stream into the live K/V rows and the library's staging, and they join at the first window boundary after the
    pass has completed (gsv_t2s_prefill_slots_staged / gsv_t2s_commit_slots).

    Which request a slot gets is decided when the slot is parked, rows are independent through every kernel, so every
    request's tokens equal the reference-order loop's (tests/test_hip_t2s.py); completion ORDER and the window a request
    joins at depend on timing."""

    def __init__(self, *args):
        super().__init__(*args)
        self.waiting = []           # (slot, request, prompt length): parked, prompt pass not launched yet
        self.waiting_since = 0      # window at which the oldest of them was parked
        self.inflight = None        # the one staged prompt pass: (group, completion event, keep-alive tensors)

    def ended(self, i):
        self.stepped.park(i)
        self.state[i] = EMPTY
        nr = self.next_request()
        if nr is None:
            return
        self.req[i] = nr[0]
        self.waiting.append((i,) + nr)
        if len(self.waiting) == 1:
            self.waiting_since = self.window

    def after_window(self, force=False):
        if self.inflight or not self.waiting:
            return
        # a prompt pass is ~120 launches whatever its row count and takes its share of the chip from the steps: a lone
        # request waits one window for company (costs 1/B of a window's tokens, saves most of a pass)
        dec = self.dec
        if not force and len(self.waiting) < dec.refill_group and self.window - self.waiting_since < dec.refill_wait:
            return
        group, self.waiting = self.waiting, []
        ev = torch.cuda.Event()
        ev.record(self.main)        # the parking writes, and every step that still wrote these slots' rows
        self.inflight = (group,) + self.prompt_pass(self.B, group, ev, with_ids=True)

    def before_window(self, block):
        """a completed prompt pass joins: staging -> live state on the steps' stream"""
        if not self.inflight:
            return
        group, done, (_, _, _, sl, ids) = self.inflight
        if block:
            done.synchronize()
        elif not done.query():
            return
        self.main.wait_event(done)
        self.dec.commit_slots(self.B, sl)
        sl.record_stream(self.main)     # allocated on the side stream's pool, read here by the steps' stream
        if self.stream_by_request:      # device sampling: the joined slots draw from their requests' noise streams
            self.stepped.rt["tok_override"].index_copy_(0, sl.long(), ids)
            ids.record_stream(self.main)
        for i, cur, n_new in group:
            self.admit(i, cur, n_new)
        self.inflight = None

    def idle(self):
        if self.waiting and not self.inflight:      # nothing left to overlap the prompt pass with
            self.after_window(force=True)
        return bool(self.inflight)


class AheadLoop(_RefillLoop):
    """The prompt passes run AHEAD of the slots that will decode them.

    `StagedLoop` starts a request's prompt pass when a slot has finished: the slot idles for the pass and for the windows
    around it (two to three windows of five steps per refill), and a pass carries the one or two requests whose slots
    happened to finish together (a pass of one costs what a pass of two costs: ~120 dependent launches).  Here up to
    `refill_ahead` of the NEXT requests are prefilled, several per pass, on a side stream into a second bound state that is
    never stepped (`_ahead_state`); a slot that finishes at a window boundary takes a finished one before the next window is
    issued (gsv_t2s_adopt_slots: its K/V rows and staged state move over, ~10 us) and decodes on.  A prompt pass is
    row-independent and packing-invariant, so every request's tokens equal the reference-order loop's
    (tests/test_hip_t2s.py); which slot and window a request gets depends on timing."""

    def __init__(self, dec, x, y, bert_feature, B, *args):
        rt = dec._rt[B]
        cap = max(b.max_kv_cache for b in dec.cuda_graph_buckets[B])
        self.sh = sh = dec._ahead_state(max(1, min(dec.refill_ahead, B)), cap)
        # tail compaction: bound BEFORE the first step (binding may re-allocate the handle's scratch), largest first
        levels = [lv for lv in sorted(set(dec.tail_levels), reverse=True) if lv < B]
        self.tails = [t for t in (dec._tail_state(lv, cap) for lv in levels) if t is not None]
        if dec._samp is not None:
            # compaction carries a slot's entry to the tail state's table (gsv_t2s_move_slots).  The ahead state is never stepped,
            # but its prompt passes penalise and suppress the first sample by ITS table and `seen`; the adopting state's token
            # kernel draws that sample, so the entry goes into both (`top_up`, `fill`)
            for t in self.tails + [sh]:
                dec._bind_sampling(t)
        for k in ("ctl", "fctl"):
            sh[k].copy_(rt[k])          # the prompt pass's first logits obey the same control words
        super().__init__(dec, x, y, bert_feature, B, *args)    # its event orders the requests' inputs AND the control words above
        self.free_src = list(range(sh["slots"]))    # slots of the ahead state holding nothing
        self.ready = []             # (source slot, request, prompt length, completion event of its pass, window), oldest first
        self.inflight = None        # completion event of the one prompt pass that may be running
        self.keep = None            # its tensors
        self.adopted_ev = None      # behind the last adopt: a later pass may overwrite the source slots it read
        self.last_stats.update({"passes": 1, "compactions": []})
        self.top_up(force=True)

    def ended(self, i):
        self.stepped.park(i)
        self.state[i], self.req[i] = EMPTY, -1

    def pass_done(self, block=False):
        """has the prompt pass in flight, if any, completed?"""
        if self.inflight is not None:
            if block:
                self.inflight.synchronize()
            elif not self.inflight.query():
                return False
            self.inflight = self.keep = None
        return True

    def top_up(self, force=False):
        """one packed prompt pass for the next requests, into the free slots of the ahead state"""
        free = self.free_src
        if self.exhausted or not free or not self.pass_done(block=force):
            return
        if not force and len(free) < max(1, self.sh["slots"] // 2) and self.ready:
            return                  # a pass of few rows costs what a pass of many costs: wait until half the slots are free
        # N ranks pull from one queue: near its end a rank takes ahead no more than its share of what is left
        # (engine.RequestSource.fair_share), so the tail is not parked in one rank's ahead slots while others idle
        share = getattr(getattr(self.nxt, "__self__", None), "fair_share", None)
        quota = len(free) if share is None else max(1, min(len(free), share()))
        group = []
        while free and len(group) < quota:
            nr = self.next_request()
            if nr is None:
                break
            group.append((free.pop(0),) + nr)
        if not group:
            return
        self.inflight, self.keep = self.prompt_pass(self.sh["batch"], group, self.adopted_ev)
        for i, c, n_new in group:
            self.ready.append((i, c, n_new, self.inflight, self.window))
        self.last_stats["passes"] += 1

    def fill(self, block):
        """empty slots take finished prompt passes, oldest first, before the next window is issued"""
        empty = [i for i in range(self.B) if self.state[i] == EMPTY]
        take = []
        while empty and self.ready:
            src, cur, n_new, done, launched = self.ready[0]
            if not done.query():
                # the steps' stream may wait for a pass that has had a window to run (it ends inside the wait, if at all);
                # a younger one would stall every slot for most of its ~1 ms: the slot idles this window instead
                if not block and self.window - launched < 1:
                    break
            self.main.wait_event(done)
            self.ready.pop(0)
            take.append((empty.pop(0), src, cur, n_new))
        if not take:
            return
        dec, rq = self.dec, [c for _, _, c, _ in take]
        dec.adopt_slots(self.B, [i for i, _, _, _ in take], self.sh["batch"], [s for _, s, _, _ in take],
                        [dec._stream_id(c) for c in rq] if self.stream_by_request else None)
        dec._put_sampling(self.B, [i for i, _, _, _ in take], rq)
        self.adopted_ev = torch.cuda.Event()
        self.adopted_ev.record(self.main)
        for i, src, cur, n_new in take:
            self.admit(i, cur, n_new)
            self.free_src.append(src)

    def compact(self):
        """queue empty, nothing prefilled ahead: the live requests continue on the smallest tail state that holds them (the
        reference keeps stepping the full batch, t2s_model.py:684-694).  Every outstanding window is read back first (its
        records name slots of the state that is left)."""
        if not self.tails or not self.exhausted or self.ready:
            return
        if not self.pass_done():    # the last prompt pass: its requests are in `ready` until adopted; nothing else will come
            return
        B, n_live = self.B, self.state.count(LIVE)
        if n_live == 0 or not any(n_live <= t["batch"] < B for t in self.tails):
            return
        self.drain()
        live = [i for i in range(B) if self.state[i] == LIVE]
        fit = [t for t in self.tails if len(live) <= t["batch"] < B]
        if not live or not fit:
            return
        rt, dst = self.stepped.rt, min(fit, key=lambda t: t["batch"])
        nb = dst["batch"]
        for k in ("ctl", "fctl"):
            dst[k].copy_(rt[k])
        dst["fused_ok"] = rt.get("fused_ok", False)
        dst["kv_len"].fill_(-1)
        self.dec.move_slots(nb, list(range(len(live))), B, live)
        self.last_stats["compactions"].append((self.window, B, nb, len(live)))
        pad = nb - len(live)
        self.state = [LIVE] * len(live) + [EMPTY] * pad
        self.req = [self.req[i] for i in live] + [-1] * pad
        self.start = [self.start[i] for i in live] + [0] * pad
        self.steps = [self.steps[i] for i in live] + [0] * pad
        self.joined = [0] * nb              # every outstanding window has been examined
        self.B, self.stepped = nb, _Stepped(self.dec, nb)

    def before_window(self, block):
        self.fill(block)
        if LIVE in self.state:
            self.compact()

    def after_window(self):
        self.top_up()

    def idle(self):
        if not self.ready:
            self.top_up(force=True)
        return bool(self.ready)


def reference_order(dec, x, y, bert_feature, batch_size, first, nxt, exhausted, bucket_i, check_interval, on_finish,
                    max_new_tokens, mode):
    """The reference's own order (t2s_model.py:620-734): every window is waited for, the slots that finished in it are
    refilled by one packed prompt pass on the steps' stream while all slots wait, idle slots keep stepping (parked).
    `bucket_i`: the bucket the first prompt pass chose."""
    rt, dev, EOS = dec._rt[batch_size], dec.device, dec.EOS
    caps = [b.max_kv_cache for b in dec.cuda_graph_buckets[batch_size]]
    actual = len(first)
    rows = torch.arange(batch_size, device=dev)
    pred, orig = [], []
    stats = dec.last_stats = {"slots": batch_size, "steps": 0, "kv_rows": 0, "prefill_rows": actual, "refills": 0}
    slot_orig = first + [-1] * (batch_size - actual)
    steps = [0] * batch_size
    ignore = [i >= actual for i in range(batch_size)]
    stop = False
    idx = 0
    since = 0
    while not stop:
        at = idx
        n, idx = next_window(at, check_interval)
        dec._decode(batch_size, n)
        for b in range(batch_size):
            steps[b] += n
        stats["steps"] += n
        since += n
        if not reference_tests(at, n, check_interval):
            continue
        dec._flush(batch_size)
        kv = rt["kv_len"].clone()
        samples = rt["pre_tokens"][rows, kv.clamp(max=rt["T"])]
        kv_h, smp = torch.stack([kv, samples.to(kv.dtype)]).tolist()   # one device->host copy per window
        stats["kv_rows"] += sum(kv_h) * since       # ~ K/V rows read by the steps since the previous window
        since = 0
        cap = caps[min(bucket_i, len(caps) - 1)]
        reached = [k + check_interval >= cap for k in kv_h]
        eos = [t == EOS for t in smp]
        if max_new_tokens is not None:   # a token budget ends a request like an EOS would
            eos = [e or (slot_orig[b] >= 0 and steps[b] - 1 >= max_new_tokens[slot_orig[b]]) for b, e in enumerate(eos)]
        fin = [(not ignore[b]) and (eos[b] or reached[b]) for b in range(batch_size)]
        if not any(fin):
            continue
        if any(reached):
            bucket_i += 1
            if bucket_i < len(caps):
                reached = [False] * batch_size
        fin = [(not ignore[b]) and (eos[b] or reached[b]) for b in range(batch_size)]
        if not any(fin):
            continue
        refill = []   # (slot, request) pairs of this window: the reference prefills them one by one in this order
        fin_idx = [b for b in range(batch_size) if fin[b]]
        fin_rows = rt["pre_tokens"][fin_idx].cpu().numpy()      # one copy for every sequence that finished
        for j, i in enumerate(fin_idx):
            a0, b0 = kv_h[i] - steps[i] + 1, kv_h[i]
            hit = np.nonzero(fin_rows[j, a0:b0] == EOS)[0]   # cut at the first EOS (t2s_model.py:675-678)
            n_keep = int(hit[0]) if hit.size else max(0, b0 - a0)
            if max_new_tokens is not None:
                n_keep = min(n_keep, int(max_new_tokens[slot_orig[i]]))
            seg = rt["pre_tokens"][i, a0: a0 + n_keep]
            pred.append(seg.clone())
            orig.append(slot_orig[i])
            if on_finish is not None:
                on_finish(slot_orig[i], pred[-1])
            steps[i] = 0
            kv_h[i] = 0
            rt["kv_len"][i] = 0
            mx = max(kv_h)
            bucket_i = len(caps) - 1
            for j, c in enumerate(caps):
                if c >= mx + check_interval:
                    bucket_i = j
                    break
            cur = None if exhausted else nxt()
            if cur is None:
                exhausted = True
                ignore[i] = True
                rt["kv_len"][i] = -1       # parked (gsv_tts_hip.h): an idle slot's steps attend over one row, not a growing cache
                if all(ignore):
                    stop = True
                    break
            else:
                n_new = int(x[cur].shape[0]) + int(y[cur].shape[0])
                if n_new > caps[-1]:
                    raise ValueError("prompt longer than the largest KV bucket")
                refill.append((i, cur))
                kv_h[i] = n_new            # what the slot holds once refilled: the next slots' bucket choice sees it
                slot_orig[i] = cur
        if refill and not stop:
            # rows are independent through the prefill, so the window's refills run as ONE packed prefill into their
            # scattered slots (gsv_t2s_prefill_slots) instead of one 170-launch chain per sequence
            req = [c for _, c in refill]
            xy1, xl1, yl1, _, _ = dec.embed_prompt([x[c] for c in req], [y[c] for c in req], [bert_feature[c] for c in req])
            dec._put_request(batch_size, [i for i, _ in refill], req, dec._seed_tokens(req, y))
            dec.prefill_slots(batch_size, [i for i, _ in refill], xy1, xl1, yl1)
            stats["refills"] += len(refill)
            if mode == 2:
                rt["tok_override"][torch.tensor([i for i, _ in refill], device=dev)] = \
                    torch.tensor([dec._stream_id(c) for _, c in refill], dtype=torch.int64, device=dev)
    return pred, torch.tensor(orig, device=dev)
