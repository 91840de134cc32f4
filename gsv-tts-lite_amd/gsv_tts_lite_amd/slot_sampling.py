"""Per-request sampling parameters of the continuous-batching loop: the host side of the per-slot sampling table
(gsv_t2s_set_slot_sampling, include/gsv_tts_hip.h).

`Text2SemanticDecoder.infer_batched` takes top_k / top_p / temperature / seed as scalars (one set per call, as the
reference, t2s_model.py:555-734) or as sequences indexed like its requests.  This module turns them into one entry per
request -- {sample_mode, top_k, temperature, top_p, seed, noise stream} -- and does nothing else: no torch, no device.

The anti-loop rules of `infer` (t2s_model.py:415-416, 444-447) ride in the same entry: `repetition_penalty` as a SEQUENCE
(a number is ignored by the batched loop, as in the reference, :637-651) and `initial_suppression_steps` (0: none).
"""
from __future__ import annotations

from numbers import Integral, Real

_ARGS = ("top_k", "top_p", "temperature", "seed", "repetition_penalty", "initial_suppression_steps")


def is_sequence(v) -> bool:
    """a per-request argument: anything indexable with a length that is not a scalar (a 0-d tensor / array is a scalar)"""
    if v is None or isinstance(v, (Real, str, bytes)):
        return False
    if hasattr(v, "ndim"):          # numpy array, torch tensor
        return v.ndim > 0
    return hasattr(v, "__len__") and hasattr(v, "__getitem__")


def per_request(name: str, value, n: int):
    """`value` as a list of n Python scalars; a sequence of another length raises ValueError naming both lengths"""
    if not is_sequence(value):
        return [value] * n
    if len(value) != n:
        raise ValueError("%s has %d entries for %d requests" % (name, len(value), n))
    return [v.item() if hasattr(v, "item") else v for v in value]


def per_segment(name: str, value, n_texts: int, seg2orig):
    """TTS.infer_batched: one value per TEXT; the segments cut from a text inherit its value.  Scalars pass through."""
    if not is_sequence(value):
        return value
    vals = per_request(name, value, n_texts)
    return [vals[int(t)] for t in seg2orig]


def _number(name, i, v, kind, allow_none=False):
    if v is None and allow_none:
        return None
    if isinstance(v, bool) or not isinstance(v, kind):
        raise TypeError("%s[%d] is %r: expected %s" % (name, i, v, "an integer" if kind is Integral else "a number"))
    return v


def split_seed(seed: int):
    """a seed as the two 31-bit control words the kernels read (ctl[5], ctl[6])"""
    return int(seed) & 0x7fffffff, (int(seed) >> 31) & 0x7fffffff


class Entry(tuple):
    """one request's table entry: the six sampling words (sample_mode, top_k, temperature, top_p, seed_lo, seed_hi) as the tuple
    itself, and the two anti-loop words beside them as `rep_penalty` / `suppress_steps`; `words()` is all eight in the order
    of gsv_t2s_slot_sampling"""

    def __new__(cls, sampling, rep_penalty, suppress_steps):
        e = super().__new__(cls, sampling)
        e.rep_penalty, e.suppress_steps = float(rep_penalty), int(suppress_steps)
        return e

    def words(self):
        return tuple(self) + (self.rep_penalty, self.suppress_steps)


class RequestSampling:
    """one entry per request; `begin` fixes the call's seed, `entry(i)` is what goes into the slot that takes request i"""

    def __init__(self, n, top_k, top_p, temperature, seed, repetition_penalty=None, initial_suppression_steps=0):
        ks = per_request("top_k", top_k, n)
        ps = per_request("top_p", top_p, n)
        ts = per_request("temperature", temperature, n)
        ss = per_request("seed", seed, n)
        self.n = n
        self.top_k = [int(_number("top_k", i, 0 if v is None else v, Integral)) for i, v in enumerate(ks)]
        # top_p of None or outside (0, 1) is off, as in the kernel (csrc/t2s_decode.h::t2s_sample_wave)
        self.top_p = [1.0 if v is None or not 0.0 < float(v) < 1.0 else float(v)
                      for v in (_number("top_p", i, v, Real, True) for i, v in enumerate(ps))]
        self.temperature = [float(_number("temperature", i, v, Real)) for i, v in enumerate(ts)]
        self.seed = [None if v is None else int(v) for v in (_number("seed", i, v, Integral, True) for i, v in enumerate(ss))]
        # top_k == 1 is the argmax: greedy for that request, as _sampling_mode decides for a whole call
        self.mode = [0 if k == 1 else 2 for k in self.top_k]
        self.call_seed = 0
        # a NUMBER for repetition_penalty is the reference's batched behaviour: ignored (t2s_model.py:637-651); None: 1.0
        rs = per_request("repetition_penalty", repetition_penalty, n) if is_sequence(repetition_penalty) else [None] * n
        self.rep_penalty = [1.0 if v is None else float(v)
                            for v in (_number("repetition_penalty", i, v, Real, True) for i, v in enumerate(rs))]
        for i, v in enumerate(self.rep_penalty):
            if not (0.0 < v < float("inf")):
                raise ValueError("repetition_penalty[%d] is %r: expected a finite number > 0" % (i, v))
        ns = per_request("initial_suppression_steps", initial_suppression_steps, n)
        self.suppress_steps = [int(_number("initial_suppression_steps", i, v, Integral)) for i, v in enumerate(ns)]
        for i, v in enumerate(self.suppress_steps):
            if v < 0:
                raise ValueError("initial_suppression_steps[%d] is %r: expected an integer >= 0" % (i, v))

    @property
    def any_sampled(self) -> bool:
        return any(m == 2 for m in self.mode)

    @property
    def any_penalised(self) -> bool:
        """ctl[2] of the call: the steps keep `seen` up to date iff a request penalises"""
        return any(r != 1.0 for r in self.rep_penalty)

    def penalised(self, i: int) -> bool:
        return self.rep_penalty[i] != 1.0

    def begin(self, draw_seed):
        """(ctl[0], the call's seed): the seed is drawn ONCE, and only if a request samples -- what a scalar call does, so a
        generator in the same state seeds a mixed call and a scalar call alike"""
        if not self.any_sampled:
            return 0, 0
        self.call_seed = int(draw_seed())
        return 2, self.call_seed

    def stream(self, i: int) -> int:
        """tok_override of the slot that takes request i: noise stream + 1.  Keyed by the request index under the call's seed;
        stream 0 under the request's own seed (its samples then do not depend on its index in the call)"""
        return i + 1 if self.seed[i] is None else 1

    def entry(self, i: int):
        """(sample_mode, top_k, temperature, top_p, seed_lo, seed_hi) of request i, with .rep_penalty / .suppress_steps (`Entry`);
        a penalty of 1.0 goes into the table as 0: off, the slot's logits are not scaled at all"""
        lo, hi = split_seed(self.call_seed if self.seed[i] is None else self.seed[i])
        return Entry((self.mode[i], self.top_k[i], self.temperature[i], self.top_p[i], lo, hi),
                     self.rep_penalty[i] if self.penalised(i) else 0.0, self.suppress_steps[i])


def _nonzero_steps(v) -> bool:
    """anything but the scalar integer 0: a sequence, a count, or a value whose type the table's validation will name"""
    if hasattr(v, "item") and not is_sequence(v):
        v = v.item()            # a 0-d array / tensor is a scalar
    return not (isinstance(v, Integral) and not isinstance(v, bool) and v == 0)


def resolve(n: int, top_k, top_p, temperature, seed=None, repetition_penalty=None, initial_suppression_steps=0):
    """None when the call has one set of parameters (all scalars, no seed, a scalar repetition_penalty -- which the batched loop
    ignores -- and no suppression): no table is bound and the call is the scalar one"""
    if (seed is None and not any(is_sequence(v) for v in (top_k, top_p, temperature, repetition_penalty))
            and not _nonzero_steps(initial_suppression_steps)):
        return None
    return RequestSampling(n, top_k, top_p, temperature, seed, repetition_penalty, initial_suppression_steps)
