"""Text2SemanticDecoder: host-side mirror of the reference's GPT runtime, driving the HIP path.

Mirrors gsv_tts/GPT_SoVITS/GPT/t2s_model.py (class Text2SemanticDecoder): the same
constructor config, `initialize_runtime(dtype, device, gpt_cache)`, `infer`, `infer_batched`,
bucket bookkeeping and return conventions -- but every tensor op of the reference's hot loop
(embedding, 24 post-LN blocks, nested KV cache, logits, greedy sampling, next-token
embedding) is one C-ABI call into libgsv_hip.so.  torch is used for device memory, the
current stream, and (only when top_k != 1) the stochastic sampler.

Quirks of the reference that are reproduced on purpose:
  * the token sampled from the prefill logits is fed back but never returned;
  * `infer` output = every sample up to (excluding) the first EOS; the reference only *tests*
    EOS every `check_interval` steps, which changes when it stops, never what it returns;
  * `infer_batched`: no repetition penalty, no early suppression, capacity stop at
    kv_len + check_interval >= bucket.max_kv, completion-order output + semantic_orig_idx,
    finished slots refilled by a B=1 prefill, idle slots keep stepping.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List

import numpy as np
import torch

from . import _native as N
from . import slot_loop as SL
from . import slot_sampling as SS


class Bucket:
    """t2s_model.py:146-156 -- all buckets of a batch size alias one KV storage (nested cache)."""

    def __init__(self, batch_size, max_kv_cache, owner):
        self.batch_size = batch_size
        self.max_kv_cache = max_kv_cache
        self._o = owner

    @property
    def k_cache(self):
        return self._o["k"][:, :, :, : self.max_kv_cache]

    @property
    def v_cache(self):
        return self._o["v"][:, :, :, : self.max_kv_cache]

    @property
    def kv_cache_len(self):
        return self._o["kv_len"]


def _sine_pe(n_pos, dim):
    """embedding.py:52-69 (fp32 on host, like the reference)."""
    position = torch.arange(0, n_pos, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(n_pos, dim)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def state_spec(S, T, vocab, dim):
    """the small tensors of a decode state of S slots with T cache rows, beside its K/V cache: (key of the `rt` dict, shape, dtype)"""
    return [("kv_len", (S,), torch.int64), ("x_len", (S,), torch.int64), ("pre_tokens", (S, T + 1), torch.int64),
            ("seen", (S, vocab), torch.uint8), ("step", (S,), torch.int32), ("eos_at", (S,), torch.int32),
            ("logits", (S, vocab), torch.float32), ("hidden", (S, dim), torch.float32),
            ("tok_override", (S,), torch.int64), ("ctl", (8,), torch.int32), ("fctl", (4,), torch.float32)]


STATE_INIT = {"eos_at": -1, "fctl": 1.0}        # every other tensor starts at zero
STATE_FIELD = {"k": "k_cache", "v": "v_cache", **{key: key for key, _, _ in state_spec(1, 1, 1, 1)}}   # state key -> gsv_t2s_state field


def state_struct(batch, max_kv, ptrs):
    """the C ABI's gsv_t2s_state from {state key: device pointer}: every pointer goes to the field of its name"""
    by_field = {STATE_FIELD[key]: p for key, p in ptrs.items()}
    return N.T2SState(batch=batch, max_kv=max_kv, **{f: by_field[f] for f, _ in N.T2SState._fields_[2:]})


class Text2SemanticDecoder:
    def __init__(self, config):
        m = config["model"]
        self.config = config
        self.model_dim = m["hidden_dim"]
        self.embedding_dim = m["embedding_dim"]
        self.num_head = m["head"]
        self.num_layers = m["n_layer"]
        self.vocab_size = m["vocab_size"]
        self.phoneme_vocab_size = m["phoneme_vocab_size"]
        self.EOS = m["EOS"]
        self.suppressed_tokens = [280, 486, self.EOS]
        self.cuda_graph_buckets = {}
        self.refill_group = int(os.environ.get("GSV_REFILL_GROUP", "2"))   # staged refill: requests a prompt pass waits for ...
        self.refill_wait = int(os.environ.get("GSV_REFILL_WAIT", "1"))     # ... for at most this many windows
        self.refill_priority = int(os.environ.get("GSV_REFILL_PRIO", "0")) # stream priority of the prompt passes' side stream
        self.step_priority = int(os.environ.get("GSV_STEP_PRIO", "0"))     # ... and of the stream the slot loop's steps run on
        self.refill_ahead = int(os.environ.get("GSV_REFILL_AHEAD", "32"))  # async_refill: requests prefilled AHEAD of the slots that will run them, at most one per slot (0: the park / prompt pass / commit loop)
        # continuous batching, queue empty: the live requests move to a smaller bound state when they fit one of these sizes (0 / empty: off)
        self.tail_levels = [int(v) for v in os.environ.get("GSV_TAIL_LEVELS", "16,8,4").split(",") if v.strip() and int(v) > 0]
        self.use_graph = True
        self.fuse_token_step = os.environ.get("GSV_FUSE_TOKEN", "1") != "0"  # greedy steps: layer 0's attention kernel does the token kernel's work (<= 16 sequences)
        self._eos_pipe = None
        self._weights = None
        self._h = None
        self._rt = {}
        self._ws = self._ws_staged = None           # workspaces of the prompt passes: the current stream's, the refill stream's
        self._ahead, self._tails = None, {}         # the bound states of `_ahead_state` / `_tail_state`
        self._refill_stream = self._step_stream = None
        self._in_step_stream = False
        self._samp = None           # the RequestSampling of the infer_batched call that is running, or None (one set per call)
        self._samp_bound = []       # states whose table is bound for it
        self.sampling_binds = 0

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd):
        self._weights = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v)
                         for k, v in sd.items()}

    def eval(self):
        return self

    # ------------------------------------------------------------------ runtime
    @torch.inference_mode()
    def initialize_runtime(self, dtype, device, gpt_cache):
        """t2s_model.py:210-298 (`_build_runtime`).  Builds the native handle, uploads/repacks weights, allocates the
        nested KV cache (one root K and V; per batch size a [L,B,H,T,Dh] view; smaller buckets
        are prefix slices on T) and binds one state per batch size.  A load builds ONE runtime: the library's per-handle
        arena (64 KB sub-allocation alignment, gsv_abi.hip) and the one-block state below put every instance at the best
        step time (tools/placement_ab.py measures the spread between instances)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the MI355X hot path needs a GPU device (got %s); there is no CPU fallback" % device)
        if self._weights is None:
            raise RuntimeError("load_state_dict() first")
        L = N.lib()
        self.device, self.dtype = device, dtype
        # torch.float8_e4m3fn = GSV_FP8: e4m3 QKV / FFN weights in the batched decode step; K/V cache and the rest bf16
        kv_dtype = torch.bfloat16 if dtype == torch.float8_e4m3fn else dtype
        cfg = N.T2SConfig(self.num_layers, self.model_dim, self.num_head, self.vocab_size, self.EOS, 4000,
                          self.phoneme_vocab_size, N.dtype_code(dtype))
        h = ctypes.c_void_p()
        N.check(L.gsv_t2s_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        stream = N.current_stream_ptr(device)
        pe = _sine_pe(4000, self.embedding_dim)
        for name, t in self._weights.items():
            if name.endswith("position.alpha"):
                scaled = (t.float().reshape(1) * pe).contiguous()
                nm = name.replace("alpha", "pe_scaled")
                d = scaled.to(device)
                N.check(L.gsv_t2s_load_tensor(h, nm.encode(), d.data_ptr(), d.numel(), stream))
                continue
            d = t.detach().to(device=device, dtype=torch.float32).contiguous()
            N.check(L.gsv_t2s_load_tensor(h, name.encode(), d.data_ptr(), d.numel(), stream))
        N.check(L.gsv_t2s_finalize(h, stream))
        self.batched_min = int(L.gsv_t2s_batched_min(h))   # batch size from which the step is the batched MFMA chain
        self.ffn_slices = lambda bsz: int(N.lib().gsv_t2s_ffn_slices(self._h, int(bsz)))   # FFN slices per sequence below it (part of the bf16 arithmetic)

        for batch_size, max_kv in gpt_cache:
            self.cuda_graph_buckets.setdefault(batch_size, [])
            if max_kv not in self.cuda_graph_buckets[batch_size]:
                self.cuda_graph_buckets[batch_size].append(max_kv)
        max_elem = max(b * max(ts) for b, ts in self.cuda_graph_buckets.items())
        numel = self.num_layers * max_elem * self.model_dim
        self.k_cache_root = torch.zeros(numel, dtype=kv_dtype, device=device)
        self.v_cache_root = torch.zeros(numel, dtype=kv_dtype, device=device)
        dh = self.model_dim // self.num_head
        for b in sorted(self.cuda_graph_buckets):
            ts = sorted(self.cuda_graph_buckets[b])
            T = ts[-1]
            n = self.num_layers * b * T * self.model_dim
            rt = self._new_state(b, T, self.k_cache_root[:n].view(self.num_layers, b, self.num_head, T, dh),
                                 self.v_cache_root[:n].view(self.num_layers, b, self.num_head, T, dh),
                                 one_block=os.environ.get("GSV_STATE_SEPARATE") != "1")      # =1: tools/placement_ab.py, the pre-round-3 layout
            if b == 1:   # single-sequence loop: the EOS flag is read from a host-mapped mirror, not copied per window
                rt["eos_host"] = torch.full((b,), -1, dtype=torch.int32).pin_memory()
                N.check(L.gsv_t2s_set_eos_mirror(h, b, rt["eos_host"].data_ptr()))
            self._rt[b] = rt
            self.cuda_graph_buckets[b] = [Bucket(b, t, rt) for t in ts]
        torch.cuda.synchronize(device)

    def _new_state(self, S, T, k, v, one_block=False, **own):
        """allocates the small tensors of a decode state of S slots with T cache rows over the K/V tensors given, binds it to the
        handle and returns its `rt` dict (`own`: further entries).  one_block: the tensors live in ONE block, each on a 64 KB
        boundary, so where they land relative to each other never depends on what torch's caching allocator has free (the
        placement lottery of DESIGN 7); otherwise they are separate allocations."""
        dev = self.device
        spec = state_spec(S, T, self.vocab_size, self.model_dim)
        rt = {"batch": S, "T": T, "k": k, "v": v, **own}
        if one_block:
            al = 65536
            size = [-(-(math.prod(shp) * dt.itemsize) // al) * al for _, shp, dt in spec]
            rt["_state_block"] = block = torch.zeros(sum(size) + al, dtype=torch.uint8, device=dev)
            pos = (-block.data_ptr()) % al
            for (key, shp, dt), nb in zip(spec, size):
                rt[key] = block[pos: pos + math.prod(shp) * dt.itemsize].view(dt).view(*shp)
                pos += nb
        else:
            for key, shp, dt in spec:
                rt[key] = torch.zeros(*shp, dtype=dt, device=dev)
        for key, value in STATE_INIT.items():
            rt[key].fill_(value)
        st = state_struct(S, T, {key: rt[key].data_ptr() for key in STATE_FIELD})
        torch.cuda.synchronize(dev)       # binding may re-allocate the handle's scratch: nothing may be running on it
        N.check(N.lib().gsv_t2s_bind_state(self._h, ctypes.byref(st)))
        return rt

    def __del__(self):
        try:
            if self._h is not None:
                N.lib().gsv_t2s_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ pieces (C-ABI seams)
    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def embed_prompt(self, xs: List[torch.Tensor], ys: List[torch.Tensor], berts: List[torch.Tensor]):
        """process_single_data / process_batch_data (t2s_model.py:300-383): packed rows
        [x_b | y_b | 0-pad] -> (xy float32 [n, Lmax, D], x_lens, y_lens)."""
        n = len(xs)
        dev = self.device
        xln, yln = [int(t.shape[0]) for t in xs], [int(t.shape[0]) for t in ys]
        lens = torch.tensor([xln, yln], dtype=torch.int64)
        x_lens, y_lens = lens[0], lens[1]
        lx, ly = max(xln), max(yln)
        lmax = max(a + b for a, b in zip(xln, yln))
        if n == 1:
            # one request (TTFT): nothing to pad -- the inputs are the rows (no zero-fill and three slice copies in front of the first launch)
            xi = xs[0].to(device=dev, dtype=torch.int64).reshape(1, lx).contiguous()
            yi = ys[0].to(device=dev, dtype=torch.int64).reshape(1, ly).contiguous()
            bt = berts[0].to(device=dev, dtype=torch.float32).reshape(1, lx, 1024).contiguous()
        elif n < 4:
            xi = torch.zeros(n, lx, dtype=torch.int64, device=dev)
            yi = torch.zeros(n, ly, dtype=torch.int64, device=dev)
            bt = torch.zeros(n, lx, 1024, dtype=torch.float32, device=dev)
            for i in range(n):
                xi[i, : xln[i]] = xs[i].to(dev)
                yi[i, : yln[i]] = ys[i].to(dev)
                bt[i, : xln[i]] = berts[i].to(device=dev, dtype=torch.float32)
        else:
            # from four requests on: the padded batches by ONE concatenation + ONE indexed store per tensor (the row positions are built on the host and cross in
            # one copy): a slice copy per request and tensor was 3 n small launches -- 0.7 ms of host time in front of a 32-prompt pass
            pos_x = np.concatenate([i * lx + np.arange(k) for i, k in enumerate(xln)])
            pos_y = np.concatenate([i * ly + np.arange(k) for i, k in enumerate(yln)])
            pos = torch.from_numpy(np.concatenate([pos_x, pos_y])).to(dev)
            px, py = pos[: len(pos_x)], pos[len(pos_x):]
            xi = torch.zeros(n * lx, dtype=torch.int64, device=dev)
            yi = torch.zeros(n * ly, dtype=torch.int64, device=dev)
            bt = torch.zeros(n * lx, 1024, dtype=torch.float32, device=dev)
            xi[px] = torch.cat([t.to(dev).reshape(-1) for t in xs]).to(torch.int64)
            yi[py] = torch.cat([t.to(dev).reshape(-1) for t in ys]).to(torch.int64)
            bt[px] = torch.cat([t.to(device=dev, dtype=torch.float32).reshape(-1, 1024) for t in berts])
        lens_d = lens.to(dev)           # one host-to-device copy for both length vectors
        xl, yl = lens_d[0], lens_d[1]
        xy = torch.empty(n, lmax, self.model_dim, dtype=torch.float32, device=dev)
        scratch = torch.empty(n * lx, self.model_dim, dtype=torch.float32, device=dev)
        N.check(N.lib().gsv_t2s_embed_prompt(self._h, n, lx, ly, lmax, xi.data_ptr(), yi.data_ptr(), bt.data_ptr(),
                                              xl.data_ptr(), yl.data_ptr(), xy.data_ptr(), scratch.data_ptr(),
                                              N.current_stream_ptr(dev)))
        return xy, xl, yl, x_lens, y_lens

    def prefill(self, batch, slot0, xy, xl, yl):
        """T2STransformer.process_prompt + first logits (t2s_model.py:114-127, 414-417, 608-613)."""
        n, lmax, _ = xy.shape
        L = N.lib()
        need = L.gsv_t2s_prefill_workspace(self._h, n, lmax)
        ws = self._workspace(need)
        N.check(L.gsv_t2s_prefill(self._h, batch, slot0, n, lmax, xy.data_ptr(), xl.data_ptr(), yl.data_ptr(),
                                  ws.data_ptr(), ws.numel(), N.current_stream_ptr(self.device)))

    def prefill_slots(self, batch, slots, xy, xl, yl):
        """the same for rows that go to scattered slots: one packed prefill refills every slot that finished in a window"""
        n, lmax, _ = xy.shape
        L = N.lib()
        sl = torch.tensor(list(slots), dtype=torch.int32, device=self.device)
        ws = self._workspace(L.gsv_t2s_prefill_workspace(self._h, n, lmax))
        N.check(L.gsv_t2s_prefill_slots(self._h, batch, sl.data_ptr(), n, lmax, xy.data_ptr(), xl.data_ptr(), yl.data_ptr(),
                                        ws.data_ptr(), ws.numel(), N.current_stream_ptr(self.device)))

    def prefill_slots_staged(self, batch, sl, xy, xl, yl, stream_ptr):
        """the packed refill on ANOTHER stream than the decode step's: K/V rows into the live cache, every per-slot state
        the step also writes into the library's staging (gsv_t2s_prefill_slots_staged); `sl` int32 device slot list"""
        n, lmax, _ = xy.shape
        L = N.lib()
        need = L.gsv_t2s_prefill_workspace(self._h, n, lmax)
        with torch.cuda.stream(torch.cuda.ExternalStream(stream_ptr, device=self.device)):
            # its own workspace, allocated on ITS stream: the prompt pass of the main stream (self._ws) may be running
            if self._ws_staged is None or self._ws_staged.numel() < need:
                self._ws_staged = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws = self._ws_staged
        N.check(L.gsv_t2s_prefill_slots_staged(self._h, batch, sl.data_ptr(), n, lmax, xy.data_ptr(), xl.data_ptr(), yl.data_ptr(),
                                               ws.data_ptr(), ws.numel(), stream_ptr))

    def _ahead_state(self, n_slots, max_kv):
        """a second bound state that is never stepped: the prompt passes of the NEXT requests run into its K/V cache and its
        staging (gsv_t2s_prefill_slots_staged) while the steps of the live state run; gsv_t2s_adopt_slots moves a finished pass
        into the slot that takes the request.  Its batch size must differ from every stepped family's (states are keyed by it)
        and its cache is its own memory (the families' caches alias one root)."""
        key = (n_slots, max_kv)
        sh = self._ahead
        if sh is not None and sh["key"] == key:
            return sh
        if sh is not None:                    # a state of another shape: the handle must not keep pointers into tensors about to go
            torch.cuda.synchronize(self.device)
            N.check(N.lib().gsv_t2s_unbind_state(self._h, int(sh["batch"])))
            self._ahead = None
        S = n_slots
        while S in self._rt:
            S += 1
        self._ahead = self._new_state(S, max_kv, *self._own_kv(S, max_kv), key=key, slots=n_slots)
        return self._ahead

    def _own_kv(self, S, max_kv):
        """K and V cache of a state that does not alias the families' root"""
        kv_dtype = torch.bfloat16 if self.dtype == torch.float8_e4m3fn else self.dtype
        shape = (self.num_layers, S, self.num_head, max_kv, self.model_dim // self.num_head)
        return torch.zeros(shape, dtype=kv_dtype, device=self.device), torch.zeros(shape, dtype=kv_dtype, device=self.device)

    def adopt_slots(self, batch, slots, src_batch, src_slots, tok_override=None):
        """gsv_t2s_adopt_slots on the current stream; the slot lists are host lists (they ride in the kernel arguments)"""
        n = len(slots)
        d = (ctypes.c_int32 * n)(*[int(v) for v in slots])
        sv = (ctypes.c_int32 * n)(*[int(v) for v in src_slots])
        ov = None if tok_override is None else (ctypes.c_int64 * n)(*[int(v) for v in tok_override])
        N.check(N.lib().gsv_t2s_adopt_slots(self._h, batch, d, src_batch, sv, ov, n, N.current_stream_ptr(self.device)))

    def move_slots(self, batch_dst, slots_dst, batch_src, slots_src):
        """gsv_t2s_move_slots on the current stream: live slots of one stepped state continue in slots of another"""
        n = len(slots_dst)
        d = (ctypes.c_int32 * n)(*[int(v) for v in slots_dst])
        sv = (ctypes.c_int32 * n)(*[int(v) for v in slots_src])
        N.check(N.lib().gsv_t2s_move_slots(self._h, batch_dst, d, batch_src, sv, n, N.current_stream_ptr(self.device)))

    def _tail_state(self, n_slots, max_kv):
        """a bound state of (about) `n_slots` slots with a K/V cache of its own that IS stepped: where the last live requests of a
        continuous-batching run continue once the queue is empty (slot_loop.AheadLoop, gsv_t2s_move_slots).  Its batch size
        differs from every other bound state's (states are keyed by it): `n_slots`, or the next smaller free one."""
        key = (n_slots, max_kv)
        if key in self._tails:
            return self._tails[key]
        S = n_slots
        taken = set(self._rt) | ({self._ahead["batch"]} if self._ahead else set())
        while S in taken and S > 1:
            S -= 1
        if S in taken:
            return None
        rt = self._new_state(S, max_kv, *self._own_kv(S, max_kv), key=key, tail=True)
        self._rt[S] = rt                  # stepped like a family's state (`_decode` / `_flush` look it up); not a KV bucket family
        self._tails[key] = rt
        return rt

    def commit_slots(self, batch, sl):
        N.check(N.lib().gsv_t2s_commit_slots(self._h, batch, sl.data_ptr(), int(sl.numel()), N.current_stream_ptr(self.device)))

    def decode_hidden(self, batch, x):
        """T2STransformer.decode_next_token for an explicit x [B, D] (t2s_model.py:129-143)."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        N.check(N.lib().gsv_t2s_decode_hidden(self._h, batch, x.data_ptr(), N.current_stream_ptr(self.device)))
        return self._rt[batch]["hidden"]

    def _decode(self, batch, n):
        # bit 0: hipGraph replay; bit 1 (GSV_STEP_FUSED_TOKEN): the control block last written says "no device sampling"
        flags = (1 if self.use_graph else 0) | (2 if self.fuse_token_step and self._rt[batch].get("fused_ok", False) else 0)
        N.check(N.lib().gsv_t2s_decode(self._h, batch, n, flags, N.current_stream_ptr(self.device)))

    def _flush(self, batch):
        N.check(N.lib().gsv_t2s_flush(self._h, batch, N.current_stream_ptr(self.device)))

    def _bind_sampling(self, rt):
        """the per-slot sampling table of a bound state (gsv_t2s_set_slot_sampling): [B] entries of 8 words, all greedy at first"""
        if rt.get("samp") is None:
            rt["samp"] = torch.zeros(rt["batch"], 8, dtype=torch.int32, device=self.device)
        else:
            rt["samp"].zero_()
        torch.cuda.synchronize(self.device)     # the state's captured steps go: none of them may be running
        N.check(N.lib().gsv_t2s_set_slot_sampling(self._h, rt["batch"], rt["samp"].data_ptr()))
        self._samp_bound.append(rt)
        self.sampling_binds += 1

    def _unbind_sampling(self):
        torch.cuda.synchronize(self.device)
        for rt in self._samp_bound:
            N.check(N.lib().gsv_t2s_set_slot_sampling(self._h, rt["batch"], None))
        self._samp_bound = []

    def _put_sampling(self, batch, slots, requests):
        """the slots take these requests: their table entries, on the current stream (a scalar call has no table: nothing)"""
        samp = self._samp
        if samp is None or not len(slots):
            return
        n = len(slots)
        sl = (ctypes.c_int32 * n)(*[int(v) for v in slots])
        en = (N.SlotSampling * n)(*[N.SlotSampling(*samp.entry(int(c)).words()) for c in requests])
        N.check(N.lib().gsv_t2s_put_slot_sampling(self._h, batch, sl, en, n, N.current_stream_ptr(self.device)))

    def _seed_tokens(self, requests, y):
        """the prompt tokens of the penalising requests among `requests`, packed on the device by the current stream, and the
        row offsets (gsv_t2s_seed_seen); None when the call keeps no penalty sets"""
        samp = self._samp
        if samp is None or not samp.any_penalised or not len(requests):
            return None
        off, rows = [0], []
        for c in requests:          # a request that does not penalise gets an empty row: its slot's set is only cleared
            if samp.penalised(int(c)):
                rows.append(y[int(c)].reshape(-1))
            off.append(off[-1] + (int(rows[-1].numel()) if samp.penalised(int(c)) else 0))
        tok = torch.cat(rows).to(device=self.device, dtype=torch.int64) if rows else None
        return tok, off

    def _put_request(self, batch, slots, requests, seed):
        """the slots of state `batch` take these requests: their penalty sets (cleared; the prompt tokens of a request that
        penalises) and their table entries, on the current stream -- BEFORE the prompt pass, whose logits obey both"""
        if self._samp is None or not len(slots):
            return
        slots = [int(v) for v in slots]
        if seed is not None:
            tok, off = seed
            for r0 in range(0, len(slots), 64):         # the slot list rides in the kernel arguments: 64 rows per launch
                n = min(64, len(slots) - r0)
                sl = (ctypes.c_int32 * n)(*slots[r0: r0 + n])
                of = (ctypes.c_int32 * (n + 1))(*off[r0: r0 + n + 1])
                N.check(N.lib().gsv_t2s_seed_seen(self._h, batch, sl, None if tok is None else tok.data_ptr(), of, n,
                                                  N.current_stream_ptr(self.device)))
        self._put_sampling(batch, slots, requests)

    def _stream_id(self, c):
        """tok_override of a slot that takes request c under device sampling: its noise stream + 1"""
        return c + 1 if self._samp is None else self._samp.stream(c)

    def _set_ctl(self, rt, mode, suppress_steps, rep_enabled, rep, top_k=0, temperature=1.0, seed=0, top_p=1.0,
                 suppress_first=False):
        """mode 0 = greedy on device, 2 = device sampling (1, host-sampled tokens through tok_override, is the C ABI's and unused here); suppress_first: the
        prefill's sample never takes 280 / 486 / EOS whatever suppress_steps is (infer / infer_stream, t2s_model.py:415-416)"""
        lo, hi = int(seed) & 0x7fffffff, (int(seed) >> 31) & 0x7fffffff
        rt["fused_ok"] = int(mode) != 2
        rt["ctl"].copy_(torch.tensor([int(mode), int(suppress_steps), int(rep_enabled), 0, int(top_k or 0), lo, hi,
                                      int(bool(suppress_first))], dtype=torch.int32))
        rt["fctl"].copy_(torch.tensor([float(rep), float(temperature), float(1.0 if top_p is None else top_p), 0.0],
                                      dtype=torch.float32))

    def _sampling_mode(self, top_k, top_p, generator):
        """(mode, seed): greedy is the device argmax; every other setting (temperature, top-k up to the whole vocabulary, top-p)
        is sampled on device inside the captured step (csrc/t2s_decode.h::t2s_sample_wave).  There is no host sampling path."""
        if top_k == 1:
            return 0, 0
        if generator is not None:   # the caller's generator (CPU or device) seeds the device noise stream
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=generator.device).item())
        else:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return 2, seed

    # ------------------------------------------------------------------ drivers
    @torch.inference_mode()
    def _begin_single(self, x, y, bert_feature, top_k, top_p, temperature, repetition_penalty, initial_suppression_steps, generator):
        """what `infer` and `infer_stream` do up to the first decode step (t2s_model.py:385-417): control words, the penalty set
        seeded with the prompt's tokens, the prompt pass.  Returns (rt, prompt length, decode iterations the largest bucket leaves)."""
        rt = self._rt[1]
        max_kv = self.cuda_graph_buckets[1][-1].max_kv_cache
        Lp = int(x.shape[1]) + int(y.shape[1])
        if Lp > max_kv:
            raise ValueError("prompt of %d positions exceeds the largest KV bucket (%d)" % (Lp, max_kv))
        n_iter = max_kv - Lp
        if n_iter < 1:
            raise RuntimeError("no decode iterations: prompt fills the largest bucket")
        mode, seed = self._sampling_mode(top_k, top_p, generator)
        rep_on = repetition_penalty != 1.0
        self._set_ctl(rt, mode, initial_suppression_steps, rep_on, repetition_penalty, top_k, temperature, seed, top_p,
                      suppress_first=True)
        rt["seen"].zero_()
        if mode == 2:
            rt["tok_override"].zero_()      # noise stream = slot 0 (a batched run may have left a request's stream id here)
        if rep_on:
            rt["seen"][0, y[0].to(self.device)] = 1
        xy, xl, yl, _, _ = self.embed_prompt([x[0]], [y[0]], [bert_feature[0]])
        self.prefill(1, 0, xy, xl, yl)
        return rt, Lp, n_iter

    @torch.inference_mode()
    def infer(self, x, y, bert_feature, top_k: int = 15, top_p: float = 1.0, temperature: float = 1.0,
              repetition_penalty: float = 1.35, initial_suppression_steps: int = 10, check_interval: int = 5,
              generator=None, max_new_tokens: int = None):
        """t2s_model.py:385-464.  x int64[1,Lx], y int64[1,Ly], bert [1,Lx,1024] -> int64[1,1,N].
        `max_new_tokens` (not in the reference, whose only length limit is the largest bucket) caps the loop."""
        rt, Lp, n_iter = self._begin_single(x, y, bert_feature, top_k, top_p, temperature, repetition_penalty,
                                            initial_suppression_steps, generator)
        if max_new_tokens is not None:
            n_iter = max(1, min(n_iter, int(max_new_tokens)))
        done = 0
        eos_at = -1
        # The reference tests for EOS on the host every `check_interval` steps (t2s_model.py:451-453).  Same
        # cadence here, but the test of chunk i is read AFTER chunk i+1 has been enqueued (async copy of the
        # flag into pinned memory + an event), so the GPU never idles on the host round trip.  A chunk that
        # runs past the EOS costs nothing observable: tokens are cut at the first EOS anyway (:459-462).
        # The flag itself is not copied either: the kernels publish eos_at to a host-mapped mirror
        # (gsv_t2s_set_eos_mirror), the host reads its own memory once the window's event has fired.  (A device-to-host
        # copy between the windows cost 0 - 15 us per token, bimodal from run to run.)  The pending sample of a window
        # becomes a token at the next step, so an EOS is seen at most one window late; only the last window is flushed.
        if self._eos_pipe is None:
            self._eos_pipe = [torch.cuda.Event() for _ in range(2)]
        mirror = rt["eos_host"]
        pending = None
        pending_done = 0
        k = 0
        while done < n_iter:
            n = min(check_interval, n_iter - done)
            self._decode(1, n)
            done += n
            if done >= n_iter:
                self._flush(1)
            ev = self._eos_pipe[k]
            k ^= 1
            ev.record()
            if pending is not None:
                pending.synchronize()
                # the mirror may already hold an EOS of the window enqueued AFTER the one just waited for (the GPU runs
                # ahead of this read): only an EOS recorded by a step of the waited-for windows counts, so the number of
                # windows a run executes -- and with it the state it leaves behind -- does not depend on timing
                e = int(mirror[0])
                if 0 <= e < pending_done:
                    break
            pending = ev
            pending_done = done
        torch.cuda.current_stream(self.device).synchronize()
        eos_at = int(mirror[0])
        # sample s_i sits at kv position Lp + i; s_0 (the prefill sample) is never returned
        n_valid = done if eos_at < 0 else min(done, eos_at - 1)
        out = rt["pre_tokens"][0, Lp + 1: Lp + 1 + n_valid].clone()
        return out.unsqueeze(0).unsqueeze(0)

    def infer_stream(self, x, y, bert_feature, top_k: int = 15, top_p: float = 1.0, temperature: float = 1.0,
                     repetition_penalty: float = 1.35, initial_suppression_steps: int = 10, stream_chunk: int = 25,
                     boost_first_chunk: bool = True, debug: bool = True, generator=None):
        """t2s_model.py:466-553: generator of (cumulative tokens int64[1,1,n], is_final).  Same quirks as the
        reference: chunks are cumulative and lag one chunk behind (the first is sent at once when
        boost_first_chunk), EOS is never part of a chunk, and the final chunk after an EOS is the last `idx`
        entries of y ++ samples, i.e. it starts with the first sample s0 that infer() drops.  The decode steps
        run on device in groups of <= 5 (greedy / device sampling); a group that runs past the EOS is harmless."""
        rt, Lp, n_iter = self._begin_single(x, y, bert_feature, top_k, top_p, temperature, repetition_penalty,
                                            initial_suppression_steps, generator)
        done, first, pre_chunk = 0, True, None
        while done < n_iter:
            with torch.inference_mode():
                to_boundary = stream_chunk - done % stream_chunk
                n = min(5, to_boundary, n_iter - done)
                self._decode(1, n)
                done += n
                self._flush(1)      # materialises sample s_done; idempotent
                eos_at = int(rt["eos_at"][0].item())
                if eos_at >= 0:     # s_eos_at is the EOS: the reference breaks at idx = eos_at
                    final = rt["pre_tokens"][0, Lp: Lp + eos_at].clone()
                    break
                chunk = None
                if done % stream_chunk == 0:
                    if pre_chunk is not None:
                        chunk = pre_chunk
                    pre_chunk = rt["pre_tokens"][0, Lp + 1: Lp + 1 + done].clone()
            if done % stream_chunk == 0:
                if chunk is not None:
                    yield chunk[None, None], False
                if boost_first_chunk and first:
                    first = False
                    yield pre_chunk[None, None], False
                    pre_chunk = None
        else:
            with torch.inference_mode():
                final = rt["pre_tokens"][0, Lp + 1: Lp + 1 + n_iter].clone()
        yield final[None, None], True

    @torch.inference_mode()
    def infer_batched(self, x: List[torch.Tensor], y: List[torch.Tensor], bert_feature: List[torch.Tensor],
                      top_k: int = 15, top_p: float = 1.0, temperature: float = 1.0,
                      repetition_penalty: float = 1.35, check_interval: int = 5, generator=None,
                      source=None, slots: int = None, on_finish=None, max_new_tokens=None, async_refill: bool = False,
                      seed=None, initial_suppression_steps=0):
        """t2s_model.py:555-734: continuous batching over the slots of one batch-size family.

        `top_k`, `top_p`, `temperature` and `seed` are scalars -- one set for the call, as in the reference -- or sequences
        indexed like `x` (with `source`: by the GLOBAL request index): request i is then decoded with its own values, greedy
        (top_k 1) and sampled requests side by side in the slots of one captured step (the per-slot sampling table,
        gsv_t2s_set_slot_sampling).  With `seed` None the noise is keyed as in a scalar call: one seed drawn from `generator`,
        stream = request index.  `seed[i]` given: request i draws from (seed[i], stream 0), so its tokens depend on its own
        inputs, parameters and seed only.  All scalars and no seed: no table is bound, the call is the scalar one.

        `repetition_penalty` as a NUMBER is ignored, as in the reference's batched loop, which samples without the penalty
        (t2s_model.py:637-651); the default stays for signature compatibility.  As a SEQUENCE indexed like the requests it is
        applied: request i is penalised over its prompt's and its generated tokens as `infer` penalises (1.0: not at all) --
        `repetition_penalty=[1.35] * len(x)` is `infer`'s rule for every request.  `initial_suppression_steps` (an int for the
        call or a sequence per request; not in the reference's batched loop) is `infer`'s start rule: 0 suppresses nothing,
        n > 0 bars 280 / 486 / EOS from the prefill's sample and from every sample while idx < n (t2s_model.py:415-416, 444-447).
        Either one makes the call a table call.  With both, and top_k=1 in fp32, a request returns the tokens `infer` returns
        for it, whichever slot it lands in and however it is refilled.

        `source` (engine.RequestSource) replaces "the next request is x[cur]" (:696-700) by "the next request is
        whatever the shared queue hands this rank": x / y / bert_feature are then the GLOBAL lists, the returned
        indices are global, and `slots` names the batch-size family to run (default: as the reference, the
        smallest family that holds len(x)).  `on_finish(index, tokens)` is called as each request completes (the
        engine starts that utterance's vocoder work on a side stream while the slots keep decoding).
        `max_new_tokens` (a list indexed like x; not in the reference, which stops at EOS or a full cache only) ends
        request i once it has produced that many tokens -- tested at the same 5-step cadence as EOS, cut exactly.
        `async_refill` (not in the reference, whose slots all wait while a refill's prompt pass runs, :696-722) runs an
        asynchronous slot loop instead (slot_loop.AheadLoop; with GSV_REFILL_AHEAD=0 slot_loop.StagedLoop): same requests,
        same tokens per request, no stall."""
        samp = SS.resolve(len(x), top_k, top_p, temperature, seed, repetition_penalty, initial_suppression_steps)
        if samp is None:
            return self._infer_batched_call(x, y, bert_feature, top_k, top_p, temperature, repetition_penalty, check_interval,
                                            generator, source, slots, on_finish, max_new_tokens, async_refill)
        self._samp = samp
        try:
            return self._infer_batched_call(x, y, bert_feature, 0, 1.0, 1.0, repetition_penalty, check_interval,
                                            generator, source, slots, on_finish, max_new_tokens, async_refill)
        finally:
            self._samp = None
            self._unbind_sampling()

    def _infer_batched_call(self, x, y, bert_feature, top_k, top_p, temperature, repetition_penalty, check_interval, generator,
                            source, slots, on_finish, max_new_tokens, async_refill):
        """infer_batched behind the resolution of its sampling arguments (`self._samp`: per request, or None: the scalars here)"""
        if async_refill and self.step_priority != 0 and not self._in_step_stream:
            # the slot loop on a stream of its own priority (the steps are a chain of short dependent launches: whatever a
            # launch waits for behind a prompt pass's blocks is on the critical path, the prompt pass itself is not)
            if self._step_stream is None:
                self._step_stream = torch.cuda.Stream(device=self.device, priority=self.step_priority)
            cur = torch.cuda.current_stream(self.device)
            self._step_stream.wait_stream(cur)
            self._in_step_stream = True
            try:
                with torch.cuda.stream(self._step_stream):
                    out = self._infer_batched_call(x, y, bert_feature, top_k, top_p, temperature, repetition_penalty, check_interval,
                                             generator, source, slots, on_finish, max_new_tokens, async_refill)
            finally:
                self._in_step_stream = False
                cur.wait_stream(self._step_stream)
            return out
        begun = self._begin_batched(x, y, bert_feature, top_k, top_p, temperature, generator, source, slots, async_refill)
        if begun is None:
            return [], torch.zeros(0, dtype=torch.int64, device=self.device)
        batch_size, first, nxt, exhausted, bucket_i, mode, _ = begun
        if not async_refill:
            return SL.reference_order(self, x, y, bert_feature, batch_size, first, nxt, exhausted, bucket_i, check_interval,
                                      on_finish, max_new_tokens, mode)
        try:
            pred, orig = self._async_loop(x, y, bert_feature, begun, check_interval, on_finish, max_new_tokens).run()
            return pred, torch.tensor(orig, device=self.device)
        finally:    # also on an exception (a prompt that does not fit): no prompt pass may outlive the call
            if self._refill_stream is not None:
                self._refill_stream.synchronize()

    def _async_loop(self, x, y, bert_feature, begun, check_interval, on_finish, max_new_tokens):
        batch_size, first, nxt, exhausted, _, mode, first_len = begun
        loop = SL.AheadLoop if self.refill_ahead > 0 else SL.StagedLoop
        return loop(self, x, y, bert_feature, batch_size, first, nxt, exhausted, first_len, check_interval, on_finish,
                    max_new_tokens, mode == 2)

    def _begin_batched(self, x, y, bert_feature, top_k, top_p, temperature, generator, source, slots, async_refill):
        """a batched call up to its first window: the slot family, the control words, the first requests' prompt pass -> None
        (no request) or (slots, first requests, next-request function, queue exhausted, bucket the prompt pass chose, sampling
        mode, the first requests' prompt lengths)"""
        B = len(x)
        sizes = sorted(self.cuda_graph_buckets)
        if slots is not None:
            if slots not in self.cuda_graph_buckets:
                raise ValueError("no KV bucket family of %d slots (have %s)" % (slots, sizes))
            batch_size = slots
        else:
            batch_size = sizes[-1]
            for s in sizes:
                if s >= B:
                    batch_size = s
                    break
        if source is None:
            _it = iter(range(B))
            nxt = lambda: next(_it, None)
        else:
            nxt = source.next
        first = []
        while len(first) < batch_size:
            c = nxt()
            if c is None:
                break
            first.append(c)
        exhausted = len(first) < batch_size
        rt = self._rt[batch_size]
        buckets = self.cuda_graph_buckets[batch_size]
        caps = [b.max_kv_cache for b in buckets]
        actual = len(first)
        dev = self.device
        if actual == 0:
            return None
        if self._samp is None:
            mode, seed = self._sampling_mode(top_k, top_p, generator)
        else:       # ctl[0] = 2 if any request samples (it gates the fused token step); the call's seed is drawn as a scalar call draws it
            mode, seed = self._samp.begin(lambda: self._sampling_mode(0, None, generator)[1])
        if async_refill and self.refill_ahead > 0:
            # bound BEFORE the first prompt pass: binding a state may re-allocate the handle's per-slot scratch (pending tokens)
            self._ahead_state(max(1, min(self.refill_ahead, batch_size)), max(caps))
        # a scalar repetition_penalty is ignored, as in the reference's batched loop (t2s_model.py:637-651).  Per request, penalty
        # and suppression are table words; ctl[2] makes the steps keep `seen` up to date when any request penalises
        self._set_ctl(rt, mode, 0, self._samp is not None and self._samp.any_penalised, 1.0, top_k, temperature, seed, top_p)
        if self._samp is not None:
            self._bind_sampling(rt)
        rt["kv_len"].zero_()
        rt["x_len"].zero_()
        xy, xl, yl, x_lens_h, y_lens_h = self.embed_prompt([x[c] for c in first], [y[c] for c in first],
                                                           [bert_feature[c] for c in first])
        lmax = xy.shape[1]
        bucket_i = len(caps) - 1
        for i, c in enumerate(caps):
            if c > lmax:
                bucket_i = i
                break
        if lmax > caps[-1]:
            raise ValueError("prompt longer than the largest KV bucket")
        self._put_request(batch_size, range(actual), first, self._seed_tokens(first, y))
        self.prefill(batch_size, 0, xy, xl, yl)
        if mode == 2:       # device sampling: the noise stream of a slot is its REQUEST (placement-invariant samples)
            rt["tok_override"].zero_()
            rt["tok_override"][:actual] = torch.tensor([self._stream_id(c) for c in first], dtype=torch.int64, device=dev)
        return batch_size, first, nxt, exhausted, bucket_i, mode, [int(a) + int(b) for a, b in zip(x_lens_h, y_lens_h)]

    def infer_stream_batched(self, x: List[torch.Tensor], y: List[torch.Tensor], bert_feature: List[torch.Tensor],
                             stream_chunk: int = 25, boost_first_chunk=True, slots: int = None, top_k=15, top_p=1.0,
                             temperature=1.0, repetition_penalty=1.35, initial_suppression_steps=10, seed=None,
                             max_new_tokens=None, check_interval: int = 5, generator=None, ticks: bool = False):
        """`infer_stream` for many requests at once, on the slots of `infer_batched`'s asynchronous loop: a generator of
        (request index, cumulative tokens int64 [1,1,n] on the device, is_final).  Requests interleave as their chunks become
        known; there may be more requests than slots.

        Per request the sequence is `infer_stream`'s for that request alone, given that it ends with an EOS: cumulative chunks
        that lag one chunk behind, the first sent at once under `boost_first_chunk` (a bool, or one per request), the EOS in no
        chunk, and a final chunk that starts with sample 0.  With top_k=1 in fp32 the tokens are equal too, whichever slot
        decodes the request.  A request that ends at a full cache or at `max_new_tokens` ends with the tokens `infer_batched`
        returns for it.  A slot's end shows one window late, so a chunk is known up to `check_interval` steps after its last token.

        A scalar `repetition_penalty` applies to every request, as in `infer_stream` (`infer_batched` ignores a scalar); the
        sampling arguments are scalars or one per request, as in `infer_batched`.  The loop runs on the caller's stream.
        `ticks`: (None, None, False) is yielded behind every window too, for a caller that polls work of its own between windows.
        Closing the generator waits for the prompt passes, parks the slots and unbinds the sampling table."""
        n = len(x)
        boost = [bool(b) for b in SS.per_request("boost_first_chunk", boost_first_chunk, n)]
        if not SS.is_sequence(repetition_penalty):
            repetition_penalty = [repetition_penalty] * n
        if int(stream_chunk) < 1:
            raise ValueError("stream_chunk must be positive, got %r" % (stream_chunk,))
        self._samp = SS.resolve(n, top_k, top_p, temperature, seed, repetition_penalty, initial_suppression_steps)
        loop = None
        try:
            with torch.inference_mode():
                begun = self._begin_batched(x, y, bert_feature, 0, 1.0, 1.0, generator, None, slots, True)
                if begun is not None:
                    loop = self._async_loop(x, y, bert_feature, begun, check_interval, None, max_new_tokens)
            if loop is not None:
                for r, rows, is_final in SL.stream_chunks(loop, int(stream_chunk), boost, ticks):
                    yield r, (None if rows is None else rows[None, None]), is_final
        finally:
            if self._refill_stream is not None:
                self._refill_stream.synchronize()
            if loop is not None:
                with torch.inference_mode():
                    loop.stepped.rt["kv_len"].fill_(-1)
            self._samp = None
            self._unbind_sampling()
