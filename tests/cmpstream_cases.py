"""What test_cmpstream_cpu.py and test_hip_cmpstream.py share on the product's side: the raw gsv_cmpstream_* calls with guard bytes
behind the stated state, the record and the samples, the cuttings of DESIGN 4.27's contract (those of tests/eqstream_cases.py
rebuilt on the compressor's run, span and chunk), and the parameter sets of tests/compressor_ref.py as compressor.Compressor
objects with the clip twin of every grid signal."""
import functools

import numpy as np
import torch

import compressor_ref as R

from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import compressor as CM

RUN, SPAN, CHUNK = R.RUN, R.SPAN, R.CHUNK
REC = 40
GUARD = 64
FILL = -7.25
# the stream lengths of the contract
LENGTHS = (0, 1, RUN + 1, SPAN + 1, CHUNK, CHUNK + 1, 2 * CHUNK + SPAN + 5)


def comp_for(name):
    return CM.Compressor(*R.SETS[name])


def params_struct(c, rate):
    return CM._tables([], [], [], [c.coefficients(rate)])[1]


class RawStream:
    """one state behind the raw entries, GUARD bytes of 0xA5 behind what gsv_cmpstream_state_bytes states"""

    def __init__(self, c, rate, device="cpu", coefficients=None):
        self.device = torch.device(device)
        self.L = N.lib()
        self.need = self.L.gsv_cmpstream_state_bytes()
        self.state = torch.full((self.need + GUARD,), 0xA5, dtype=torch.uint8, device=self.device)
        tab = CM._tables([], [], [], [coefficients])[1] if coefficients is not None else params_struct(c, rate)
        if self.device.type == "cuda":
            N.check(self.L.gsv_cmpstream_init(self.state.data_ptr(), self.need, tab, N.current_stream_ptr(self.device)))
        else:
            N.check(self.L.gsv_cmpstream_init_host(self.state.data_ptr(), self.need, tab))

    def push(self, x, flush=False, inplace=False, held=None):
        """-> (samples as numpy: the whole `out` buffer of len(x) + 4 guard floats, the record's 40 bytes).  held: the length handed
        in through n_dev / n_host instead of len(x)"""
        n = len(x)
        src = torch.from_numpy(np.array(x, np.float32))
        buf = torch.full((n + 4,), FILL, dtype=torch.float32)
        buf[:n] = src
        chunk = buf.to(self.device) if self.device.type == "cuda" else buf
        out = chunk if inplace else torch.full((n + 4,), 2 * FILL, dtype=torch.float32, device=self.device)
        rec = torch.full((REC + GUARD,), 0xA5, dtype=torch.uint8, device=self.device)
        assert rec.data_ptr() % 8 == 0
        n_ptr = None
        if held is not None:
            n_t = torch.tensor([held], dtype=torch.int32, device=self.device)
            n_ptr = n_t.data_ptr()
        args = (self.state.data_ptr(), chunk.data_ptr(), n, n_ptr, int(flush), out.data_ptr(), rec.data_ptr())
        if self.device.type == "cuda":
            N.check(self.L.gsv_cmpstream_push(*args, N.current_stream_ptr(self.device)))
            torch.cuda.synchronize(self.device)
        else:
            N.check(self.L.gsv_cmpstream_push_host(*args))
        recb = rec.cpu().numpy()
        assert np.all(recb[REC:] == 0xA5), "written behind the record"
        assert bool((self.state[self.need:] == 0xA5).all()), "written behind the stated state"
        if not inplace:
            assert torch.equal(chunk[:n].cpu().view(torch.int32), src.view(torch.int32)), "out of place: the chunk was written"
        return out.cpu().numpy(), recb[:REC].tobytes()

    def run(self, x, cuts, inplace=False):
        """the stream cut at `cuts` (the last push flushes) -> (samples, the raw records)"""
        parts, recs, at = [], [], 0
        for k, n in enumerate(cuts):
            o, r = self.push(x[at: at + n], flush=k + 1 == len(cuts), inplace=inplace)
            emitted = int(np.frombuffer(r, np.int32)[0])
            assert emitted == n, (emitted, n)
            want_tail = FILL if inplace else 2 * FILL
            assert np.all(o[n:] == np.float32(want_tail)), "written behind the push's samples"
            parts.append(o[:n])
            recs.append(r)
            at += n
        assert at == len(x)
        return np.concatenate(parts), recs


def cut_every(n, step):
    return [min(step, n - at) for at in range(0, n, step)] or [0]


def cut_random(n, seed):
    """seeded cuts, short and long, with empty pushes; the flush is an empty push"""
    rng = np.random.default_rng(seed)
    cuts, at = [], 0
    while at < n:
        c = 0 if rng.random() < 0.2 else int(rng.integers(1, 40 if rng.random() < 0.5 else 3 * SPAN))
        c = min(c, n - at)
        cuts.append(c)
        at += c
    return cuts + [0]


FINE = (RUN - 1, RUN, RUN + 1)
COARSE = (SPAN - 1, SPAN, SPAN + 1, CHUNK - 1, CHUNK, CHUNK + 1)


def cuttings(n, fine=True):
    """the cuttings of the contract: single samples (n <= 97), pushes of a run, a span, a chunk and one less and one more, three
    seeded random cuttings with empty pushes, a flush carried by an empty push, a push of 2 CHUNK + 3 (two chunks completed at
    once)"""
    res = []
    if n <= 97:
        res.append(cut_every(n, 1))
    res += [cut_every(n, s) for s in (FINE if fine else ()) + COARSE]
    res += [cut_random(n, 7 * n + j) for j in range(3)]
    res.append(cut_every(n, 700 if n <= SPAN + 1 else 5000) + [0])
    res.append(cut_every(n, 2 * CHUNK + 3))
    return res


@functools.lru_cache(maxsize=None)
def clip_twin(name, kind, n, rate):
    """compressor.compress on the host over a grid signal -> (samples, CmpRecord), computed once"""
    y, rec = CM.compress(np.array(R.grid_signal(kind, n, rate, name)), rate, comp_for(name), device="cpu")
    y.setflags(write=False)
    return y, rec


def record(raw):
    return CM.stream_record(np.frombuffer(raw, np.uint8))


def bits(v):
    return np.float32(v).view(np.uint32)
