"""What test_reverb_cpu.py and test_hip_reverb.py share on the product's side: packing clips between guard words, the oracle's
parameter sets in the call's form, and the raw gsv_reverb / gsv_reverb_host call with guard bytes behind the workspace and the
records."""
import numpy as np
import torch

from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import reverb as RV

GUARD = 5           # odd, so every clip starts at an odd offset
FILL = np.float32(-7.25)
REC = 16


def params_of(ps):
    """a parameter set of reverb_ref -> the pair run_packed takes"""
    combs, aps, d, fb, gin, gw, gd = ps
    return np.array(combs + aps, np.int32), np.array([d, fb, gin, gw, gd], np.float64)


def pack(clips):
    """one buffer with GUARD words before, between and after the clips -> (x, offsets)"""
    x = np.full(GUARD + sum(len(c) + GUARD for c in clips), FILL, np.float32)
    offsets, at = [], GUARD
    for c in clips:
        x[at: at + len(c)] = c
        offsets.append(at)
        at += len(c) + GUARD
    return x, offsets


def call(x, offsets, lengths, index, params, device, mode="out"):
    """the raw call -> (out buffer as numpy, record bytes, x afterwards); mode 'inplace' or 'out'"""
    L = N.lib()
    n = len(lengths)
    clips, tab = RV._tables(offsets, lengths, index, params)
    need = L.gsv_reverb_work_bytes(clips, n, tab, len(params))
    assert need > 0
    xt = torch.from_numpy(x.copy()).to(device)
    work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=device)
    rec = torch.full((n * REC + 32,), 0xA5, dtype=torch.uint8, device=device)
    out = xt if mode == "inplace" else torch.full_like(xt, float(FILL) * 2)
    args = (xt.data_ptr(), xt.numel(), clips, n, tab, len(params), out.data_ptr(), rec.data_ptr(), work.data_ptr(), need)
    if device.type == "cuda":
        N.check(L.gsv_reverb(*args, N.current_stream_ptr(device)))
        torch.cuda.synchronize(device)
    else:
        N.check(L.gsv_reverb_host(*args))
    assert bool((work[need:] == 0xA5).all()), "written behind the stated workspace"
    recb = rec.cpu().numpy()
    assert np.all(recb[n * REC:] == 0xA5), "written behind the records"
    return out.cpu().numpy(), recb[: n * REC].tobytes(), xt.cpu().numpy()


def recs_of(raw):
    return RV.records(np.frombuffer(raw, np.uint8))
