"""Plain torch / numpy restatement of the speaker-verification path (TEST INFRASTRUCTURE): what gsv_sv_* computes on the
device, written from the published algorithms without torchaudio.

resample   torchaudio.transforms.Resample(orig, new) with default arguments (torchaudio/functional/functional.py,
           _get_sinc_resample_kernel + _apply_sinc_resample_kernel): sinc_interp_hann, lowpass_filter_width 6, rolloff
           0.99, rates reduced by their gcd, the kernel built in fp64 (cast to fp32 in torchaudio), input zero-padded by
           (width, width + orig), stride-orig correlation, phases interleaved, ceil(new * n / orig) samples kept.
fbank      torchaudio.compliance.kaldi.fbank defaults with num_mel_bins=80, sample_frequency=16000, dither=0
           (torchaudio/compliance/kaldi.py: _get_window, get_mel_banks): 400-sample frames every 160 (snip_edges), the
           frame mean removed, pre-emphasis 0.97 with the first sample replicated, Povey window hann(400,
           periodic=False) ** 0.85, zero-padded to 512, |rfft| ** 2, 80 triangular mel filters (1127 ln(1 + f / 700)) from
           20 Hz to 8000 Hz over the bins k * 31.25 Hz (k < 256) with a zero Nyquist column, log(max(e, FLT_EPSILON)).
forward3   ERes2NetV2.forward3 (gsv_tts/GPT_SoVITS/SV/ERes2NetV2.py, fusion.py) with BN in eval mode, eps 1e-5.

torchaudio is not importable where these tests run, so resample and fbank restate its source as read; the model is
pinned to the reference's own module by tests/golden/sv.npz (tools/gen_golden_sv.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

FLT_EPS = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------------- resample
def resample_params(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    return o, n, base, width


def resample_kernel(orig, new):
    """[new][2 * width + orig] in float64 (torchaudio's values before its fp32 cast), and width"""
    o, n, base, width = resample_params(orig, new)
    idx = np.arange(-width, width + o, dtype=np.float64) / o
    # torch.arange(0, -new, -1)[:, None, None] / new is an int64 tensor divided in the default dtype (float32)
    ph = (np.arange(0, -n, -1).astype(np.float32) / np.float32(n)).astype(np.float64)
    t = (ph[:, None] + idx[None, :]) * base
    t = np.clip(t, -6.0, 6.0)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    return k * window * (base / o), width


def resample_length(n, orig, new):
    o, w, _, _ = resample_params(orig, new)
    return n if o == w else -(-w * n // o)


def resample(x, orig, new, dtype=np.float64):
    """x [n] -> [ceil(new n / orig)]; dtype float64 (the reference's arithmetic in full precision) or float32 (the kernel
    cast to fp32 and fp32 sums, as torchaudio runs it)"""
    x = np.asarray(x, dtype=np.float64)
    o, n, _, _ = resample_params(orig, new)
    if o == n:
        return x.astype(dtype)
    k, width = resample_kernel(orig, new)
    if dtype == np.float32:
        k = k.astype(np.float32)
    L = k.shape[1]
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)]).astype(dtype)
    frames = (xp.shape[0] - L) // o + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[::o][:frames]     # [frames][L]
    y = (win @ k.astype(dtype).T).reshape(-1)                                 # [frames * new], phase-interleaved
    return y[:resample_length(x.shape[0], orig, new)]


# ------------------------------------------------------------------------------------------------------------- fbank
WIN, HOP, NFFT, MELS = 400, 160, 512, 80


def fbank_frames(n):
    return 0 if n < WIN else 1 + (n - WIN) // HOP


def mel_banks(dtype=np.float64):
    """[80][257] (the Nyquist column zero)"""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)
    lo, hi = mel(20.0), mel(8000.0)
    d = (hi - lo) / (MELS + 1)
    b = np.arange(MELS, dtype=np.float64)[:, None]
    left, center, right = lo + b * d, lo + (b + 1.0) * d, lo + (b + 2.0) * d
    m = mel(16000.0 / NFFT * np.arange(NFFT // 2, dtype=np.float64))[None, :]
    up = (m - left) / (center - left)
    down = (right - m) / (right - center)
    bank = np.maximum(0.0, np.minimum(up, down))
    return np.concatenate([bank, np.zeros((MELS, 1))], axis=1).astype(dtype)


def povey_window():
    i = np.arange(WIN, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * math.pi * i / (WIN - 1))) ** 0.85


def fbank(x, dtype=np.float64):
    """x [n] at 16 kHz -> [frames][80]"""
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    T = fbank_frames(x.shape[0])
    if T == 0:
        return np.zeros((0, MELS), dtype)
    fr = np.lib.stride_tricks.sliding_window_view(x, WIN)[::HOP][:T].astype(dtype)
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - dtype(0.97) * prev) * povey_window().astype(dtype)
    fr = np.concatenate([fr, np.zeros((T, NFFT - WIN), dtype)], axis=1)
    spec = np.fft.rfft(fr.astype(np.float64), axis=1)
    power = (spec.real ** 2 + spec.imag ** 2).astype(dtype)
    e = power @ mel_banks(dtype).T
    return np.log(np.maximum(e, FLT_EPS)).astype(dtype)


# ----------------------------------------------------------------------------------------------------------- model
def config(w):
    """(m_channels, blocks per stage) of a state dict"""
    m = w["conv1.weight"].shape[0]
    blocks = []
    for s in range(4):
        n = 0
        while "layer%d.%d.conv1.weight" % (s + 1, n) in w:
            n += 1
        blocks.append(n)
    return m, blocks


def _bn(x, w, p):
    return F.batch_norm(x, w[p + "running_mean"], w[p + "running_var"], w[p + "weight"], w[p + "bias"], False, 0.0, 1e-5)


def _htanh(x):
    return F.hardtanh(x, 0.0, 20.0)


def _aff(w, p, x, y):
    a = F.conv2d(torch.cat((x, y), 1), w[p + "local_att.0.weight"], w[p + "local_att.0.bias"])
    a = F.silu(_bn(a, w, p + "local_att.1."))
    a = F.conv2d(a, w[p + "local_att.3.weight"], w[p + "local_att.3.bias"])
    a = 1.0 + torch.tanh(_bn(a, w, p + "local_att.4."))
    return x * a + y * (2.0 - a)


def _block(w, p, x, stride, aff):
    width = w[p + "convs.0.weight"].shape[0]
    out = _htanh(_bn(F.conv2d(x, w[p + "conv1.weight"], stride=stride), w, p + "bn1."))
    spx = torch.split(out, width, 1)
    outs = []
    for i in range(4):
        if i == 0:
            sp = spx[0]
        elif aff:
            sp = _aff(w, p + "fuse_models.%d." % (i - 1), sp, spx[i])
        else:
            sp = sp + spx[i]
        sp = _htanh(_bn(F.conv2d(sp, w[p + "convs.%d.weight" % i], padding=1), w, p + "bns.%d." % i))
        outs.append(sp)
    out = _bn(F.conv2d(torch.cat(outs, 1), w[p + "conv3.weight"]), w, p + "bn3.")
    if p + "shortcut.0.weight" in w:
        res = _bn(F.conv2d(x, w[p + "shortcut.0.weight"], stride=stride), w, p + "shortcut.1.")
    else:
        res = x
    return _htanh(out + res)


def forward3(weights, feat, dtype=torch.float64, taps=None):
    """ERes2NetV2.forward3(feat[None]) -> [20480-like] (index c * 10 + f); feat [T][80].  taps: a dict that receives the
    layer1 / layer3 / fuse34 activations [C][F][T]."""
    w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    m, blocks = config(w)
    x = torch.as_tensor(np.asarray(feat)).to(dtype).t()[None, None]      # [1, 1, F, T]
    out = F.relu(_bn(F.conv2d(x, w["conv1.weight"], padding=1), w, "bn1."))
    outs = []
    for s in range(4):
        for b in range(blocks[s]):
            out = _block(w, "layer%d.%d." % (s + 1, b), out, 2 if (b == 0 and s > 0) else 1, s >= 2)
        outs.append(out)
    ds = F.conv2d(outs[2], w["layer3_ds.weight"], padding=1, stride=2)
    fuse = _aff(w, "fuse34.", outs[3], ds)
    if taps is not None:
        taps["layer1"], taps["layer3"], taps["fuse34"] = outs[0][0], outs[2][0], fuse[0]
    return fuse.flatten(1, 2).mean(-1)[0]
