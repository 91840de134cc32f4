"""ERes2NetV2 on the device: the speaker-verification embedding TTS.cache_spk_audio computes for v2Pro / v2ProPlus
(gsv_tts/TTS.py:1346-1389, 1591-1610; GPT_SoVITS/SV/sv.py, ERes2NetV2.py, fusion.py) -- csrc/sv.h behind the gsv_sv_*
entry points.

    sv_emb = SVNative(weights, device).embed(wav32k, 32000)    # [1, 20480], fp32, on the device

restates, in the reference's order, torchaudio.transforms.Resample(sr, 16000) (default arguments), Kaldi.fbank(wav,
num_mel_bins=80, sample_frequency=16000, dither=0) and ERes2NetV2(baseWidth=24, scale=4, expansion=4).forward3.  fp32
whatever the engine's numerics mode: it runs once per speaker and feeds every later stage.  `resample` needs no model
and also serves the CN-HuBERT prompt path.  No CPU path."""
import ctypes

import torch

from . import _native as N

SAMPLE_RATE = 16000
FEAT_DIM = 80


def infer_config(weights) -> N.SvConfig:
    """The ERes2NetV2 configuration a state dict describes (m_channels, blocks per stage, split width per stage); ValueError
    for anything this build does not run: scale or expansion other than 4, feat_dim other than 80, no AFF in stages 3-4."""
    shape = lambda k: tuple(weights[k].shape)
    if "conv1.weight" not in weights or shape("conv1.weight")[1:] != (1, 3, 3):
        raise ValueError("ERes2NetV2: no stem conv1.weight [m, 1, 3, 3] in the state dict")
    m = shape("conv1.weight")[0]
    blocks, width = [], []
    for s in range(4):
        n = 0
        while "layer%d.%d.conv1.weight" % (s + 1, n) in weights:
            n += 1
        if n == 0:
            raise ValueError("ERes2NetV2: stage %d has no blocks" % (s + 1))
        blocks.append(n)
        width.append(shape("layer%d.0.convs.0.weight" % (s + 1))[0])
    scale = 0
    while "layer1.0.convs.%d.weight" % scale in weights:
        scale += 1
    if scale != 4:
        raise ValueError("ERes2NetV2: scale %d is not supported (baseWidth=24, scale=4, expansion=4 only)" % scale)
    expansion = shape("layer1.0.conv3.weight")[0] // m
    if expansion != 4 or shape("layer1.0.conv3.weight")[0] != 4 * m:
        raise ValueError("ERes2NetV2: expansion %d is not supported (4 only)" % expansion)
    feat_dim = FEAT_DIM
    if "seg_1.weight" in weights:   # seg_1: Linear(int(feat_dim / 8) * m * 8 * expansion * 2, embedding_size)
        feat_dim = shape("seg_1.weight")[1] // (m * 8 * expansion * 2) * 8
    if feat_dim != FEAT_DIM:
        raise ValueError("ERes2NetV2: feat_dim %d is not supported (80-bin fbank only)" % feat_dim)
    for s in (2, 3):
        if "layer%d.0.fuse_models.0.local_att.0.weight" % (s + 1) not in weights:
            raise ValueError("ERes2NetV2: stage %d has no AFF fusion (BasicBlockERes2NetV2AFF expected)" % (s + 1))
    if "layer1.0.fuse_models.0.local_att.0.weight" in weights:
        raise ValueError("ERes2NetV2: stage 1 has AFF fusion; only stages 3-4 may")
    return N.SvConfig(m_channels=m, blocks=(ctypes.c_int * 4)(*blocks), width=(ctypes.c_int * 4)(*width), scale=scale,
                      expansion=expansion, feat_dim=feat_dim)


def _unused(name: str) -> bool:
    """tensors forward3 never reads: the pooling / segment head and BN's batch counters"""
    return name.startswith(("seg_1.", "seg_2.", "seg_bn_1.", "pool.")) or name.endswith("num_batches_tracked")


def _mono(x, what):
    a = torch.as_tensor(x)
    if a.dim() == 2 and a.shape[0] == 1:
        a = a[0]
    if a.dim() != 1:
        raise ValueError("%s takes one mono waveform ([n] or [1, n]); got shape %s" % (what, tuple(a.shape)))
    return a


def resample_length(n: int, orig_sr: int, new_sr: int) -> int:
    return N.lib().gsv_sv_resample_length(int(n), int(orig_sr), int(new_sr))


def resample(x, orig_sr: int, new_sr: int, device=None):
    """torchaudio.transforms.Resample(orig_sr, new_sr)(x) with default arguments, on the device: x [n] or [1, n] fp32 ->
    [resample_length(n)] fp32"""
    a = _mono(x, "resample")
    dev = torch.device(device) if device is not None else (a.device if a.is_cuda else torch.device("cuda", 0))
    if dev.type != "cuda":
        raise RuntimeError("resampling runs on the MI355X only (gsv_sv_resample); got device %s" % dev)
    a = a.to(device=dev, dtype=torch.float32).contiguous()
    n = a.numel()
    if n < 1:
        raise ValueError("resample: empty waveform")
    L = N.lib()
    n_out = L.gsv_sv_resample_length(n, int(orig_sr), int(new_sr))
    y = torch.empty(max(n_out, 1), dtype=torch.float32, device=dev)
    ws = torch.empty(max(L.gsv_sv_resample_workspace(int(orig_sr), int(new_sr)), 16), dtype=torch.uint8, device=dev)
    N.check(L.gsv_sv_resample(a.data_ptr(), n, int(orig_sr), int(new_sr), y.data_ptr(), ws.data_ptr(), ws.numel(),
                              N.current_stream_ptr(dev)))
    return y[:n_out]


class SVNative:
    """weights: an ERes2NetV2 state dict (torch or numpy), the shapes of ERes2NetV2(baseWidth=24, scale=4, expansion=4)
    at any m_channels / blocks per stage.  embed(wav, sample_rate) -> sv_emb [1, 32 * m_channels * 10] on `device`."""

    def __init__(self, weights, device):
        self._h = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ERes2NetV2 runs on the MI355X only (gsv_sv_*); got device %s -- there is no CPU path"
                               % self.device)
        weights = {k: torch.as_tensor(v) for k, v in weights.items()}
        cfg = infer_config(weights)
        self.m_channels = cfg.m_channels
        self.emb_dim = 32 * cfg.m_channels * (FEAT_DIM // 8)
        L = N.lib()
        h = ctypes.c_void_p()
        N.check(L.gsv_sv_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        st = N.current_stream_ptr(self.device)
        for name, t in weights.items():
            if _unused(name):
                continue
            d = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            N.check(L.gsv_sv_load_tensor(h, name.encode(), d.data_ptr(), d.numel(), st))
        N.check(L.gsv_sv_finalize(h, st))
        self._ws = None

    def __del__(self):
        try:
            if self._h is not None:
                N.lib().gsv_sv_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def frames(self, n_samples: int, sample_rate: int = SAMPLE_RATE) -> int:
        """fbank frames of n_samples at sample_rate once resampled to 16 kHz (0: shorter than one 400-sample frame)"""
        return N.lib().gsv_sv_frames(self._h, int(n_samples), int(sample_rate))

    def _workspace(self, n_samples, sample_rate):
        return self._grow_ws(N.lib().gsv_sv_workspace(self._h, int(n_samples), int(sample_rate)))

    def _grow_ws(self, need: int):
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _wave(self, wav, sample_rate):
        a = _mono(wav, "ERes2NetV2").to(device=self.device, dtype=torch.float32).contiguous()
        if self.frames(a.numel(), sample_rate) < 1:
            raise ValueError("ERes2NetV2: %d samples at %d Hz are too short for one fbank frame (400 samples at 16 kHz)"
                             % (a.numel(), sample_rate))
        return a

    def resample(self, wav, orig_sr: int, new_sr: int = SAMPLE_RATE):
        return resample(wav, orig_sr, new_sr, self.device)

    def fbank(self, wav16k):
        """Kaldi.fbank(wav16k, num_mel_bins=80, sample_frequency=16000, dither=0) -> [T, 80]"""
        a = self._wave(wav16k, SAMPLE_RATE)
        n = a.numel()
        T = self.frames(n)
        ws = self._workspace(n, SAMPLE_RATE)
        feat = torch.empty(T, FEAT_DIM, dtype=torch.float32, device=self.device)
        N.check(N.lib().gsv_sv_fbank(self._h, a.data_ptr(), n, feat.data_ptr(), ws.data_ptr(), ws.numel(),
                                     N.current_stream_ptr(self.device)))
        return feat

    def forward3(self, feat):
        """ERes2NetV2.forward3: feat [T, 80] or [1, T, 80] -> [1, emb_dim] (fuse34.flatten(1, 2).mean(-1))"""
        f = torch.as_tensor(feat)
        if f.dim() == 3 and f.shape[0] == 1:
            f = f[0]
        if f.dim() != 2 or f.shape[1] != FEAT_DIM or f.shape[0] < 1:
            raise ValueError("forward3 takes fbank features [T, 80] or [1, T, 80], T >= 1; got %s" % (tuple(f.shape),))
        f = f.to(device=self.device, dtype=torch.float32).contiguous()
        T = f.shape[0]
        ws = self._workspace(400 + 160 * (T - 1), SAMPLE_RATE)
        emb = torch.empty(1, self.emb_dim, dtype=torch.float32, device=self.device)
        N.check(N.lib().gsv_sv_forward(self._h, f.data_ptr(), T, emb.data_ptr(), ws.data_ptr(), ws.numel(),
                                       N.current_stream_ptr(self.device)))
        return emb

    def embed(self, wav, sample_rate: int):
        """ERes2Net.compute_embedding3(Resample(sample_rate, 16000)(wav)): wav [n] or [1, n] mono fp32 (peak-normalised as
        TTS._get_spec leaves it) -> sv_emb [1, emb_dim]"""
        a = self._wave(wav, sample_rate)
        n = a.numel()
        ws = self._workspace(n, sample_rate)
        emb = torch.empty(1, self.emb_dim, dtype=torch.float32, device=self.device)
        N.check(N.lib().gsv_sv_embed(self._h, a.data_ptr(), n, int(sample_rate), emb.data_ptr(), ws.data_ptr(), ws.numel(),
                                     N.current_stream_ptr(self.device)))
        return emb

    # Batches: every conv runs once for all clips of a chunk of AUX_MAX_CLIPS (gsv_sv_*_batch); row i is bit-identical
    # to the single-clip call on clip i whatever else is in the list.
    def forward3_batch(self, feats):
        """forward3 of every feature matrix in the list ([T_i, 80] or [1, T_i, 80]) -> [n, emb_dim]"""
        fs = []
        for i, f in enumerate(feats):
            f = torch.as_tensor(f)
            if f.dim() == 3 and f.shape[0] == 1:
                f = f[0]
            if f.dim() != 2 or f.shape[1] != FEAT_DIM or f.shape[0] < 1:
                raise ValueError("forward3_batch: clip %d is not fbank features [T, 80] or [1, T, 80], T >= 1; got %s"
                                 % (i, tuple(f.shape)))
            fs.append(f.to(device=self.device, dtype=torch.float32).contiguous())
        L = N.lib()
        emb = torch.empty(len(fs), self.emb_dim, dtype=torch.float32, device=self.device)
        for c0 in range(0, len(fs), N.AUX_MAX_CLIPS):
            chunk = fs[c0:c0 + N.AUX_MAX_CLIPS]
            T = (ctypes.c_int * len(chunk))(*[f.shape[0] for f in chunk])
            n16 = (ctypes.c_int * len(chunk))(*[400 + 160 * (f.shape[0] - 1) for f in chunk])
            ws = self._grow_ws(L.gsv_sv_batch_workspace(self._h, n16, len(chunk), SAMPLE_RATE))
            feat = torch.cat(chunk)
            N.check(L.gsv_sv_forward_batch(self._h, feat.data_ptr(), T, len(chunk), emb[c0].data_ptr(), ws.data_ptr(),
                                           ws.numel(), N.current_stream_ptr(self.device)))
        return emb

    def embed_batch(self, wavs, sample_rate: int):
        """embed of every waveform in the list ([n_i] or [1, n_i], all at sample_rate) -> sv_emb [n, emb_dim]; ValueError
        naming the index of a clip that is not mono or is shorter than one fbank frame"""
        clips = []
        for i, w in enumerate(wavs):
            a = _mono(w, "ERes2NetV2 (clip %d)" % i).to(device=self.device, dtype=torch.float32).contiguous()
            if self.frames(a.numel(), sample_rate) < 1:
                raise ValueError("ERes2NetV2: clip %d: %d samples at %d Hz are too short for one fbank frame (400 samples "
                                 "at 16 kHz)" % (i, a.numel(), sample_rate))
            clips.append(a)
        L = N.lib()
        emb = torch.empty(len(clips), self.emb_dim, dtype=torch.float32, device=self.device)
        for c0 in range(0, len(clips), N.AUX_MAX_CLIPS):
            chunk = clips[c0:c0 + N.AUX_MAX_CLIPS]
            ns = (ctypes.c_int * len(chunk))(*[a.numel() for a in chunk])
            ws = self._grow_ws(L.gsv_sv_batch_workspace(self._h, ns, len(chunk), int(sample_rate)))
            wav = torch.cat(chunk)
            N.check(L.gsv_sv_embed_batch(self._h, wav.data_ptr(), ns, len(chunk), int(sample_rate), emb[c0].data_ptr(),
                                         ws.data_ptr(), ws.numel(), N.current_stream_ptr(self.device)))
        return emb


def load_sv(path, device) -> SVNative:
    """a pretrained_eres2netv2w24s4ep4.ckpt state dict (loader.read_sv) on the device"""
    from .loader import read_sv
    return SVNative(read_sv(path), device)
