"""CN-HuBERT on the device: the model TTS._get_prompt runs on every new prompt (gsv_tts/TTS.py:1556-1570;
GPT_SoVITS/Featurizer/cnhubert.py wraps transformers.HubertModel) -- csrc/hubert.h behind the gsv_hubert_* entry points.

    ssl = CNHubertNative(weights, config, device).prompt_ssl(wav16k)    # [1, 768, Th], fp32, on the device

restates HubertModel(wav16k + 0.3 s of zeros)["last_hidden_state"].transpose(1, 2) exactly as _get_prompt calls it: no
Wav2Vec2FeatureExtractor normalisation, batch 1, no mask.  fp32 whatever the engine's numerics mode: it runs once per
prompt and feeds every token after it.  The waveform must already be mono at 16 kHz: resampling is outside this build
(the reference uses torchaudio's Resample, which is not available to pin a restatement against).  No CPU path."""
import ctypes

import torch

from . import _native as N

SAMPLE_RATE = 16000
PROMPT_PAD = int(SAMPLE_RATE * 0.3)   # TTS._get_prompt appends 0.3 s of silence

# HubertConfig() fields this build reads, with the library defaults
_DEFAULTS = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2],
                 num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, feat_extract_norm="group",
                 do_stable_layer_norm=False, conv_bias=False, hidden_act="gelu", feat_extract_activation="gelu",
                 feat_proj_layer_norm=True, conv_pos_batch_norm=False, layer_norm_eps=1e-5)


def check_config(config: dict) -> dict:
    """The config.json fields with HubertConfig's defaults filled in; ValueError for anything this build does not run."""
    c = dict(_DEFAULTS)
    c.update({k: v for k, v in dict(config).items() if k in _DEFAULTS})
    if c["feat_extract_norm"] != "group":
        raise ValueError("CN-HuBERT: feat_extract_norm=%r is not supported (only 'group': GroupNorm on the first conv)"
                         % c["feat_extract_norm"])
    if c["do_stable_layer_norm"]:
        raise ValueError("CN-HuBERT: do_stable_layer_norm=True (pre-LN layers) is not supported; this build runs the "
                         "post-LN order of HubertConfig()")
    if c["conv_bias"]:
        raise ValueError("CN-HuBERT: conv_bias=True is not supported (the feature-encoder convs have no bias)")
    for k in ("hidden_act", "feat_extract_activation"):
        if c[k] != "gelu":
            raise ValueError("CN-HuBERT: %s=%r is not supported (only exact 'gelu')" % (k, c[k]))
    if not c["feat_proj_layer_norm"]:
        raise ValueError("CN-HuBERT: feat_proj_layer_norm=False is not supported")
    if c["conv_pos_batch_norm"]:
        raise ValueError("CN-HuBERT: conv_pos_batch_norm=True is not supported (weight-normed positional conv only)")
    n = len(c["conv_dim"])
    if not (1 <= n <= N.HUBERT_MAX_CONV) or len(c["conv_kernel"]) != n or len(c["conv_stride"]) != n:
        raise ValueError("CN-HuBERT: conv_dim / conv_kernel / conv_stride must have the same length, 1..%d" % N.HUBERT_MAX_CONV)
    H, heads = c["hidden_size"], c["num_attention_heads"]
    if H % 64 or H > 1024 or heads * 64 != H:
        raise ValueError("CN-HuBERT: hidden_size %d with %d heads is not supported (head dim 64, hidden a multiple of 64 "
                         "up to 1024)" % (H, heads))
    if any(d % 64 or d > 1024 or d < 64 for d in c["conv_dim"]):
        raise ValueError("CN-HuBERT: conv_dim %s is not supported (multiples of 64 up to 1024)" % (c["conv_dim"],))
    k, G = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    if k % 2 or k < 2 or H % G:
        raise ValueError("CN-HuBERT: positional conv k=%d, groups=%d is not supported (even k, groups dividing hidden)" % (k, G))
    return c


def native_config(config: dict) -> N.HubertConfig:
    c = check_config(config)
    n = len(c["conv_dim"])
    pad = lambda v: (ctypes.c_int * N.HUBERT_MAX_CONV)(*(list(v) + [0] * (N.HUBERT_MAX_CONV - n)))
    return N.HubertConfig(hidden=c["hidden_size"], n_layer=c["num_hidden_layers"], n_head=c["num_attention_heads"],
                          ffn=c["intermediate_size"], n_conv=n, conv_dim=pad(c["conv_dim"]), conv_kernel=pad(c["conv_kernel"]),
                          conv_stride=pad(c["conv_stride"]), pos_k=c["num_conv_pos_embeddings"],
                          pos_groups=c["num_conv_pos_embedding_groups"], eps=float(c["layer_norm_eps"]))


def fold_pos_conv_weight(weights) -> torch.Tensor:
    """The positional conv's effective weight w = v * (g / ||v||), the norm over dims 0 and 1 for every tap (weight norm
    with dim=2) -- what the device computes at finalize; CPU fp32."""
    g = weights["encoder.pos_conv_embed.conv.weight_g"].float()
    v = weights["encoder.pos_conv_embed.conv.weight_v"].float()
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


class CNHubertNative:
    """weights: HubertModel state dict (torch or numpy; weight norm as weight_g / weight_v or parametrizations.*),
    config: config.json fields.  __call__(wav16k) -> ssl [1, hidden, Th] fp32 on `device`."""

    def __init__(self, weights, config, device):
        self._h = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CN-HuBERT runs on the MI355X only (gsv_hubert_*); got device %s -- there is no CPU path"
                               % self.device)
        L = N.lib()
        cfg = native_config(config)
        self.hidden = cfg.hidden
        h = ctypes.c_void_p()
        N.check(L.gsv_hubert_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        st = N.current_stream_ptr(self.device)
        for name, t in weights.items():
            if not name.startswith(("feature_extractor.", "feature_projection.", "encoder.")):
                continue   # masked_spec_embed: training-time masking only
            d = torch.as_tensor(t).detach().to(device=self.device, dtype=torch.float32).contiguous()
            N.check(L.gsv_hubert_load_tensor(h, name.encode(), d.data_ptr(), d.numel(), st))
        N.check(L.gsv_hubert_finalize(h, st))
        self._ws = None

    def __del__(self):
        try:
            if self._h is not None:
                N.lib().gsv_hubert_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def frames(self, n_samples: int) -> int:
        """output frames for n_samples input samples (0: too short for the feature encoder)"""
        return N.lib().gsv_hubert_frames(self._h, int(n_samples))

    def __call__(self, wav16k):
        """wav16k [n] or [1, n] fp32, mono 16 kHz, as the model reads it -> last_hidden_state^T [1, hidden, Th]"""
        a = torch.as_tensor(wav16k)
        if a.dim() == 2 and a.shape[0] == 1:
            a = a[0]
        if a.dim() != 1:
            raise ValueError("CN-HuBERT takes one mono 16 kHz waveform ([n] or [1, n]); got shape %s" % (tuple(a.shape),))
        a = a.to(device=self.device, dtype=torch.float32).contiguous()
        n = a.numel()
        Th = self.frames(n)
        if Th < 1:
            raise ValueError("CN-HuBERT: %d samples are too short for the feature encoder" % n)
        need = N.lib().gsv_hubert_workspace(self._h, n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ssl = torch.empty(1, self.hidden, Th, dtype=torch.float32, device=self.device)
        N.check(N.lib().gsv_hubert_forward(self._h, a.data_ptr(), n, ssl.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                           N.current_stream_ptr(self.device)))
        return ssl

    def prompt_ssl(self, wav16k):
        """TTS._get_prompt's ssl_content: the waveform + 0.3 s of zeros through the model, [1, hidden, Th]"""
        a = torch.as_tensor(wav16k).to(device=self.device, dtype=torch.float32).reshape(-1)
        return self(torch.cat([a, a.new_zeros(PROMPT_PAD)]))

    def _grow_ws(self, need: int):
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def batch(self, wavs):
        """a list of waveforms as __call__ takes them -> [ssl [1, hidden, Th_i]]: the clips run packed
        (gsv_hubert_forward_batch, AUX_MAX_CLIPS per call), each result bit-identical to self(wav) whatever else is in the
        list.  ValueError naming the index of a clip that is not one mono waveform or is too short."""
        clips = []
        for i, w in enumerate(wavs):
            a = torch.as_tensor(w)
            if a.dim() == 2 and a.shape[0] == 1:
                a = a[0]
            if a.dim() != 1:
                raise ValueError("CN-HuBERT: clip %d is not one mono 16 kHz waveform ([n] or [1, n]); got shape %s"
                                 % (i, tuple(a.shape)))
            if self.frames(a.numel()) < 1:
                raise ValueError("CN-HuBERT: clip %d: %d samples are too short for the feature encoder" % (i, a.numel()))
            clips.append(a.to(device=self.device, dtype=torch.float32).contiguous())
        L, out = N.lib(), []
        for c0 in range(0, len(clips), N.AUX_MAX_CLIPS):
            chunk = clips[c0:c0 + N.AUX_MAX_CLIPS]
            ns = (ctypes.c_int * len(chunk))(*[a.numel() for a in chunk])
            Th = [self.frames(a.numel()) for a in chunk]
            ws = self._grow_ws(L.gsv_hubert_batch_workspace(self._h, ns, len(chunk)))
            audio = torch.cat(chunk)
            ssl = torch.empty(self.hidden * sum(Th), dtype=torch.float32, device=self.device)
            N.check(L.gsv_hubert_forward_batch(self._h, audio.data_ptr(), ns, len(chunk), ssl.data_ptr(), ws.data_ptr(),
                                               ws.numel(), N.current_stream_ptr(self.device)))
            off = 0
            for t in Th:
                out.append(ssl[self.hidden * off:self.hidden * (off + t)].view(1, self.hidden, t))
                off += t
        return out

    def prompt_ssl_batch(self, wavs):
        """prompt_ssl of every waveform in the list, run as one batch: [ssl [1, hidden, Th_i]]"""
        padded = []
        for w in wavs:
            a = torch.as_tensor(w).to(device=self.device, dtype=torch.float32).reshape(-1)
            padded.append(torch.cat([a, a.new_zeros(PROMPT_PAD)]))
        return self.batch(padded)


def load_cnhubert(path, device) -> CNHubertNative:
    """a Hugging Face chinese-hubert-base directory (loader.read_cnhubert) on the device"""
    from .loader import read_cnhubert
    config, weights = read_cnhubert(path)
    return CNHubertNative(weights, config, device)
