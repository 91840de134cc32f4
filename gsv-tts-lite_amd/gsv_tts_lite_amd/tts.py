"""`TTS`: the reference's engine facade (gsv_tts/TTS.py) over the MI355X hot path.

Drop-in surface kept from the reference:
    TTS(gpt_cache, sovits_cache, models_dir, device, dtype, use_flash_attn, use_bert, auto_bert,
        use_jieba_fast, always_load_cnhubert, always_load_sv)                 TTS.py:39-52
    infer(...) -> AudioClip                                                    TTS.py:150-286
    infer_batched(...) -> tuple[AudioClip]                                     TTS.py:507-868
    infer_stream(...) -> generator of AudioClip, infer_vc(...), *_async wrappers  TTS.py:289-504, 871-1262
    to_safetensors, cache_* / del_* / get_*_list                                TTS.py:1346-1523
    load_gpt_model / load_sovits_model / unload_* / get_*_list                 TTS.py:1264-1345
    AudioClip(audio_data, samplerate, audio_len_s, subtitles, orig_text)       Player.py:68-99

CN-HuBERT runs on the device (hubert.py, loaded lazily from models_dir/chinese-hubert-base as TTS.py:111 does), and
so do ERes2NetV2 with its 16 kHz resampling and Kaldi fbank (sv.py, from models_dir/sv/pretrained_eres2netv2w24s4ep4.ckpt,
TTS.py:113) and Chinese RoBERTa (roberta.py, from models_dir/chinese-roberta-wwm-ext-large, TTS.py:112): use_bert=True
loads it in __init__, auto_bert=True (the default) loads it on the first infer / infer_stream / infer_batched whose text
holds a CJK ideograph (the reference asks LangSegment for "zh", which is not available here, so kanji-only Japanese
text loads it too).  Either sets tts_config.cnroberta, so a frontend written as
`lambda t: get_phones_and_bert(t, tts.tts_config)` gets device BERT features; without the directory one warning is
logged and bert2 stays zeros.  Reference audio given as a path that names an existing WAV file (PCM or IEEE float, mono
or stereo) or FLAC file (8..24 bits, mono or stereo) is read as TTS._load_audio reads it: the container parsed on the
host, the samples converted to fp32 mono on the device (wavio.py) -- FLAC frames decoded there first (flacio.py) -- so
infer("spk.wav", "prompt.flac", ...) works as in the reference.  Going out, AudioClip.save("x.flac") writes 16-bit FLAC
whose frames are encoded on the device (flacio.py, csrc/flacenc.h; on the CPU by the same arithmetic without a GPU) and
AudioClip.to_flac() returns those bytes; other extensions get the 16-bit WAV writer.  What else sits in front of the
hot path in the reference -- G2P text frontends and decoding lossy compressed audio (mp3, ogg) -- is OUT OF SCOPE of this
build (CPU string processing and third-party packages not installable here).  Their
*outputs* enter through the same caches the reference keeps:
    cache_spk_audio(path)  or  cache_spk_audio(path, ge=...)  or
    cache_spk_audio(path, audio=<waveform>[, sample_rate=<model rate>][, sv_emb=<ERes2Net embedding>])
                                   (resampling to the model rate, spectrogram + get_ge on the device, and for v2Pro /
                                   v2ProPlus without sv_emb the ERes2NetV2 embedding as well; the reference: TTS.py:1346,
                                   1576)
    cache_prompt_audio(path, text[, phones1=..., bert1=...])  or
    cache_prompt_audio(path, text, prompt=... | ssl_content=<CN-HuBERT features> | audio=<waveform>[, sample_rate=16000],
                       phones1=..., bert1=...)
                                   (resampling + CN-HuBERT + extract_latent on the device; TTS.py:1391, 1556)
    verify_speaker(a, b)           cosine similarity of two ERes2NetV2 embeddings (TTS.py:1205-1245)
    set_text_frontend(fn)   fn(text) -> (phones2, word2ph, bert2[P,1024], norm_text)
With those in place infer()/infer_batched()/infer_stream() behave as in the reference, including
`return_subtitles=True`: the frame->phoneme alignment runs on the device (subtitles.viterbi_monotonic ->
gsv_align_viterbi, replacing TTS.py:1744-1797) and the word-timing / text-span bookkeeping is subtitles.py.
"""
from __future__ import annotations

import logging
import numbers
import os
import re
import threading
from pathlib import Path

import numpy as np
import torch

from . import finish, slot_sampling
from .finish import _check_loudness_seed, _check_true_peak  # noqa: F401  (the names tests and callers import from here)
from ._native import VOC_MAX_SEGMENTS
from . import subtitles as sub
from .batchmath import balance_order, per_text_values, split_bounds
from .stream import ChunkEmitter, ChunkSplicer
from .track import TrackFormat
from .loader import Gpt, Sovits, convert_to_safetensors, get_gpt_weights, get_sovits_weights

log = logging.getLogger("gsv_tts_lite_amd")

PAUSE_MARKS = tuple("…。？！.?!,，:：;；~、・—")


class Config:
    def __init__(self):
        if torch.cuda.is_available():
            self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
            self.dtype = torch.bfloat16
        else:
            self.device = torch.device("cpu")
            self.dtype = torch.float32
        self.use_flash_attn = False
        self.gpt_cache = []
        self.sovits_cache = []
        self.cnroberta = None   # Config.py:95: the BERT featurizer get_phones_and_bert calls (roberta.CNRobertaNative)


class AudioClip:
    """Player.py:68-99 fields; playback needs `sounddevice`, saving uses `soundfile` when present.  Without it a path
    ending in .flac is written as 16-bit FLAC, encoded on the GPU when there is one and by the same arithmetic on the CPU
    otherwise (flacio.save_flac), and every other path by a 16-bit PCM WAV writer.  to_flac() returns the FLAC file's
    bytes instead of writing them.  A saved .flac is valid reference audio: tts.infer("gen.flac", ...)."""

    def __init__(self, audio_queue, audio_data, samplerate, audio_len_s, subtitles, orig_text):
        self.audio_queue = audio_queue
        self.audio_data = audio_data
        self.samplerate = samplerate
        self.audio_len_s = audio_len_s
        self.subtitles = subtitles
        self.orig_text = orig_text
        self.pcm = None             # a stream with track=: int16 [k, packet * channels], the whole packets this clip completed
        self.pcm_rate = None        # and the track's sample rate
        self.lufs = None            # a clip made with loudness= (or by normalised()): the integrated loudness before the gain,
        self.gain = None            # the gain applied (np.float32: audio_data is the unnormalised samples times it)
        self.limited = None         # and whether the peak limit, not the target, set that gain
        self.dbtp = None            # a clip made with true_peak= (or by limited_to()): its true peak in dBTP behind the limiter;
                                    # `limited` then says whether the limiter had to act
        self.dbtp_in = None         # a clip of a stream made with true_peak=: the highest true peak in dBTP of the UNLIMITED stream so
        self.gain_min = None        # far, and the smallest gain among this clip's samples; `limited`: the limiter has acted so far
        self.eq = None              # a clip made with eq= (or by equalised()): the eq.EqRecord -- peak_in, peak_out, sections;
                                    # a clip of a stream made with eq=: the eq.EqStreamRecord of its push
        self.comp = None            # a clip made with compress= (or by compressed()): the compressor.CmpRecord -- peak_in, peak_out,
                                    # min_gain, compressed; a clip of a stream made with compress=: the
                                    # compressor.CmpStreamRecord of its push
        self.ambience = None        # a clip made with ambience= (or by ambient()): the reverb.RvbRecord -- peak_in, peak_out,
                                    # reverbed

    def play(self, volume: float = 1.0):
        if self.audio_queue is None:
            raise RuntimeError("audio playback needs the optional `sounddevice` package")
        data = self.audio_data if volume == 1.0 else np.clip(self.audio_data * volume, -1.0, 1.0)
        self.audio_queue.put(data)

    def save(self, save_path: str, is_save_subtitles: bool = False):
        try:
            import soundfile as sf
            sf.write(save_path, self.audio_data, self.samplerate)
        except ImportError:
            if str(save_path).lower().endswith(".flac"):
                from . import flacio
                flacio.save_flac(save_path, self.audio_data, self.samplerate, bits=16)
            else:
                self._save_wav(save_path)
        if is_save_subtitles:
            import json
            with open(os.path.splitext(save_path)[0] + ".json", "w", encoding="utf-8") as f:
                json.dump(self.subtitles, f, ensure_ascii=False, indent=2)

    def to_flac(self, bits: int = 16) -> bytes:
        """the clip as the bytes of a FLAC file (mono, `bits` 16 or 24, the quantiser of flacio.encode_flacs), for a
        server that returns the file in a response: what save("x.flac") writes, without the file"""
        from . import flacio
        return flacio.encode_flac(self.audio_data, self.samplerate, bits=bits)

    def to_pcm16(self, rate: int = 48000, channels: int = 1, packet_ms=20) -> np.ndarray:
        """the clip as the packets of a real-time track (track.pcm16): int16 [k, packet * channels] at `rate`, the last packet
        filled with zeros.  What a stream with track=TrackFormat(rate, channels, packet_ms) carries in its clips' `pcm`, all
        clips of a text together, bit for bit."""
        from . import track
        return track.pcm16(self.audio_data, self.samplerate, track.TrackFormat(rate, channels, packet_ms))

    def loudness(self) -> float:
        """ITU-R BS.1770 integrated loudness of audio_data in LUFS (loudness.integrated_loudness: measured on the GPU when there
        is one, by the same arithmetic on the CPU otherwise); -inf for a clip with nothing to measure"""
        from . import loudness
        return loudness.integrated_loudness(self.audio_data, self.samplerate)

    def normalised(self, target: float = -18.0, peak_limit: float = 1.0) -> "AudioClip":
        """a new clip at `target` LUFS -- or as close as peak_limit lets its peak come --, same subtitles and text; its
        lufs / gain / limited say what was measured and done (loudness.normalise)"""
        from . import loudness
        audio, rec = loudness.normalise(self.audio_data, self.samplerate, target, peak_limit)
        return finish.with_records(self._derived(audio, "eq", "comp", "ambience"), {"loudness": rec})

    def equalised(self, eq="voice") -> "AudioClip":
        """a new clip through the equaliser `eq` -- an eq.EQ or a preset name (eq.py) --, same subtitles and text; its
        `eq` is the eq.EqRecord: the peak before and after, which boosts may lift above 1.0 (limited_to() holds a ceiling)"""
        from . import eq as eqm
        if not isinstance(eq, (str, eqm.EQ)):
            raise ValueError("eq: a preset name (%s) or an eq.EQ, not %r" % (", ".join(eqm.PRESETS), type(eq).__name__))
        audio, rec = eqm.equalise(self.audio_data, self.samplerate, eq)
        return finish.with_records(self._derived(audio, "comp", "ambience"), {"eq": rec})

    def compressed(self, c="voice") -> "AudioClip":
        """a new clip through the compressor `c` -- a compressor.Compressor or a preset name (compressor.py) --, same
        subtitles and text; its `comp` is the compressor.CmpRecord: the peak before and after, the smallest gain and whether the
        compressor acted; `eq` is kept"""
        from . import compressor as cm
        if not isinstance(c, (str, cm.Compressor)):
            raise ValueError("compress: a preset name (%s) or a compressor.Compressor, not %r" % (", ".join(cm.PRESETS), type(c).__name__))
        audio, rec = cm.compress(self.audio_data, self.samplerate, c)
        return finish.with_records(self._derived(audio, "eq", "ambience"), {"compress": rec})

    def ambient(self, r="voice") -> "AudioClip":
        """a new clip through the reverb `r` -- a reverb.Reverb or a preset name (reverb.py) --, same subtitles, text
        and length (the tail behind the clip is cut); its `ambience` is the reverb.RvbRecord: the peak before and after, which the
        dry gain may lift above 1.0 (limited_to() holds a ceiling); `eq` and `comp` are kept"""
        from . import reverb as rv
        if not isinstance(r, (str, rv.Reverb)):
            raise ValueError("ambience: a preset name (%s) or a reverb.Reverb, not %r" % (", ".join(rv.PRESETS), type(r).__name__))
        audio, rec = rv.reverberate(self.audio_data, self.samplerate, r)
        return finish.with_records(self._derived(audio, "eq", "comp"), {"ambience": rec})

    def true_peak(self) -> float:
        """the true peak of audio_data in dBTP (limiter.true_peak: the largest magnitude of the clip oversampled 4x, measured on
        the GPU when there is one, by the same arithmetic on the CPU otherwise); -inf for silence"""
        from . import limiter
        return limiter.true_peak(self.audio_data, self.samplerate)

    def limited_to(self, ceiling_db: float = -1.0) -> "AudioClip":
        """a new clip held at or under `ceiling_db` dBTP by the look-ahead limiter (limiter.limit), same subtitles and text; its
        dbtp / limited say what came out and whether the limiter acted, lufs / gain are kept"""
        from . import limiter
        audio, rec = limiter.limit(self.audio_data, self.samplerate, ceiling_db)
        return finish.with_records(self._derived(audio, "lufs", "gain", "eq", "comp", "ambience"), {"true_peak": rec})

    def _derived(self, audio, *keep):
        """a clip like this one -- same subtitles and text -- with new samples; of the stages' records it keeps the fields named"""
        out = AudioClip(self.audio_queue, audio, self.samplerate, self.audio_len_s, self.subtitles, self.orig_text)
        for field in keep:
            setattr(out, field, getattr(self, field))
        return out

    def _save_wav(self, save_path):
        import wave
        pcm = (np.clip(self.audio_data, -1.0, 1.0) * 32767.0).astype("<i2")
        with wave.open(save_path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(self.samplerate)
            w.writeframes(pcm.tobytes())


def cut_text(text: str, minlen: int = 10) -> list:
    """Split text into sentence-like segments at pause punctuation, merging segments shorter than
    `minlen` into their neighbour (role of TextProcessor.cut_text, TextProcessor.py:18-59; the
    reference delegates sentence boundaries to pysbd, unavailable here)."""
    parts = [p for p in re.split(r"(?<=[。！？!?\.…;；\n])", text) if p and p.strip()]
    out, cur = [], ""
    for p in parts:
        cur += p
        if len(cur) >= minlen:
            out.append(cur)
            cur = ""
    if cur:
        if out:
            out[-1] += cur
        else:
            out.append(cur)
    return [s.strip() for s in out if s.strip()]


class _EngineLock:
    """One inference at a time per TTS (the reference's `_infer_lock`, TTS.py:145).  A streaming generator owns the
    engine -- KV cache, enc_p overlap state -- from its first chunk to its last, so the lock stays held across its
    yields; what must not happen is the SAME thread calling back in between two chunks and waiting for itself forever:
    that raises instead.  An abandoned generator releases the lock when it is closed or collected."""

    def __init__(self):
        self._lock = threading.Lock()
        self._owner = None

    def __enter__(self):
        me = threading.get_ident()
        if self._owner == me:
            raise RuntimeError("this TTS is in the middle of an infer_stream() on this thread: exhaust or close() the "
                               "generator before starting another inference")
        self._lock.acquire()
        self._owner = me
        return self

    def __exit__(self, *exc):
        self._owner = None
        self._lock.release()
        return False


class _TextLine:
    """One text of TTS.infer_stream_batched: the vocoder side of its stream, strictly sequential -- what TTS.infer_stream keeps in
    local variables and in `vq.enc_p.y_overlap`, per text."""

    def __init__(self, text, cuts, ge, overlap_samples, speed, noise_scale, cut_mute, generator, chain):
        self.text, self.cuts, self.ge, self.speed, self.noise_scale = text, cuts, ge, speed, noise_scale
        self.cut_mute, self.generator = cut_mute, generator
        self.segs = []                              # per segment: (phoneme ids [1, P] on the device, word2ph, norm_text)
        self.waiting = [[] for _ in cuts]           # per segment: (cumulative tokens, is_final) not decoded yet
        self.in_flight = []                         # (ChunkEmitter handle, frame -> phoneme path in pinned host memory or None, is_final, first of its segment)
        self.chain = chain                          # the text's own finish.StreamChain: its stages' states and its track's
        self.emitter = ChunkEmitter(overlap_samples, **chain.emitter_keywords())
        self.seg, self.final_issued = 0, False      # the segment being vocoded; its final chunk is in flight
        self.y_overlap, self.valid_start_idx, self.chunk_idx, self.last_subtitles_end, self.head_offset = None, 0, 0, 0, 0
        self.cur_text_l, self.last_end_s, self.audio_len_s = 0, 0, 0.0

    @property
    def done(self):
        return self.seg >= len(self.cuts)


class TTS:
    def __init__(self, gpt_cache=[(1, 512), (1, 768), (1, 1024), (4, 512), (4, 1024)], sovits_cache=[50, 55],
                 models_dir: str = None, device: str = None, dtype: str = None, use_flash_attn: bool = False,
                 use_bert: bool = False, auto_bert: bool = True, use_jieba_fast: bool = False,
                 always_load_cnhubert: bool = False, always_load_sv: bool = False):
        self.tts_config = Config()
        if device is not None:
            self.tts_config.device = torch.device(device)
        if dtype is not None:
            self.tts_config.dtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}.get(dtype.lower())
            if self.tts_config.dtype is None:
                raise ValueError("dtype must be float32 or bfloat16 on the MI355X path (float16 is not implemented)")
        if use_flash_attn:
            log.warning("use_flash_attn is ignored: the HIP decode kernel already reads only kv_len entries")
        self.tts_config.gpt_cache = list(gpt_cache)
        self.tts_config.sovits_cache = list(sovits_cache)
        self.models_dir = models_dir if models_dir is not None else Path.home() / ".cache" / "gsv"
        self.default_gpt_path = Path(self.models_dir) / "s1v3.ckpt"
        self.default_sovits_path = Path(self.models_dir) / "s2Gv2ProPlus.pth"
        self.cnhubert_path = Path(self.models_dir) / "chinese-hubert-base"
        self.always_load_cnhubert = always_load_cnhubert
        self.cnhubert_model = None
        self.sv_path = Path(self.models_dir) / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"
        self.always_load_sv = always_load_sv
        self.sv_model = None
        self.cnroberta_path = Path(self.models_dir) / "chinese-roberta-wwm-ext-large"
        self.auto_bert = auto_bert
        self._bert_loaded = False
        self._bert_missing_warned = False
        self.gpt_models: dict = {}
        self.sovits_models: dict = {}
        self.spk_audio_cache: dict = {}
        self.prompt_audio_cache: dict = {}
        self.samplerate, self.gpt_hz, self.sovits_hz = 32000, 25, 50
        self.audio_queue = None
        self._infer_lock = _EngineLock()
        self._text_frontend = None
        # multi-GPU (one process per GPU): the rank on which infer_batched returns the clips; the other ranks return None.
        # None = every rank gets every clip (an all-gather of the audio instead of point-to-point sends to one rank)
        self.gather_dst = 0
        if use_bert:
            self._ensure_bert_loaded(force=True)

    # ------------------------------------------------------------------ model management
    def load_gpt_model(self, *model_paths):
        for p in (model_paths or (self.default_gpt_path,)):
            self.gpt_models[p] = get_gpt_weights(p, self.tts_config)
            log.info("Loaded GPT model: %s", p)

    def load_sovits_model(self, *model_paths):
        for p in (model_paths or (self.default_sovits_path,)):
            self.sovits_models[p] = get_sovits_weights(p, self.tts_config)
            log.info("Loaded SoVITS model: %s", p)

    def unload_gpt_model(self, *model_paths):
        try:
            for p in model_paths:
                if self.gpt_models.pop(p, None) is None:
                    log.warning("GPT model %s not found.", p)
        finally:
            self._empty_cache()

    def unload_sovits_model(self, *model_paths):
        try:
            for p in model_paths:
                if self.sovits_models.pop(p, None) is None:
                    log.warning("SoVITS model %s not found.", p)
                for a in self.spk_audio_cache.values():
                    a["ge"].pop(p, None)
        finally:
            self._empty_cache()

    def to_safetensors(self, checkpoint_path: str, output_dir: str = None):
        """TTS.py:1482-1523: convert a .pth / .ckpt checkpoint to the safetensors directory form."""
        try:
            out = convert_to_safetensors(checkpoint_path, output_dir)
            log.info("Successfully converted and saved to: %s", out)
        finally:
            self._empty_cache()

    def get_gpt_list(self):
        return list(self.gpt_models.keys())

    def get_sovits_list(self):
        return list(self.sovits_models.keys())

    def _empty_cache(self):
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    # ------------------------------------------------------------------ front-of-hot-path inputs
    def set_text_frontend(self, fn):
        """fn(text) -> (phones2 list[int], word2ph dict, bert2 [P,1024] tensor, norm_text)"""
        self._text_frontend = fn

    def cache_spk_audio(self, spk_audio_paths, sovits_model=None, ge=None, audio=None, sv_emb=None, sample_rate=None):
        """TTS.py:1346-1389.  Either the finished embedding `ge` [1, gin, 1], or the reference waveform `audio`
        (mono fp32 at `sample_rate`, None: the model rate; resampled to the model rate on the device, what TTS._load_audio
        + _resample give), or neither when the key names an existing WAV or FLAC file, which is then read (wavio.load_wav, flacio.load_flac) and
        resampled to the model rate: then the spectrogram (TTS._get_spec) and get_ge run on the device.  v2Pro / v2ProPlus add the ERes2Net embedding sv_emb [1, 20480]: the one passed, else the
        one this path's cache entry holds, else ERes2NetV2 on the device (16 kHz resample + fbank + forward3) from
        models_dir/sv/pretrained_eres2netv2w24s4ep4.ckpt, kept loaded only when always_load_sv is set.  Without that
        checkpoint ge has no sv term (a warning says so).  The entry keeps the sv_emb, so another SoVITS model reuses it.

        A list of keys caches many speakers in one call (what the reference's cache_spk_audio(*paths) does): `audio` a list
        with one waveform per key, `ge` / `sv_emb` None or lists of the same length (None entries allowed).  ERes2NetV2 is
        loaded once and runs every clip that needs an sv_emb in one batched pass; each entry equals what a single-key call
        gives; `sample_rate` is then one rate for all or a list, and keys with neither audio nor ge that name WAV or FLAC files
        are read in one packed pass (wavio.load_wavs).  Any other key (a str, a tuple) is one key, as before."""
        if isinstance(spk_audio_paths, list):
            return self._cache_spk_batch(spk_audio_paths, sovits_model, ge, audio, sv_emb, sample_rate)
        sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
        entry = self.spk_audio_cache.get(spk_audio_paths)
        if ge is None:
            if audio is None:
                path = self._wav_file(spk_audio_paths)
                if path is None:
                    raise NotImplementedError("%r is no existing WAV file, and decoding / resampling audio files is outside "
                                              "this build's scope; pass ge=[1, gin, 1], or audio=<waveform> (+ sv_emb=[1, "
                                              "20480])" % (spk_audio_paths,))
                audio, sample_rate = self._read_files([path])[0]
            if sovits_model not in self.sovits_models:
                self.load_sovits_model(sovits_model)
            sovits = self.sovits_models[sovits_model]
            vq = sovits.vq_model
            audio = self._spk_wave(audio, sample_rate, self._model_rate(sovits))
            if sv_emb is None and getattr(vq, "is_v2pro", False):
                if entry is not None and entry.get("sv_emb") is not None:
                    sv_emb = entry["sv_emb"]
                elif os.path.isfile(self.sv_path):
                    sv_emb = self._sv_embed(audio, self._model_rate(sovits))
                else:
                    log.warning("ERes2NetV2 checkpoint %s not found: ge of %s has no speaker-verification term; pass "
                                "sv_emb=[1, 20480] or install the checkpoint", self.sv_path, spk_audio_paths)
            ge = vq.get_ge(vq.spectrogram(audio), sv_emb)
        entry = self.spk_audio_cache.setdefault(spk_audio_paths, {"ge": {}})
        entry["ge"][sovits_model] = ge.to(self.tts_config.device)
        if sv_emb is not None:
            entry["sv_emb"] = torch.as_tensor(sv_emb).to(self.tts_config.device).float().reshape(1, -1)

    @staticmethod
    def _per_key(v, n, name, one):
        """v for each of n keys: [v] * n when one(v) holds, else v as a list of n entries (ValueError otherwise)"""
        if one(v):
            return [v] * n
        if not isinstance(v, (list, tuple)):
            raise ValueError("%s must be a list with one entry per key (%d keys); got %s" % (name, n, type(v).__name__))
        if len(v) != n:
            raise ValueError("%s has %d entries for %d keys" % (name, len(v), n))
        return list(v)

    def _cache_spk_batch(self, keys, sovits_model, ge, audio, sv_emb, sample_rate):
        n = len(keys)
        ges = self._per_key(ge, n, "ge", lambda v: v is None)
        svs = self._per_key(sv_emb, n, "sv_emb", lambda v: v is None)
        auds = self._per_key(audio, n, "audio", lambda v: v is None)
        rates = self._per_key(sample_rate, n, "sample_rate", lambda v: v is None or isinstance(v, numbers.Integral))
        files = {}
        for i in range(n):
            if ges[i] is None and auds[i] is None:
                files[i] = self._wav_file(keys[i])
                if files[i] is None:
                    raise NotImplementedError("decoding / resampling audio files is outside this build's scope; key %d "
                                              "(%r) needs ge=[1, gin, 1] or audio=<waveform>, or to name an existing WAV "
                                              "file" % (i, keys[i]))
        sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
        todo = [i for i in range(n) if ges[i] is None]
        if todo:
            if files:
                for i, (w, sr) in zip(files, self._read_files(list(files.values()))):
                    auds[i], rates[i] = w, sr
            if sovits_model not in self.sovits_models:
                self.load_sovits_model(sovits_model)
            sovits = self.sovits_models[sovits_model]
            vq = sovits.vq_model
            wav = {i: self._spk_wave(auds[i], rates[i], self._model_rate(sovits)) for i in todo}
            if getattr(vq, "is_v2pro", False):
                need = []
                for i in todo:
                    entry = self.spk_audio_cache.get(keys[i])
                    if svs[i] is None and entry is not None and entry.get("sv_emb") is not None:
                        svs[i] = entry["sv_emb"]
                    elif svs[i] is None:
                        need.append(i)
                if need and os.path.isfile(self.sv_path):
                    e = self._sv_embed_batch([wav[i] for i in need], self._model_rate(sovits))
                    for j, i in enumerate(need):
                        svs[i] = e[j:j + 1]
                elif need:
                    log.warning("ERes2NetV2 checkpoint %s not found: ge of %s has no speaker-verification term; pass "
                                "sv_emb=[1, 20480] or install the checkpoint", self.sv_path, [keys[i] for i in need])
            for i in todo:
                ges[i] = vq.get_ge(vq.spectrogram(wav[i]), svs[i])
        for i, k in enumerate(keys):
            entry = self.spk_audio_cache.setdefault(k, {"ge": {}})
            entry["ge"][sovits_model] = ges[i].to(self.tts_config.device)
            if svs[i] is not None:
                entry["sv_emb"] = torch.as_tensor(svs[i]).to(self.tts_config.device).float().reshape(1, -1)

    @staticmethod
    def _wav_file(key):
        """key when it is a path (str or os.PathLike) naming an existing file, read as WAV; None for any other key"""
        return key if isinstance(key, (str, os.PathLike)) and os.path.isfile(key) else None

    def _read_files(self, paths):
        """TTS._load_audio of existing files -> [(fp32 mono on the device, the file's rate)], each at its own path's
        index.  A file that starts with the FLAC marker goes to flacio (frames decoded on the device), every other one
        to wavio as before (which names what it cannot read); all WAV files are read in one load_wavs and all FLAC files
        in one load_flacs, whatever order they come in."""
        from .flacio import load_flacs
        from .wavio import load_wavs
        flac = []
        for i, p in enumerate(paths):
            with open(p, "rb") as f:
                if f.read(4) == b"fLaC":
                    flac.append(i)
        wav = [i for i in range(len(paths)) if i not in set(flac)]
        res = [None] * len(paths)
        for idx, load in ((wav, load_wavs), (flac, load_flacs)):
            if idx:
                for i, r in zip(idx, load([paths[i] for i in idx], self.tts_config.device)):
                    res[i] = r
        return res

    def _spk_wave(self, audio, sample_rate, rate):
        """TTS._get_spec's waveform: audio at sample_rate (None: already at `rate`) -> fp32 [1, n] on the device at the
        model rate `rate` (sv.resample when the rates differ), then peak-normalised"""
        a = torch.as_tensor(audio).to(self.tts_config.device).float().reshape(1, -1)
        if sample_rate is not None and int(sample_rate) != rate:
            from .sv import resample
            a = resample(a, int(sample_rate), rate, self.tts_config.device).reshape(1, -1)
        peak = a.abs().max()
        if peak > 1:                       # TTS.py:1586-1588
            a = a / min(2, float(peak))
        return a

    @staticmethod
    def _model_rate(sovits) -> int:
        try:
            return int(sovits.hps.data.sampling_rate)
        except (AttributeError, KeyError, TypeError):
            return 32000

    def _sv_embed(self, audio, sample_rate):
        """ERes2Net.compute_embedding3 of a model-rate waveform (TTS._get_spec: resampled to 16 kHz), on the device"""
        from .sv import load_sv
        try:
            if self.sv_model is None:
                self.sv_model = load_sv(self.sv_path, self.tts_config.device)
            return self.sv_model.embed(audio, sample_rate)
        finally:
            if not self.always_load_sv:
                self.sv_model = None

    def _sv_embed_batch(self, wavs, sample_rate):
        """_sv_embed of every waveform in the list, one batched pass -> [n, 20480]"""
        from .sv import load_sv
        try:
            if self.sv_model is None:
                self.sv_model = load_sv(self.sv_path, self.tts_config.device)
            return self.sv_model.embed_batch(wavs, sample_rate)
        finally:
            if not self.always_load_sv:
                self.sv_model = None

    def verify_speaker(self, speaker1_audio, speaker2_audio) -> float:
        """TTS.py:1205-1245: cosine similarity (eps 1e-6) of two speakers' ERes2NetV2 embeddings.  Each argument is a
        cache_spk_audio key whose entry holds an sv_emb, a path that is no cached key and names an existing WAV or FLAC file (read
        and resampled to the model rate as cache_spk_audio does; nothing is cached), or a mono fp32 waveform at the model
        rate (that of the first loaded SoVITS model, 32 kHz when none is loaded), peak-normalised here as TTS._get_spec
        does."""
        rate = self._model_rate(next(iter(self.sovits_models.values()))) if self.sovits_models else 32000

        def emb(a):
            if isinstance(a, (str, Path)):
                path = None if a in self.spk_audio_cache else self._wav_file(a)
                if path is not None:
                    return self._sv_embed(self._spk_wave(*self._read_files([path])[0], rate), rate)
                e = self.spk_audio_cache.get(a, {}).get("sv_emb")
                if e is None:
                    raise NotImplementedError("decoding / resampling audio files is outside this build's scope; cache %r "
                                              "with cache_spk_audio(audio=...) first, or pass its waveform" % (a,))
                return e.to(self.tts_config.device).float().reshape(1, -1)
            return self._sv_embed(self._spk_wave(a, None, rate), rate)
        try:
            e1, e2 = emb(speaker1_audio), emb(speaker2_audio)
            return float(torch.cosine_similarity(e1, e2, dim=-1, eps=1e-6).item())
        finally:
            self._empty_cache()

    def cache_prompt_audio(self, prompt_audio_paths, prompt_audio_texts, prompt=None, phones1=None, bert1=None,
                           ssl_content=None, sovits_model=None, audio=None, sample_rate=16000):
        """TTS.py:1391-1440.  `prompt` int64 [1, Ly], or `ssl_content` [1, 768, Th] (CN-HuBERT last_hidden_state,
        transposed as in TTS._get_prompt), or `audio`, the prompt waveform as mono fp32 at 16 kHz ([n] or [1, n]): then
        CN-HuBERT (TTS._get_prompt: + 0.3 s of zeros) and extract_latent run on the device.  CN-HuBERT is loaded from
        models_dir/chinese-hubert-base on first use and kept only when always_load_cnhubert is set.  Audio at another
        `sample_rate` is first resampled to 16 kHz on the device (torchaudio Resample defaults, sv.resample).  With none of
        prompt / ssl_content / audio, a key that names an existing WAV or FLAC file is read (wavio.load_wav, flacio.load_flac) and takes that path at
        the file's rate; phones1 (and bert1) then come from the text frontend when not given, as the reference's
        get_phones_and_bert(prompt_audio_text) (TTS.py:1424).

        A list of keys caches many prompts in one call (the reference's list form): `audio` a list with one waveform per
        key, `prompt_audio_texts` one str for all or a list, `phones1` one list[int] for all or a list of them, `bert1`
        None or a list, `sample_rate` one int or a list.  A key whose audio is None (or every key, without audio) that
        names an existing WAV or FLAC file is read, all such files in one packed pass; when every key is read from a file,
        phones1 may be left out and comes from the text frontend.  CN-HuBERT is loaded once and runs every clip in one
        batched pass, then extract_latent runs per clip; each entry equals what a single-key call gives.  Lengths and
        empty texts are checked before any device work.  Any other key (a str, a tuple) is one key, as before."""
        if isinstance(prompt_audio_paths, list):
            return self._cache_prompt_batch(prompt_audio_paths, prompt_audio_texts, prompt, phones1, bert1, ssl_content,
                                            sovits_model, audio, sample_rate)
        if not prompt_audio_texts:
            raise ValueError("prompt_audio_text must not be empty")
        path = self._wav_file(prompt_audio_paths) if prompt is None and ssl_content is None and audio is None else None
        if path is not None:
            if phones1 is None and self._text_frontend is not None:      # TTS.py:1424
                phones1, _, fb, _ = self._phones_and_bert(prompt_audio_texts)
                bert1 = fb if bert1 is None else bert1
            audio, sample_rate = self._read_files([path])[0]
        if prompt is None and ssl_content is None and audio is not None:
            if int(sample_rate) != 16000:
                from .sv import resample
                audio = resample(audio, int(sample_rate), 16000, self.tts_config.device)
            ssl_content = self._cnhubert_ssl(audio)
        if prompt is None and ssl_content is not None:
            sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
            if sovits_model not in self.sovits_models:
                self.load_sovits_model(sovits_model)
            prompt = self.sovits_models[sovits_model].vq_model.extract_latent(ssl_content)[0, 0].unsqueeze(0)
        if prompt is None or phones1 is None:
            raise NotImplementedError("decoding / resampling audio files and G2P are outside this build's scope; pass "
                                      "prompt=int64[1,Ly], ssl_content=[1,768,Th] or audio=<mono fp32 16 kHz waveform>, and "
                                      "phones1=list[int] (and bert1=[Lx1,1024])")
        if bert1 is None:
            bert1 = torch.zeros(len(phones1), 1024)
        self.prompt_audio_cache[prompt_audio_paths] = {
            "prompt": prompt.to(self.tts_config.device), "phones1": list(phones1),
            "bert1": bert1.to(self.tts_config.device), "text": prompt_audio_texts}

    def _cnhubert_ssl(self, audio):
        """TTS._get_prompt's ssl_content from a 16 kHz waveform, on the device (hubert.py)"""
        from .hubert import load_cnhubert
        try:
            if self.cnhubert_model is None:
                self.cnhubert_model = load_cnhubert(self.cnhubert_path, self.tts_config.device)
            a = torch.as_tensor(audio)
            if a.dim() == 2 and a.shape[0] == 1:
                a = a[0]
            if a.dim() != 1:
                raise ValueError("audio must be one mono waveform at 16 kHz ([n] or [1, n]); resampling and channel mixing "
                                 "are outside this build's scope; got shape %s" % (tuple(a.shape),))
            return self.cnhubert_model.prompt_ssl(a)
        finally:
            if not self.always_load_cnhubert:
                self.cnhubert_model = None

    def _cache_prompt_batch(self, keys, texts, prompt, phones1, bert1, ssl_content, sovits_model, audio, sample_rate):
        n = len(keys)
        if prompt is not None or ssl_content is not None:
            raise ValueError("a list of keys takes audio=[one waveform per key]; prompt= / ssl_content= are single-key forms")
        texts = self._per_key(texts, n, "prompt_audio_texts", lambda v: isinstance(v, str))
        for i, t in enumerate(texts):
            if not t:
                raise ValueError("prompt_audio_texts[%d] must not be empty" % i)
        auds = self._per_key(audio, n, "audio", lambda v: v is None)
        files = {}
        for i in range(n):
            if auds[i] is None:
                files[i] = self._wav_file(keys[i])
                if files[i] is None and audio is None:
                    raise NotImplementedError("decoding / resampling audio files and G2P are outside this build's scope; a "
                                              "list of keys needs audio=[one mono fp32 waveform per key] and phones1, or "
                                              "keys that name existing WAV files")
                if files[i] is None:
                    raise NotImplementedError("decoding / resampling audio files is outside this build's scope; key %d (%r) "
                                              "needs audio=<waveform> or to name an existing WAV file" % (i, keys[i]))
        fronts = None
        if phones1 is None:
            if len(files) < n or self._text_frontend is None:
                raise NotImplementedError("G2P is outside this build's scope; pass phones1=list[int] or one list[int] per key")
            fronts = [self._phones_and_bert(t) for t in texts]        # TTS.py:1424
            phones1 = [f[0] for f in fronts]
        phones = self._per_key(phones1, n, "phones1",
                               lambda v: isinstance(v, (list, tuple)) and (not v or isinstance(v[0], numbers.Integral)))
        berts = self._per_key(bert1, n, "bert1", lambda v: v is None)
        if fronts is not None:
            berts = [f[2] if b is None else b for f, b in zip(fronts, berts)]
        rates = self._per_key(sample_rate, n, "sample_rate", lambda v: isinstance(v, numbers.Integral))
        if files:
            for i, (w, sr) in zip(files, self._read_files(list(files.values()))):
                auds[i], rates[i] = w, sr
        wavs = []
        for i, a in enumerate(auds):
            a = torch.as_tensor(a)
            if a.dim() == 2 and a.shape[0] == 1:
                a = a[0]
            if a.dim() != 1:
                raise ValueError("audio[%d] must be one mono waveform ([n] or [1, n]); resampling and channel mixing are "
                                 "outside this build's scope; got shape %s" % (i, tuple(a.shape)))
            wavs.append(a)
        for i, r in enumerate(rates):
            if int(r) != 16000:
                from .sv import resample
                wavs[i] = resample(wavs[i], int(r), 16000, self.tts_config.device)
        ssl = self._cnhubert_ssl_batch(wavs)
        sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
        if sovits_model not in self.sovits_models:
            self.load_sovits_model(sovits_model)
        vq = self.sovits_models[sovits_model].vq_model
        for i, k in enumerate(keys):
            p = vq.extract_latent(ssl[i])[0, 0].unsqueeze(0)
            b = berts[i] if berts[i] is not None else torch.zeros(len(phones[i]), 1024)
            self.prompt_audio_cache[k] = {
                "prompt": p.to(self.tts_config.device), "phones1": list(phones[i]),
                "bert1": b.to(self.tts_config.device), "text": texts[i]}

    def _cnhubert_ssl_batch(self, wavs):
        """_cnhubert_ssl of every 16 kHz waveform in the list, one batched pass (hubert.py)"""
        from .hubert import load_cnhubert
        try:
            if self.cnhubert_model is None:
                self.cnhubert_model = load_cnhubert(self.cnhubert_path, self.tts_config.device)
            return self.cnhubert_model.prompt_ssl_batch(wavs)
        finally:
            if not self.always_load_cnhubert:
                self.cnhubert_model = None

    def del_spk_audio(self, *spk_audio_list):
        """TTS.py:1436-1448"""
        for p in spk_audio_list:
            if self.spk_audio_cache.pop(p, None) is None:
                log.warning("Speaker audio %s not found in cache.", p)

    def del_prompt_audio(self, *prompt_audio_list):
        """TTS.py:1450-1462"""
        for p in prompt_audio_list:
            if self.prompt_audio_cache.pop(p, None) is None:
                log.warning("Prompt audio %s not found in cache.", p)

    def get_spk_audio_list(self):
        return list(self.spk_audio_cache.keys())

    def get_prompt_audio_list(self):
        return list(self.prompt_audio_cache.keys())

    def _pick(self, table, name, default):
        if name is None:
            name = next(iter(table)) if table else default
        return name

    def _phones_and_bert(self, text):
        if self._text_frontend is None:
            raise NotImplementedError("no text frontend installed: call set_text_frontend(fn); the reference's G2P stack "
                                      "(pypinyin/jieba/pyopenjtalk/...) is outside this build's scope")
        phones2, word2ph, bert2, norm_text = self._text_frontend(text)
        if not phones2:
            raise ValueError("text produced no phonemes")
        if bert2 is None:
            bert2 = torch.zeros(len(phones2), 1024)
        return list(phones2), word2ph, bert2.to(self.tts_config.device), norm_text

    @staticmethod
    def _contains_chinese(text: str) -> bool:
        """TTS.py:1525-1531 asks LangSegment for a "zh" segment; here any CJK ideograph counts (kanji-only Japanese too)"""
        return any(0x4E00 <= ord(c) <= 0x9FFF or 0x3400 <= ord(c) <= 0x4DBF or 0x20000 <= ord(c) <= 0x2FA1F or
                   0xF900 <= ord(c) <= 0xFAFF for c in text)

    def _ensure_bert_loaded(self, force: bool = False):
        """TTS.py:1533-1551: load Chinese RoBERTa once and set tts_config.cnroberta.  There is no download: without the
        directory one warning is logged and BERT features stay zeros, as before."""
        if self._bert_loaded or not (force or self.auto_bert):
            return
        if not os.path.isdir(self.cnroberta_path):
            if not self._bert_missing_warned:
                log.warning("Chinese RoBERTa directory %s not found: BERT features stay zeros; install "
                            "chinese-roberta-wwm-ext-large there to use them", self.cnroberta_path)
                self._bert_missing_warned = True
            return
        from .roberta import load_cnroberta
        self.tts_config.cnroberta = load_cnroberta(self.cnroberta_path, self.tts_config.device, self.tts_config.dtype)
        self._bert_loaded = True
        log.info("BERT model loaded for Chinese text")

    def _ge_for(self, spk_audio_path, sovits_model):
        def one(p):
            if p not in self.spk_audio_cache or sovits_model not in self.spk_audio_cache[p]["ge"]:
                self.cache_spk_audio(p, sovits_model=sovits_model)
            return self.spk_audio_cache[p]["ge"][sovits_model]
        if isinstance(spk_audio_path, dict):  # multi-speaker fusion, TTS.py:668-679
            total = sum(spk_audio_path.values())
            ge = None
            for p, wgt in spk_audio_path.items():
                g = one(p) * (wgt / total)
                ge = g if ge is None else ge + g
            return ge
        return one(spk_audio_path)

    def _prompt_for(self, path, text):
        if path not in self.prompt_audio_cache:
            self.cache_prompt_audio(path, text)
        c = self.prompt_audio_cache[path]
        return c["prompt"], c["phones1"], c["bert1"]

    # ------------------------------------------------------------------ multi-GPU (one process per GPU, engine.py)
    def _engine(self, t2s):
        """the continuous-batching engine of this process group, or None in a single process"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return None
        from .engine import ContinuousBatchingEngine, SpeakerBook
        if getattr(self, "_speaker_book", None) is None:
            self._speaker_book = SpeakerBook(self.tts_config.device)
        return ContinuousBatchingEngine(t2s, slots=max(t2s.cuda_graph_buckets), chunk=2)

    def _sync_speakers(self, prompt_paths, prompt_texts, spk_paths, sovits_model, src=0):
        """SPMD: every rank calls infer_batched with the same arguments; the reference-audio models ran on rank `src`
        only (cache_spk_audio / cache_prompt_audio there).  Each prompt / speaker key is broadcast once, ever."""
        import torch.distributed as dist
        book, me = self._speaker_book, dist.get_rank()
        dev = self.tts_config.device
        for p, text in dict(zip(prompt_paths, prompt_texts)).items():
            key = "prompt:%s" % p
            if key in book.entries:
                continue
            c = self.prompt_audio_cache.get(p) if me == src else None
            if me == src and c is None:
                self.cache_prompt_audio(p, text)
                c = self.prompt_audio_cache[p]
            got = book.sync(key, [c["prompt"], torch.tensor(c["phones1"], dtype=torch.int64, device=dev), c["bert1"]] if me == src else None, src=src)
            if me != src:
                self.prompt_audio_cache[p] = {"prompt": got[0], "phones1": got[1].tolist(), "bert1": got[2], "text": text}
        names = []
        for sp in spk_paths:
            names += list(sp.keys()) if isinstance(sp, dict) else [sp]
        for p in dict.fromkeys(names):
            key = "ge:%s:%s" % (sovits_model, p)
            if key in book.entries:
                continue
            if me == src and (p not in self.spk_audio_cache or sovits_model not in self.spk_audio_cache[p]["ge"]):
                self.cache_spk_audio(p, sovits_model=sovits_model)
            got = book.sync(key, [self.spk_audio_cache[p]["ge"][sovits_model]] if me == src else None, src=src)
            if me != src:
                self.spk_audio_cache.setdefault(p, {"ge": {}})["ge"][sovits_model] = got[0]

    # ------------------------------------------------------------------ trimming (TTS.py:1629-1664)
    @staticmethod
    def _rms_frames(x, frame=512, hop=256):
        if x.shape[0] < frame:
            return x.new_zeros(0)
        return x.unfold(0, frame, hop).pow(2).mean(dim=1).sqrt()

    def _find_head_threshold_offsets(self, audio, threshold=0.02, search_len=64000, margin=3200):
        head = audio[:search_len]
        idx = torch.nonzero(self._rms_frames(head) > threshold)
        return max(0, int(idx[0]) * 256 - margin) if idx.numel() else head.shape[0]

    def _find_tail_threshold_offsets(self, audio, threshold=0.01, search_len=64000, margin=3200):
        tail = audio[-search_len:]
        idx = torch.nonzero(self._rms_frames(tail) > threshold)
        return max(1, tail.shape[0] - int(idx[-1]) * 256 - margin) if idx.numel() else tail.shape[0]

    @staticmethod
    def _check_pause(text):
        return len(text) > 0 and text[-1] in PAUSE_MARKS

    def _close_subtitles(self, subtitles, word2ph, tail_s):
        """TTS.py:255-261 / 472-478 / 772-777: make the list end on a pause mark (a zero-length entry for the
        last word when it is not one) and let that last entry cover the trailing silence."""
        if not self._check_pause(subtitles[-1]["text"]):
            subtitles.append({"text": word2ph["word"][-1], "start_s": subtitles[-1]["end_s"], "end_s": subtitles[-1]["end_s"]})
        if tail_s is not None:
            subtitles[-1]["end_s"] += tail_s

    # ------------------------------------------------------------------ inference
    @torch.inference_mode()
    def infer(self, spk_audio_path, prompt_audio_path, prompt_audio_text, text, return_subtitles=False, top_k=15,
              top_p=1.0, temperature=1.0, repetition_penalty=1.35, noise_scale=0.5, speed=1.0, gpt_model=None,
              sovits_model=None, loudness=None, true_peak=None, eq=None, compress=None, ambience=None):
        """eq: None, a preset name ("voice": the three filters of the reference WebUI's enhance_audio) or an eq.EQ: the clip that
        would have been returned -- after the peak rule, trailing 0.2 s of zeros included -- goes through that equaliser on the
        device before the download (eq.py), ahead of loudness= and true_peak= as in the reference's chain; the clip
        then carries `eq`, the record with the peak before and after.  Nothing clamps that peak: true_peak= holds a ceiling.

        compress: None, a preset name ("voice": -18 dB, 3.5 : 1, 1 ms / 100 ms, the compressor of enhance_audio) or a
        compressor.Compressor: the clip goes through that compressor on the device (compressor.py) behind eq= and
        ahead of loudness= and true_peak=, the reference's order; the clip then carries `comp`, the record with the peaks, the
        smallest gain and whether the compressor acted.

        ambience: None, a preset name ("voice": room 0.1, damping 0.5, 3 % wet, 97 % dry, the reverb of enhance_audio) or a
        reverb.Reverb: the clip goes through that Freeverb on the device (reverb.py) behind compress= and ahead of
        loudness= and true_peak=, the reference's order; it keeps its length, and carries `ambience`, the record with the peak
        before and after.  Nothing clamps that peak (the preset's dry gain is 1.94): loudness= and true_peak= set the level.

        loudness: None, or a target in LUFS (-18.0 is the reference WebUI's): the clip that would have been returned -- after the
        peak rule, trailing 0.2 s of zeros included -- is measured and scaled to it on the device before the download
        (loudness.py); the clip then carries lufs (before the gain), gain and limited.

        true_peak: None, or a ceiling in dBTP <= 0 (-1.0 is EBU R128's): the clip that would have been returned is held under it
        by the look-ahead limiter on the device (limiter.py) and carries dbtp (its true peak behind the limiter) and
        limited (the limiter acted).  With loudness= as well the gain to the target is applied whatever the peak becomes, and the
        limiter then holds the ceiling: the loudness that comes out is what the limiter leaves."""
        chain = finish.resolve(self.samplerate, eq=eq, compress=compress, ambience=ambience, loudness=loudness, true_peak=true_peak)
        with self._infer_lock:
            try:
                if self._contains_chinese(text):
                    self._ensure_bert_loaded()
                if not self._check_pause(text):
                    text += "."
                gpt_model = self._pick(self.gpt_models, gpt_model, self.default_gpt_path)
                sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
                if gpt_model not in self.gpt_models:
                    self.load_gpt_model(gpt_model)
                if sovits_model not in self.sovits_models:
                    self.load_sovits_model(sovits_model)
                t2s = self.gpt_models[gpt_model].t2s_model
                vq = self.sovits_models[sovits_model].vq_model
                dev = self.tts_config.device
                ge = self._ge_for(spk_audio_path, sovits_model)
                prompt, phones1, bert1 = self._prompt_for(prompt_audio_path, prompt_audio_text)
                phones2, word2ph, bert2, norm_text = self._phones_and_bert(text)
                ids = torch.tensor(phones1 + phones2, dtype=torch.int64, device=dev).unsqueeze(0)
                bert = torch.cat([bert1, bert2]).unsqueeze(0)
                pred = t2s.infer(ids, prompt, bert, top_k=top_k, top_p=top_p, temperature=temperature,
                                 repetition_penalty=repetition_penalty)
                audio, attn = vq.decode(pred, torch.tensor(phones2, dtype=torch.int64, device=dev).unsqueeze(0), ge,
                                        noise_scale=noise_scale, speed=speed)
                audio = audio[0, 0, :]
                subtitles = []
                if return_subtitles:   # TTS.py:250-263 (the reference aligns even when nobody asked; only done on request here)
                    subtitles = sub.get_subtitles(word2ph, sub.viterbi_monotonic(attn), speed, sovits_hz=self.sovits_hz)
                    self._close_subtitles(subtitles, word2ph, 0.2)
                    subtitles = sub.sub2text_index(subtitles, norm_text, text)
                head_offset = self._find_head_threshold_offsets(audio)
                audio = audio[head_offset:]
                if subtitles:
                    sub.increment_subtitle_times(subtitles, -head_offset / self.samplerate)
                    subtitles[0]["start_s"] = max(0, subtitles[0]["start_s"])
                if finish.asked(chain):
                    audio, recs = finish.finish_clip(audio.float(), chain, self.samplerate)
                    return finish.with_records(AudioClip(self.audio_queue, audio, self.samplerate, len(audio) / self.samplerate, subtitles,
                                                         text), recs)
                audio = audio.float().cpu().numpy()
                peak = np.abs(audio).max() if audio.size else 0.0
                if peak > 1:
                    audio = audio / peak
                audio = np.concatenate([audio, np.zeros(int(0.2 * self.samplerate), dtype=audio.dtype)])
                return AudioClip(self.audio_queue, audio, self.samplerate, len(audio) / self.samplerate, subtitles, text)
            finally:
                self._empty_cache()

    @torch.inference_mode()
    def infer_vc(self, spk_audio_path, prompt_audio_path, prompt_audio_text, noise_scale=0.5, speed=1.0, sovits_model=None,
                 loudness=None, true_peak=None, eq=None, compress=None, ambience=None):
        """TTS.py:871-964, voice conversion: the prompt's own semantic tokens and phonemes go straight to the SoVITS
        decoder with the target speaker's `ge`; word timings always come back (the reference aligns unconditionally here).
        loudness, true_peak, eq, compress, ambience: as in infer."""
        chain = finish.resolve(self.samplerate, eq=eq, compress=compress, ambience=ambience, loudness=loudness, true_peak=true_peak)
        with self._infer_lock:
            try:
                if not self._check_pause(prompt_audio_text):
                    prompt_audio_text += "."
                sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
                if sovits_model not in self.sovits_models:
                    self.load_sovits_model(sovits_model)
                vq = self.sovits_models[sovits_model].vq_model
                dev = self.tts_config.device
                ge = self._ge_for(spk_audio_path, sovits_model)
                if prompt_audio_path not in self.prompt_audio_cache:
                    self.cache_prompt_audio(prompt_audio_path, prompt_audio_text)
                prompt = self.prompt_audio_cache[prompt_audio_path]["prompt"]
                phones, word2ph, _, norm_text = self._phones_and_bert(prompt_audio_text)
                audio, attn = vq.decode(prompt.unsqueeze(0), torch.tensor(phones, dtype=torch.int64, device=dev).unsqueeze(0), ge,
                                        noise_scale=noise_scale, speed=speed)
                if finish.asked(chain):
                    audio, recs = finish.finish_clip(audio[0, 0, :].float(), chain, self.samplerate)
                else:
                    audio = audio[0, 0, :].float().cpu().numpy()
                subtitles = sub.get_subtitles(word2ph, sub.viterbi_monotonic(attn), speed, sovits_hz=self.sovits_hz)
                self._close_subtitles(subtitles, word2ph, 0.2)
                subtitles = sub.sub2text_index(subtitles, norm_text, prompt_audio_text)
                if finish.asked(chain):
                    return finish.with_records(AudioClip(self.audio_queue, audio, self.samplerate, len(audio) / self.samplerate, subtitles,
                                                         prompt_audio_text), recs)
                peak = np.abs(audio).max() if audio.size else 0.0
                if peak > 1:
                    audio = audio / peak
                audio = np.concatenate([audio, np.zeros(int(0.2 * self.samplerate), dtype=audio.dtype)])
                return AudioClip(self.audio_queue, audio, self.samplerate, len(audio) / self.samplerate, subtitles, prompt_audio_text)
            finally:
                self._empty_cache()

    # ------------------------------------------------------------------ asyncio front (TTS.py:966-1262)
    # The reference's wrappers take the engine lock around the synchronous call inside an executor thread; here the
    # synchronous methods hold that (non-reentrant) lock themselves, so the wrappers only move the call off the loop.
    async def infer_async(self, *args, executor=None, **kwargs):
        import asyncio
        import functools
        return await asyncio.get_running_loop().run_in_executor(executor, functools.partial(self.infer, *args, **kwargs))

    async def infer_batched_async(self, *args, executor=None, **kwargs):
        import asyncio
        import functools
        return await asyncio.get_running_loop().run_in_executor(executor, functools.partial(self.infer_batched, *args, **kwargs))

    async def infer_stream_async(self, *args, executor=None, **kwargs):
        """async generator of AudioClip chunks: infer_stream runs in an executor thread and hands chunks over a queue"""
        import asyncio
        loop = asyncio.get_running_loop()
        queue = asyncio.Queue()
        failure = []

        def pump():
            try:
                for chunk in self.infer_stream(*args, **kwargs):
                    loop.call_soon_threadsafe(queue.put_nowait, chunk)
            except BaseException as exc:        # surfaced on the consumer side instead of dying in the worker
                failure.append(exc)
            finally:
                loop.call_soon_threadsafe(queue.put_nowait, None)
        loop.run_in_executor(executor, pump)
        while True:
            chunk = await queue.get()
            if chunk is None:
                break
            yield chunk
        if failure:
            raise failure[0]

    def _sola_algorithm(self, f1_overlap, f2, overlap_len, search_len: int = 320):
        """TTS.py:1612-1627, kept by name for callers of the reference's method: one library call (stream.sola -> gsv_sola)."""
        from .stream import sola
        out, k = sola(f1_overlap.reshape(-1)[-overlap_len:], f2.reshape(-1), search_len)
        return out.reshape(1, 1, -1), torch.tensor([[k]], device=f2.device)

    def infer_stream(self, spk_audio_path, prompt_audio_path, prompt_audio_text, text, return_subtitles=False,
                     is_cut_text=True, cut_minlen=10, cut_mute=0.4,
                     cut_mute_scale_map={"…": 2.0, ".": 1.5, "。": 1.5, "?": 1.5, "？": 1.5, "!": 1.5, "！": 1.5, ",": 1.0,
                                         "，": 1.0, ":": 1.0, "：": 1.0, ";": 1.0, "；": 1.0, "~": 1.0, "、": 0.8, "・": 0.8},
                     stream_mode="token", stream_chunk=25, overlap_len=5, boost_first_chunk=True, top_k=15, top_p=1.0,
                     temperature=1.0, repetition_penalty=1.35, noise_scale=0.5, speed=1.0, gpt_model=None,
                     sovits_model=None, debug=True, track=None, loudness=None, loudness_seed=None, true_peak=None, eq=None,
                     compress=None):
        """TTS.py:289-504: generator of AudioClip chunks.  Per text segment the GPT streams cumulative token
        chunks (t2s.infer_stream); every chunk is decoded from the start of the segment with
        decode(stream_mode=True) -- only frames past `valid_start_idx` reach the flow / Generator -- and joined
        to the previous one by SOLA over `overlap_len` frames.

        track: a track.TrackFormat, or None.  With one, every clip also carries `pcm` -- int16 [k, packet * channels], the whole
        packets of a real-time track at `pcm_rate` that its samples completed (k may be 0) --: one resampler state spans the
        text, its segments and the mutes between them, and the text's final clip flushes it.  The concatenated `pcm` is
        AudioClip.to_pcm16 of the concatenated audio_data, bit for bit.  Nothing else about the clips changes.

        loudness: None, or a target in LUFS: the text's audio -- its segments and the mutes between them, one stream -- goes through
        a running BS.1770 gain on the device (level.StreamLeveller) before it is handed out and before the track's
        resampler: the concatenated audio_data is level.level() of the concatenated unlevelled clips, bit for bit.  Each clip then
        carries lufs (the running loudness of the UNLEVELLED stream at its end), gain (of its last sample) and limited (a sample of
        the stream so far was set to the peak limit).  loudness_seed: the last `lufs` of the same voice, to start at the right gain
        instead of converging to it (None, or the -inf of a clip without a measurement: no seed); nothing is remembered between
        calls.

        true_peak: None, or a ceiling in dBTP <= 0: the text's audio -- one stream, as for loudness= -- goes through the stream
        limiter on the device (limiter.StreamLimiter) behind the leveller and before the track's resampler: the
        concatenated audio_data is limiter.limit_stream() of the concatenated unlimited clips, bit for bit, and `pcm` is made from
        it.  The limiter looks ahead, so it hands samples out D = look-ahead + 5 samples late (53 samples, 1.66 ms at 32 kHz): the
        number and order of the clips stay, the text's first clip is D samples shorter and its final clip, which flushes the
        limiter, D longer; a chunk shorter than D gives a clip with empty audio_data.  audio_len_s counts the samples handed out.
        Subtitle times are unchanged: the audio runs D / samplerate late against them.  Each clip carries limited (the limiter has
        acted on the stream so far), dbtp_in (the highest true peak of the unlimited stream so far) and gain_min (the smallest gain
        among its samples), and no dbtp: there is no trim and the output's true peak is not measured; 4.23 states by how much it
        can pass the ceiling.  With loudness= as well the leveller's own peak limit is off and the limiter holds the ceiling, as
        for clips.

        eq: None, a preset name ("voice") or an eq.EQ: the text's audio -- one stream, as for loudness= -- goes through the stream
        equaliser on the device (eq.StreamEQ) first of all, ahead of the leveller and the limiter as on the clip path:
        the concatenated audio_data is eq.equalise() of the concatenated unequalised clips, bit for bit, and the leveller measures
        equalised audio.  An equaliser is causal: no delay, the clips keep their lengths.  Each clip carries `eq`, the
        eq.EqStreamRecord: the peaks before and after of its samples and of the stream so far, which nothing clamps (peak_out_run
        may exceed 1.0; true_peak= holds a ceiling), and `total`, the stream's samples so far.  An EQ that is the identity is as
        no EQ.

        compress: None, a preset name ("voice") or a compressor.Compressor: the text's audio -- one stream, as for loudness= -- goes
        through the stream compressor on the device (compressor.StreamCompressor) behind the equaliser and ahead of
        the leveller and the limiter, the clip path's order (eq -> compress -> level -> limit -> track): the concatenated
        audio_data is compressor.compress() of the concatenated uncompressed clips, bit for bit.  The compressor is causal: no
        delay, the clips keep their lengths.  Each clip carries `comp`, the compressor.CmpStreamRecord: the peaks before and after
        and the smallest gain of its samples and of the stream so far, and `total`, the stream's samples so far.  A compressor
        that is the identity is as none."""
        chain = finish.resolve(self.samplerate, eq=eq, compress=compress, loudness=loudness, loudness_seed=loudness_seed, true_peak=true_peak)
        with self._infer_lock:
            try:
                if self._contains_chinese(text):
                    self._ensure_bert_loaded()
                if not self._check_pause(text):
                    text += "."
                if stream_mode == "sentence":
                    stream_chunk = 10000
                if not is_cut_text:
                    cut_minlen = 10000
                cut_mute = cut_mute / speed
                gpt_model = self._pick(self.gpt_models, gpt_model, self.default_gpt_path)
                sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
                if gpt_model not in self.gpt_models:
                    self.load_gpt_model(gpt_model)
                if sovits_model not in self.sovits_models:
                    self.load_sovits_model(sovits_model)
                t2s = self.gpt_models[gpt_model].t2s_model
                vq = self.sovits_models[sovits_model].vq_model
                dev = self.tts_config.device
                ge = self._ge_for(spk_audio_path, sovits_model)
                prompt, phones1, bert1 = self._prompt_for(prompt_audio_path, prompt_audio_text)
                overlap_samples = overlap_len * vq.samples_per_frame
                audio_len_s, cur_text_l, last_end_s = 0.0, 0, 0
                cuts = cut_text(text, cut_minlen)
                stages = finish.StreamChain(chain, self.samplerate, dev, track)
                for i, text_cut in enumerate(cuts):
                    phones2, word2ph, bert2, norm_text = self._phones_and_bert(text_cut)
                    ids = torch.tensor(phones1 + phones2, dtype=torch.int64, device=dev).unsqueeze(0)
                    bert = torch.cat([bert1, bert2]).unsqueeze(0)
                    phones2_t = torch.tensor(phones2, dtype=torch.int64, device=dev).unsqueeze(0)
                    splicer, valid_start_idx, chunk_idx, last_subtitles_end = ChunkSplicer(overlap_samples), 0, 0, 0
                    for pred, is_final in t2s.infer_stream(ids, prompt, bert, top_k=top_k, top_p=top_p, temperature=temperature,
                                                           repetition_penalty=repetition_penalty, stream_chunk=stream_chunk,
                                                           boost_first_chunk=boost_first_chunk if i == 0 else False, debug=debug):
                        with torch.inference_mode():
                            audio, attn = vq.decode(pred, phones2_t, ge, noise_scale=noise_scale, speed=speed, stream_mode=True,
                                                    valid_start_idx=valid_start_idx, overlap_len=overlap_len)
                            audio = splicer.push(audio, is_final)     # aligned to the previous chunk's tail, its own tail kept back
                            if not is_final:
                                attn = attn[:, :-overlap_len, :]
                                valid_start_idx = attn.shape[1]
                            subtitles = []
                            if return_subtitles:   # TTS.py:444-451: a chunk whose path is mostly single frames is not trusted yet
                                assign = sub.viterbi_monotonic(attn)
                                if is_final or sub.is_normal_assign(assign):
                                    subtitles = sub.get_subtitles(word2ph, assign, speed, last_end_s=last_end_s, sovits_hz=self.sovits_hz)
                            if chunk_idx == 0:
                                head_offset = self._find_head_threshold_offsets(audio)
                                audio = audio[head_offset:]
                            if subtitles:
                                sub.increment_subtitle_times(subtitles, -head_offset / self.samplerate)
                                subtitles[0]["start_s"] = max(last_end_s, subtitles[0]["start_s"])
                            if is_final:
                                if text_cut[-1] in cut_mute_scale_map:
                                    scale = cut_mute_scale_map[text_cut[-1]]
                                elif "…" in cut_mute_scale_map and text_cut[-3:] in ["...", "。。。"]:
                                    scale = cut_mute_scale_map["…"]
                                else:
                                    scale = 1.0
                                audio = torch.cat([audio, torch.zeros(int(cut_mute * scale * self.samplerate), dtype=audio.dtype, device=audio.device)])
                                if subtitles:
                                    self._close_subtitles(subtitles, word2ph, cut_mute * scale)
                                    last_end_s = subtitles[-1]["end_s"]
                            new_subtitles = []
                            if subtitles:   # TTS.py:481-486: chunks are cumulative, hand out what is new; the last word stays open
                                subtitles = sub.sub2text_index(subtitles, norm_text, text_cut)
                                sub.increment_subtitle_indices(subtitles, cur_text_l)
                                new_subtitles = subtitles[last_subtitles_end:]
                                last_subtitles_end = len(subtitles) - 1
                                if not is_final and new_subtitles:
                                    new_subtitles[-1]["end_s"] = None
                            audio = stages.push_tensor(audio, flush=is_final and i == len(cuts) - 1)
                            audio = audio.float().cpu().numpy()
                        audio_len_s += len(audio) / self.samplerate
                        yield stages.attach(AudioClip(self.audio_queue, audio, self.samplerate, audio_len_s, new_subtitles, text))
                        chunk_idx += 1
                    vq.enc_p.y_overlap = None
                    cur_text_l += len(text_cut)
            finally:
                try:   # an abandoned stream must not leave its cross-fade state to the next one (other speed -> other shape)
                    self.sovits_models[sovits_model].vq_model.enc_p.y_overlap = None
                except Exception:
                    pass
                self._empty_cache()

    def infer_stream_batched(self, spk_audio_paths, prompt_audio_paths, prompt_audio_texts, texts, return_subtitles=False,
                             is_cut_text=True, cut_minlen=10, cut_mute=0.4,
                             cut_mute_scale_map={"…": 2.0, ".": 1.5, "。": 1.5, "?": 1.5, "？": 1.5, "!": 1.5, "！": 1.5,
                                                 ",": 1.0, "，": 1.0, ":": 1.0, "：": 1.0, ";": 1.0, "；": 1.0, "~": 1.0,
                                                 "、": 0.8, "・": 0.8},
                             stream_mode="token", stream_chunk=25, overlap_len=5, boost_first_chunk=True, top_k=15, top_p=1.0,
                             temperature=1.0, repetition_penalty=1.35, noise_scale=0.5, speed=1.0, gpt_model=None,
                             sovits_model=None, debug=True, slots=None, seed=None, track=None, loudness=None, loudness_seed=None,
                             true_peak=None, eq=None, compress=None):
        """`infer_stream` for many texts at once: a generator of (text index, AudioClip).  Per text the clips are the ones
        `infer_stream` yields for that text -- audio, audio_len_s, subtitles, in that order (equal bit for bit for greedy fp32
        requests that end with an EOS and noise_scale 0) --; texts interleave as their chunks become ready.

        Every segment `cut_text` makes of every text is a request of the continuous-batching slots
        (Text2SemanticDecoder.infer_stream_batched), queued as segment 0 of each text, then segment 1, ...; `slots` names the
        slot family (default: the smallest that holds them, else the largest).  The vocoder side of a text is sequential: its
        chunks are decoded in order with the text's own overlap state, a later segment's chunks wait as token tensors until the
        final clip of the segment before has been handed out.  What follows a chunk's decode runs on the device
        (stream.ChunkEmitter); the samples -- and with return_subtitles the frame-to-phoneme path -- reach the host by an
        asynchronous copy into pinned memory that is polled behind every window, so the
        loop waits for nothing but the slots' own read-back while a slot is live.

        top_k / top_p / temperature / seed / speed / noise_scale: one value or one per text.  With a seed, a text's vocoder noise
        is drawn from a generator seeded with it: the text's audio does not depend on its neighbours.  The speaker and the
        prompt are broadcast as in `infer_batched`.  Not available under a multi-rank engine.

        track: as in `infer_stream`; every text has its own resampler state, and its push is enqueued behind the chunk's epilogue
        with the chunk's length read on the device, so the loop still waits for nothing.

        loudness / loudness_seed: as in `infer_stream`, one value or one per text, None allowed per text (a wrong length raises
        ValueError).  Every text with a value has its own leveller, enqueued between the chunk's epilogue and the track's push, in
        place with the chunk's length read on the device: the loop still waits for nothing, a text's audio does not depend on its
        neighbours, and a text without a value gets the clips it gets today.

        true_peak: as in `infer_stream`, one value or one per text, None allowed per text (a wrong length raises ValueError).
        Every text with a value has its own limiter, enqueued behind the leveller and in front of the track's push, which then
        reads its length from the limiter's record on the device: the loop still waits for nothing.

        eq: as in `infer_stream`, None, a preset name or an eq.EQ for every text, or a list with one of those per TEXT (a wrong
        length raises ValueError; a bare list of eq.Band objects is not an equaliser: wrap it in eq.EQ).  Every text with one has
        its own equaliser state, enqueued directly behind the chunk's epilogue, in place and in front of the leveller, with the
        chunk's length read on the device: the loop still waits for nothing, and a text with None gets the clips it gets today.

        compress: as in `infer_stream`, None, a preset name or a compressor.Compressor for every text, or a list with one of those
        per TEXT (a wrong length raises ValueError).  Every text with one has its own compressor state, enqueued behind the
        equaliser and in front of the leveller, in place, with the chunk's length read on the device from the stage in front: the
        loop still waits for nothing, and a text with None gets the clips it gets today."""
        with self._infer_lock:
            vq, gen = None, None
            try:
                if isinstance(texts, str):
                    texts = [texts]
                n = len(texts)
                if n == 0:
                    return
                chains = finish.resolve(self.samplerate, n, eq=eq, compress=compress, loudness=loudness, loudness_seed=loudness_seed,
                                        true_peak=true_peak)
                speed = slot_sampling.per_request("speed", speed, n)
                noise_scale = slot_sampling.per_request("noise_scale", noise_scale, n)
                if not all(s > 0 for s in speed):
                    raise ValueError("speed must be positive, got %r" % (speed,))
                if any(self._contains_chinese(t) for t in texts):
                    self._ensure_bert_loaded()
                texts = [t if self._check_pause(t) else t + "." for t in texts]
                if stream_mode == "sentence":
                    stream_chunk = 10000
                if not is_cut_text:
                    cut_minlen = 10000
                bc = lambda v, kinds: [v] * n if isinstance(v, kinds) else list(v)
                spk_audio_paths = bc(spk_audio_paths, (str, dict))
                prompt_audio_paths = bc(prompt_audio_paths, str)
                prompt_audio_texts = bc(prompt_audio_texts, str)
                gpt_model = self._pick(self.gpt_models, gpt_model, self.default_gpt_path)
                sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
                if gpt_model not in self.gpt_models:
                    self.load_gpt_model(gpt_model)
                if sovits_model not in self.sovits_models:
                    self.load_sovits_model(sovits_model)
                t2s = self.gpt_models[gpt_model].t2s_model
                vq = self.sovits_models[sovits_model].vq_model
                if self._engine(t2s) is not None:
                    raise NotImplementedError("infer_stream_batched runs in a single process: multi-GPU streaming is not built")
                dev = self.tts_config.device
                seeds = slot_sampling.per_request("seed", seed, n)
                lines = []
                for t, text in enumerate(texts):
                    gen_t = None if seeds[t] is None else torch.Generator().manual_seed(int(seeds[t]))
                    lines.append(_TextLine(text, cut_text(text, cut_minlen), self._ge_for(spk_audio_paths[t], sovits_model),
                                           overlap_len * vq.samples_per_frame, speed[t], noise_scale[t], cut_mute / speed[t], gen_t,
                                           finish.StreamChain(finish.chain_of(chains, t), self.samplerate, dev, track)))
                # the queue: segment 0 of every text, then segment 1, ...
                req = [(t, j) for j in range(max(len(ln.cuts) for ln in lines)) for t, ln in enumerate(lines) if j < len(ln.cuts)]
                seg2orig = [t for t, _ in req]
                ids, prompts, berts = [], [], []
                for t, j in req:
                    phones2, word2ph, bert2, norm_text = self._phones_and_bert(lines[t].cuts[j])
                    prompt, ph1, b1 = self._prompt_for(prompt_audio_paths[t], prompt_audio_texts[t])
                    ids.append(torch.tensor(ph1 + phones2, dtype=torch.int64, device=dev))
                    prompts.append(prompt.squeeze(0))
                    berts.append(torch.cat([b1, bert2]))
                    lines[t].segs.append((torch.tensor(phones2, dtype=torch.int64, device=dev).unsqueeze(0), word2ph, norm_text))
                sampling = {k: slot_sampling.per_segment(k, v, n, seg2orig) for k, v in
                            (("top_k", top_k), ("top_p", top_p), ("temperature", temperature), ("seed", seed),
                             ("repetition_penalty", repetition_penalty))}
                boost = slot_sampling.per_request("boost_first_chunk", boost_first_chunk, n)
                gen = t2s.infer_stream_batched(ids, prompts, berts, stream_chunk=stream_chunk,
                                               boost_first_chunk=[bool(boost[t]) and j == 0 for t, j in req], slots=slots,
                                               ticks=True, **sampling)
                mute = lambda ln, cut: self._stream_mute(ln.cut_mute, cut, cut_mute_scale_map)
                for r, pred, is_final in gen:       # one turn per window of the slot loop
                    if r is not None:
                        t, j = req[r]
                        lines[t].waiting[j].append((pred, is_final))
                    for t, ln in enumerate(lines):
                        self._stream_decode(ln, vq, overlap_len, return_subtitles, mute)
                        while ln.in_flight and ln.in_flight[0][0].ready():
                            yield t, self._stream_clip(ln, mute)
                gen = None
                while any(not ln.done for ln in lines):      # no slot is live: what is left is waited for, text by text in turn
                    moved = False
                    for t, ln in enumerate(lines):
                        self._stream_decode(ln, vq, overlap_len, return_subtitles, mute)
                        if ln.in_flight:
                            moved = True
                            yield t, self._stream_clip(ln, mute)
                    if not moved:
                        raise RuntimeError("infer_stream_batched: a segment ended without its final chunk")
            finally:
                if gen is not None:
                    gen.close()         # waits for the refill stream, parks the slots
                if vq is not None and vq.enc_p is not None:
                    vq.enc_p.y_overlap = None
                self._empty_cache()

    def _stream_mute(self, cut_mute, text_cut, scale_map):
        """seconds of silence behind a segment's final chunk (TTS.py:456-462)"""
        if text_cut[-1] in scale_map:
            return cut_mute * scale_map[text_cut[-1]]
        if "…" in scale_map and text_cut[-3:] in ["...", "。。。"]:
            return cut_mute * scale_map["…"]
        return cut_mute * 1.0

    def _stream_decode(self, ln, vq, overlap_len, return_subtitles, mute):
        """enqueue the vocoder pass and the epilogue of every chunk of the text's current segment that has its tokens"""
        while not ln.done and ln.waiting[ln.seg] and not ln.final_issued:
            pred, is_final = ln.waiting[ln.seg].pop(0)
            phones2_t = ln.segs[ln.seg][0]
            with torch.inference_mode():
                vq.enc_p.y_overlap = ln.y_overlap       # the text's own cross-fade state goes through the holder decode() reads
                try:
                    audio, attn = vq.decode(pred, phones2_t, ln.ge, noise_scale=ln.noise_scale, speed=ln.speed, stream_mode=True,
                                            valid_start_idx=ln.valid_start_idx, overlap_len=overlap_len, generator=ln.generator)
                    ln.y_overlap = vq.enc_p.y_overlap
                finally:
                    vq.enc_p.y_overlap = None
                if not is_final:
                    attn = attn[:, :-overlap_len, :]
                    ln.valid_start_idx = attn.shape[1]
                assign = None
                if return_subtitles:
                    # the frame -> phoneme path goes to the host the way the samples go: an asynchronous copy into pinned memory,
                    # queued in front of the emitter's copy on the same stream, so the handle's event covers both
                    path = sub.viterbi_monotonic(attn)
                    assign = torch.empty(path.shape, dtype=path.dtype, pin_memory=True)
                    assign.copy_(path, non_blocking=True)
                first = ln.chunk_idx == 0
                if first:
                    ln.emitter.new_segment()
                n_mute = int(mute(ln, ln.cuts[ln.seg]) * self.samplerate) if is_final else 0
                handle = ln.emitter.push(audio, is_final, trim_head=first, mute_samples=n_mute,
                                         flush=is_final and ln.seg == len(ln.cuts) - 1)
            ln.in_flight.append((handle, assign, is_final, first))
            ln.chunk_idx += 1
            ln.final_issued = is_final

    def _stream_clip(self, ln, mute):
        """the oldest chunk in flight of a text as its AudioClip (waits for its copy): the host rules of infer_stream behind the
        samples -- subtitles, audio_len_s -- with the head offset the device chose.  `assign` is on the host by then (its copy was
        queued before the samples'), so nothing here reads the device"""
        handle, assign, is_final, first = ln.in_flight.pop(0)
        audio, _, head = handle.result()[:3]
        if first:
            ln.head_offset = head
        text_cut = ln.cuts[ln.seg]
        _, word2ph, norm_text = ln.segs[ln.seg]
        subtitles = []
        if assign is not None and (is_final or sub.is_normal_assign(assign)):
            subtitles = sub.get_subtitles(word2ph, assign, ln.speed, last_end_s=ln.last_end_s, sovits_hz=self.sovits_hz)
        if subtitles:
            sub.increment_subtitle_times(subtitles, -ln.head_offset / self.samplerate)
            subtitles[0]["start_s"] = max(ln.last_end_s, subtitles[0]["start_s"])
        if is_final and subtitles:
            self._close_subtitles(subtitles, word2ph, mute(ln, text_cut))
            ln.last_end_s = subtitles[-1]["end_s"]
        new_subtitles = []
        if subtitles:
            subtitles = sub.sub2text_index(subtitles, norm_text, text_cut)
            sub.increment_subtitle_indices(subtitles, ln.cur_text_l)
            new_subtitles = subtitles[ln.last_subtitles_end:]
            ln.last_subtitles_end = len(subtitles) - 1
            if not is_final and new_subtitles:
                new_subtitles[-1]["end_s"] = None
        ln.audio_len_s += len(audio) / self.samplerate
        if is_final:        # the next segment starts clean (TTS.py:498): its chunks may be decoded from now on
            ln.cur_text_l += len(text_cut)
            ln.seg, ln.y_overlap, ln.valid_start_idx, ln.chunk_idx, ln.last_subtitles_end = ln.seg + 1, None, 0, 0, 0
            ln.final_issued = False
        return ln.chain.attach(AudioClip(self.audio_queue, audio, self.samplerate, ln.audio_len_s, new_subtitles, ln.text), handle)

    async def infer_stream_batched_async(self, *args, executor=None, **kwargs):
        """async generator of (text index, AudioClip): infer_stream_batched in an executor thread, handed over a queue"""
        import asyncio
        loop = asyncio.get_running_loop()
        queue = asyncio.Queue()
        failure = []

        def pump():
            try:
                for item in self.infer_stream_batched(*args, **kwargs):
                    loop.call_soon_threadsafe(queue.put_nowait, item)
            except BaseException as exc:
                failure.append(exc)
            finally:
                loop.call_soon_threadsafe(queue.put_nowait, None)
        loop.run_in_executor(executor, pump)
        while True:
            item = await queue.get()
            if item is None:
                break
            yield item
        if failure:
            raise failure[0]

    @torch.inference_mode()
    def infer_batched(self, spk_audio_paths, prompt_audio_paths, prompt_audio_texts, texts, return_subtitles=False,
                      is_cut_text=True, cut_minlen=10, cut_mute=0.4,
                      cut_mute_scale_map={"…": 2.0, ".": 1.5, "。": 1.5, "?": 1.5, "？": 1.5, "!": 1.5, "！": 1.5,
                                          ",": 1.0, "，": 1.0, ":": 1.0, "：": 1.0, ";": 1.0, "；": 1.0, "~": 1.0,
                                          "、": 0.8, "・": 0.8},
                      top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, noise_scale=0.5, speed=1.0,
                      bert_batch_size=20, sovits_batch_size=10, gpt_model=None, sovits_model=None, seed=None,
                      initial_suppression_steps=0, loudness=None, true_peak=None, eq=None, compress=None, ambience=None):
        """top_k / top_p / temperature / seed: one value for the call, or one per TEXT (the segments `cut_text` makes of a text
        inherit its values); see Text2SemanticDecoder.infer_batched.

        repetition_penalty: a NUMBER is ignored, as in the reference's batched loop; a sequence with one value per TEXT is
        applied to that text's segments as `infer` applies it (`[1.35] * len(texts)` for every text).  initial_suppression_steps:
        0 (none, the reference's batched behaviour), an int for the call, or one per TEXT: `infer`'s start rule for those
        segments.  A sequence of the wrong length raises ValueError.

        speed / noise_scale: a number for the call -- the reference's path: each vocoder batch is resampled as one signal
        and cut with `split_bounds` -- or a sequence with one value per TEXT (a wrong length raises ValueError).  With a
        sequence for either, every segment is resampled on its own to its text's speed and gets its own noise stream
        (SynthesizerTrn.decode_segments: no frame blends two utterances), the clips are cut at exact frame boundaries, the
        mute after a segment is cut_mute / speed of its text, and return_subtitles aligns each segment on its own block of
        the attention with its own speed; the last entry of a segment ends where that segment's audio ends.  A vocoder
        batch then holds at most 64 segments (sovits_batch_size is capped there).

        loudness: None, a target in LUFS for every text, or one value or None per TEXT (a wrong length raises ValueError).  The
        finished clips -- mutes between segments included -- of the texts with a value are measured and scaled in ONE packed
        gsv_loudness call (loudness.py), on the gathering rank under a multi-rank engine; those clips carry lufs,
        gain and limited.  A text with None comes back exactly as without the parameter.

        true_peak: None, a ceiling in dBTP <= 0 for every text, or one value or None per TEXT (a wrong length raises ValueError).
        The finished clips of the texts with a value -- behind the gain to their loudness target, which is then applied whatever
        the peak becomes -- are held under it in ONE packed gsv_limiter call (limiter.py) and carry dbtp and
        limited, as in infer.

        eq: None, a preset name or an eq.EQ for every text, or a list with one of those per TEXT (a wrong length raises
        ValueError; a bare list of eq.Band objects is not an equaliser: wrap it in eq.EQ).  The finished clips of the texts with
        one go through their equalisers in ONE packed gsv_eq call (eq.py) ahead of the loudness call, the distinct
        designs passed once, and carry `eq`, as in infer.  A text with None comes back exactly as without the parameter.

        compress: None, a preset name or a compressor.Compressor for every text, or a list with one of those per TEXT (a wrong
        length raises ValueError).  The finished clips of the texts with one go through their compressors in ONE packed
        gsv_compressor call (compressor.py) behind the equaliser call and ahead of the loudness call, the distinct
        parameter sets passed once, and carry `comp`, as in infer.  A text with None comes back exactly as without the parameter.

        ambience: None, a preset name or a reverb.Reverb for every text, or a list with one of those per TEXT (a wrong length
        raises ValueError).  The finished clips of the texts with one go through their reverbs in ONE packed gsv_reverb call
        (reverb.py) behind the compressor call and ahead of the loudness call, the distinct parameter sets passed
        once, and carry `ambience`, as in infer.  A text with None comes back exactly as without the parameter."""
        with self._infer_lock:
            try:
                if isinstance(texts, str):
                    texts = [texts]
                chains = finish.resolve(self.samplerate, len(texts), eq=eq, compress=compress, ambience=ambience, loudness=loudness,
                                        true_peak=true_peak)
                segmented = slot_sampling.is_sequence(speed) or slot_sampling.is_sequence(noise_scale)
                if segmented:   # one value per text: the lengths are checked before any device work
                    speed = slot_sampling.per_request("speed", speed, len(texts))
                    noise_scale = slot_sampling.per_request("noise_scale", noise_scale, len(texts))
                    if not all(s > 0 for s in speed):
                        raise ValueError("speed must be positive, got %r" % (speed,))
                if any(self._contains_chinese(t) for t in texts):
                    self._ensure_bert_loaded()
                texts = [t if self._check_pause(t) else t + "." for t in texts]
                if not is_cut_text:
                    cut_minlen = 10000
                cut_mute = [cut_mute / s for s in speed] if segmented else cut_mute / speed
                n = len(texts)
                bc = lambda v, kinds: [v] * n if isinstance(v, kinds) else list(v)
                spk_audio_paths = bc(spk_audio_paths, (str, dict))
                prompt_audio_paths = bc(prompt_audio_paths, str)
                prompt_audio_texts = bc(prompt_audio_texts, str)
                gpt_model = self._pick(self.gpt_models, gpt_model, self.default_gpt_path)
                sovits_model = self._pick(self.sovits_models, sovits_model, self.default_sovits_path)
                if gpt_model not in self.gpt_models:
                    self.load_gpt_model(gpt_model)
                if sovits_model not in self.sovits_models:
                    self.load_sovits_model(sovits_model)
                t2s = self.gpt_models[gpt_model].t2s_model
                vq = self.sovits_models[sovits_model].vq_model
                dev = self.tts_config.device

                segs, seg2orig = [], []
                for i, t in enumerate(texts):
                    for c in cut_text(t, cut_minlen):
                        segs.append(c)
                        seg2orig.append(i)
                sampling = {k: slot_sampling.per_segment(k, v, n, seg2orig) for k, v in
                            (("top_k", top_k), ("top_p", top_p), ("temperature", temperature), ("seed", seed),
                             ("repetition_penalty", repetition_penalty),
                             ("initial_suppression_steps", initial_suppression_steps))}
                if segmented:   # host lists, the same on every rank: nothing about them is exchanged
                    seg_speed = per_text_values("speed", speed, n, seg2orig)
                    seg_noise = per_text_values("noise_scale", noise_scale, n, seg2orig)
                    sovits_batch_size = min(sovits_batch_size, VOC_MAX_SEGMENTS)
                eng = self._engine(t2s)     # None in a single process
                if eng is not None:         # reference-speaker tensors exist on rank 0 only: ONE broadcast per new key
                    self._sync_speakers(prompt_audio_paths, prompt_audio_texts, spk_audio_paths, sovits_model)
                feats = [self._phones_and_bert(s) for s in segs]
                ids, prompts, berts, ges, phones2_all = [], [], [], [], []
                word2ph_all = [f[1] for f in feats]
                norm_all = [f[3] for f in feats]
                for k, (ph2, _, b2, _) in enumerate(feats):
                    o = seg2orig[k]
                    prompt, ph1, b1 = self._prompt_for(prompt_audio_paths[o], prompt_audio_texts[o])
                    ids.append(torch.tensor(ph1 + ph2, dtype=torch.int64, device=dev))
                    prompts.append(prompt.squeeze(0))
                    berts.append(torch.cat([b1, b2]))
                    ges.append(self._ge_for(spk_audio_paths[o], sovits_model).squeeze(0))
                    phones2_all.append(ph2)

                if eng is None:
                    # staged refill: same tokens per request as the reference-order loop (greedy: rows are independent;
                    # sampling: the noise stream is the request's), no stall of the other slots on a prompt pass
                    pred, orig_idx = t2s.infer_batched(ids, prompts, berts, async_refill=True, **sampling)
                    tokens = [None] * len(segs)
                    for p_, o in zip(pred, orig_idx.tolist()):
                        tokens[o] = p_
                else:   # this rank's share of the segment queue (engine.py), then every rank learns every segment's tokens
                    pred, orig_idx = eng.run_gpt(ids, prompts, berts, costs=[int(i.shape[0]) for i in ids],
                                                 async_refill=True, **sampling)
                    tokens = eng.exchange({int(o): p_ for p_, o in zip(pred, orig_idx.tolist())}, len(segs), dst=None)
                    eng._retire_cursors(None)
                # TTS.py:705-716 sorts the COMPLETION-order list by length; completion order depends on slot timing (and on
                # the rank count), the request order does not: the balance runs over the request-order lengths, so one
                # process and N ranks form the same vocoder batches and return the same samples
                lengths_all = torch.tensor([len(p_) for p_ in tokens])
                order_all = balance_order(lengths_all)
                batches = [order_all[s:s + sovits_batch_size] for s in range(0, len(order_all), sovits_batch_size)]
                my_batches = range(len(batches)) if eng is None else eng.deal_batches(len(batches))

                audios, subs_out, orig_done = [], [], []
                for b in my_batches:
                    oi = batches[b].tolist()
                    sem = [tokens[o] for o in oi]
                    ln = lengths_all[batches[b]]
                    orig_done += oi
                    ge_cat = torch.cat([ges[o].expand(-1, int(l)) for o, l in zip(oi, ln)], dim=1).unsqueeze(0)
                    ph_cat = torch.cat([torch.tensor(phones2_all[o], dtype=torch.int64, device=dev) for o in oi]).unsqueeze(0)
                    plens = torch.tensor([len(phones2_all[o]) for o in oi], device=dev)
                    ends = torch.cumsum(plens, 0)
                    pairs = torch.stack([ends - plens, ends], dim=1)
                    slice_indices = torch.repeat_interleave(pairs, (ln * 2).to(dev), dim=0)
                    if segmented:   # per-segment speed / noise: exact frame bounds, one alignment per segment
                        sp = [seg_speed[o] for o in oi]
                        audio, attn, bounds = vq.decode_segments(torch.cat(sem).unsqueeze(0).unsqueeze(0), ph_cat, ge_cat, ln.tolist(), sp,
                                                                 [seg_noise[o] for o in oi], slice_indices=slice_indices)
                        audio = audio[0, 0, :]
                        peak = audio.abs().max()
                        if peak > 1.0:
                            audio = audio / peak
                        row, prange = 0, pairs.tolist()
                        for k, (o, (lo, hi)) in enumerate(zip(oi, bounds)):
                            a = audio[lo:hi]
                            h, t = self._find_head_threshold_offsets(a), self._find_tail_threshold_offsets(a)
                            audios.append(a[h:-t].float())
                            rows = 2 * int(ln[k])
                            if return_subtitles:
                                assign = sub.viterbi_monotonic(attn[:, row:row + rows, prange[k][0]:prange[k][1]])
                                part = sub.get_subtitles(word2ph_all[o], assign, sp[k], sovits_hz=self.sovits_hz)
                                self._close_subtitles(part, word2ph_all[o], None)
                                part[-1]["end_s"] = max(part[-1]["end_s"], (hi - lo) / self.samplerate)   # the segment's own audio
                                part[0]["start_s"] += h / self.samplerate
                                part[-1]["end_s"] -= t / self.samplerate
                                subs_out.append(sub.sub2text_index(part, norm_all[o], segs[o]))
                            row += rows
                        continue
                    audio, attn = vq.decode(torch.cat(sem).unsqueeze(0).unsqueeze(0), ph_cat, ge_cat, noise_scale=noise_scale,
                                            speed=speed, cuda_graph=False, slice_indices=slice_indices)
                    audio = audio[0, 0, :]
                    if return_subtitles:   # TTS.py:768-777: one alignment over the time-concatenated batch
                        w2p_cat = {"word": [w for o in oi for w in word2ph_all[o]["word"]],
                                   "ph": [c for o in oi for c in word2ph_all[o]["ph"]]}
                        subtitles = sub.get_subtitles(w2p_cat, sub.viterbi_monotonic(attn), speed, sovits_hz=self.sovits_hz)
                        self._close_subtitles(subtitles, w2p_cat, None)
                    peak = audio.abs().max()
                    if peak > 1.0:
                        audio = audio / peak
                    if return_subtitles:   # TTS.py:783-804: the word timings, not the token counts, cut the batch apart
                        last_i = 0
                        for o in oi:
                            best_i = sub.find_subtitles(subtitles, word2ph_all[o], last_i)
                            part = subtitles[last_i:best_i]
                            last_i = best_i
                            a = audio[int(part[0]["start_s"] * self.samplerate):int(part[-1]["end_s"] * self.samplerate)]
                            h, t = self._find_head_threshold_offsets(a), self._find_tail_threshold_offsets(a)
                            audios.append(a[h:-t].float())
                            part[0]["start_s"] += h / self.samplerate
                            part[-1]["end_s"] -= t / self.samplerate
                            subs_out.append(sub.sub2text_index(part, norm_all[o], segs[o]))
                        continue
                    for lo, hi in split_bounds(ln.tolist(), vq.samples_per_frame, speed):   # TTS.py:806-811
                        a = audio[lo:hi]
                        h, t = self._find_head_threshold_offsets(a), self._find_tail_threshold_offsets(a)
                        audios.append(a[h:-t].float())

                if eng is None:
                    ordered = [None] * len(segs)
                    ordered_subs = [None] * len(segs)
                    for cur, o in enumerate(orig_done):
                        ordered[o] = audios[cur].cpu().numpy()
                        if return_subtitles:
                            ordered_subs[o] = subs_out[cur]
                else:   # every rank vocoded its batches; the samples meet on rank `gather_dst` over RCCL (TTS.py:820-865)
                    dst = self.gather_dst
                    full = eng.exchange({int(o): audios[cur].contiguous() for cur, o in enumerate(orig_done)}, len(segs), dst=dst)
                    ordered_subs = [None] * len(segs)
                    if return_subtitles:
                        ordered_subs = eng.gather({int(o): subs_out[cur] for cur, o in enumerate(orig_done)}, len(segs), dst=dst)
                    if full is None:
                        return None     # not the gathering rank
                    ordered = [a.cpu().numpy() for a in full]
                per_text = [[] for _ in range(n)]
                per_text_subs = [[] for _ in range(n)]
                last_orig, cur_text_l = None, 0
                for k, a in enumerate(ordered):
                    per_text[seg2orig[k]].append(a)
                    tail = segs[k][-1]
                    if tail in cut_mute_scale_map:
                        sc = cut_mute_scale_map[tail]
                    elif "…" in cut_mute_scale_map and segs[k][-3:] in ("...", "。。。"):
                        sc = cut_mute_scale_map["…"]
                    else:
                        sc = 1.0
                    mute = cut_mute[seg2orig[k]] if segmented else cut_mute
                    per_text[seg2orig[k]].append(np.zeros(int(mute * sc * self.samplerate), dtype=a.dtype))
                    if return_subtitles:   # TTS.py:843-852: spans are per segment; shift them into the whole text
                        if seg2orig[k] != last_orig:
                            cur_text_l, last_orig = 0, seg2orig[k]
                        ordered_subs[k][-1]["end_s"] += mute * sc
                        sub.increment_subtitle_indices(ordered_subs[k], cur_text_l)
                        per_text_subs[seg2orig[k]].append(ordered_subs[k])
                        cur_text_l += len(segs[k])
                clips = []
                for parts, sparts, t in zip(per_text, per_text_subs, texts):
                    a = np.concatenate(parts) if parts else np.zeros(0, np.float32)
                    subtitles = sub.cat_subtitles(*sparts) if return_subtitles else []
                    clips.append(AudioClip(self.audio_queue, a, self.samplerate, len(a) / self.samplerate, subtitles, t))
                finish.finish_clips(clips, chains, self.samplerate, dev)
                return tuple(clips)
            finally:
                self._empty_cache()
