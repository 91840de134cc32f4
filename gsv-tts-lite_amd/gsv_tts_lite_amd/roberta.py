"""Chinese RoBERTa on the device: the BERT features get_phones_and_bert asks tts_config.cnroberta for on every Chinese
text (gsv_tts/TextProcessor.py:62-127; GPT_SoVITS/Featurizer/cnroberta.py wraps transformers BertForMaskedLM) --
csrc/roberta.h behind the gsv_roberta_* entry points.

    feats = CNRobertaNative(weights, config, tokenizer, device, dtype)(word2ph_list)   # list of [sum(ph), 1024]

restates CNRoberta._forward_pytorch: texts "".join(word2ph["word"]), tokenized as BertTokenizer does (truncated to 512),
hidden_states[-3], every text's rows without [CLS] / [SEP], repeated by word2ph["ph"].  The texts run packed (no padding
rows), which the padded batch's key mask makes equivalent; a text's features are bit-identical alone or in any batch.
The model runs fp32 whatever the engine's numerics mode; the features come back in `dtype` as the reference returns them.
WordPieceTokenizer reads tokenizer.json (or vocab.txt) itself: neither transformers nor tokenizers is needed.  No CPU
path."""
import ctypes
import json
import os
import re
import unicodedata

import torch

from . import _native as N

MAX_LENGTH = 512   # the reference's tokenizer call: truncation=True, max_length=512

# BertConfig() fields this build reads, with chinese-roberta-wwm-ext-large's values as defaults
_DEFAULTS = dict(model_type="bert", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                 vocab_size=21128, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                 hidden_act="gelu", position_embedding_type="absolute")


def check_config(config: dict) -> dict:
    """The config.json fields with the defaults above filled in; ValueError naming the field for anything this build
    does not run.  max_position_embeddings must cover the reference's 512-token truncation (it is not shortened)."""
    c = dict(_DEFAULTS)
    c.update({k: v for k, v in dict(config).items() if k in _DEFAULTS})
    if c["model_type"] != "bert":
        raise ValueError("RoBERTa: model_type=%r is not supported (only 'bert', what chinese-roberta-wwm-ext-large uses)"
                         % c["model_type"])
    if c["position_embedding_type"] != "absolute":
        raise ValueError("RoBERTa: position_embedding_type=%r is not supported (only 'absolute')" % c["position_embedding_type"])
    if c["hidden_act"] != "gelu":
        raise ValueError("RoBERTa: hidden_act=%r is not supported (only exact 'gelu')" % c["hidden_act"])
    H, heads = c["hidden_size"], c["num_attention_heads"]
    if H % 64 or H < 64 or H > 1024:
        raise ValueError("RoBERTa: hidden_size=%d is not supported (a multiple of 64 up to 1024)" % H)
    if heads * 64 != H:
        raise ValueError("RoBERTa: num_attention_heads=%d over hidden_size %d is not supported (head dim 64)" % (heads, H))
    if c["num_hidden_layers"] < 2:
        raise ValueError("RoBERTa: num_hidden_layers=%d is not supported (hidden_states[-3] needs at least 2)"
                         % c["num_hidden_layers"])
    if c["intermediate_size"] % 64 or c["intermediate_size"] < 64:
        raise ValueError("RoBERTa: intermediate_size=%d is not supported (a multiple of 64)" % c["intermediate_size"])
    if c["max_position_embeddings"] < MAX_LENGTH:
        raise ValueError("RoBERTa: max_position_embeddings=%d is not supported (at least %d: texts are truncated to %d "
                         "tokens, as the reference does)" % (c["max_position_embeddings"], MAX_LENGTH, MAX_LENGTH))
    if c["vocab_size"] < 1 or c["type_vocab_size"] < 1:
        raise ValueError("RoBERTa: vocab_size=%d / type_vocab_size=%d is not supported" % (c["vocab_size"], c["type_vocab_size"]))
    if not c["layer_norm_eps"] > 0:
        raise ValueError("RoBERTa: layer_norm_eps=%r is not supported (> 0)" % c["layer_norm_eps"])
    return c


def native_config(config: dict) -> N.RobertaConfig:
    c = check_config(config)
    return N.RobertaConfig(hidden=c["hidden_size"], n_layer=c["num_hidden_layers"], n_head=c["num_attention_heads"],
                           ffn=c["intermediate_size"], vocab=c["vocab_size"], max_pos=c["max_position_embeddings"],
                           type_vocab=c["type_vocab_size"], eps=float(c["layer_norm_eps"]))


def used_tensor(name: str, n_layer: int) -> bool:
    """whether hidden_states[-3] reads the tensor (names without the "bert." prefix): the embeddings and layers
    0 .. n_layer - 3; not the last two layers, the pooler or cls.*"""
    if name.startswith("embeddings."):
        return name != "embeddings.position_ids"
    m = re.match(r"encoder\.layer\.(\d+)\.", name)
    return bool(m) and int(m.group(1)) < n_layer - 2


# ---------------------------------------------------------------------------------------------------------------------
# BERT WordPiece tokenizer (the BertNormalizer / BertPreTokenizer / WordPiece pipeline of the tokenizers library)
# ---------------------------------------------------------------------------------------------------------------------
_SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


def _is_control(ch: str) -> bool:
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_whitespace(ch: str) -> bool:
    return ch in "\t\n\r" or ch.isspace()


def _is_punct(ch: str) -> bool:
    cp = ord(ch)
    return 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126 or unicodedata.category(ch).startswith("P")


class WordPieceTokenizer:
    """BertTokenizer(Fast) as the reference calls it: encode(text) -> [CLS] ids [SEP], at most max_length ids.
    vocab {token: id}; the special tokens present in the vocabulary are matched verbatim in the raw text first."""

    def __init__(self, vocab: dict, lowercase: bool = True, strip_accents=None, clean_text: bool = True,
                 handle_chinese_chars: bool = True, unk_token: str = "[UNK]", prefix: str = "##",
                 max_input_chars_per_word: int = 100, cls_token: str = "[CLS]", sep_token: str = "[SEP]",
                 special_tokens=_SPECIALS, max_length: int = MAX_LENGTH):
        self.vocab = dict(vocab)
        for t in (unk_token, cls_token, sep_token):
            if t not in self.vocab:
                raise ValueError("RoBERTa tokenizer: the vocabulary has no %s token" % t)
        self.lowercase, self.clean_text, self.handle_chinese_chars = bool(lowercase), bool(clean_text), bool(handle_chinese_chars)
        self.strip_accents = self.lowercase if strip_accents is None else bool(strip_accents)
        self.unk, self.prefix, self.max_chars = self.vocab[unk_token], prefix, int(max_input_chars_per_word)
        self.cls, self.sep, self.max_length = self.vocab[cls_token], self.vocab[sep_token], int(max_length)
        specials = sorted({t for t in special_tokens if t in self.vocab}, key=len, reverse=True)
        self._special_re = re.compile("(" + "|".join(map(re.escape, specials)) + ")") if specials else None

    @classmethod
    def from_tokenizer_json(cls, path, **kw):
        """a tokenizers-library tokenizer.json; anything but BertNormalizer + BertPreTokenizer + WordPiece is refused"""
        with open(path, encoding="utf-8") as f:
            j = json.load(f)
        norm, pre, model = j.get("normalizer") or {}, j.get("pre_tokenizer") or {}, j.get("model") or {}
        if norm.get("type") != "BertNormalizer":
            raise ValueError("RoBERTa tokenizer: %s has normalizer %r (only BertNormalizer is supported)" % (path, norm.get("type")))
        if pre.get("type") != "BertPreTokenizer":
            raise ValueError("RoBERTa tokenizer: %s has pre_tokenizer %r (only BertPreTokenizer is supported)" % (path, pre.get("type")))
        if model.get("type") != "WordPiece" or not isinstance(model.get("vocab"), dict):
            raise ValueError("RoBERTa tokenizer: %s has model %r (only WordPiece is supported)" % (path, model.get("type")))
        specials = [t["content"] for t in j.get("added_tokens") or [] if t.get("special")] or list(_SPECIALS)
        return cls(model["vocab"], lowercase=norm.get("lowercase", True), strip_accents=norm.get("strip_accents"),
                   clean_text=norm.get("clean_text", True), handle_chinese_chars=norm.get("handle_chinese_chars", True),
                   unk_token=model.get("unk_token", "[UNK]"), prefix=model.get("continuing_subword_prefix", "##"),
                   max_input_chars_per_word=model.get("max_input_chars_per_word", 100), special_tokens=specials, **kw)

    @classmethod
    def from_vocab_txt(cls, path, lowercase: bool = True, **kw):
        """one token per line, the id being the line number (BertTokenizer's vocab.txt)"""
        with open(path, encoding="utf-8") as f:
            vocab = {line.rstrip("\n"): i for i, line in enumerate(f)}
        return cls(vocab, lowercase=lowercase, **kw)

    @classmethod
    def from_dir(cls, path):
        """tokenizer.json when the directory has one, else vocab.txt (do_lower_case from tokenizer_config.json)"""
        path = str(path)
        tj = os.path.join(path, "tokenizer.json")
        if os.path.isfile(tj):
            return cls.from_tokenizer_json(tj)
        vt = os.path.join(path, "vocab.txt")
        if os.path.isfile(vt):
            lower = True
            tc = os.path.join(path, "tokenizer_config.json")
            if os.path.isfile(tc):
                with open(tc, encoding="utf-8") as f:
                    lower = json.load(f).get("do_lower_case", True)
            return cls.from_vocab_txt(vt, lowercase=lower)
        raise FileNotFoundError("RoBERTa tokenizer: %s holds neither tokenizer.json nor vocab.txt" % path)

    def normalize(self, text: str) -> str:
        if self.clean_text:
            text = "".join(" " if _is_whitespace(c) else c for c in text
                           if not (c == "\0" or c == "\ufffd" or _is_control(c)))
        if self.handle_chinese_chars:
            text = "".join(" %s " % c if _is_cjk(ord(c)) else c for c in text)
        if self.strip_accents:
            text = "".join(c for c in unicodedata.normalize("NFD", text) if unicodedata.category(c) != "Mn")
        if self.lowercase:
            text = text.lower()
        return text

    @staticmethod
    def pre_tokenize(text: str) -> list:
        words, cur = [], []
        for c in text:
            if _is_whitespace(c) or _is_punct(c):
                if cur:
                    words.append("".join(cur))
                    cur = []
                if not _is_whitespace(c):
                    words.append(c)
            else:
                cur.append(c)
        if cur:
            words.append("".join(cur))
        return words

    def wordpiece(self, word: str) -> list:
        if len(word) > self.max_chars:
            return [self.unk]
        out, start = [], 0
        while start < len(word):
            end, hit = len(word), None
            while start < end:
                piece = word[start:end] if start == 0 else self.prefix + word[start:end]
                if piece in self.vocab:
                    hit = self.vocab[piece]
                    break
                end -= 1
            if hit is None:
                return [self.unk]
            out.append(hit)
            start = end
        return out

    def tokenize(self, text: str) -> list:
        """ids without [CLS] / [SEP], not truncated"""
        parts = self._special_re.split(text) if self._special_re else [text]
        ids = []
        for i, part in enumerate(parts):
            if i % 2:
                ids.append(self.vocab[part])
                continue
            for w in self.pre_tokenize(self.normalize(part)):
                ids += self.wordpiece(w)
        return ids

    def encode(self, text: str) -> list:
        return [self.cls] + self.tokenize(text)[:self.max_length - 2] + [self.sep]

    def __len__(self):
        return len(self.vocab)


# ---------------------------------------------------------------------------------------------------------------------
class CNRobertaNative:
    """weights: BertModel state dict without the "bert." prefix (torch or numpy; unused tensors are skipped), config:
    config.json fields, tokenizer: WordPieceTokenizer.  __call__(word2ph_list) -> list of [sum(ph), hidden] in `dtype`
    on `device`; hidden(texts) -> list of hidden_states[-3] [len(ids), hidden] fp32."""

    def __init__(self, weights, config, tokenizer, device, dtype=torch.float32):
        self._h = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RoBERTa runs on the MI355X only (gsv_roberta_*); got device %s -- there is no CPU path"
                               % self.device)
        self.dtype = dtype
        self.tokenizer = tokenizer
        L = N.lib()
        c = check_config(config)
        cfg = native_config(c)
        self.hidden_size, self.vocab_size, self.max_len = cfg.hidden, cfg.vocab, min(MAX_LENGTH, cfg.max_pos)
        h = ctypes.c_void_p()
        N.check(L.gsv_roberta_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        st = N.current_stream_ptr(self.device)
        for name, t in weights.items():
            if not used_tensor(name, cfg.n_layer):
                continue
            d = torch.as_tensor(t).detach().to(device=self.device, dtype=torch.float32).contiguous()
            N.check(L.gsv_roberta_load_tensor(h, name.encode(), d.data_ptr(), d.numel(), st))
            del d
        N.check(L.gsv_roberta_finalize(h, st))
        self._ws = None

    def __del__(self):
        try:
            if self._h is not None:
                N.lib().gsv_roberta_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _pack(self, ids_list):
        for i, ids in enumerate(ids_list):
            if not 2 <= len(ids) <= self.max_len:
                raise ValueError("RoBERTa: text %d has %d ids (2 .. %d, [CLS] and [SEP] included)" % (i, len(ids), self.max_len))
            if min(ids) < 0 or max(ids) >= self.vocab_size:
                raise ValueError("RoBERTa: text %d has an id outside the vocabulary of %d" % (i, self.vocab_size))
        starts = [0]
        for ids in ids_list:
            starts.append(starts[-1] + len(ids))
        flat = [t for ids in ids_list for t in ids]
        dev = self.device
        ids_t = torch.tensor(flat, dtype=torch.int32).to(dev, non_blocking=False)
        starts_t = torch.tensor(starts, dtype=torch.int32).to(dev, non_blocking=False)
        max_len = max(len(ids) for ids in ids_list)
        need = N.lib().gsv_roberta_workspace(self._h, len(flat), len(ids_list), max_len)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return ids_t, starts_t, starts, max_len

    def hidden_ids(self, ids_list):
        """token id lists ([CLS] .. [SEP] each) -> list of hidden_states[-3] [len(ids), hidden] fp32, one packed call"""
        ids_t, starts_t, starts, max_len = self._pack(ids_list)
        out = torch.empty(starts[-1], self.hidden_size, dtype=torch.float32, device=self.device)
        N.check(N.lib().gsv_roberta_forward(self._h, ids_t.data_ptr(), starts_t.data_ptr(), len(ids_list), starts[-1], max_len,
                                            out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                            N.current_stream_ptr(self.device)))
        return [out[starts[i]:starts[i + 1]] for i in range(len(ids_list))]

    def hidden(self, texts):
        """texts -> hidden_states[-3] at each text's unmasked rows, [CLS] and [SEP] included (the parity seam)"""
        return self.hidden_ids([self.tokenizer.encode(t) for t in texts])

    def __call__(self, word2ph_list):
        """CNRoberta.forward: list of {"word": [...], "ph": [...]} -> list of [sum(ph), hidden] phone features"""
        ids_list, phs = [], []
        for i, w2p in enumerate(word2ph_list):
            ids = self.tokenizer.encode("".join(w2p["word"]))
            ph = [int(p) for p in w2p["ph"]]
            if len(ids) - 2 != len(ph):
                raise ValueError("RoBERTa: text %d tokenizes to %d tokens but word2ph has %d entries (a Latin word split into "
                                 "WordPiece pieces, or more than %d characters)" % (i, len(ids) - 2, len(ph), self.max_len - 2))
            if any(p < 0 for p in ph):
                raise ValueError("RoBERTa: text %d has a negative phone count" % i)
            ids_list.append(ids)
            phs.append(ph)
        if not ids_list:
            return []
        ids_t, starts_t, starts, max_len = self._pack(ids_list)
        index, counts = [], []
        for i, ph in enumerate(phs):
            for j, p in enumerate(ph):
                index += [starts[i] + 1 + j] * p
            counts.append(sum(ph))
        P = len(index)
        out = torch.empty(P, self.hidden_size, dtype=torch.float32, device=self.device)
        if P:
            index_t = torch.tensor(index, dtype=torch.int32).to(self.device)
            N.check(N.lib().gsv_roberta_features(self._h, ids_t.data_ptr(), starts_t.data_ptr(), len(ids_list), starts[-1], max_len,
                                                 index_t.data_ptr(), P, out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                 N.current_stream_ptr(self.device)))
        out = out.to(self.dtype)
        return list(torch.split(out, counts))

    forward = __call__


def load_cnroberta(path, device, dtype=torch.float32) -> CNRobertaNative:
    """a Hugging Face chinese-roberta-wwm-ext-large directory (loader.read_roberta + its tokenizer) on the device"""
    from .loader import read_roberta
    config, weights = read_roberta(path)
    return CNRobertaNative(weights, config, WordPieceTokenizer.from_dir(path), device, dtype)
