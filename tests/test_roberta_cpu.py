"""CPU tests of the Chinese RoBERTa host side: the self-contained WordPiece tokenizer against BertTokenizer's ids
(tests/golden/roberta.npz tok_*, read from tokenizer.json and from vocab.txt), loader.read_roberta's formats and filters,
check_config / tokenizer refusals, and the plain-torch restatement tests/roberta_ref.py against the reference's
hidden_states[-3] and phone features (full size, 24 layers).
Tolerance: the fp32 restatement sits ~4e-6 from float64 on these weights (bounded by test_restatement_spread), so 1e-4
on layer-normed rows (rms ~1) leaves room for summation order and nothing more."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roberta_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402
from gsv_tts_lite_amd.roberta import WordPieceTokenizer, check_config  # noqa: E402

TOL = 1e-4


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "roberta.npz"))


@pytest.fixture(scope="module")
def tok_json(golden_dir):
    return os.path.join(golden_dir, "roberta_tokenizer.json")


@pytest.fixture(scope="module")
def full():
    cfg = synth.roberta_config()
    return synth.roberta_weights(cfg, 1234, run_only=True), cfg


def _split(flat, lens):
    return np.split(flat, np.cumsum(lens)[:-1])


def test_tokenizer_json_matches_bert_tokenizer(gold, tok_json):
    tok = WordPieceTokenizer.from_tokenizer_json(tok_json)
    assert len(tok) == len(synth.roberta_vocab())
    for text, want in zip(gold["tok_texts"], _split(gold["tok_ids"], gold["tok_len"])):
        assert tok.encode(str(text)) == want.tolist(), repr(str(text))


def test_vocab_txt_matches_bert_tokenizer(gold, tok_json, tmp_path):
    vocab = json.load(open(tok_json, encoding="utf-8"))["model"]["vocab"]
    with open(tmp_path / "vocab.txt", "w", encoding="utf-8") as f:
        f.write("".join(t + "\n" for t, _ in sorted(vocab.items(), key=lambda kv: kv[1])))
    tok = WordPieceTokenizer.from_dir(tmp_path)
    for text, want in zip(gold["tok_texts"], _split(gold["tok_ids"], gold["tok_len"])):
        assert tok.encode(str(text)) == want.tolist(), repr(str(text))


def test_synth_tokenizer_equals_fixture(tok_json, tmp_path):
    """the tokenizer.json synth writes for model directories reads the same as BertTokenizer's own"""
    a = WordPieceTokenizer.from_tokenizer_json(tok_json)
    with open(tmp_path / "tokenizer.json", "w", encoding="utf-8") as f:
        json.dump(synth.roberta_tokenizer_json(), f, ensure_ascii=False)
    b = WordPieceTokenizer.from_dir(tmp_path)
    for t in ("你好，世界！", "Hello walking cafés [SEP]", "龘" * 3):
        assert a.encode(t) == b.encode(t)


@pytest.mark.parametrize("part,kind", [("normalizer", "Sequence"), ("pre_tokenizer", "Whitespace"), ("model", "BPE")])
def test_tokenizer_refuses_other_kinds(tok_json, tmp_path, part, kind):
    j = json.load(open(tok_json, encoding="utf-8"))
    j[part]["type"] = kind
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(j), encoding="utf-8")
    with pytest.raises(ValueError, match=part):
        WordPieceTokenizer.from_tokenizer_json(p)


@pytest.mark.parametrize("field,value", [("model_type", "roberta"), ("position_embedding_type", "relative_key"),
                                         ("hidden_act", "gelu_new"), ("hidden_size", 1088), ("num_attention_heads", 8),
                                         ("num_hidden_layers", 1), ("max_position_embeddings", 256),
                                         ("intermediate_size", 1000)])
def test_check_config_refuses(field, value):
    with pytest.raises(ValueError, match=field):
        check_config(synth.roberta_config(**{field: value}))


def test_check_config_accepts_edge():
    c = check_config(synth.roberta_config(num_hidden_layers=2, hidden_size=128, num_attention_heads=2))
    assert c["num_hidden_layers"] == 2 and c["layer_norm_eps"] == 1e-12


@pytest.mark.parametrize("fmt,prefix", [("safetensors", True), ("bin", True), ("safetensors", False), ("bin", False)])
def test_read_roberta_formats(tmp_path, fmt, prefix):
    from gsv_tts_lite_amd.loader import read_roberta
    cfg = synth.roberta_config(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=4,
                               vocab_size=600)
    synth.write_roberta_dir(str(tmp_path), cfg, seed=3, fmt=fmt, prefix=prefix)
    config, w = read_roberta(tmp_path)
    want = synth.roberta_weights(cfg, 3, run_only=True)
    assert sorted(w) == sorted(want)
    assert not any(k.startswith(("cls.", "pooler.", "bert.")) or k.startswith(("encoder.layer.2.", "encoder.layer.3.")) for k in w)
    for k, a in want.items():
        assert torch.equal(w[k], torch.from_numpy(a)), k
    assert config["num_hidden_layers"] == 4


def test_read_roberta_gamma_beta_and_errors(tmp_path):
    from gsv_tts_lite_amd.loader import read_roberta
    cfg = synth.roberta_config(hidden_size=64, num_attention_heads=1, intermediate_size=128, num_hidden_layers=3, vocab_size=600)
    sd = {}
    for k, a in synth.roberta_weights(cfg, 4).items():
        k = k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
        sd["bert." + k] = torch.from_numpy(a)
    sd["bert.pooler.dense.weight"] = torch.zeros(64, 64)
    sd["bert.embeddings.position_ids"] = torch.arange(512)[None]
    torch.save(sd, tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    _, w = read_roberta(tmp_path)
    assert "embeddings.LayerNorm.weight" in w and "encoder.layer.0.output.LayerNorm.bias" in w
    assert not any("pooler" in k or "position_ids" in k or k.startswith("encoder.layer.1.") for k in w)
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, hidden_act="relu")))
    with pytest.raises(ValueError, match="hidden_act"):
        read_roberta(tmp_path)
    with pytest.raises(FileNotFoundError):
        read_roberta(tmp_path / "missing")


def test_restatement_spread(full, gold, tok_json):
    w, cfg = full
    tok = WordPieceTokenizer.from_tokenizer_json(tok_json)
    ids = tok.encode(str(gold["short_text"]))
    a = roberta_ref.forward(w, cfg, ids)
    b = roberta_ref.forward(w, cfg, ids, dtype=torch.float64)
    assert (a.double() - b).abs().max().item() < TOL / 4


def test_restatement_matches_reference_hidden(full, gold, tok_json):
    w, cfg = full
    tok = WordPieceTokenizer.from_tokenizer_json(tok_json)
    for case in ("short", "long"):
        ids = tok.encode(str(gold[case + "_text"]))
        h = roberta_ref.forward(w, cfg, ids).numpy()
        assert np.abs(h[gold[case + "_rows"]] - gold[case + "_hid"]).max() <= TOL, case
    texts = [str(t) for t in gold["batch_texts"]]
    hs = [roberta_ref.forward(w, cfg, tok.encode(t)).numpy() for t in texts]
    got = np.stack([hs[i][r] for i, r in zip(gold["batch_text_idx"], gold["batch_rows"])])
    assert np.abs(got - gold["batch_hid"]).max() <= TOL


def test_restatement_matches_reference_phones(full, gold, tok_json):
    w, cfg = full
    tok = WordPieceTokenizer.from_tokenizer_json(tok_json)
    feats = []
    for text, ph in zip(gold["ph_words"], _split(gold["ph_ph"], gold["ph_len"])):
        feats.append(roberta_ref.expand(roberta_ref.forward(w, cfg, tok.encode(str(text))), ph).numpy())
        assert feats[-1].shape == (int(ph.sum()), 1024)
    got = np.stack([feats[i][r] for i, r in zip(gold["ph_text_idx"], gold["ph_rows"])])
    assert np.abs(got - gold["ph_feat"]).max() <= TOL


def test_restatement_edge_two_layers(gold, tok_json):
    cfg = json.loads(str(gold["edge_config"]))
    w = synth.roberta_weights(cfg, int(gold["seed"]), run_only=True)
    assert not any(k.startswith("encoder.") for k in w)
    tok = WordPieceTokenizer.from_tokenizer_json(tok_json)
    h = roberta_ref.forward(w, cfg, tok.encode(str(gold["edge_text"]))).numpy()
    assert h.shape == gold["edge_hid"].shape
    assert np.abs(h - gold["edge_hid"]).max() <= TOL


def test_ph_mismatch_raises_before_the_device():
    """a Latin word that WordPiece splits, or a text over 510 characters, gives len(ids) - 2 != len(ph)"""
    from gsv_tts_lite_amd.roberta import CNRobertaNative
    m = CNRobertaNative.__new__(CNRobertaNative)
    m._h, m.max_len = None, 512
    m.tokenizer = WordPieceTokenizer(synth.roberta_tokenizer_json()["model"]["vocab"])
    with pytest.raises(ValueError, match="text 1"):
        m([{"word": ["你", "好"], "ph": [2, 2]}, {"word": ["walking"], "ph": [3]}])
    with pytest.raises(ValueError, match="text 0"):
        m([{"word": ["学"] * 511, "ph": [1] * 511}])


def test_native_refuses_cpu_device():
    from gsv_tts_lite_amd.roberta import CNRobertaNative
    with pytest.raises(RuntimeError):
        CNRobertaNative({}, synth.roberta_config(), None, "cpu")
