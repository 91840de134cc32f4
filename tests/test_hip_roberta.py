"""GPU parity of Chinese RoBERTa (csrc/roberta.h behind gsv_roberta_*): hidden_states[-3] against the reference's
CNRoberta over transformers (tests/golden/roberta.npz, full size: 24 layers, H 1024) and, in full, against the plain-torch
restatement tests/roberta_ref.py at lengths around the 64-key tile and at 512; bit-identical batch invariance and
reproducibility; CNRobertaNative(word2ph_list) against the reference's phone features; the facade's use_bert / auto_bert.
Tolerance: 2e-4 max abs on layer-normed rows (rms ~1), the CN-HuBERT bound; the fp32 restatement's own spread against
float64 is ~4e-6 here (test_roberta_cpu.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roberta_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "roberta.npz"))


@pytest.fixture(scope="module")
def tok(golden_dir):
    from gsv_tts_lite_amd.roberta import WordPieceTokenizer
    return WordPieceTokenizer.from_tokenizer_json(os.path.join(golden_dir, "roberta_tokenizer.json"))


@pytest.fixture(scope="module")
def model(dev, gold, tok):
    from gsv_tts_lite_amd.roberta import CNRobertaNative
    cfg = synth.roberta_config()
    w = synth.roberta_weights(cfg, int(gold["seed"]), run_only=True)
    return CNRobertaNative(w, cfg, tok, dev), w, cfg


def _ids(name, T, vocab=21128):
    return [101] + synth.hashed_ints(name, T - 2, 5, vocab).tolist() + [102]


def test_golden_hidden(model, gold):
    m, _, _ = model
    for case in ("short", "long"):
        (h,) = m.hidden([str(gold[case + "_text"])])
        assert h.dtype == torch.float32 and h.device.type == "cuda"
        err = np.abs(h.cpu().numpy()[gold[case + "_rows"]] - gold[case + "_hid"]).max()
        print("%s: T %d max|err| %.2e" % (case, h.shape[0], err))
        assert err <= TOL, case
    hs = m.hidden([str(t) for t in gold["batch_texts"]])
    assert [h.shape[0] for h in hs] == [len(str(t)) + 2 for t in gold["batch_texts"]]
    got = np.stack([hs[i].cpu().numpy()[r] for i, r in zip(gold["batch_text_idx"], gold["batch_rows"])])
    err = np.abs(got - gold["batch_hid"]).max()
    print("batch: max|err| %.2e" % err)
    assert err <= TOL


@pytest.mark.parametrize("T", [3, 63, 64, 65, 512])
def test_vs_restatement(model, T):
    m, w, cfg = model
    ids = _ids("T%d" % T, T)
    (got,) = m.hidden_ids([ids])
    want = roberta_ref.forward(w, cfg, ids)
    assert got.shape == want.shape == (T, 1024) and torch.isfinite(got).all()
    assert (got.cpu() - want).abs().max().item() <= TOL


def test_vs_restatement_packed(model):
    m, w, cfg = model
    lens = [2, 130, 7, 64, 65, 33]
    batch = [_ids("P%d" % i, T) for i, T in enumerate(lens)]
    got = m.hidden_ids(batch)
    for ids, g in zip(batch, got):
        assert (g.cpu() - roberta_ref.forward(w, cfg, ids)).abs().max().item() <= TOL, len(ids)


def test_batch_invariance_bit_identical(model):
    m, _, _ = model
    lens = [int(n) for n in synth.hashed_ints("inv", 20, 2, 90)]
    batch = [_ids("inv%d" % i, T) for i, T in enumerate(lens)]
    alone = [m.hidden_ids([ids])[0].clone() for ids in batch]
    for n in (2, 7, 20):
        for off in range(0, 20, n):
            got = m.hidden_ids(batch[off:off + n])
            for j, g in enumerate(got):
                assert torch.equal(g, alone[off + j]), (n, off + j)


def test_bit_reproducible_and_workspace_reuse(model):
    m, _, _ = model
    a = [_ids("r0", 40), _ids("r1", 9)]
    big = [_ids("r2", 512)] * 4
    first = [h.clone() for h in m.hidden_ids(a)]
    for h, f in zip(m.hidden_ids(a), first):
        assert torch.equal(h, f)
    m.hidden_ids(big)
    for h, f in zip(m.hidden_ids(a), first):
        assert torch.equal(h, f)
    with pytest.raises(ValueError):
        m.hidden_ids([_ids("r3", 513)])
    with pytest.raises(ValueError):
        m.hidden_ids([[101, 21128, 102]])


def _tasks(gold):
    out, off = [], 0
    for text, n in zip(gold["ph_words"], gold["ph_len"]):
        out.append({"word": list(str(text)), "ph": gold["ph_ph"][off:off + n].tolist()})
        off += n
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_phone_features_golden(model, gold, dev, dtype):
    m, _, _ = model
    tasks = _tasks(gold)
    m.dtype = dtype
    try:
        feats = m(tasks)
    finally:
        m.dtype = torch.float32
    assert len(feats) == len(tasks)
    for f, t in zip(feats, tasks):
        assert f.shape == (sum(t["ph"]), 1024) and f.dtype == dtype and f.device == dev
    got = np.stack([feats[i][r].float().cpu().numpy() for i, r in zip(gold["ph_text_idx"], gold["ph_rows"])])
    want = gold["ph_feat"]
    # bf16: the fp32 result rounded once, so within TOL plus half a bf16 ulp (2^-9 relative)
    bound = TOL + (np.abs(want) * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert (np.abs(got - want) <= bound).all()
    if dtype == torch.float32:
        # the one-call path equals hidden rows gathered on the host
        hs = m.hidden(["".join(t["word"]) for t in tasks])
        for f, h, t in zip(feats, hs, tasks):
            assert torch.equal(f.cpu(), roberta_ref.expand(h.cpu(), t["ph"]))
    with pytest.raises(ValueError, match="text 1"):
        m([tasks[0], {"word": ["walking"], "ph": [3]}])


def test_two_layer_edge(dev, gold, tok):
    from gsv_tts_lite_amd.roberta import CNRobertaNative
    cfg = json.loads(str(gold["edge_config"]))
    m = CNRobertaNative(synth.roberta_weights(cfg, int(gold["seed"])), cfg, tok, dev)
    (h,) = m.hidden([str(gold["edge_text"])])
    assert np.abs(h.cpu().numpy() - gold["edge_hid"]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------------ facade
def _frontend(tts):
    """get_phones_and_bert's shape: BERT features from tts_config.cnroberta for Chinese text, zeros otherwise"""
    def fe(text):
        words = [c for c in text if not c.isspace()]
        ph = [2 if "一" <= c <= "鿿" else 1 for c in words]
        ids = [1 + (ord(c) * 7 + k) % 690 for c, p in zip(words, ph) for k in range(p)]
        w2p = {"word": words, "ph": ph}
        cn = tts.tts_config.cnroberta
        bert = cn([w2p])[0] if cn is not None and tts._contains_chinese(text) else None
        return ids, w2p, bert, text
    return fe


def _tts(dev, models_dir, **kw):
    from gsv_tts import TTS
    tts = TTS(gpt_cache=[(1, 128)], sovits_cache=[50, 55], models_dir=str(models_dir), device=str(dev), dtype="float32", **kw)
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=1.0")
    tts.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    tts.set_text_frontend(_frontend(tts))
    tts.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    tts.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    return tts


@pytest.fixture(scope="module")
def roberta_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("models")
    synth.write_roberta_dir(str(d / "chinese-roberta-wwm-ext-large"), synth.roberta_config(num_hidden_layers=4), seed=7)
    return d


def test_facade_auto_bert(dev, roberta_dir):
    from gsv_tts_lite_amd.roberta import CNRobertaNative
    tts = _tts(dev, roberta_dir)
    assert tts.tts_config.cnroberta is None
    en = tts.infer("spk.wav", "prompt.wav", "prompt text.", "Hello there", top_k=1, noise_scale=0.0)
    assert tts.tts_config.cnroberta is None and np.isfinite(en.audio_data).all()
    zh_text = "你好世界，我们在中国"
    clip = tts.infer("spk.wav", "prompt.wav", "prompt text.", zh_text, top_k=1, noise_scale=0.0)
    assert isinstance(tts.tts_config.cnroberta, CNRobertaNative)
    # the same features handed over explicitly give the same tokens, hence the same audio
    ids, w2p, bert, norm = _frontend(tts)(zh_text + ".")
    assert bert is not None and bert.shape == (len(ids), 1024) and bert.abs().max() > 0
    tts.set_text_frontend(lambda t: (ids, w2p, bert.clone(), norm))
    again = tts.infer("spk.wav", "prompt.wav", "prompt text.", zh_text, top_k=1, noise_scale=0.0)
    assert clip.audio_data.shape == again.audio_data.shape
    np.testing.assert_allclose(clip.audio_data, again.audio_data, atol=1e-5)
    clips = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", [zh_text, "Hello there"], top_k=1, noise_scale=0.0)
    assert len(clips) == 2
    t2 = _tts(dev, roberta_dir, use_bert=True, auto_bert=False)
    assert isinstance(t2.tts_config.cnroberta, CNRobertaNative)


def test_facade_missing_dir_warns_once(dev, tmp_path, caplog):
    zh_text = "你好世界，我们在中国"
    base = _tts(dev, tmp_path, auto_bert=False).infer("spk.wav", "prompt.wav", "prompt text.", zh_text, top_k=1, noise_scale=0.0)
    tts = _tts(dev, tmp_path)
    with caplog.at_level("WARNING", logger="gsv_tts_lite_amd"):
        a = tts.infer("spk.wav", "prompt.wav", "prompt text.", zh_text, top_k=1, noise_scale=0.0)
        list(tts.infer_stream("spk.wav", "prompt.wav", "prompt text.", zh_text, top_k=1, noise_scale=0.0, debug=False))
    assert sum("Chinese RoBERTa" in r.getMessage() for r in caplog.records) == 1
    assert tts.tts_config.cnroberta is None
    np.testing.assert_allclose(a.audio_data, base.audio_data, atol=1e-5)
