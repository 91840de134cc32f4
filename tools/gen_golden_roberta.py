"""TEST INFRASTRUCTURE -- writes tests/golden/roberta.npz and tests/golden/roberta_tokenizer.json from the reference's own
CNRoberta (GPT_SoVITS/Featurizer/cnroberta.py, loaded by path with its package stubbed: the package __init__ needs av)
over transformers BertForMaskedLM and BertTokenizer.

Runs only where `transformers` and the reference tree are available (the build container); the tests read the outputs
and need neither.  Weights are not stored: synth.roberta_weights(cfg, seed) regenerates them bit-identically.

    python tools/gen_golden_roberta.py [/path/to/reference]

roberta_tokenizer.json   BertTokenizer(vocab=synth.roberta_vocab(), do_lower_case=True).save_pretrained's tokenizer.json
                         (a list of names and settings).  vocab_file= is not used: transformers 5.x silently keeps only
                         the special tokens with it, so the vocabulary size and known ids are asserted before writing.
roberta.npz (seed 1234, all 1024 channels at the rows named `<case>_rows`; random fp32 does not compress)
  tok_*      ~30 strings and their input_ids (CJK, punctuation, digits, ## pieces, accents, control characters and
             spaces, unknown characters, special tokens, a 600-character string truncated to 512 ids)
  short      hidden_states[-3] of one short text, full size (24 layers, H 1024, vocab 21128)
  long       one text of 510 characters (T = 512)
  batch      a padded batch of 4 texts of different lengths: rows under the attention mask only
  ph         CNRoberta(word2ph_list) phone features of one batch of 3 tasks
  edge       num_hidden_layers = 2 (hidden_states[-3] = the embedding LayerNorm), H 128, every row
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

from gsv_tts_lite_amd import synth  # noqa: E402

SEED = 1234
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GSV_REFERENCE", "/root/reference")
CJK = [t for t in synth.roberta_vocab() if len(t) == 1 and 0x4E00 <= ord(t) <= 0x9FFF]

TOK_CASES = [
    "你好世界", "我们在中国。", "你好，世界！", "他说：“好的”。", "1024个gpu", "2024年10月", "10%的人", "hello world",
    "Hello World!", "unable", "walking", "cafés", "naïve", "ÜNABLE", "\t你\n好\r", "a\x00b​c\x07d", "x　y",
    "你😀好", "龘", "[CLS]你好[SEP]", "[unk]", "e.g.", "(括号)", "《书名》", "a-b_c", "", "   ", "!!!", "ＡＢＣ", "a" * 101,
    "学" * 600,
]


def text_of(name, n):
    return "".join(CJK[int(i)] for i in synth.hashed_ints(name, n, 0, len(CJK), SEED))


def load_reference_cnroberta():
    """CNRoberta from the reference tree under a private package name, gsv_tts.Config stubbed"""
    pkg = "_gsvref"
    for name in (pkg, pkg + ".GPT_SoVITS", pkg + ".GPT_SoVITS.Featurizer"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    cfg_mod = types.ModuleType(pkg + ".Config")
    cfg_mod.Config = type("Config", (), {})
    sys.modules[pkg + ".Config"] = cfg_mod
    path = os.path.join(REF, "gsv_tts", "GPT_SoVITS", "Featurizer", "cnroberta.py")
    spec = importlib.util.spec_from_file_location(pkg + ".GPT_SoVITS.Featurizer.cnroberta", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.CNRoberta


def fixture_tokenizer(out_dir):
    from transformers import BertTokenizer
    vocab = synth.roberta_vocab()
    tok = BertTokenizer(vocab={t: i for i, t in enumerate(vocab)}, do_lower_case=True)
    assert len(tok) == len(vocab), (len(tok), len(vocab))
    for t in ("[CLS]", "[SEP]", "[UNK]", "你", "##ing", "，"):
        assert tok.convert_tokens_to_ids(t) == vocab.index(t), t
    tok.save_pretrained(out_dir)
    with open(os.path.join(out_dir, "tokenizer.json"), encoding="utf-8") as f:
        j = json.load(f)
    assert j["model"]["vocab"] == {t: i for i, t in enumerate(vocab)}
    return j


def model_dir(path, cfg, tok_json):
    synth.write_roberta_dir(path, cfg, SEED)
    with open(os.path.join(path, "tokenizer.json"), "w", encoding="utf-8") as f:
        json.dump(tok_json, f, ensure_ascii=False)
    return path


def reference_hidden(cnr, texts):
    """what CNRoberta._forward_pytorch computes before the expansion: hidden_states[-3], rows under the mask"""
    with torch.no_grad():
        inputs = cnr.tokenizer(texts, return_tensors="pt", padding=True, truncation=True, max_length=512)
        hs = cnr.bert_model(**inputs, output_hidden_states=True)["hidden_states"][-3]
    return [hs[i][inputs["attention_mask"][i] == 1].numpy() for i in range(len(texts))]


def main():
    CNRoberta = load_reference_cnroberta()
    conf = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32)
    out = {"seed": np.int64(SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        tok_json = fixture_tokenizer(os.path.join(tmp, "tok"))
        with open(os.path.join(ROOT, "tests", "golden", "roberta_tokenizer.json"), "w", encoding="utf-8") as f:
            json.dump(tok_json, f, ensure_ascii=False, indent=0)
        from transformers import AutoTokenizer
        at = AutoTokenizer.from_pretrained(os.path.join(tmp, "tok"))
        ids = [at(t, truncation=True, max_length=512)["input_ids"] for t in TOK_CASES]
        out["tok_texts"] = np.array(TOK_CASES)
        out["tok_ids"] = np.concatenate([np.asarray(i, np.int32) for i in ids])
        out["tok_len"] = np.array([len(i) for i in ids], np.int32)
        assert len(ids[-1]) == 512

        cfg = synth.roberta_config()
        cnr = CNRoberta(model_dir(os.path.join(tmp, "full"), cfg, tok_json), conf)
        short = text_of("short", 13) + "。"
        (h,) = reference_hidden(cnr, [short])
        out["short_text"], out["short_rows"] = np.array(short), np.array([0, 5, 10, len(h) - 1], np.int32)
        out["short_hid"] = h[out["short_rows"]]
        long = text_of("long", 510)
        (h,) = reference_hidden(cnr, [long])
        assert len(h) == 512
        out["long_text"], out["long_rows"] = np.array(long), np.array(list(range(0, 512, 32)) + [511], np.int32)
        out["long_hid"] = h[out["long_rows"]]
        batch = [text_of("batch%d" % i, n) for i, n in enumerate((5, 37, 62, 120))]
        hs = reference_hidden(cnr, batch)
        out["batch_texts"] = np.array(batch)
        ti, rows, hid = [], [], []
        for i, h in enumerate(hs):
            assert len(h) == len(batch[i]) + 2
            for r in (0, len(h) // 2, len(h) - 1):
                ti.append(i), rows.append(r), hid.append(h[r])
        out["batch_text_idx"], out["batch_rows"], out["batch_hid"] = np.array(ti, np.int32), np.array(rows, np.int32), np.stack(hid)
        tasks = []
        for i, n in enumerate((9, 30, 4)):
            words = list(text_of("ph%d" % i, n - 1)) + ["，" if i % 2 else "。"]
            tasks.append({"word": words, "ph": [int(p) for p in synth.hashed_ints("ph%d" % i, n, 1, 4, SEED)]})
        feats = cnr(tasks)
        out["ph_words"] = np.array(["".join(t["word"]) for t in tasks])
        out["ph_ph"] = np.concatenate([np.asarray(t["ph"], np.int32) for t in tasks])
        out["ph_len"] = np.array([len(t["ph"]) for t in tasks], np.int32)
        ti, rows, hid = [], [], []
        for i, f in enumerate(feats):
            assert tuple(f.shape) == (sum(tasks[i]["ph"]), 1024) and f.dtype == torch.float32
            for r in np.unique(np.linspace(0, f.shape[0] - 1, 6).astype(int)):
                ti.append(i), rows.append(int(r)), hid.append(f[r].numpy())
        out["ph_text_idx"], out["ph_rows"], out["ph_feat"] = np.array(ti, np.int32), np.array(rows, np.int32), np.stack(hid)
        del cnr

        ecfg = synth.roberta_config(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                                    vocab_size=len(synth.roberta_vocab()))
        cnr = CNRoberta(model_dir(os.path.join(tmp, "edge"), ecfg, tok_json), conf)
        edge = text_of("edge", 11)
        (h,) = reference_hidden(cnr, [edge])
        out["edge_config"], out["edge_text"], out["edge_hid"] = np.array(json.dumps(ecfg)), np.array(edge), h
    dst = os.path.join(ROOT, "tests", "golden", "roberta.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
