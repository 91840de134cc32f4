"""CPU tests of the CN-HuBERT port (no GPU, no transformers, no reference tree): the plain-torch restatement
tests/hubert_ref.py against tests/golden/hubert.npz (written from transformers.HubertModel by tools/gen_golden_hubert.py),
loader.read_cnhubert on both weight-norm namings and both file formats, config refusal in Python and in the C ABI,
and no CPU fallback behind TTS.cache_prompt_audio(audio=...)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubert_ref  # noqa: E402

from gsv_tts_lite_amd import synth  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "hubert.npz"))


@pytest.fixture(scope="module")
def weights(gold):
    return synth.hubert_weights(synth.hubert_config(), int(gold["seed"]))


def _prompt_wav(i, secs, seed):
    return np.concatenate([synth.synth_wav16k(i, secs, seed), np.zeros(4800, np.float32)])


@pytest.mark.parametrize("name,i", [("bare400", 0), ("bare8000", 1)])
def test_ref_matches_golden_bare(gold, weights, name, i):
    cfg = synth.hubert_config()
    n = int(gold[name + "_n"])
    last, inter = hubert_ref.forward(weights, cfg, synth.synth_audio(100 + i, n, int(gold["seed"])))
    rows = gold[name + "_rows"]
    assert tuple(last.shape) == (int(gold[name + "_Th"]), 768) and last.shape[0] == hubert_ref.frames(cfg, n)
    np.testing.assert_allclose(inter["features"].numpy()[rows], gold[name + "_features"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(inter["pre_ln"].numpy()[rows], gold[name + "_pre_ln"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(last.numpy()[rows], gold[name + "_last"], atol=1e-4, rtol=0)


def test_ref_matches_golden_prompts(gold, weights):
    cfg = synth.hubert_config()
    seed = int(gold["seed"])
    last3, _ = hubert_ref.forward(weights, cfg, _prompt_wav(2, 3.0, seed))
    assert last3.shape[0] == int(gold["prompt3s_Th"]) == 164
    np.testing.assert_allclose(last3.numpy()[gold["prompt3s_rows"]], gold["prompt3s_last"], atol=1e-4, rtol=0)
    last10, _ = hubert_ref.forward(weights, cfg, _prompt_wav(3, 10.0, seed))
    assert last10.shape[0] == int(gold["prompt10s_Th"]) == 514
    np.testing.assert_allclose(last10.numpy()[gold["prompt10s_rows"]], gold["prompt10s_last"], atol=1e-4, rtol=0)


def test_frame_counts():
    cfg = synth.hubert_config()
    assert [hubert_ref.frames(cfg, n) for n in (399, 400, 719, 720, 52800, 164800)] == [0, 1, 1, 2, 164, 514]


@pytest.mark.parametrize("naming,fmt", [("parametrizations", "safetensors"), ("weight_g", "bin"), ("weight_g", "safetensors")])
def test_read_cnhubert(tmp_path, gold, naming, fmt):
    from gsv_tts_lite_amd.hubert import fold_pos_conv_weight
    from gsv_tts_lite_amd.loader import read_cnhubert
    seed = int(gold["seed"])
    d = synth.write_hubert_dir(str(tmp_path / "chinese-hubert-base"), seed=seed, naming=naming, fmt=fmt)
    config, w = read_cnhubert(d)
    assert config["hidden_size"] == 768 and config["num_hidden_layers"] == 12
    want = synth.hubert_weights(synth.hubert_config(), seed)
    for k, a in want.items():
        assert np.array_equal(w[k].numpy(), a), k
    wf = fold_pos_conv_weight(w)
    assert wf.shape == (768, 48, 128)
    got = wf[gold["pos_w_rows"]][:, :, ::int(gold["pos_w_tap_step"])].numpy()
    np.testing.assert_allclose(got, gold["pos_w_slice"], rtol=1e-5, atol=1e-8)


BAD = [dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(conv_bias=True), dict(hidden_act="gelu_new"),
       dict(feat_extract_activation="relu"), dict(num_attention_heads=16), dict(num_conv_pos_embeddings=127),
       dict(conv_dim=[512] * 6)]


@pytest.mark.parametrize("bad", BAD, ids=[next(iter(b)) for b in BAD])
def test_unsupported_config_refused(tmp_path, bad):
    from gsv_tts_lite_amd.hubert import check_config
    from gsv_tts_lite_amd.loader import read_cnhubert
    with pytest.raises(ValueError, match="CN-HuBERT"):
        check_config(synth.hubert_config(**bad))
    d = synth.write_hubert_dir(str(tmp_path / "h"), cfg=synth.hubert_config(num_hidden_layers=1))
    with open(os.path.join(d, "config.json")) as f:
        cfg = json.load(f)
    cfg.update(bad)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="CN-HuBERT"):
        read_cnhubert(d)


def test_abi_config_and_frames():
    """gsv_hubert_create refuses shapes the kernels do not run; gsv_hubert_frames follows the conv floors (host only)"""
    import __graft_entry__ as g
    g.build_hip()
    from gsv_tts_lite_amd import _native as N
    from gsv_tts_lite_amd.hubert import native_config
    L = N.lib()
    h = ctypes.c_void_p()
    assert L.gsv_hubert_create(ctypes.byref(native_config(synth.hubert_config())), ctypes.byref(h)) == 0
    try:
        for n, th in ((399, 0), (400, 1), (401, 1), (719, 1), (720, 2), (52800, 164), (164800, 514)):
            assert L.gsv_hubert_frames(h, n) == th, n
        assert L.gsv_hubert_workspace(h, 399) == 0 and L.gsv_hubert_workspace(h, 400) > 0
    finally:
        L.gsv_hubert_destroy(h)
    for field, val in (("n_head", 16), ("pos_k", 127), ("hidden", 800), ("n_conv", 9)):
        c = native_config(synth.hubert_config())
        setattr(c, field, val)
        h2 = ctypes.c_void_p()
        assert L.gsv_hubert_create(ctypes.byref(c), ctypes.byref(h2)) == 1, field   # GSV_ERR_ARG
        assert b"hubert" in L.gsv_last_error()


def test_cache_prompt_audio_on_cpu_fails_loudly(tmp_path):
    from gsv_tts_lite_amd.tts import TTS
    synth.write_hubert_dir(str(tmp_path / "chinese-hubert-base"), cfg=synth.hubert_config(num_hidden_layers=1))
    tts = TTS(models_dir=str(tmp_path), device="cpu", dtype="float32", always_load_cnhubert=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tts.cache_prompt_audio("p.wav", "prompt text.", audio=torch.from_numpy(synth.synth_wav16k(0, 1.0)), phones1=[1, 2, 3])
    assert "p.wav" not in tts.prompt_audio_cache and tts.cnhubert_model is None
    with pytest.raises(NotImplementedError, match="16 kHz"):
        tts.cache_prompt_audio("p.wav", "prompt text.", phones1=[1, 2, 3])
