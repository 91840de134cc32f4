"""TEST INFRASTRUCTURE -- writes tests/golden/hubert.npz from transformers.HubertModel and the reference's extract_latent.

Runs only where `transformers` and the reference tree are importable (the build container); the tests read the npz and
need neither.  Weights are not stored: synth.hubert_weights(seed) regenerates them bit-identically everywhere.

    python tools/gen_golden_hubert.py

Cases (seed 1234, waveforms synth.synth_wav16k).  Random fp32 does not compress, so every hidden-state tensor is stored at
the frames `<case>_rows` only (all 768 channels of each); the tests compare full outputs against tests/hubert_ref.py, which
these rows pin to transformers.  The file stays near 0.2 MB.
  bare400, bare8000      HubertModel(wav)["last_hidden_state"] at n = 400 (the shortest input, Th = 1) and 0.5 s (every 4th
                         frame), plus the feature-encoder output and the encoder.layer_norm input at the same frames
  prompt3s, prompt10s    the TTS._get_prompt form (wav + 0.3 s of zeros): last_hidden_state every 16th / 32nd frame, and
                         the prompt codes of the reference's SynthesizerTrn.extract_latent (v2Pro synthetic ssl_proj /
                         codebook, synth.ref_audio_weights) with each code's best-vs-second distance margin
  pos_w_slice            the positional conv's effective weight as transformers computes it, one output channel per group
                         (rows pos_w_rows = 0, 48, ...) and every 8th tap: [::48, :, ::8]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")]

from gsv_tts_lite_amd import synth  # noqa: E402

SEED = 1234
BARE = [("bare400", 0, 400), ("bare8000", 1, 8000)]
PROMPT = [("prompt3s", 2, 3.0), ("prompt10s", 3, 10.0)]
ROW_STEP = {"bare400": 1, "bare8000": 4, "prompt3s": 16, "prompt10s": 32}
POS_ROW_STEP, POS_TAP_STEP = 48, 8


def hf_model(seed):
    from transformers import HubertConfig, HubertModel
    cfg = synth.hubert_config()
    hc = HubertConfig(attn_implementation="eager")
    for k, v in cfg.items():
        if k != "model_type":
            assert getattr(hc, k) == (tuple(v) if isinstance(v, list) else v) or list(getattr(hc, k)) == v, k
    m = HubertModel(hc).eval()
    sd = {}
    for k, a in synth.hubert_weights(cfg, seed).items():
        k = k.replace("conv.weight_g", "conv.parametrizations.weight.original0").replace(
            "conv.weight_v", "conv.parametrizations.weight.original1")
        sd[k] = torch.from_numpy(a)
    sd["masked_spec_embed"] = torch.zeros(hc.hidden_size)
    m.load_state_dict(sd, strict=True)
    return m


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = hf_model(SEED)
    out = {"seed": np.int64(SEED), "torch_version": torch.__version__}
    with torch.inference_mode():
        for name, i, n in BARE:
            wav = torch.from_numpy(synth.synth_audio(100 + i, n, SEED))
            feats = m.feature_extractor(wav[None])[0].transpose(0, 1)
            hs = m.feature_projection(feats[None])
            pre = hs + m.encoder.pos_conv_embed(hs)
            last = m(wav[None])["last_hidden_state"][0]
            rows = np.arange(0, last.shape[0], ROW_STEP[name])
            out[name + "_n"] = np.int64(n)
            out[name + "_Th"] = np.int64(last.shape[0])
            out[name + "_rows"] = rows
            out[name + "_last"] = last.numpy()[rows]
            out[name + "_features"] = feats.numpy()[rows]
            out[name + "_pre_ln"] = pre[0].numpy()[rows]
            print(name, "n", n, "Th", last.shape[0], "rms %.3f" % last.pow(2).mean().sqrt().item())
        out["pos_w_rows"] = np.arange(0, 768, POS_ROW_STEP)
        out["pos_w_tap_step"] = np.int64(POS_TAP_STEP)
        out["pos_w_slice"] = m.encoder.pos_conv_embed.conv.weight[::POS_ROW_STEP, :, ::POS_TAP_STEP].detach().numpy().copy()

        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        from ref_harness import import_reference
        _, _, Syn = import_reference()
        hps = synth.sovits_hps("v2Pro")
        vq = Syn(1025, 32, n_speakers=300, **hps["model"]).eval()
        sd = {k: torch.from_numpy(v) for k, v in synth.ref_audio_weights(hps, SEED).items()}
        sd["quantizer.vq.layers.0._codebook.inited"] = torch.ones(1)   # a trained checkpoint: no k-means re-init
        assert not vq.load_state_dict(sd, strict=False).unexpected_keys
        for name, i, secs in PROMPT:
            wav16k = torch.from_numpy(synth.synth_wav16k(i, secs, SEED))
            wav = torch.cat([wav16k, torch.zeros(int(16000 * 0.3))])          # TTS._get_prompt
            ssl = m(wav[None])["last_hidden_state"].transpose(1, 2)
            codes = vq.extract_latent(ssl)
            # the distance gap behind every code (EuclideanCodebook.quantize: -(|x|^2 - 2 x.e + |e|^2))
            x = vq.ssl_proj(ssl)[0].transpose(0, 1)
            e = vq.quantizer.vq.layers[0]._codebook.embed
            dist = -(x.pow(2).sum(1, keepdim=True) - 2 * x @ e.t() + e.pow(2).sum(1)[None])
            top = dist.topk(2, dim=1).values
            assert torch.equal(dist.argmax(1), codes[0, 0])
            last = ssl[0].transpose(0, 1)
            out[name + "_seconds"] = np.float64(secs)
            out[name + "_Th"] = np.int64(last.shape[0])
            rows = np.arange(0, last.shape[0], ROW_STEP[name])
            out[name + "_rows"] = rows
            out[name + "_last"] = last.numpy()[rows]
            out[name + "_codes"] = codes[0, 0].numpy()
            out[name + "_margin"] = (top[:, 0] - top[:, 1]).numpy()
            print(name, "Th", last.shape[0], "codes", tuple(codes.shape), "min margin %.3g" % (top[:, 0] - top[:, 1]).min().item())
    path = os.path.join(ROOT, "tests", "golden", "hubert.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
