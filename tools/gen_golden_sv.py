"""TEST INFRASTRUCTURE -- writes tests/golden/sv.npz from the reference's ERes2NetV2 module (SV/ERes2NetV2.py, fusion.py).

Runs only where the reference tree is present (the build container); the tests read the npz and need neither.  The
reference's SV package __init__ imports sv.py, which needs torchaudio, so the packages above ERes2NetV2.py are stubbed
and only ERes2NetV2.py / fusion.py / pooling_layers.py are imported from the tree.  Weights are not stored:
synth.sv_weights(seed, m_channels) regenerates them bit-identically everywhere; inputs are synth.sv_feat.

    python tools/gen_golden_sv.py

Cases (seed 1234).  Random fp32 does not compress, so the file keeps to ~0.2 MB by storing:
  m64_T1, m64_T37         forward3 output, all 20480 values (ERes2NetV2(baseWidth=24, scale=4, expansion=4))
  m64_T298, m64_T998      forward3 output at every 4th index (<case>_step)
  m16_T37, m16_T298       the same model at m_channels=16, all 5120 values
  m64_T37_{layer1, layer3, fuse34}   activations [C][F][T] at the strided slice <name>_slice (start, step per dim)
torchaudio is not importable here, so the resample / fbank restatement in tests/sv_ref.py is checked against it only
when it is (see check_torchaudio); otherwise that part stays unpinned, as DESIGN notes.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gsv-tts-lite_amd"), os.path.join(ROOT, "tests")]

from gsv_tts_lite_amd import synth  # noqa: E402

SEED = 1234
CASES = [("m64_T1", 64, 1, 1), ("m64_T37", 64, 37, 1), ("m64_T298", 64, 298, 4), ("m64_T998", 64, 998, 4),
         ("m16_T37", 16, 37, 1), ("m16_T298", 16, 298, 1)]
# activations stored at [start::step] per dim of [C][F][T]
TAP_SLICES = {"layer1": (7, 3, 1), "layer3": (5, 2, 1), "fuse34": (3, 1, 1)}
TAP_STEPS = {"layer1": (32, 8, 4), "layer3": (64, 4, 4), "fuse34": (128, 2, 2)}


def import_eres2netv2():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_harness import REF_ROOT
    base = os.path.join(REF_ROOT, "gsv_tts")
    for name, path in (("gsv_tts", base), ("gsv_tts.GPT_SoVITS", os.path.join(base, "GPT_SoVITS")),
                       ("gsv_tts.GPT_SoVITS.SV", os.path.join(base, "GPT_SoVITS", "SV"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    return importlib.import_module("gsv_tts.GPT_SoVITS.SV.ERes2NetV2").ERes2NetV2


def check_torchaudio():
    """resample / fbank restatement against torchaudio, where it is importable"""
    try:
        import torchaudio
    except ImportError:
        print("torchaudio not importable: resample / fbank restatement unpinned")
        return
    import sv_ref
    a = synth.synth_audio(3, 32000 * 2, SEED)
    want = torchaudio.transforms.Resample(32000, 16000)(torch.from_numpy(a)[None])[0].numpy()
    got = sv_ref.resample(a, 32000, 16000)
    print("resample vs torchaudio max|d| %.3g" % np.abs(got - want).max())
    import torchaudio.compliance.kaldi as kaldi
    fw = kaldi.fbank(torch.from_numpy(want)[None], num_mel_bins=80, sample_frequency=16000, dither=0).numpy()
    print("fbank vs torchaudio max|d| %.3g" % np.abs(sv_ref.fbank(want) - fw).max())


def main():
    torch.set_num_threads(16)
    ERes2NetV2 = import_eres2netv2()
    out = {"seed": np.int64(SEED), "torch_version": torch.__version__}
    models = {}
    with torch.inference_mode():
        for name, m, T, step in CASES:
            if m not in models:
                net = ERes2NetV2(baseWidth=24, scale=4, expansion=4, m_channels=m).eval()
                sd = {k: torch.from_numpy(v) for k, v in synth.sv_weights(SEED, m).items()}
                missing, unexpected = net.load_state_dict(sd, strict=False)
                assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
                models[m] = net
            net = models[m]
            feat = torch.from_numpy(synth.sv_feat(T, T, SEED))[None]
            emb = net.forward3(feat.clone())[0].numpy()
            out[name + "_T"] = np.int64(T)
            out[name + "_step"] = np.int64(step)
            out[name + "_emb"] = emb[::step]
            print(name, "emb", emb.shape, "mean|.| %.3f" % np.abs(emb).mean())
        net = models[64]
        feat = torch.from_numpy(synth.sv_feat(37, 37, SEED))[None]
        x = feat.permute(0, 2, 1)[:, None]
        o = torch.relu(net.bn1(net.conv1(x)))
        o1 = net.layer1(o)
        o3 = net.layer3(net.layer2(o1))
        o4 = net.layer4(o3)
        fuse = net.fuse34(o4, net.layer3_ds(o3))
        for tap, v in (("layer1", o1[0]), ("layer3", o3[0]), ("fuse34", fuse[0])):
            st, sp = TAP_SLICES[tap], TAP_STEPS[tap]
            sl = v[st[0]::sp[0], st[1]::sp[1], st[2]::sp[2]].numpy().copy()
            out["m64_T37_" + tap] = sl
            out["m64_T37_%s_slice" % tap] = np.array([st, sp], np.int64)
            if tap != "fuse34":
                print(tap, tuple(v.shape), "Hardtanh-clipped fraction %.4f (at 0: %.3f)" % ((v >= 20).float().mean().item(),
                                                                                          (v <= 0).float().mean().item()))
    check_torchaudio()
    path = os.path.join(ROOT, "tests", "golden", "sv.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
