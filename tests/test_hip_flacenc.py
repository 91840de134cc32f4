"""GPU checks of the FLAC writer: the frames encoded on the device (flac_enc_frames_kernel behind gsv_flac_encode and
flacio.encode_flacs) byte for byte against the serial host encoder built from the same scalar pieces, batches against
single clips, and the facade: a generated clip saved as FLAC and handed back as reference audio."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flacenc_cases as E  # noqa: E402
import wav_writer as ww  # noqa: E402

from gsv_tts_lite_amd import _native as N  # noqa: E402
from gsv_tts_lite_amd import flacio, synth  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 1234
PRO = "synthetic://sovits?version=v2Pro&seed=%d" % SEED
RATES = (8000, 32000, 44100, 11025, 12345)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("bits", E.BITS)
@pytest.mark.parametrize("block", E.BLOCKS)
def test_device_equals_host(dev, tmp_path, block, bits):
    clips = [(name, x, RATES[i % len(RATES)]) for i, (name, x) in enumerate(E.grid_clips(block, bits))]
    for c0 in range(0, len(clips), N.AUX_MAX_CLIPS):
        part = clips[c0:c0 + N.AUX_MAX_CLIPS]
        args = ([x for _, x, _ in part], [r for _, _, r in part], [bits] * len(part), [block] * len(part))
        host, got = E.encode_abi(*args), E.encode_abi(*args, dev=dev)
        assert host.rc == 0 and got.rc == 0, N.lib().gsv_last_error()
        assert np.array_equal(got.offsets, host.offsets)
        total = int(host.offsets[-1])
        bad = np.nonzero(got.data[:total] != host.data[:total])[0]
        if len(bad):
            f = int(np.searchsorted(host.offsets, bad[0], side="right")) - 1
            raise AssertionError("frame %d differs at its byte %d: device %s, host %s" % (
                f, bad[0] - host.offsets[f], got.choice(f), host.choice(f)))
        assert bytes(got.choices) == bytes(host.choices)
        assert np.all(got.data[total:] == 0xA5), "bytes behind the last frame were written"
    # the files, read back on the device: q / 2^(bits-1) as fp32
    files = flacio.encode_flacs([torch.from_numpy(x).to(dev) for _, x, _ in clips], [r for _, _, r in clips], bits=bits,
                                block_size=block)
    paths = []
    for (name, _, _), data in zip(clips, files):
        paths.append(str(tmp_path / (name + ".flac")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    for (name, x, rate), (w, sr) in zip(clips, flacio.load_flacs(paths, dev)):
        assert sr == rate and w.device == dev and w.dtype == torch.float32
        assert torch.equal(w.cpu(), torch.from_numpy((E.quantise(x, bits) / 2.0 ** (bits - 1)).astype(np.float32))), name


def test_the_measuring_entry_writes_the_same_bytes(dev):
    """gsv_flac_encode_timed, with the lane-split CRC-16 and with the one-lane pass it is measured against, gives the bytes,
    offsets and choices of gsv_flac_encode: VERBATIM 24-bit frames (the longest), a short last frame, 16-bit speech-like"""
    xs = [E.signal("noise", 2 * 4608 + 5, seed=1), E.signal("tone", 4096 + 37, seed=2), E.signal("outlier", 1000, seed=3),
          E.signal("special", 65, seed=4), E.signal("const", 17, seed=5)]
    args = (xs, [32000] * 5, [24, 16, 16, 24, 16], [4608, 4096, 1000, 16, 192])
    want = E.encode_abi(*args, dev=dev)
    assert want.rc == 0
    for serial in (0, 1):
        got = E.encode_abi(*args, dev=dev, timed=serial)
        assert got.rc == 0, N.lib().gsv_last_error()
        assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.data, want.data)
        assert bytes(got.choices) == bytes(want.choices)
        assert all(0 <= t < 1000 for t in got.ms), got.ms


def test_batch_equals_single(dev):
    rng = np.random.default_rng(11)
    n = N.AUX_MAX_CLIPS + 1                                     # 65 clips: past one call's cap
    lengths = [int(v) for v in rng.integers(1, 3 * 4096, n)]
    lengths[:4] = [1, 4096, 4097, 2 * 4096 + 37]
    xs = [E.signal(E.SIGNALS[i % len(E.SIGNALS)], ln, seed=i) for i, ln in enumerate(lengths)]
    bits = [(16, 24)[i % 2] for i in range(n)]
    rates = [RATES[i % len(RATES)] for i in range(n)]
    blocks = [(4096, 1000, 4608, 192)[i % 4] for i in range(n)]
    single = [flacio.encode_flac(x, r, bits=b, block_size=bs, device=dev) for x, r, b, bs in zip(xs, rates, bits, blocks)]
    order = [int(i) for i in np.random.default_rng(5).permutation(n)]
    packed = torch.from_numpy(np.concatenate(xs)).to(dev)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    views = [packed[starts[i]:starts[i + 1]] for i in range(n)]             # read in place
    apart = [torch.from_numpy(x).to(dev) for x in xs]                       # packed with one torch.cat
    for o in (list(range(n)), order):
        pick = lambda seq: [seq[i] for i in o]      # noqa: E731
        for waves in (pick(xs), pick(views), pick(apart), pick([x.astype(np.float64) for x in xs])):
            got = flacio.encode_flacs(waves, pick(rates), bits=pick(bits), block_size=pick(blocks), device=dev)
            assert len(got) == n
            for j, i in enumerate(o):
                assert got[j] == single[i], (o[:3], i)
    host = flacio.encode_flacs(xs, rates, bits=bits, block_size=blocks, device="cpu")
    assert host == single


# ------------------------------------------------------------------------------------------------------------ facade
def _toy_frontend(text):
    ids = [1 + (ord(c) * 7) % 690 for c in text if not c.isspace()]
    return ids, {"word": list(text), "ph": [1] * len(text)}, None, text


def _wav(path, rate, seconds, i):
    w = synth.synth_audio(i, int(rate * seconds)).astype(np.float64)
    x = np.clip(np.round(w * 2.0 ** 15), -2.0 ** 15, 2.0 ** 15 - 1).astype(np.int64)[:, None]
    return ww.write(path, x, "s16", rate)


def test_a_generated_clip_saved_as_flac_is_reference_audio(dev, tmp_path):
    from gsv_tts import TTS
    models = tmp_path / "models"
    synth.write_hubert_dir(str(models / "chinese-hubert-base"), seed=SEED)
    synth.write_sv_ckpt(str(models / "sv" / "pretrained_eres2netv2w24s4ep4.ckpt"), seed=SEED)
    tts = TTS(gpt_cache=[(1, 128), (1, 160)], sovits_cache=[50, 55], models_dir=str(models), device=str(dev), dtype="bfloat16")
    tts.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=1.0")
    tts.load_sovits_model(PRO)
    tts.set_text_frontend(_toy_frontend)
    spk, prm = _wav(tmp_path / "spk.wav", 32000, 1.5, 3), _wav(tmp_path / "prompt.wav", 16000, 1.0, 7)
    clip = tts.infer(spk, prm, "prompt text.", "Hello there, to a file", top_k=1, noise_scale=0.0, return_subtitles=True)
    assert len(clip.audio_data) > 6400
    gen = str(tmp_path / "gen.flac")
    clip.save(gen, is_save_subtitles=True)
    with open(tmp_path / "gen.json", encoding="utf-8") as f:
        assert json.load(f) == clip.subtitles
    with open(gen, "rb") as f:
        raw = f.read()
    assert raw[:4] == b"fLaC" and clip.to_flac() == raw
    q = E.quantise(clip.audio_data, 16)
    want = torch.from_numpy((q / 2.0 ** 15).astype(np.float32))
    w, sr = flacio.load_flac(gen, dev)
    assert sr == clip.samplerate and torch.equal(w.cpu(), want)
    info, frames, data = flacio.parse_flac(gen)
    rc, (ints,), status = E.decode_host([(info, frames, data)])
    assert rc == 0 and not status.any() and np.array_equal(ints[:, 0], q)
    tts.cache_spk_audio(gen, sovits_model=PRO)
    tts.cache_spk_audio("gen-arr", sovits_model=PRO, audio=want, sample_rate=clip.samplerate)
    assert torch.equal(tts.spk_audio_cache[gen]["ge"][PRO], tts.spk_audio_cache["gen-arr"]["ge"][PRO])
    again = tts.infer(gen, prm, "prompt text.", "Hello again", top_k=1, noise_scale=0.0)
    assert len(again.audio_data) > 3200 and np.isfinite(again.audio_data).all()
