"""CPU tests of the host arithmetic of the segmented decode: batchmath.segment_frames, the per-text expansion of speed /
noise_scale to segments, and the argument checks TTS.infer_batched makes before it touches a device."""
import pytest

from gsv_tts_lite_amd.batchmath import per_text_values, segment_frames


def test_segment_frames_is_the_reference_count_per_utterance():
    """int(2 l / speed) + 1 in Python doubles (models.py:217), 2 l at speed 1; (110 frames, 1.1) and (9 frames, 0.6) are the pairs
    test_decode_frame_count_is_the_callers_at_every_speed names as those where an fp32 evaluation disagrees"""
    assert segment_frames([55], [1.1]) == [(int(110 / 1.1) + 1, 0)] == [(100, 0)]      # 110 / 1.1 is 99.99999999999999 in doubles
    lengths, speeds = [], []
    for l in list(range(1, 160)) + [1000, 4095]:
        for s in (1, 1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.25, 1.3, 1.7, 2.0, 3.0):
            lengths.append(l)
            speeds.append(s)
    got = segment_frames(lengths, speeds)
    first = 0
    for l, s, (frames, f0) in zip(lengths, speeds, got):
        assert frames == (2 * l if s == 1 else int(2 * l / s) + 1), (l, s)
        assert isinstance(frames, int) and isinstance(f0, int) and frames >= 1
        assert f0 == first
        first += frames
    # 9 frames is a streaming chunk (an odd count does not occur here); 9 TOKENS at 0.6 are 18 / 0.6 = 30.000000000000004 -> 31
    assert segment_frames([9], [0.6]) == [(int(18 / 0.6) + 1, 0)] == [(31, 0)]
    assert segment_frames([7, 140, 1], [1.0, 1.3, 2.0]) == [(14, 0), (216, 14), (2, 230)]
    assert segment_frames([], []) == []


def test_segment_frames_refuses_bad_input():
    with pytest.raises(ValueError):
        segment_frames([3, 4], [1.0])
    with pytest.raises(ValueError):
        segment_frames([0], [1.0])
    with pytest.raises(ValueError):
        segment_frames([3], [0.0])
    with pytest.raises(ValueError):
        segment_frames([3], [-1.0])


def test_per_text_values_follow_seg2orig():
    """the segments cut from a text inherit its value, as slot_sampling.per_segment does for the sampling arguments"""
    from gsv_tts_lite_amd.slot_sampling import per_segment
    seg2orig = [0, 0, 1, 2, 2, 2]
    assert per_text_values("speed", [1.0, 1.25, 0.8], 3, seg2orig) == [1.0, 1.0, 1.25, 0.8, 0.8, 0.8]
    assert per_text_values("speed", [1.0, 1.25, 0.8], 3, seg2orig) == per_segment("speed", [1.0, 1.25, 0.8], 3, seg2orig)
    assert per_text_values("noise_scale", 0.5, 3, seg2orig) == [0.5] * 6
    import numpy as np
    vals = per_text_values("speed", np.array([1.0, 2.0]), 2, [1, 0])
    assert vals == [2.0, 1.0] and all(type(v) is float for v in vals)
    with pytest.raises(ValueError):
        per_text_values("speed", [1.0, 1.25], 3, seg2orig)


def test_infer_batched_checks_list_lengths_before_any_device_work():
    """a TTS with no model loaded and no device: the wrong-length list must be what stops the call"""
    from gsv_tts_lite_amd.tts import TTS
    tts = TTS(device="cpu", dtype="float32")
    texts = ["one.", "two.", "three."]
    with pytest.raises(ValueError, match="speed has 2 entries for 3"):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt.", texts, speed=[1.0, 1.25])
    with pytest.raises(ValueError, match="noise_scale has 4 entries for 3"):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt.", texts, speed=[1.0, 1.25, 0.8], noise_scale=[0.0] * 4)
    with pytest.raises(ValueError, match="positive"):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt.", texts, speed=[1.0, 0.0, 0.8])
    assert tts.gpt_models == {} and tts.sovits_models == {}
