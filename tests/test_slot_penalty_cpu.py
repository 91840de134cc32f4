"""CPU checks of the per-request repetition penalty and start suppression of infer_batched (gsv_tts_lite_amd.slot_sampling):
when the two arguments make a call a table call, what a request's entry carries, validation, inheritance by segments, the
layout of the table entry and the public signatures.  Host functions only."""
import ctypes
import inspect

import numpy as np
import pytest

from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import slot_sampling as SS


def test_a_penalty_sequence_or_nonzero_steps_makes_a_table_call():
    assert SS.resolve(4, 15, 1.0, 1.0) is None
    assert SS.resolve(4, 15, 1.0, 1.0, None, 1.35, 0) is None                  # a scalar penalty is ignored, steps 0: the scalar call
    assert SS.resolve(4, 15, 1.0, 1.0, repetition_penalty=None, initial_suppression_steps=np.int64(0)) is None
    assert SS.resolve(4, 15, 1.0, 1.0, repetition_penalty=[1.35] * 4) is not None
    assert SS.resolve(4, 15, 1.0, 1.0, repetition_penalty=np.full(4, 1.35, np.float32)) is not None
    assert SS.resolve(4, 15, 1.0, 1.0, initial_suppression_steps=10) is not None
    assert SS.resolve(4, 15, 1.0, 1.0, initial_suppression_steps=[0, 0, 0, 0]) is not None


def test_entry_carries_the_two_fields():
    s = SS.resolve(4, 1, 1.0, 1.0, repetition_penalty=[1.35, 1.0, None, 2], initial_suppression_steps=[10, 0, 3, 10])
    assert [s.entry(i).rep_penalty for i in range(4)] == [1.35, 0.0, 0.0, 2.0]     # 1.0 / None: off, written as 0
    assert [s.entry(i).suppress_steps for i in range(4)] == [10, 0, 3, 10]
    assert s.any_penalised and [s.penalised(i) for i in range(4)] == [True, False, False, True]
    assert s.entry(0)[:4] == (0, 1, 1.0, 1.0) and len(s.entry(0)) == 6             # the sampling words stay where they were
    assert s.entry(3).words() == (0, 1, 1.0, 1.0, 0, 0, 2.0, 10)
    # a scalar penalty beside per-request steps stays ignored; scalar steps apply to every request
    s = SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=1.35, initial_suppression_steps=7)
    assert not s.any_penalised and [s.entry(i).words()[6:] for i in range(3)] == [(0.0, 7)] * 3
    # the other per-request arguments alone leave both off
    s = SS.resolve(2, [1, 15], 1.0, 1.0)
    assert [s.entry(i).words()[6:] for i in range(2)] == [(0.0, 0)] * 2


def test_validation_names_argument_and_index():
    with pytest.raises(ValueError, match=r"repetition_penalty\[2\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[1.35, 1.0, 0.0])
    with pytest.raises(ValueError, match=r"repetition_penalty\[0\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[-1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match=r"repetition_penalty\[1\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[1.0, float("nan"), 1.0])
    with pytest.raises(ValueError, match=r"repetition_penalty\[1\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[1.0, float("inf"), 1.0])
    with pytest.raises(TypeError, match=r"repetition_penalty\[1\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[1.0, "strong", 1.0])
    with pytest.raises(TypeError, match=r"repetition_penalty\[0\]"):
        SS.resolve(3, 15, 1.0, 1.0, repetition_penalty=[True, 1.0, 1.0])
    with pytest.raises(ValueError, match=r"initial_suppression_steps\[1\]"):
        SS.resolve(3, 15, 1.0, 1.0, initial_suppression_steps=[0, -1, 0])
    with pytest.raises(ValueError, match=r"initial_suppression_steps\[0\]"):
        SS.resolve(3, 15, 1.0, 1.0, initial_suppression_steps=-2)
    with pytest.raises(TypeError, match=r"initial_suppression_steps\[2\]"):
        SS.resolve(3, 15, 1.0, 1.0, initial_suppression_steps=[1, 2, 2.5])
    with pytest.raises(TypeError, match=r"initial_suppression_steps\[0\]"):
        SS.resolve(3, 15, 1.0, 1.0, initial_suppression_steps=2.5)
    for name in ("repetition_penalty", "initial_suppression_steps"):
        with pytest.raises(ValueError) as e:
            SS.resolve(4, 15, 1.0, 1.0, **{name: [1, 1, 1]})
        assert name in str(e.value) and "3" in str(e.value) and "4" in str(e.value)


def test_segments_inherit_their_texts_penalty_and_steps():
    seg2orig = [0, 0, 1, 2, 2, 2]
    assert SS.per_segment("repetition_penalty", [1.35, 1.0, 2.0], 3, seg2orig) == [1.35, 1.35, 1.0, 2.0, 2.0, 2.0]
    assert SS.per_segment("initial_suppression_steps", (10, 0, 3), 3, seg2orig) == [10, 10, 0, 3, 3, 3]
    assert SS.per_segment("repetition_penalty", 1.35, 3, seg2orig) == 1.35          # a number stays a number: ignored downstream
    assert SS.per_segment("initial_suppression_steps", 10, 3, seg2orig) == 10
    with pytest.raises(ValueError, match="repetition_penalty.*2.*3"):
        SS.per_segment("repetition_penalty", [1.35, 1.0], 3, seg2orig)


def test_table_entry_is_32_bytes_with_the_two_fields_at_24_and_28():
    assert ctypes.sizeof(N.SlotSampling) == 32
    assert N.SlotSampling.rep_penalty.offset == 24 and N.SlotSampling.suppress_steps.offset == 28
    s = SS.resolve(1, 15, 0.9, 0.8, seed=[(5 << 31) | 9], repetition_penalty=[1.35], initial_suppression_steps=10)
    raw = bytes(N.SlotSampling(*s.entry(0).words()))
    assert np.frombuffer(raw, np.int32)[[0, 1, 4, 5, 7]].tolist() == [2, 15, 9, 5, 10]
    assert np.frombuffer(raw, np.float32)[[2, 3, 6]].tolist() == [np.float32(0.8), np.float32(0.9), np.float32(1.35)]
    assert bytes(N.SlotSampling(2, 15, 0.8, 0.9, 9, 5))[24:] == bytes(8)            # an entry written as before: both off


def test_both_infer_batched_signatures_have_the_new_keyword():
    from gsv_tts_lite_amd.t2s import Text2SemanticDecoder
    from gsv_tts_lite_amd.tts import TTS
    for fn in (Text2SemanticDecoder.infer_batched, TTS.infer_batched):
        p = inspect.signature(fn).parameters
        assert p["initial_suppression_steps"].default == 0
        assert p["repetition_penalty"].default == 1.35
    assert "gsv_t2s_seed_seen" in N.EXPORTS
