"""CPU checks of the per-request sampling arguments of infer_batched (gsv_tts_lite_amd.slot_sampling): scalar or
per-request, lengths and types, greedy / top-p rules, seeds and noise streams, and how the segments cut from a text inherit
the text's values.  Host functions only: the product itself still raises without a GPU (tests/test_abi.py)."""
import ctypes

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import _native as N
from gsv_tts_lite_amd import slot_sampling as SS


def test_all_scalars_bind_no_table():
    assert SS.resolve(5, 15, 1.0, 1.0) is None
    assert SS.resolve(5, 1, None, 0.8, None) is None
    assert SS.resolve(5, np.int64(15), torch.tensor(0.9), np.float32(1.0)) is None      # 0-d values are scalars
    assert SS.resolve(5, [15] * 5, 1.0, 1.0) is not None
    assert SS.resolve(5, 15, 1.0, 1.0, seed=7) is not None                               # a seed asks for the request-keyed noise
    assert SS.resolve(5, 15, 1.0, 1.0, seed=[None] * 5) is not None


@pytest.mark.parametrize("name", ["top_k", "top_p", "temperature", "seed"])
def test_wrong_length_names_the_argument_and_both_lengths(name):
    kw = {"top_k": 15, "top_p": 1.0, "temperature": 1.0, "seed": None}
    kw[name] = [1, 1, 1]
    with pytest.raises(ValueError) as e:
        SS.resolve(4, **kw)
    msg = str(e.value)
    assert name in msg and "3" in msg and "4" in msg


def test_types_are_checked_per_entry():
    with pytest.raises(TypeError, match=r"top_k\[1\]"):
        SS.resolve(2, [5, 2.5], 1.0, 1.0)
    with pytest.raises(TypeError, match=r"temperature\[0\]"):
        SS.resolve(2, 5, 1.0, ["hot", 1.0])
    with pytest.raises(TypeError, match=r"seed\[1\]"):
        SS.resolve(2, 5, 1.0, 1.0, seed=[1, 1.5])
    with pytest.raises(TypeError, match=r"top_k\[0\]"):
        SS.resolve(2, [True, 3], 1.0, 1.0)


def test_modes_top_p_and_sequence_kinds():
    s = SS.resolve(5, np.array([1, 5, 15, 0, 50]), torch.tensor([1.0, 0.9, 0.0, 0.5, 1.5]), (1.0, 0.8, 1.2, 1.0, 0.6))
    assert s.mode == [0, 2, 2, 2, 2]                      # top_k == 1 is greedy for that request
    assert s.top_k == [1, 5, 15, 0, 50]
    assert s.top_p == [1.0, pytest.approx(0.9), 1.0, 0.5, 1.0]     # outside (0, 1): off
    assert s.temperature == [1.0, 0.8, 1.2, 1.0, 0.6]
    assert SS.resolve(2, [3, 4], None, 1.0).top_p == [1.0, 1.0]
    assert SS.resolve(2, [3, 4], [None, 0.3], 1.0).top_p == [1.0, 0.3]
    assert SS.resolve(3, [1, 1, 1], 1.0, 1.0).any_sampled is False


def test_call_seed_is_drawn_once_and_only_if_a_request_samples():
    draws = []
    draw = lambda: draws.append(1) or (5 << 31 | 9)
    s = SS.resolve(3, [1, 1, 1], 1.0, 1.0)
    assert s.begin(draw) == (0, 0) and not draws
    s = SS.resolve(3, [1, 15, 5], 1.0, 1.0)
    assert s.begin(draw) == (2, 5 << 31 | 9) and len(draws) == 1
    # the call's seed, stream = request index + 1: what a scalar call writes into ctl[5], ctl[6] / tok_override
    assert s.entry(1) == (2, 15, 1.0, 1.0, 9, 5) and s.stream(1) == 2 and s.stream(2) == 3
    assert s.entry(0)[0] == 0


def test_own_seed_means_stream_zero_whatever_the_index():
    s = SS.resolve(3, 15, 1.0, 1.0, seed=[None, 77, (3 << 31) + 4])
    s.begin(lambda: 1000)
    assert [s.stream(i) for i in range(3)] == [1, 1, 1]
    assert s.entry(0)[4:] == (1000, 0) and s.entry(1)[4:] == (77, 0) and s.entry(2)[4:] == (4, 3)
    one = SS.resolve(1, 15, 1.0, 1.0, seed=[77])
    one.begin(lambda: 5)
    assert one.entry(0) == s.entry(1) and one.stream(0) == s.stream(1)
    assert SS.split_seed(2 ** 62 - 1) == (0x7fffffff, 0x7fffffff)


def test_segments_inherit_their_texts_values():
    seg2orig = [0, 0, 0, 1, 2, 2]                         # text 0 cut into three segments, text 2 into two
    assert SS.per_segment("top_k", [1, 5, 15], 3, seg2orig) == [1, 1, 1, 5, 15, 15]
    assert SS.per_segment("seed", (7, None, 9), 3, seg2orig) == [7, 7, 7, None, 9, 9]
    assert SS.per_segment("temperature", 0.8, 3, seg2orig) == 0.8       # a scalar stays one value for the call
    assert SS.per_segment("top_p", None, 3, seg2orig) is None
    with pytest.raises(ValueError, match="temperature.*2.*3"):
        SS.per_segment("temperature", [0.8, 1.0], 3, seg2orig)


def test_table_entry_layout_matches_the_header():
    assert ctypes.sizeof(N.SlotSampling) == 32
    e = N.SlotSampling(2, 15, 0.8, 0.9, 9, 5)
    words = np.frombuffer(bytes(e), dtype=np.int32)
    assert words[:2].tolist() == [2, 15] and words[4:].tolist() == [9, 5, 0, 0]
    assert np.frombuffer(bytes(e), dtype=np.float32)[2:4].tolist() == [np.float32(0.8), np.float32(0.9)]
