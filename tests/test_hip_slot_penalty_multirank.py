"""Per-text repetition penalty and start suppression through TTS.infer_batched in two processes (in the form of
tests/test_hip_slot_sampling_multirank.py): the lists are arguments of the collective call, every rank holds them, and a request
is penalised against its own prompt and tokens only -- so two ranks return, sample for sample, what one process returns."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_hip_multirank import TEXTS, _free_port, _make_tts, _spk

pytestmark = pytest.mark.gpu

PENALTY = [1.35, 1.0, 1.1, 2.0, 1.35, 1.0, 1.5]
STEPS = [10, 0, 3, 10, 0, 5, 10]


def _call(tts, **kw):
    return tts.infer_batched(_spk(), "prompt.wav", "prompt text.", TEXTS, top_k=1, noise_scale=0.0, cut_minlen=8,
                             sovits_batch_size=3, **kw)


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tts = _make_tts(dev, with_refs=(rank == 0))
    tts.gather_dst = None
    clips = _call(tts, repetition_penalty=PENALTY, initial_suppression_steps=STEPS)
    ret[rank] = [c.audio_data for c in clips]
    dist.barrier()
    dist.destroy_process_group()


def test_penalised_call_two_ranks_equal_one_process():
    assert torch.cuda.is_available()
    assert len(PENALTY) == len(STEPS) == len(TEXTS)
    dev = torch.device("cuda:0")
    tts = _make_tts(dev, True)
    single = _call(tts, repetition_penalty=PENALTY, initial_suppression_steps=STEPS)
    assert len(single) == len(TEXTS) and all(len(c.audio_data) > 3200 for c in single)
    with pytest.raises(ValueError, match="initial_suppression_steps.*2.*%d" % len(TEXTS)):
        _call(tts, initial_suppression_steps=[10, 0])
    world, port = 2, _free_port()
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    for clips in (ret[0], ret[1]):
        assert len(clips) == len(single)
        for a, b in zip(clips, single):
            assert a.shape == b.audio_data.shape and np.array_equal(a, b.audio_data)
