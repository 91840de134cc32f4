"""Per-text sampling parameters through TTS.infer_batched in two processes (in the form of tests/test_hip_multirank.py): the
lists are arguments of the collective call, every rank holds them, and a request's tokens depend on its own parameters and
seed only -- so two ranks return, sample for sample, what one process returns for a call that mixes greedy and sampled texts."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_hip_multirank import TEXTS, _free_port, _make_tts, _spk

pytestmark = pytest.mark.gpu

TOP_K = [15, 1, 5, 15, 1, 50, 0]
TEMP = [1.2, 1.0, 0.8, 1.0, 1.0, 0.6, 1.0]
TOP_P = [0.9, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]
SEED = [101, 102, 103, 104, 105, 106, 107]      # own seeds: no rank draws a call seed from its own generator


def _call(tts):
    return tts.infer_batched(_spk(), "prompt.wav", "prompt text.", TEXTS, top_k=TOP_K, temperature=TEMP, top_p=TOP_P, seed=SEED,
                             noise_scale=0.0, cut_minlen=8, sovits_batch_size=3)


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tts = _make_tts(dev, with_refs=(rank == 0))
    tts.gather_dst = None
    clips = _call(tts)
    ret[rank] = [c.audio_data for c in clips]
    dist.barrier()
    dist.destroy_process_group()


def test_mixed_call_two_ranks_equal_one_process():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    tts = _make_tts(dev, True)
    single = _call(tts)
    assert len(single) == len(TEXTS) and all(len(c.audio_data) > 3200 for c in single)
    world, port = 2, _free_port()
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    for clips in (ret[0], ret[1]):
        assert len(clips) == len(single)
        for a, b in zip(clips, single):
            assert a.shape == b.audio_data.shape and np.array_equal(a, b.audio_data)
