"""Index arithmetic of TTS.infer_batched around the vocoder batches, as functions so that it can be pinned against the
reference's own statements (tests/golden/facade.npz is produced by executing gsv_tts/TTS.py:705-720 and :806-816)."""
from __future__ import annotations

import torch


def balance_order(lengths: torch.Tensor) -> torch.Tensor:
    """TTS.py:705-716: sort the utterances by token count, then interleave the sorted list from both ends
    (shortest, longest, 2nd shortest, 2nd longest, ...) so that consecutive vocoder batches carry similar totals.
    Returns the permutation to apply to the completion-order lists."""
    order = torch.argsort(lengths)
    n = len(order)
    inter = torch.zeros(n, dtype=torch.long, device=lengths.device)
    srt = torch.arange(n, device=lengths.device)
    inter[0::2] = srt[:(n + 1) // 2]
    inter[1::2] = srt[(n + 1) // 2:].flip(0)
    return order[inter]


def split_bounds(lengths, samples_per_frame: int, speed: float):
    """TTS.py:806-811: sample ranges of the utterances inside one time-concatenated vocoder batch.  The running end is
    a float (lengths * 2 * samples_per_frame / speed accumulates un-rounded); each slice is [int(start), int(end))."""
    out, pos = [], 0
    for l in lengths:
        nxt = pos + l * 2 * samples_per_frame / speed
        out.append((int(pos), int(nxt)))
        pos = nxt
    return out


def segment_frames(lengths, speeds):
    """Per-utterance frame counts of a segmented vocoder batch (SynthesizerTrn.decode_segments): utterance i of l_i tokens
    at speed_i becomes 2 l_i frames at speed 1 and int(2 l_i / speed_i) + 1 otherwise -- the count models.py:217 gives that
    utterance decoded alone, in Python doubles -- and starts at the running sum of the counts before it.
    Returns [(out_frames, first_frame)]; the sample range of utterance i is (first_frame * hop, (first_frame + out_frames) * hop),
    integers throughout (no accumulated float, unlike split_bounds)."""
    if len(lengths) != len(speeds):
        raise ValueError("%d lengths for %d speeds" % (len(lengths), len(speeds)))
    out, first = [], 0
    for l, s in zip(lengths, speeds):
        l = int(l)
        if l < 1:
            raise ValueError("an utterance of %d tokens" % l)
        if not s > 0:
            raise ValueError("speed %r: must be positive" % (s,))
        frames = 2 * l if s == 1 else int(2 * l / s) + 1
        out.append((frames, first))
        first += frames
    return out


def per_text_values(name: str, value, n_texts: int, seg2orig):
    """TTS.infer_batched's per-text speed / noise_scale: one value per SEGMENT (the segments cut from a text inherit its
    value); a number is repeated, a sequence of another length than the texts raises ValueError."""
    from .slot_sampling import per_request
    vals = per_request(name, value, n_texts)
    return [vals[int(t)] for t in seg2orig]
