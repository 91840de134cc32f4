"""The oracle of the stream-limiter tests: DESIGN 4.23 restated in fp64.  A stream is limited as ONE clip by stages 1 - 6 of 4.22
(limiter_ref.Limited up to y1: the envelope, the gain each sample needs, the hold, the release, the attack, the product), with no
trim and no rule for a clip under its ceiling; sample n is final once x[n + L + 5] has arrived, so after N samples max(0, N - D)
have been emitted, D = L + 5, and a flush emits the rest.  In fp64 a window of ones averages to one, so the local rule of 4.23
changes nothing here.  Nothing here is shared with the product code (csrc/limstream.h, gsv_tts_lite_amd/limiter.py)."""
import numpy as np

import limiter_ref as R


def delay(L):
    return L + 5


class StreamLimited:
    """y: the stream's output; overshoot: the true peak of y over T (what the missing trim would have taken away; 1 or less when
    nothing passes the ceiling)"""

    def __init__(self, x, ceiling_db, L, Rel):
        ref = R.Limited(x, ceiling_db, L, Rel)
        self.T, self.e, self.c, self.h, self.r, self.g = ref.T, ref.e, ref.c, ref.h, ref.r, ref.g
        self.y = ref.y1
        self.true_peak_in = ref.true_peak_in
        self.true_peak_y = ref.true_peak_y1
        self.overshoot = ref.true_peak_y1 / ref.T


def counts(cuts, L):
    """cuts: the lengths of the pushes, the last one flushing -> what each emits"""
    D, seen, out, res = delay(L), 0, 0, []
    for k, n in enumerate(cuts):
        seen += n
        due = seen if k + 1 == len(cuts) else max(0, seen - D)
        res.append(due - out)
        out = due
    return res


def cut_every(n, step):
    """pushes of `step` samples and the rest; the last one flushes"""
    cuts = [min(step, n - at) for at in range(0, n, step)]
    return cuts or [0]


def cut_random(n, seed, flush_empty=True):
    """a seeded cutting with short, long and empty pushes; the flush an empty push of its own"""
    rng = np.random.default_rng(seed)
    cuts, at = [], 0
    while at < n:
        m = 0 if rng.random() < 0.2 else int(rng.integers(1, 40 if rng.random() < 0.5 else 1500))
        m = min(m, n - at)
        cuts.append(m)
        at += m
    if flush_empty or not cuts:
        cuts.append(0)
    return cuts
