"""The bounds of tests/test_hip_prefill_edges.py discriminate -- shown on the oracle alone, no GPU.

That file holds the HIP prompt pass to `oracle.prefill` within 1e-2 (bf16 handles, max |hidden|; fp32 handles 2e-5).  Here
the oracle itself runs three off-by-one masks a kernel could compute (prefill_edges_cases.mutant_masks) at every shape of
the single-row grid: each must move the hidden states by at least 5 x 1e-2, so a kernel with such a mask cannot pass; and
the bf16-mode and fp32 oracles must stay closer than 1e-2 to each other at 3 layers, so the bound is not loose against the
precision of the format either.  The share of rows whose first sample the GPU file asserts is a property of the seeds:
it is asserted here too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_edges_cases as C  # noqa: E402

BOUND = 1e-2          # the GPU file's ceiling on max |hidden - oracle| of a bf16 handle
FACTOR = 5            # a mutant must move the hidden states by at least FACTOR x BOUND


@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("lx,ly", C.GRID)
def test_every_mask_mutant_moves_the_hidden_states_beyond_the_bound(numerics, lx, ly):
    o = C.oracle(numerics, 1)
    ref = C.reference(numerics, 1, ((lx, ly),))[0]
    masks = C.mutant_masks(lx, ly)
    # the first two change the mask at every shape (there is an audio query and a text query everywhere); the third does not
    # where the last key tile holds the last query's own key only
    assert {"audio_misses_own_key", "text_sees_key_lx"} <= set(masks)
    assert ("last_query_loses_last_tile" in masks) == ((lx + ly - 1) % 32 != 0)
    for name, mask in masks.items():
        h, _, _ = C.run_row(o, ref["embed"], mask)
        d = float(np.abs(h - ref["hidden"]).max())
        print("(%d, %d) %s %s: max |hidden - true| %.3e" % (lx, ly, numerics, name, d))
        assert d >= FACTOR * BOUND, (name, d)


def test_bf16_and_fp32_oracles_are_closer_than_the_bound_at_3_layers():
    worst = (0.0, 0.0)
    for lx, ly in C.GRID + [C.FULL]:
        a = C.reference("bf16", 3, ((lx, ly),))[0]["hidden"]
        b = C.reference("fp32", 3, ((lx, ly),))[0]["hidden"]
        d = np.abs(a - b)
        print("(%d, %d): bf16 vs fp32 oracle, 3 layers: max %.2e mean %.2e" % (lx, ly, d.max(), d.mean()))
        assert d.max() < BOUND, (lx, ly, d.max())
        worst = (max(worst[0], float(d.max())), max(worst[1], float(d.mean())))
    print("bf16 vs fp32 oracle over the grid: max %.2e, largest mean %.2e" % worst)


def test_first_sample_margin_share_of_the_seeds():
    share = C.margin_share(C.all_cases())
    print("rows whose oracle top-1 / top-2 gap clears the margin: %s" % share)
    for reg, (ok, n) in share.items():
        assert n > 50 and ok >= C.MARGIN_SHARE * n, (reg, ok, n)
