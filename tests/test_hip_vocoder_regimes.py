"""Every kernel regime of the bf16 vocoder against the CPU oracle, at the smallest shapes that reach it.

The bf16 vocoder picks its kernels by length (csrc/gsv_voc.hip, csrc/voc_launch.h): the flow runs flowmerge_* up to 1 024 frames,
the staged flowstage_kernel up to 2 048 and flowfuse_kernel beyond; the Generator's 256-channel stage runs wdma.h below 16 384 rows
and cgemm.h from there on; cgemm.h K-splits its launches only while 3 * tiles <= 256.  The other oracle tests stop at T = 500, and
the tests that go further compare two HIP passes with each other.  Here each regime is compared with VocoderOracle(numerics="bf16"):
at its real thresholds (from both sides), and -- with the host-side switches GSV_FLOW_MERGED_MAX_T / GSV_FLOW_STAGED_MAX_T /
GSV_CGEMM256_MIN_ROWS / GSV_CGEMM_NO_SPLIT -- at lengths around ONE tile of each form, where a last tile of 1 row or of tile - 1 rows
and the k = 5 halo across a tile edge show.  GSV_VOC_TRACE=1 makes the launchers say which family ran, and every case asserts it, so a
case can never move silently to another path.

The switches are read once per process: every environment is ONE child process (all its lengths), run strictly one after another; the
child writes an .npz and its stderr is the trace.  The oracle runs here, on the CPU.

Bounds come from the oracle pair alone.  D = |oracle_bf16 - oracle_fp32| on the same input is the reference's own rounding distance;
with err = |hip - oracle_bf16|:
    mean(err) <= 1.5 * mean(D)   and   max(err) <= 2 * max(D)
    T >= 48: the mean error of EVERY frame (192 flow channels / 640 samples) <= 2.0 * the global mean error
    T <  48: mean(err) <= 2 * mean(D) only
bf16 noise is uniform over time (the oracle pair's own per-frame ratio is asserted <= 1.5 here), while one wrong halo row or one
misplaced tile is hundreds of times the mean in its frame and invisible in a mean over 2 500 frames: the per-frame rule is the one
that localises.

Long Generator lengths use WINDOWED oracle passes: the Generator's receptive field is finite, oracle.dec(z[:, a:b]) equals
oracle.dec(z)[a * 640 : b * 640] bit for bit 12 frames from a cut (test_generator_window_identity_cpu), so the HIP side runs the whole
length and the oracle 160-frame windows, compared 32 frames from each cut side.

MEASURED on MI355X (every case prints its line: err/D of the means, err/D of the maxima, worst frame's mean error over the global mean
error; in brackets the oracle pair's own worst frame ratio):
    flow, mean(D) 3.0e-3 .. 3.1e-3, max(D) 1.4e-2 .. 2.5e-2:
        merged  T = 27 .. 1 024      0.56 .. 0.66 | 0.73 .. 1.36 | 1.24 .. 1.42   (1.09 .. 1.18)
        staged  T = 1 025 .. 2 048   0.67         | 1.11 .. 1.50 | 1.42 .. 1.48   (1.18 .. 1.22)
        fused   T = 2 049, 2 500     0.67         | 1.28, 1.39   | 1.49, 1.40     (1.21, 1.24)
        staged, forced, T = 31 .. 131   0.57 .. 0.72 | 0.80 .. 1.09 | 1.27 .. 1.39   (1.12 .. 1.19)
        fused, forced, T = 47 .. 625    0.64 .. 0.68 | 0.80 .. 1.40 | 1.25 .. 1.48   (1.12 .. 1.26)
        T = 1 (all three forms): err/D mean 0.03, max 0.40
        fp32, T = 2 800, unfused: max 2.3e-6, mean 3.7e-7 against the fp32 oracle
    Generator, mean(D) 2.3e-3 .. 3.3e-3, max(D) 1.7e-2 .. 2.6e-2:
        v2Pro cgemm<256> at 10 / 260 / 1 310 rows   0.88 / 0.96 / 0.97 | 1.01 / 1.07 / 0.99 | - / 1.32 / 1.17   (- / 1.32 / 1.13)
        v2Pro cgemm<256> at 16 390 rows             0.97 | 0.97 | 1.13   (1.13)
        v2Pro wdma<256> at 16 380 rows              0.98 | 1.05 | 1.16   (1.17)
        v2ProPlus T = 9 / 136 / 137                 0.97 / 0.99 / 0.99 | 0.85 / 1.09 / 0.94 | - / 1.15 / 1.15   (1.14)
        v2ProPlus T = 537 / 538 (windows)           0.99 / 0.99 | 0.90 / 1.02 | 1.20 / 1.13   (1.14 / 1.11)
        v2ProPlus unsplit T = 9 / 136               0.97 / 0.99 | 1.06 / 0.98 | - / 1.14   (1.14)
The max rule's closest case is the staged flow at T = 1 550 (1.50 of 2); the per-frame rule's, the fused flow at T = 2 049 (1.49 of 2).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gsv_tts_lite_amd import synth

pytestmark = pytest.mark.gpu
SEED = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN, MARGIN = 160, 32          # oracle window / frames from a cut that are not compared


# ---- inputs (the issue's: hashed_uniform("ff.z%d"), seed 11, last 9 frames masked, ge broadcast or per frame) ---------------------

def _mask(T):
    m = np.ones(T, np.float32)
    if T > 20:
        m[T - 9:] = 0.0
    return m


def _z(T, scale):
    return synth.hashed_uniform("ff.z%d" % T, (1, 192, T), SEED) * np.float32(scale)


def _ge_spec(T, per_frame):
    """[(speaker, frames)]: broadcast = one column; per frame = four utterances of three speakers, the first coming back, the
    speaker changes near 20 / 50 / 80 % of the length and never on a multiple of a tile size (28, 32, 48)."""
    if not per_frame:
        return [(3, 1)]
    cuts, lo = [], 1
    for f in (0.2, 0.5, 0.8):
        c = max(lo, int(T * f))
        while c % 28 == 0 or c % 32 == 0 or c % 48 == 0:
            c += 1
        cuts.append(c)
        lo = c + 1
    assert cuts[-1] < T, T
    edges = [0] + cuts + [T]
    return [(s, edges[i + 1] - edges[i]) for i, s in enumerate((3, 4, 5, 3))]


def _ge(spec):
    return np.concatenate([np.repeat(synth.synth_ge(i, 1024, SEED), n, axis=2) for i, n in spec], axis=2)


# ---- the children: one per environment, every length of that environment in it ---------------------------------------------------

PER_FRAME_FLOW = {27, 29, 131, 1024, 1025, 2048, 2049}        # default child: the two ge forms alternate, the thresholds take per-frame
FLOW_DEFAULT = [(T, "flow_merged") for T in (1, 27, 28, 29, 56, 131, 1024)] + [(T, "flow_staged") for T in (1025, 1550, 2048)] + \
               [(T, "flow_fused") for T in (2049, 2500)]
FLOW_STAGED_SMALL = [(T, "flow_staged") for T in (1, 31, 32, 33, 131)]
FLOW_FUSED_SMALL = [(T, "flow_fused") for T in (1, 47, 48, 49, 131, 625)]


def _flow_case(T, per_frame):
    return {"name": "flow%d" % T, "op": "flow", "T": T, "ge": _ge_spec(T, per_frame)}


def _dec_case(T, per_frame):
    return {"name": "dec%d" % T, "op": "dec", "T": T, "ge": _ge_spec(T, per_frame)}


def _alternate(Ts):
    return [(T, bool(i & 1)) for i, T in enumerate(Ts)]


CHILDREN = {
    "pro-default": dict(ver="v2Pro", dtype="bfloat16", env={},
                        cases=[_flow_case(T, T in PER_FRAME_FLOW) for T, _ in FLOW_DEFAULT] + [_dec_case(1639, True), _dec_case(1638, True)]),
    "pro-staged-small": dict(ver="v2Pro", dtype="bfloat16", env={"GSV_FLOW_MERGED_MAX_T": "0"},
                             cases=[_flow_case(T, pf) for T, pf in _alternate([T for T, _ in FLOW_STAGED_SMALL])]),
    "pro-fused-small": dict(ver="v2Pro", dtype="bfloat16", env={"GSV_FLOW_STAGED_MAX_T": "0"},
                            cases=[_flow_case(T, pf) for T, pf in _alternate([T for T, _ in FLOW_FUSED_SMALL])]),
    "pro-cgemm256-small": dict(ver="v2Pro", dtype="bfloat16", env={"GSV_CGEMM256_MIN_ROWS": "1", "GSV_CGEMM_NO_SPLIT": "1"},
                               cases=[_dec_case(T, pf) for T, pf in _alternate([1, 26, 131])]),
    "plus-default": dict(ver="v2ProPlus", dtype="bfloat16", env={},
                         cases=[_dec_case(T, pf) for T, pf in _alternate([9, 136, 137])] + [_dec_case(537, True), _dec_case(538, True)]),
    "plus-nosplit": dict(ver="v2ProPlus", dtype="bfloat16", env={"GSV_CGEMM_NO_SPLIT": "1"},
                         cases=[_dec_case(T, pf) for T, pf in _alternate([9, 136])]),
    "pro-fp32": dict(ver="v2Pro", dtype="float32", env={}, cases=[_flow_case(2800, True)]),
}
SWITCHES = ("GSV_FLOW_MERGED_MAX_T", "GSV_FLOW_STAGED_MAX_T", "GSV_FLOW_STAGED_RPB", "GSV_CGEMM256_MIN_ROWS", "GSV_CGEMM_NO_SPLIT", "GSV_NO_CGEMM",
            "GSV_NO_WDMA", "GSV_NO_WUPS", "GSV_NO_RBFUSE", "GSV_NO_GE_SEGMENTS", "GSV_FF_NOROT", "GSV_FF_DEBUG", "GSV_VOC_TRACE")

CHILD_CODE = r"""
import json, sys
import numpy as np, torch
job = json.load(open(sys.argv[1]))
sys.path[:0] = job["path"]
from gsv_tts_lite_amd import synth
from gsv_tts_lite_amd.sovits import _VocoderNative
inp = np.load(job["inputs"])
dev = torch.device("cuda:0")
hps = synth.sovits_hps(job["ver"])
w = synth.sovits_weights(hps, seed=job["seed"], hot_path_only=True)
v = _VocoderNative(hps["model"], {k: torch.from_numpy(a) for k, a in w.items()}, getattr(torch, job["dtype"]), dev)
out = {}
for c in job["cases"]:
    name, T = c["name"], c["T"]
    ge = np.concatenate([np.repeat(synth.synth_ge(i, 1024, job["seed"]), n, axis=2) for i, n in c["ge"]], axis=2)
    z, g = torch.from_numpy(inp[name + "_z"]).to(dev), torch.from_numpy(ge).to(dev)
    torch.cuda.synchronize()
    sys.stderr.write("[case] %s\n" % name); sys.stderr.flush()
    if c["op"] == "flow":
        o = v.flow(z, torch.from_numpy(inp[name + "_mask"]).to(dev).reshape(1, 1, T), g)
    else:
        o = v.dec(z, g)
    torch.cuda.synchronize()
    out[name] = o.cpu().numpy()
np.savez(job["out"], **out)
"""


def _case_input(c):
    """what the child AND the oracle see: the flow's z_p, or the Generator's z with the masked frames zeroed"""
    T = c["T"]
    if c["op"] == "flow":
        return _z(T, 1.3)
    return _z(T, 1.2) * _mask(T)[None, None, :]


class _Children:
    """runs a child at most once; after a child that died (signal, abort, time limit) no further child is started"""

    def __init__(self, tmp):
        self.tmp, self.done, self.dead = tmp, {}, None

    def get(self, key):
        if key not in self.done:
            if self.dead:
                pytest.fail("child %r ended abnormally earlier in this module: no further child is started on the device" % self.dead)
            self.done[key] = self._run(key)
        p, outs, trace = self.done[key]
        assert p.returncode == 0, "child %s exit %s\n%s" % (key, p.returncode, p.stderr[-2000:])
        return outs, trace

    def _run(self, key):
        ch = CHILDREN[key]
        inputs = {}
        for c in ch["cases"]:
            inputs[c["name"] + "_z"] = _case_input(c)
            if c["op"] == "flow":
                inputs[c["name"] + "_mask"] = _mask(c["T"])
        fin, fout, fjob = (str(self.tmp / (key + s)) for s in (".in.npz", ".out.npz", ".json"))
        np.savez(fin, **inputs)
        with open(fjob, "w") as f:
            json.dump(dict(path=[ROOT, os.path.join(ROOT, "gsv-tts-lite_amd")], inputs=fin, out=fout, ver=ch["ver"], dtype=ch["dtype"],
                           seed=SEED, cases=ch["cases"]), f)
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(ch["env"])
        env["GSV_VOC_TRACE"] = "1"
        try:
            p = subprocess.run([sys.executable, "-c", CHILD_CODE, fjob], env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            self.dead = key
            raise
        if p.returncode != 0:
            if p.returncode < 0 or p.returncode in (134, 137, 139):
                self.dead = key
            return p, None, None
        trace, cur = {}, None
        for line in p.stderr.splitlines():
            if line.startswith("[case] "):
                cur = trace.setdefault(line[7:].strip(), [])
            elif line.startswith("[voc] ") and cur is not None:
                cur.append(line[6:].strip())
        return p, np.load(fout), trace


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    return _Children(tmp_path_factory.mktemp("regimes"))


# ---- the oracle pair, computed once per (model, case) and shared -----------------------------------------------------------------

_ORACLES, _REF = {}, {}


def _oracle(ver):
    if ver not in _ORACLES:
        from oracle import oracle as orc
        hps = synth.sovits_hps(ver)
        w = synth.sovits_weights(hps, seed=SEED, hot_path_only=True)
        _ORACLES[ver] = (orc.VocoderOracle(hps, w, numerics="bf16"), orc.VocoderOracle(hps, w))
    return _ORACLES[ver]


def _flow_ref(ver, c):
    key = (ver, c["name"], json.dumps(c["ge"]))
    if key not in _REF:
        o16, o32 = _oracle(ver)
        z, m, ge = _case_input(c)[0], _mask(c["T"]), _ge(c["ge"])[0]
        _REF[key] = (o16.flow(z, m, ge), o32.flow(z, m, ge))
    return _REF[key]


def _windows(T, which):
    """[(a, b, first compared frame, one past the last compared frame)]: the true start and the true end are not cuts"""
    if which == "full":
        return [(0, T, 0, T)]
    w = []
    if "head" in which:
        w.append((0, WIN, 0, WIN - MARGIN))
    if "mid" in which:
        a = (T - WIN) // 2
        w.append((a, a + WIN, a + MARGIN, a + WIN - MARGIN))
    if "tail" in which:
        w.append((T - WIN, T, T - WIN + MARGIN, T))
    return w


def _dec_ref(ver, c, which):
    """the oracle pair's samples of the compared frames, and those frames: ([n_frames][640] bf16, [n_frames][640] fp32, frame numbers)"""
    key = (ver, c["name"], json.dumps(c["ge"]), which)
    if key not in _REF:
        o16, o32 = _oracle(ver)
        T = c["T"]
        z, ge = _case_input(c)[0], _ge(c["ge"])[0]
        r16, r32, frames = [], [], []
        for a, b, lo, hi in _windows(T, which):
            g = ge if ge.shape[1] == 1 else ge[:, a:b]
            for o, dst in ((o16, r16), (o32, r32)):
                dst.append(o.dec(np.ascontiguousarray(z[:, a:b]), np.ascontiguousarray(g)).reshape(b - a, 640)[lo - a:hi - a])
            frames.append(np.arange(lo, hi))
        _REF[key] = (np.concatenate(r16), np.concatenate(r32), np.concatenate(frames))
    return _REF[key]


# ---- the rules -----------------------------------------------------------------------------------------------------------------

def _check(tag, T, hip, r16, r32, frames):
    """hip / r16 / r32: [n_frames][values per frame] over the compared frames `frames`"""
    assert hip.shape == r16.shape and np.isfinite(hip).all(), tag
    err = np.abs(hip.astype(np.float64) - r16)
    D = np.abs(r16.astype(np.float64) - r32)
    ferr, fD = err.mean(axis=1), D.mean(axis=1)
    worst = int(np.argmax(ferr))
    print("%s: err/D mean %.2f (%.2e / %.2e) max %.2f (%.2e / %.2e); worst frame %d at %.2f x the mean error; oracle pair alone %.2f"
          % (tag, err.mean() / D.mean(), err.mean(), D.mean(), err.max() / D.max(), err.max(), D.max(), int(frames[worst]),
             ferr[worst] / err.mean(), fD.max() / D.mean()))
    if T < 48:
        assert err.mean() <= 2.0 * D.mean(), (tag, err.mean(), D.mean())
        return
    assert fD.max() <= 1.5 * D.mean(), (tag, "the oracle pair itself is not uniform over the frames: change the input", fD.max() / D.mean())
    broken = []                    # every rule is evaluated, so a failure names all it breaks -- the per-frame one says WHERE
    if not err.mean() <= 1.5 * D.mean():
        broken.append("mean(err) %.3e > 1.5 * mean(D) %.3e" % (err.mean(), D.mean()))
    if not err.max() <= 2.0 * D.max():
        broken.append("max(err) %.3e > 2 * max(D) %.3e" % (err.max(), D.max()))
    if not ferr[worst] <= 2.0 * err.mean():
        broken.append("frame %d: mean error %.3e > 2 * the global mean error %.3e" % (int(frames[worst]), ferr[worst], err.mean()))
    assert not broken, (tag, broken)


def _check_flow(children, child, T, family):
    ch = CHILDREN[child]
    c = next(c for c in ch["cases"] if c["name"] == "flow%d" % T)
    outs, trace = children.get(child)
    flows = [l for l in trace[c["name"]] if l.startswith("flow_")]
    assert flows == ["%s C=192 rows=%d" % (family, T)], (child, T, flows)
    out = outs[c["name"]]
    assert out.shape == (1, 192, T)
    out, m = out[0], _mask(T)
    f16, f32 = _flow_ref(ch["ver"], c)
    assert np.isfinite(out).all()
    if T > 20:
        assert np.abs(out[:, T - 9:]).max() == 0.0, "masked frames must come back exactly 0.0"
    keep = np.nonzero(m)[0]
    return out, f16, f32, keep


# ---- flow ------------------------------------------------------------------------------------------------------------------------

def _flow_regime(children, child, T, family):
    out, f16, f32, keep = _check_flow(children, child, T, family)
    _check("%s flow T=%d %s" % (child, T, family), T, out[:, keep].T, f16[:, keep].T, f32[:, keep].T, keep)


@pytest.mark.parametrize("T,family", FLOW_DEFAULT)
def test_flow_bf16_shipped_regimes_vs_bf16_oracle(children, T, family):
    """What ships, nothing forced: flowmerge_* up to 1 024 frames (last tile of 1 / 27 / 28 rows of FM_VR = 28, the halo across a tile
    edge), flowstage_kernel at 1 025 / 1 550 / 2 048, flowfuse_kernel at 2 049 (43 tiles, per_xcd 22, one empty slot) and 2 500 (53
    tiles, per_xcd 27), both thresholds from both sides and with per-frame ge.  Measured ratios: the module docstring."""
    _flow_regime(children, "pro-default", T, family)


@pytest.mark.parametrize("T,family", FLOW_STAGED_SMALL)
def test_flow_bf16_staged_form_at_tile_edges_vs_bf16_oracle(children, T, family):
    """GSV_FLOW_MERGED_MAX_T=0: the ten-launch staged form (ships at 1 025 .. 2 048 frames) around one FS_ROWS = 32 tile: a last tile
    of 1 and of 31 rows, the k = 5 halo read from the neighbour tile's rows."""
    _flow_regime(children, "pro-staged-small", T, family)


@pytest.mark.parametrize("T,family", FLOW_FUSED_SMALL)
def test_flow_bf16_fused_kernel_at_tile_edges_vs_bf16_oracle(children, T, family):
    """GSV_FLOW_STAGED_MAX_T=0: flowfuse_kernel (ships above 2 048 frames; the only flow kernel infer_batched and the continuous-batching
    vocoder stage run) around one FF_VR = 48 tile: a last tile of 1 and of 47 rows, the halo across the edge, and 625 frames = 14 tiles,
    so the rot_k walk (tile % 12) wraps."""
    _flow_regime(children, "pro-fused-small", T, family)


def test_flow_fp32_unfused_at_the_grid_cap_vs_fp32_oracle(children):
    """fp32 flow at T = 2 800, where the 2 048-block grid caps of the element-wise kernels (flip, gate) wrap, against the fp32 oracle
    with the bound this suite holds fp32 to (test_hip_vocoder.py: atol 1e-4).  In a child of its own: the trace switch is read once per
    process."""
    T = 2800
    out, _, f32, _ = _check_flow(children, "pro-fp32", T, "flow_unfused")
    err = np.abs(out - f32)
    print("fp32 flow T=%d vs fp32 oracle: max %.2e mean %.2e" % (T, err.max(), err.mean()))
    np.testing.assert_allclose(out, f32, atol=1e-4)


# ---- Generator -------------------------------------------------------------------------------------------------------------------

def _launches(trace, family, C):
    return [l for l in trace if l.startswith("%s C=%d " % (family, C))]


def _dec_regime(children, child, T, which, expect):
    """expect: [(family, C, rows, split or None, launches)] that the trace must hold, [(family, C)] with launches = 0 that it must not"""
    ch = CHILDREN[child]
    c = next(c for c in ch["cases"] if c["name"] == "dec%d" % T)
    outs, trace = children.get(child)
    tr = trace[c["name"]]
    for family, C, rows, split, n in expect:
        got = _launches(tr, family, C)
        if n == 0:
            assert got == [], (child, T, got)
            continue
        want = "%s C=%d rows=%d" % (family, C, rows) + (" split=%s" % split if split else "")
        assert got == [want] * n, (child, T, want, got)
    out = outs[c["name"]]
    assert out.shape == (1, 1, T * 640) and np.isfinite(out).all()
    r16, r32, frames = _dec_ref(ch["ver"], c, which)
    _check("%s dec T=%d %s" % (child, T, which), T, out.reshape(T, 640)[frames], r16, r32, frames)


@pytest.mark.parametrize("T", [1, 26, 131])
def test_generator_bf16_cgemm256_small_tiles_vs_bf16_oracle(children, T):
    """GSV_CGEMM256_MIN_ROWS=1 GSV_CGEMM_NO_SPLIT=1: cgemm_kernel<256,128,256,4> (ships from 16 384 rows on, never K-split: its 128
    tiles fail 3 * tiles <= 256) at 10 rows, at 260 rows (the second 256-row tile holds 4) and at 1 310 rows (the sixth holds 30)."""
    _dec_regime(children, "pro-cgemm256-small", T, "full", [("cgemm", 256, 10 * T, "1,1,1", 6), ("wdma", 256, 0, None, 0)])


def test_generator_bf16_cgemm256_at_its_threshold_vs_bf16_oracle(children):
    """Nothing forced: T = 1 639 = 16 390 rows, the first length on cgemm<256> (65 row tiles, the last with 6 rows); head, middle
    (across a speaker change) and tail windows."""
    _dec_regime(children, "pro-default", 1639, "head+mid+tail", [("cgemm", 256, 16390, "1,1,1", 6), ("wdma", 256, 0, None, 0)])


def test_generator_bf16_wdma256_at_its_largest_row_count_vs_bf16_oracle(children):
    """Nothing forced: T = 1 638 = 16 380 rows, the largest row count wdma_kernel<256, ...> ships at; tail window."""
    _dec_regime(children, "pro-default", 1638, "tail", [("wdma", 256, 16380, None, 6), ("cgemm", 256, 0, None, 0)])


@pytest.mark.parametrize("T,split192", [(9, "3,1,1"), (136, "3,1,1"), (137, "1,1,1")])
def test_generator_bf16_v2proplus_cgemm192_split_threshold_vs_bf16_oracle(children, T, split192):
    """v2ProPlus, nothing forced: the 192-channel stage (80 rows per frame) K-splits at T = 136 (85 tiles) and not at 137 (86); the
    384-channel stage splits at all three."""
    _dec_regime(children, "plus-default", T, "full", [("cgemm", 384, 10 * T, "3,2,1", 6), ("cgemm", 192, 80 * T, split192, 6)])


@pytest.mark.parametrize("T,split384", [(537, "3,2,1"), (538, "1,1,1")])
def test_generator_bf16_v2proplus_cgemm384_split_threshold_vs_bf16_oracle(children, T, split384):
    """v2ProPlus, nothing forced: the 384-channel stage (10 rows per frame, two channel tiles) K-splits at T = 537 (84 tiles) and not
    at 538 (86); head and tail windows."""
    _dec_regime(children, "plus-default", T, "head+tail", [("cgemm", 384, 10 * T, split384, 6), ("cgemm", 192, 80 * T, "1,1,1", 6)])


@pytest.mark.parametrize("T", [9, 136])
def test_generator_bf16_v2proplus_cgemm_unsplit_vs_bf16_oracle(children, T):
    """v2ProPlus with GSV_CGEMM_NO_SPLIT=1: the one-block-per-tile form of cgemm<384> / cgemm<192> at the lengths the default splits."""
    _dec_regime(children, "plus-nosplit", T, "full", [("cgemm", 384, 10 * T, "1,1,1", 6), ("cgemm", 192, 80 * T, "1,1,1", 6)])


# ---- the window identity the long cases lean on (CPU work only; it rides with this file's mark) --------------------------------------------------------------------------

def test_generator_window_identity_cpu():
    """oracle.dec(z[:, a:b]) == oracle.dec(z)[a * 640 : b * 640] bit for bit once 12 frames from a cut, in both numerics, with the
    window's own slice of a per-frame ge (T = 260, window [60, 200))."""
    T, a, b, far = 260, 60, 200, 12
    c = _dec_case(T, True)
    z, ge = _case_input(c)[0], _ge(c["ge"])[0]
    for o in _oracle("v2Pro"):
        full = o.dec(z, ge).reshape(T, 640)
        win = o.dec(np.ascontiguousarray(z[:, a:b]), np.ascontiguousarray(ge[:, a:b])).reshape(b - a, 640)
        assert np.array_equal(win[far:b - a - far], full[a + far:b - far]), o.numerics
        assert not np.array_equal(win[:far], full[a:a + far]), "the cut must show near the cut (else this test compares nothing)"
