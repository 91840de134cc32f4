"""The cases of the decode-step K/V edge tests above 16 sequences and their oracle side, shared by tests/test_hip_decode_kv_edges.py
(the HIP kernels against the oracle) and tests/test_decode_kv_edges_cpu.py (the proof, on the oracle alone, that the bounds of the
former separate a correct row mask from an off-by-one).  Nothing here touches a GPU.

A regime is (handle dtype, cache bucket T, start lengths): one sequence per start length, -1 = a parked slot.  One layer everywhere:
decode_hidden hands `xin` to layer 0 directly.

Why the inputs are built and not drawn: with K / V ~ N(0, 1) a row of a sequence of n >= 255 rows holds a softmax weight of ~1 / n, and
dropping it moves the hidden state by 9e-4 .. 3e-3 -- inside the one-layer bf16 bound (3e-3).  So (build()):
  1. every row of K and V, the rows at and behind a sequence's length included, is seeded N(0, 1) rounded to bf16 (a stale row looks
     like what a finished request left there);
  2. q = xin @ Wqkv[:512].T + b[:512], per head;
  3. the DESIGNATED rows of a live sequence of n >= 1 rows -- 0, m - 1, m (m = 64 * floor((n - 1) / 64): either side of the last 64-row
     chunk edge below the last live row) and n - 1 -- get the key q_h * t in every head, t such that q.k / sqrt(32) = ln n + |q_h|^2 / 64:
     an ordinary row's score is N(0, |q_h|^2 / 32), so n of them sum to ~ n exp(|q_h|^2 / 64) and each designated row holds about as much
     softmax mass as all ordinary rows together;
  4. every row from n to T - 1 gets the same aligned key (row n is the one the step overwrites): a dead row that leaks into the softmax
     moves the result as much as a designated row that is skipped.  All values are finite.
`xin` is N(0, 1) per sequence, redrawn until no element of the K / V row the step appends is smaller than MIN_ROW_ABS (evaluated in
float64 on the operands the regime's QKV dots take, appended_rows_exact()).  The GPU file holds that row to ONE bf16 ulp of the oracle's,
|d| <= 2^-7 |value|, which presumes that the two fp32 summation orders differ by less than an ulp of the value.  That fails where a
512-term dot of terms of ~5e-2 cancels to a residue: at -6.3e-06 (the first draw of control-chain-1024, sequence 5, K element 360) the
fp32 oracle is itself three bf16 ulps from the float64 value of the same dot.  The oracle's fp32 dots are at most ORACLE_DOT_ERR from
float64 (test_decode_kv_edges_cpu.py measures it); an ulp of a value of MIN_ROW_ABS is 2^-8 x 4e-3 = 1.6e-05, 7 x that error, so that
with a kernel whose sums are a few times worse than the oracle's the two roundings are still at most one ulp apart.  About one draw in
nine passes.

Which pair of `multi-fp32` shows what (t2s_attn_multi_kernel<.., 2>: sequences 2k and 2k + 1 share a block; the issue's order had both
parked slots in the first place of their pair, so 767 and the second parked slot changed places):
  (1023, 1)   long with short: the second sequence's first chunk is prefetched in the first one's LAST chunk, not its first
  (0, 127)    short with short; a sequence without cache rows
  (128, 129)  either side of the 128-row iteration edge, (255, 256) of the 256-row chunk edge, (383, 384) / (385, 511) / (512, 513) /
              (768, 769): edge with edge
  (-1, 257)   a parked slot in the FIRST place, (767, -1) in the SECOND
  (1022,)     B = 21 is odd: the last block repeats its only sequence
`multi-bf16-long` (B = 17): (2047, -1) has the parked slot in the second place, (700,) is the odd block."""
import functools
import math

import numpy as np

from gsv_tts_lite_amd import synth

W_SEED = 4321
BATCHED_MIN = 17         # the library's default switch to the batched chain (gsv_t2s_batched_min); the GPU file passes the handle's own
FFN_SLICES = 32          # gsv_t2s_ffn_slices above 4 sequences
H, DH, D = 16, 32, 512
MIN_ROW_ABS = 4e-3       # smallest |element| of an appended K / V row (module docstring)
ORACLE_DOT_ERR = 2e-6    # ceiling on |oracle's fp32 QKV dot - the float64 one| over the regimes (measured 1.5e-6: test_decode_kv_edges_cpu.py)

# id: (handle, T, start lengths)
REGIMES = {
    "chain-1024": ("bf16", 1024, (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 383, 384, 385, 511, 512, 513, 640, 641,
                                  767, 768, 769, 1022, 1023, -1, -1)),
    "chain-512": ("bf16", 512, (0, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 510, 511, -1, 300)),
    "chain-256": ("bf16", 256, (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 254, 255, -1, 100, -1)),
    "multi-fp32": ("fp32", 1024, (1023, 1, 0, 127, 128, 129, 255, 256, -1, 257, 383, 384, 385, 511, 512, 513, 767, -1, 768, 769, 1022)),
    "multi-bf16-long": ("bf16", 2048, (0, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2046, 2047, -1, 700)),
}
EDGE_IDS = tuple(REGIMES)


def control_lengths(lens):
    """the lengths of a regime moved inside their 64-row chunk to 5 .. 58 rows behind its edge: at least 5 rows from every multiple of
    64, and from T (a multiple of 64).  Parked slots stay parked."""
    return tuple(n if n < 0 else 64 * (n // 64) + 5 + (7 * n) % 54 for n in lens)


for _id in EDGE_IDS:      # one control per regime: the same handle, B and T
    REGIMES["control-" + _id] = REGIMES[_id][:2] + (control_lengths(REGIMES[_id][2]),)
CONTROL_IDS = tuple("control-" + i for i in EDGE_IDS)


def round_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def config_weights():
    cfg = synth.gpt_config(n_layer=1)
    return cfg, synth.gpt_weights(cfg, seed=W_SEED)


def designated_rows(n):
    """the designated rows of a live sequence of n rows, deduplicated, in the order (0, m - 1, m, n - 1)"""
    if n < 1:
        return ()
    m = 64 * ((n - 1) // 64)
    out = []
    for r in (0, m - 1, m, n - 1):
        if 0 <= r < n and r not in out:
            out.append(r)
    return tuple(out)


def appended_rows_exact(handle, T, xin, fp32_weights=False):
    """[B, 1024] float64: the K and V row a step appends for xin [B, 512], before any rounding of the result, on the operands the QKV
    dots of the regime take: bf16 weights on a bf16 handle, and bf16 activations too on the batched chain (a cache of at most 1024 rows;
    every regime has >= BATCHED_MIN sequences); fp32 both on an fp32 handle (or with fp32_weights: what the fp32 oracle multiplies)"""
    bf16 = handle == "bf16" and not fp32_weights
    wkv, bias = _kv_weights64(bf16)
    x = np.asarray(xin, np.float32)
    if bf16 and T <= 1024:
        x = round_bf16(x)
    return x.astype(np.float64) @ wkv.T + bias


@functools.lru_cache(maxsize=None)
def _kv_weights64(bf16):
    _, w = config_weights()
    wkv = w["t2s_transformer.blocks.0.qkv.weight"][D:]
    return (round_bf16(wkv) if bf16 else wkv).astype(np.float64), w["t2s_transformer.blocks.0.qkv.bias"][D:].astype(np.float64)


@functools.lru_cache(maxsize=None)
def build(rid):
    """dict(handle, T, B, lens, live, xin [B, 512], k, v [1, B, 16, T, 32] (bf16-representable fp32), kv_len int64 [B], q [B, 16, 32],
    rows (per sequence: its designated rows)); every array read-only"""
    handle, T, lens = REGIMES[rid]
    B = len(lens)
    _, w = config_weights()
    rng = np.random.default_rng(1 + sorted(REGIMES).index(rid))
    xin = rng.normal(size=(B, D)).astype(np.float32)
    redraw = np.random.default_rng(1001 + sorted(REGIMES).index(rid))
    for b in range(B):       # no appended K / V element below MIN_ROW_ABS (module docstring)
        while np.abs(appended_rows_exact(handle, T, xin[b:b + 1])).min() < MIN_ROW_ABS:
            xin[b] = redraw.normal(size=D).astype(np.float32)
    k = round_bf16(rng.normal(size=(1, B, H, T, DH)).astype(np.float32))
    v = round_bf16(rng.normal(size=(1, B, H, T, DH)).astype(np.float32))
    wq = np.asarray(w["t2s_transformer.blocks.0.qkv.weight"], np.float64)[:D]
    bq = np.asarray(w["t2s_transformer.blocks.0.qkv.bias"], np.float64)[:D]
    q = (xin.astype(np.float64) @ wq.T + bq).reshape(B, H, DH)
    rows = []
    for b, n in enumerate(lens):
        rows.append(designated_rows(n))
        if n < 0:
            continue
        qq = (q[b] ** 2).sum(-1)                                                    # [H]
        t = (math.log(max(n, 1)) + qq / 64.0) * math.sqrt(DH) / qq
        key = round_bf16((q[b] * t[:, None]).astype(np.float32))                    # [H, 32]
        for r in rows[-1]:
            k[0, b, :, r] = key
        k[0, b, :, n:] = key[:, None, :]
    assert np.isfinite(k).all() and np.isfinite(v).all()
    case = dict(handle=handle, T=T, B=B, lens=tuple(lens), live=tuple(b for b, n in enumerate(lens) if n >= 0), xin=xin, k=k, v=v,
                kv_len=np.array(lens, np.int64), q=q.astype(np.float32), rows=tuple(rows))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def run_oracle(case, numerics, batched_min=BATCHED_MIN, n_sl=FFN_SLICES, k=None, kv_len=None):
    """one decode step of the oracle on the case's inputs (or on the K cache / lengths given instead): (hidden [B, 512], K, V after the
    step).  The oracle knows no parked slots: such a sequence is stepped at T - 1 (where the library parks its row), and its hidden row
    is returned as NaN -- nothing may compare it."""
    from oracle import oracle as orc
    cfg, w = config_weights()
    B, T = case["B"], case["T"]
    o = orc.T2SOracle(cfg, w, [(B, T)], numerics=numerics, batched_min=batched_min, ffn_slices=lambda bsz: n_sl)
    kc, vc = o.cache[B]
    kc[...] = case["k"] if k is None else k
    vc[...] = case["v"]
    kv = np.array(case["kv_len"] if kv_len is None else kv_len, np.int64)
    parked = kv < 0
    kv[parked] = T - 1
    assert (kv >= 0).all() and (kv <= T - 1).all()
    hid = o.decode(case["xin"], B, kv)
    hid[parked] = np.nan
    return hid, kc, vc


@functools.lru_cache(maxsize=None)
def reference(rid, numerics=None, batched_min=BATCHED_MIN, n_sl=FFN_SLICES):
    """(hidden, K, V) of the oracle in `numerics` (default: the handle's), computed once per process and read-only"""
    case = build(rid)
    out = run_oracle(case, numerics or case["handle"], batched_min, n_sl)
    for a in out:
        a.setflags(write=False)
    return out


def perturbations(case):
    """[(name, K cache or None, kv_len or None, sequences it changes)]: what a kernel with a wrong row mask would compute.
    (a) per designated-row kind (row 0, m - 1, m, n - 1): that row's key becomes -8 q in every head -- weight 0, a skipped row;
    (b) every sequence with n < T - 1 decoded at kv_len + 1: the first stale row admitted."""
    out = []
    B, T = case["B"], case["T"]
    for j, kind in enumerate(("row 0", "row m-1", "row m", "row n-1")):
        seqs = []
        k = case["k"].copy()
        for b in case["live"]:
            n = case["lens"][b]
            m = 64 * ((n - 1) // 64) if n >= 1 else 0
            r = (0, m - 1, m, n - 1)[j]
            if n >= 1 and 0 <= r < n and r not in (0, m - 1, m, n - 1)[:j]:
                assert r in case["rows"][b]
                k[0, b, :, r] = round_bf16(-8.0 * case["q"][b])
                seqs.append(b)
        if seqs:
            out.append(("(a) skips " + kind, k, None, tuple(seqs)))
    kv = case["kv_len"].copy()
    seqs = tuple(b for b in case["live"] if case["lens"][b] < T - 1)
    kv[list(seqs)] += 1
    out.append(("(b) admits row n", None, kv, seqs))
    covered = {(b, r) for b in case["live"] for r in case["rows"][b]}
    assert sum(len(p[3]) for p in out[:-1]) == len(covered)      # every designated row of every live sequence, once
    return out
