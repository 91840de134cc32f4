"""GPU parity of the chunk epilogue of a stream (csrc/sola.h behind gsv_stream_emit) against what TTS.infer_stream does on the
host between a chunk's decode and its hand-out: `oracle.sola` for the offset, `stream.sola` for the spliced samples (bit for bit),
the head rule of TTS._find_head_threshold_offsets restated in float64, the tail kept back and the mute behind a final chunk; and
ChunkEmitter, which drives it, against ChunkSplicer's protocol."""
import numpy as np
import pytest
import torch

from oracle.gen_golden_inputs import facade_audio

pytestmark = pytest.mark.gpu

SR = 32000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _emit(dev, tail, chunk, ov, search, final, trim, mute):
    """the raw C call -> (out cut to rec[0], tail_out, rec)"""
    from gsv_tts_lite_amd import _native as N
    L = N.lib()
    x = torch.from_numpy(chunk).to(dev)
    t = None if tail is None else torch.from_numpy(tail).to(dev)
    n = int(x.numel())
    ws = torch.empty(L.gsv_stream_emit_workspace(search, n), dtype=torch.uint8, device=dev)
    out = torch.full((n + mute + 16,), 7.0, dtype=torch.float32, device=dev)       # 16 guard samples behind the capacity
    tail_out = torch.full((ov + 16,), 7.0, dtype=torch.float32, device=dev)
    rec = torch.full((4,), -5, dtype=torch.int32, device=dev)
    N.check(L.gsv_stream_emit(None if t is None else t.data_ptr(), x.data_ptr(), n, ov, search, int(final), int(trim), mute,
                              out.data_ptr(), tail_out.data_ptr(), rec.data_ptr(), ws.data_ptr(), ws.numel(),
                              N.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    rec = rec.tolist()
    out, tail_out = out.cpu().numpy(), tail_out.cpu().numpy()
    assert 0 <= rec[0] <= n + mute
    assert np.all(out[rec[0]:] == 7.0) and np.all(tail_out[ov:] == 7.0), "written past what the record names"
    return out[:rec[0]], tail_out[:ov], rec


def _head64(body):
    """TTS._find_head_threshold_offsets (tts.py:726-729) in float64; refuses a case the fp32 sum order could decide"""
    head = body[:64000].astype(np.float64)
    if head.shape[0] < 512:
        return head.shape[0]
    rms = np.sqrt((np.lib.stride_tricks.sliding_window_view(head, 512)[::256] ** 2).mean(axis=1))
    assert np.all(np.abs(rms - 0.02) > 0.01 * 0.02), "a frame's RMS within 1 % of the threshold"
    hit = np.nonzero(rms > 0.02)[0]
    return max(0, int(hit[0]) * 256 - 3200) if hit.size else head.shape[0]


def _want(dev, tail, chunk, ov, search, final, trim, mute):
    """the host's order (TTS.infer_stream): splice, keep the tail back, trim the head, append the mute"""
    from oracle import oracle as orc
    from gsv_tts_lite_amd.stream import sola
    if tail is None:
        s, k = chunk.copy(), 0
    else:
        s, k = sola(torch.from_numpy(tail).to(dev), torch.from_numpy(chunk).to(dev), search)
        s = s.cpu().numpy()
        assert k == orc.sola(tail, chunk, ov, search)[1]
    m = s.shape[0]
    body = s if final else s[: m - ov]
    h = _head64(body) if trim else 0
    out = np.concatenate([body[h:], np.zeros(mute if final else 0, np.float32)])
    return out, s[m - ov:], k, h


def _check(dev, tail, chunk, ov, search, final, trim, mute):
    want, want_tail, k, h = _want(dev, tail, chunk, ov, search, final, trim, mute)     # asserts the 1 % margin on the CPU first
    got, got_tail, rec = _emit(dev, tail, chunk, ov, search, final, trim, mute)
    assert rec == [want.shape[0], k, h, 0], (rec, want.shape[0], k, h)
    assert np.array_equal(got, want), "samples differ from stream.sola's"
    assert np.array_equal(got_tail, want_tail)
    return rec


def _tone(n, amp=0.3):
    return (amp * np.sin(2 * np.pi * 220.0 * np.arange(n) / SR)).astype(np.float32)


def test_splice_cases_equal_the_host_path(dev):
    rng = np.random.default_rng(23)
    for n, ov, search, final in [(5000, 640, 320, False), (700, 640, 320, False), (640, 640, 320, True), (12800, 3200, 0, False),
                                 (5000, 640, 320, True)]:
        base = rng.standard_normal(n + 2 * search + ov + 8).astype(np.float32)
        base = np.convolve(base, np.ones(7, np.float32) / 7, mode="same").astype(np.float32)
        shift = int(rng.integers(0, max(1, min(search, max(0, n - ov)) + 1)))
        at = search + 4
        tail = base[at: at + ov].copy()
        chunk = (base[at - shift: at - shift + n] + 0.05 * rng.standard_normal(n)).astype(np.float32)
        for trim in (False, True):      # a trim behind a splice: the head rule reads the cross-faded samples
            rec = _check(dev, tail, chunk, ov, search, final, trim, 0)
            assert rec[1] == shift, (n, ov, search, rec, shift)


def test_head_trim_cases(dev):
    ov = 640
    quiet_then_tone = np.concatenate([np.zeros(9000, np.float32), _tone(8000)])
    rec = _check(dev, None, quiet_then_tone, ov, 320, False, True, 0)
    assert rec[2] == 34 * 256 - 3200 and rec[0] == 17000 - ov - rec[2]           # frame 34 is the first to reach the tone
    assert _check(dev, None, quiet_then_tone, ov, 320, False, False, 0)[2] == 0     # not asked for: no trim
    rec = _check(dev, None, np.zeros(5000, np.float32), ov, 320, False, True, 0)    # all silence: the length searched
    assert rec[2] == 5000 - ov and rec[0] == 0
    rec = _check(dev, None, _tone(1000), ov, 320, False, True, 0)                   # a body under 512 samples
    assert rec[2] == 360 and rec[0] == 0
    late = np.concatenate([np.zeros(66000, np.float32), _tone(4000)])               # onset behind sample 64 000
    rec = _check(dev, None, late, ov, 320, False, True, 0)
    assert rec[2] == 64000 and rec[0] == 70000 - ov - 64000
    rec = _check(dev, None, _tone(6000), ov, 320, False, True, 0)                   # loud at once: frame 0, margin clamps to 0
    assert rec[2] == 0


def test_final_chunk_gets_its_mute(dev):
    rng = np.random.default_rng(5)
    ov, n, mute = 640, 5000, 19200
    tail = (0.2 * rng.standard_normal(ov)).astype(np.float32)
    chunk = np.concatenate([np.zeros(50, np.float32), tail, (0.2 * rng.standard_normal(n - ov - 50)).astype(np.float32)])
    rec = _check(dev, tail, chunk, ov, 320, True, False, mute)
    assert rec[1] == 50 and rec[0] == n - 50 + mute
    rec = _check(dev, None, np.concatenate([np.zeros(9000, np.float32), _tone(3000)]), ov, 320, True, True, mute)
    assert rec[2] > 0 and rec[0] == 12000 - rec[2] + mute
    assert _check(dev, tail, chunk, ov, 320, False, False, mute)[0] == n - 50 - ov  # no mute behind a chunk that is not the last


def test_stream_emit_rejects_bad_arguments(dev):
    from gsv_tts_lite_amd import _native as N
    L = N.lib()
    assert L.gsv_stream_emit_workspace(-1, 100) == 0 and L.gsv_stream_emit_workspace(320, -1) == 0
    assert L.gsv_stream_emit_workspace(320, 100) >= 321 * 4
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    tail, other, chunk, out, ws = z(100), z(100), z(400), z(500), torch.empty(4096, dtype=torch.uint8, device=dev)
    rec = torch.zeros(4, dtype=torch.int32, device=dev)
    st = N.current_stream_ptr(dev)

    def call(prev, n, ov, search, mute, tail_out, ws_bytes):
        return L.gsv_stream_emit(prev, chunk.data_ptr(), n, ov, search, 0, 0, mute, out.data_ptr(), tail_out, rec.data_ptr(),
                                 ws.data_ptr(), ws_bytes, st)
    assert call(tail.data_ptr(), 400, 100, 320, 0, other.data_ptr(), ws.numel()) == 0
    bad = [call(tail.data_ptr(), 50, 100, 320, 0, other.data_ptr(), ws.numel()),        # chunk shorter than the overlap, with a tail
           call(tail.data_ptr(), 400, 100, 320, -1, other.data_ptr(), ws.numel()),      # negative sizes
           call(tail.data_ptr(), 400, 100, -1, 0, other.data_ptr(), ws.numel()),
           call(tail.data_ptr(), -1, 100, 320, 0, other.data_ptr(), ws.numel()),
           call(tail.data_ptr(), 400, 0, 320, 0, other.data_ptr(), ws.numel()),
           call(tail.data_ptr(), 400, 100, 320, 0, other.data_ptr(), 64),               # workspace too small
           call(tail.data_ptr(), 400, 100, 320, 0, tail.data_ptr(), ws.numel()),        # tail_out aliases prev_tail
           call(tail.data_ptr(), 400, 100, 320, 0, None, ws.numel())]
    assert bad == [1] * len(bad), bad           # GSV_ERR_ARG (include/gsv_tts_hip.h), not a failed launch (GSV_ERR_HIP = 2)
    with pytest.raises(RuntimeError):
        N.check(bad[0])
    assert b"stream_emit" in N.lib().gsv_last_error()
    torch.cuda.synchronize(dev)
    from gsv_tts_lite_amd.stream import ChunkEmitter
    with pytest.raises(RuntimeError):
        ChunkEmitter(640).push(torch.zeros(1000), False)                                # host tensors: no CPU path


def test_chunk_emitter_protocol(dev):
    """the five-chunk signal of test_chunk_splicer_protocol (tests/test_hip_sola.py): the emitter hands out what the splicer plus
    the host rules hand out, bit for bit, with every chunk in flight at once"""
    from gsv_tts_lite_amd.stream import ChunkEmitter, ChunkSplicer
    ov, n_chunk, mute = 640, 6400, 1234
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    sp, em = ChunkSplicer(ov), ChunkEmitter(ov)
    handles, want, pos, shifts = [], [], 0, [0, 13, 200, 0, 77]
    for c, sh in enumerate(shifts):
        final = c == len(shifts) - 1
        start = pos - sh if c else 0
        chunk = torch.from_numpy(sm[start: start + n_chunk].copy()).to(dev)
        handles.append(em.push(chunk[None, None], final, trim_head=c == 0, mute_samples=mute if final else 0))
        want.append(sp.push(chunk[None, None], final).cpu().numpy())
        pos = start + n_chunk if final else start + n_chunk - ov
    got = [h.result() for h in handles]
    assert all(h.ready() for h in handles)
    assert [k for _, k, _ in got[1:]] == shifts[1:] == sp.offsets and got[0][1] == 0
    h0 = _head64(want[0])
    assert got[0][2] == h0 and all(h == 0 for _, _, h in got[1:])
    want[0] = want[0][h0:]
    want[-1] = np.concatenate([want[-1], np.zeros(mute, np.float32)])
    for g, w in zip(got, want):
        assert g[0].dtype == np.float32 and np.array_equal(g[0], w)
    whole = np.concatenate([g[0] for g in got])
    assert whole.shape[0] == pos - h0 + mute and np.abs(whole[: pos - h0] - sm[h0:pos]).max() < 1e-6
    # a second segment starts without a tail, on buffers of the first
    em.new_segment()
    again = em.push(torch.from_numpy(sm[:n_chunk].copy()).to(dev), False).result()
    assert again[1] == 0 and np.array_equal(again[0], sm[: n_chunk - ov])


def test_chunk_emitter_with_every_subset_of_the_stages(dev):
    """every subset of {eq, compress, level, limit}, with and without a track -- 32 emitters -- over one three-chunk segment and a
    one-chunk second segment: each handle's samples, records and packets are the plain emitter's samples pushed through host
    stage objects in the chain's order.  4 + n + mute is odd in the first and the last push and even in the other two, so every
    record is placed both with and without its alignment pad."""
    import itertools
    from gsv_tts_lite_amd import compressor as CM
    from gsv_tts_lite_amd import eq as EQM
    from gsv_tts_lite_amd import level as LV
    from gsv_tts_lite_amd import limiter as LM
    from gsv_tts_lite_amd.stream import ChunkEmitter
    from gsv_tts_lite_amd.track import TrackFormat, TrackResampler
    ov, fmt = 640, TrackFormat(48000, 1, 20)
    e = EQM.EQ([EQM.Band("highpass", 80.0), EQM.Band("peak", 300.0, q=1.0, gain_db=9.0)])
    c = CM.Compressor(-30.0, 4.0, 1.0, 100.0, 3.0)
    # in the chain's order: ChunkEmitter's keyword, the handle's record, the record's class, the stage on a device
    stages = (("eq", "eq", EQM.EqStreamRecord, lambda d: EQM.StreamEQ(e, SR, d)),
              ("compress", "comp", CM.CmpStreamRecord, lambda d: CM.StreamCompressor(c, SR, d)),
              ("level", "level", LV.LevelRecord, lambda d: LV.StreamLeveller(-10.0, SR, d, seed=-30.0)),
              ("limit", "limit", LM.StreamLimiterRecord, lambda d: LM.StreamLimiter(-6.0, SR, d)))
    cases = []
    for r in range(len(stages) + 1):
        for subset in itertools.combinations(stages, r):
            for tracked in (False, True):
                em = ChunkEmitter(ov, track=TrackResampler(fmt, SR, dev) if tracked else None, **{s[0]: s[3](dev) for s in subset})
                cases.append((em, subset, [s[3]("cpu") for s in subset], TrackResampler(fmt, SR, "cpu") if tracked else None))
    assert len(cases) == 32 and not cases[0][1] and cases[0][0].track is None
    sig = facade_audio(300, 40000, 0, 0, 0.5)
    sm = np.convolve(sig, np.ones(5, np.float32) / 5, mode="same").astype(np.float32)
    # (start, samples, final, first of its segment, mute, flush)
    pushes = [(0, 3001, False, True, 0, False), (2361 - 13, 3002, False, False, 0, False), (4710 - 200, 3001, True, False, 1233, False),
              (9000, 3001, True, True, 0, True)]
    assert [(4 + n + m) & 1 for _, n, _, _, m, _ in pushes] == [1, 0, 0, 1]
    handles = []
    for start, n, final, first, mute, flush in pushes:
        chunk = torch.from_numpy(sm[start: start + n].copy()).to(dev)
        if first:
            for em, _, _, _ in cases:
                em.new_segment()
        handles.append([em.push(chunk[None, None], final, trim_head=first, mute_samples=mute, flush=flush) for em, _, _, _ in cases])
    same = lambda p, q, cls: type(p) is cls and all(getattr(p, f) == getattr(q, f) for f in cls.__slots__)
    emitted = np.zeros(len(cases), np.int64)
    for i, ((_, n, final, _, mute, flush), row) in enumerate(zip(pushes, handles)):
        plain = row[0].result()
        assert len(plain) == 3 and plain[0].dtype == np.float32 and len(plain[0]) > 0
        for j, (h, (em, subset, host, h_track)) in enumerate(zip(row, cases)):
            got = h.result()
            assert len(got) == (3 if h_track is None else 4) and got[1:3] == plain[1:3], (i, j)
            want = plain[0]
            for (_, attr, cls, _), stage in zip(subset, host):
                want = stage.push(want, flush)
                assert same(getattr(h, attr), stage.rec, cls), (i, j, attr, getattr(h, attr), stage.rec)
            assert got[0].dtype == np.float32 and got[0].tobytes() == want.tobytes(), (i, j)
            assert all(getattr(h, s[1]) is None for s in stages if s not in subset), (i, j)
            if h_track is not None:
                assert np.array_equal(got[3], h_track.push(want, flush)), (i, j)
            emitted[j] += len(got[0])
    assert np.all(emitted == emitted[0])        # the flush hands out what a limiter held back
