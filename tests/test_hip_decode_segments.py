"""GPU tests of the segmented decode: gsv_voc_decode_segments (csrc/vocseg.h + gsv_voc.hip), SynthesizerTrn.decode_segments and
TTS.infer_batched with one speed / noise_scale per text.

Expected values come from the torch restatement of enc_p (oracle/sovits_encoder.py), oracle.device_normal and torch on the
device's fp32: enc_p at speed 1 over the whole concatenation, then F.interpolate(mode="linear") of EACH utterance's
[m_p | logs_p] on its own (the 1x1 `proj` commutes with it, as the speed-1.3 case of test_hip_encp.py relies on), the nearest
resize of its conditioning, its own noise, and the product's flow_dec.  fp32 handles with random weights, v2Pro."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gsv_tts_lite_amd import synth, _native as N
from gsv_tts_lite_amd.batchmath import balance_order, segment_frames, split_bounds

pytestmark = pytest.mark.gpu

C = 192          # inter_channels of every SoVITS version here
MASK64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vq(dev):
    from gsv_tts_lite_amd.sovits import SynthesizerTrn
    from oracle.sovits_encoder import TextEncoder, DecodeRestatement, codebook_decode
    hps = synth.sovits_hps("v2Pro")
    m = SynthesizerTrn(1025, 32, n_speakers=300, **hps["model"])
    m.load_state_dict(synth.sovits_weights(hps, seed=7))
    m.initialize_runtime(torch.float32, dev, [64])
    m.ref_enc = TextEncoder(m.hps_model, m._weights, dev)
    m.ref_decode = DecodeRestatement(m.hps_model, m._weights, dev, m.flow_dec)
    m.ref_codebook = codebook_decode
    return m


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _seeds(seed, noise_scales):
    """the seeds decode_segments draws from a generator seeded with `seed`: one per utterance with noise, in order"""
    g = _gen(seed)
    return [int(torch.empty((), dtype=torch.int64).random_(generator=g).item()) & MASK64 if ns != 0 else 0 for ns in noise_scales]


def _batch(dev, lengths, plens, speakers, seed):
    """a time-concatenated batch: codes [1, 1, N], text [1, P], per-token ge [1, 1024, N], slice_indices [2N, 2]"""
    rng = np.random.default_rng(seed)
    n, P = sum(lengths), sum(plens)
    codes = torch.from_numpy(rng.integers(0, 1024, (1, 1, n))).to(dev)
    text = torch.from_numpy(rng.integers(1, 700, (1, P))).to(dev)
    ge = torch.cat([torch.from_numpy(synth.synth_ge(s, 1024, 7)).to(dev).expand(-1, -1, l) for s, l in zip(speakers, lengths)], 2)
    ends = np.cumsum(plens)
    sl = torch.tensor([[int(e - p), int(e)] for l, p, e in zip(lengths, plens, ends) for _ in range(2 * l)], device=dev)
    return codes, text, ge, sl


@torch.inference_mode()
def _restate(vq, codes, text, ge, sl, lengths, speeds, noise_scales, seeds):
    """what decode_segments must compute, utterance by utterance -> (audio, attn, z_p)"""
    from oracle import oracle as orc
    dev = codes.device
    ge2 = F.interpolate(ge.float(), size=ge.shape[-1] * 2, mode="nearest")
    q = F.interpolate(vq.ref_codebook(vq._weights, codes), scale_factor=2, mode="nearest")
    m, logs, _ = vq.ref_enc.infer(q, text, vq.ref_enc.ge_to512(ge2), 1, slice_indices=sl)
    attn = vq.ref_enc.mrte.cross_attention.attn[0].clone()
    stats = torch.cat([m, logs], 1)
    zs, gs, s = [], [], 0
    for l, (frames, _), ns, seed in zip(lengths, segment_frames(lengths, speeds), noise_scales, seeds):
        st, g = stats[:, :, s:s + 2 * l], ge2[:, :, s:s + 2 * l]
        if frames != 2 * l:
            st = F.interpolate(st, size=frames, mode="linear")
            g = F.interpolate(g, size=frames, mode="nearest")
        z = st[:, :C]
        if ns != 0:
            noise = torch.from_numpy(orc.device_normal(seed, C * frames).astype(np.float32)).reshape(1, C, frames).to(dev)
            z = z + noise * torch.exp(st[:, C:]) * ns
        zs.append(z)
        gs.append(g)
        s += 2 * l
    z_p, ge_fr = torch.cat(zs, 2).contiguous(), torch.cat(gs, 2).contiguous()
    return vq.flow_dec(z_p, torch.ones(1, 1, z_p.shape[-1], device=dev), ge_fr), attn, z_p


def _int_bounds(lengths, speeds, hop):
    return [(first * hop, (first + f) * hop) for f, first in segment_frames(lengths, speeds)]


THREE = dict(lengths=[7, 140, 1], plens=[5, 40, 3], speakers=[1, 2, 1], speeds=[1.0, 1.3, 2.0])    # frames 14 + 216 + 2


@pytest.mark.parametrize("speed,ns", [(1, 0.0), (1.3, 0.0), (0.6, 0.5)])
def test_one_segment_is_the_old_call(vq, dev, speed, ns):
    """one utterance through the segmented call draws the same seed and computes the same samples, bit for bit, as decode()"""
    rng = np.random.default_rng(9)
    n, P = 37, 29
    codes = torch.from_numpy(rng.integers(0, 1024, (1, 1, n))).to(dev)
    text = torch.from_numpy(rng.integers(1, 700, (1, P))).to(dev)
    ge = torch.from_numpy(synth.synth_ge(1, 1024, 7)).to(dev)
    o, attn = vq.decode(codes, text, ge, noise_scale=ns, speed=speed, cuda_graph=False, generator=_gen(77))
    o2, attn2, bounds = vq.decode_segments(codes, text, ge, [n], [speed], [ns], generator=_gen(77))
    T_out = 2 * n if speed == 1 else int(2 * n / speed) + 1
    assert o2.shape == o.shape == (1, 1, T_out * vq.samples_per_frame)
    assert torch.equal(o, o2) and torch.equal(attn, attn2)
    assert bounds == [(0, T_out * vq.samples_per_frame)]


def test_mixed_speeds_match_the_per_utterance_restatement(vq, dev):
    """three utterances (7, 140 and 1 tokens; speeds 1.0, 1.3, 2.0; two speakers; slice_indices): a copied segment, a resampled
    one, a 1-token one, with segment boundaries inside a 256-lane tile.  (T_out is 232 here, one tile wide; the case with a tile
    boundary inside a segment is test_resampling_stays_inside_the_segment.)  Bounds of test_hip_encp.py's speed-1.3 case:
    1e-4 on the waveform, 1e-5 on attn.  Then the same call through the ABI into a NaN-guarded buffer."""
    lengths, speeds = THREE["lengths"], THREE["speeds"]
    codes, text, ge, sl = _batch(dev, lengths, THREE["plens"], THREE["speakers"], 11)
    hop = vq.samples_per_frame
    o, attn, bounds = vq.decode_segments(codes, text, ge, lengths, speeds, [0.0] * 3, slice_indices=sl)
    o_r, attn_r, _ = _restate(vq, codes, text, ge, sl, lengths, speeds, [0.0] * 3, [0] * 3)
    T_out = 14 + 216 + 2
    assert o.shape == o_r.shape == (1, 1, T_out * hop)
    e, ea = float((o - o_r).abs().max()), float((attn - attn_r).abs().max())
    print("mixed speeds vs restatement: waveform max %.2e, attn max %.2e" % (e, ea))
    assert e < 1e-4 and ea < 1e-5
    assert bounds == _int_bounds(lengths, speeds, hop) == [(0, 14 * hop), (14 * hop, 230 * hop), (230 * hop, 232 * hop)]
    # through the ABI: every sample up to T_out * hop written, nothing after
    n, P = sum(lengths), text.shape[-1]
    table = (N.VocSegment * 3)()
    for t, l, (f, _) in zip(table, lengths, segment_frames(lengths, speeds)):
        t.n_codes, t.out_frames, t.noise_scale, t.seed = l, f, 0.0, 0
    L, h = N.lib(), vq._voc._h
    need = L.gsv_voc_decode_segments_workspace(h, n, P, n, table, 3)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    buf = torch.full((T_out * hop + 4 * hop,), float("nan"), device=dev)
    c1, t1, g1 = codes.reshape(-1).contiguous(), text.reshape(-1).contiguous(), ge.float().reshape(1024, -1).contiguous()
    N.check(L.gsv_voc_decode_segments(h, c1.data_ptr(), n, t1.data_ptr(), P, g1.data_ptr(), n, sl.contiguous().data_ptr(), table, 3,
                                      buf.data_ptr(), 0, ws.data_ptr(), ws.numel(), N.current_stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:T_out * hop]).all()) and bool(torch.isnan(buf[T_out * hop:]).all())
    assert torch.equal(buf[:T_out * hop], o.reshape(-1))


def test_per_segment_noise(vq, dev):
    """noise_scales [0.5, 0, 0.8]: utterance i's noise is device_normal(seed_i, 192 * out_i) with the seeds the generator hands
    out (none for the utterance without noise); a re-seeded rerun is identical; which of two equal utterances is the silent
    one matters."""
    lengths, speeds, nss = THREE["lengths"], THREE["speeds"], [0.5, 0.0, 0.8]
    codes, text, ge, sl = _batch(dev, lengths, THREE["plens"], THREE["speakers"], 11)
    seeds = _seeds(123, nss)
    assert seeds[1] == 0 and seeds[0] != seeds[2]
    o, _, _ = vq.decode_segments(codes, text, ge, lengths, speeds, nss, slice_indices=sl, generator=_gen(123))
    o_r, _, z_r = _restate(vq, codes, text, ge, sl, lengths, speeds, nss, seeds)
    _, _, z_0 = _restate(vq, codes, text, ge, sl, lengths, speeds, [0.0] * 3, [0] * 3)
    # the restatement itself: noise where asked for, none on the utterance without (two torch runs of enc_p agree to rounding,
    # not bit for bit; the noise term is 0.5 * N(0,1) * exp(logs_p))
    assert float((z_r[:, :, 14:230] - z_0[:, :, 14:230]).abs().max()) < 1e-5
    assert float((z_r[:, :, :14] - z_0[:, :, :14]).abs().max()) > 0.1 and float((z_r[:, :, 230:] - z_0[:, :, 230:]).abs().max()) > 0.1
    e = float((o - o_r).abs().max())
    print("per-segment noise vs restatement + device_normal: max %.2e" % e)
    assert e < 1e-4
    o2, _, _ = vq.decode_segments(codes, text, ge, lengths, speeds, nss, slice_indices=sl, generator=_gen(123))
    assert torch.equal(o, o2)
    lengths2 = [9, 9]
    codes, text, ge, sl = _batch(dev, lengths2, [6, 6], [1, 2], 12)
    a, _, _ = vq.decode_segments(codes, text, ge, lengths2, [1.0, 1.0], [0.5, 0.0], slice_indices=sl, generator=_gen(5))
    b, _, _ = vq.decode_segments(codes, text, ge, lengths2, [1.0, 1.0], [0.0, 0.5], slice_indices=sl, generator=_gen(5))
    assert a.shape == b.shape and not torch.equal(a, b)


def test_resampling_stays_inside_the_segment(vq, dev):
    """two utterances at speed 1.3 (100 and 90 tokens -> 154 + 139 frames: the 256-lane tile boundary falls inside the second
    one): the segmented call resamples each on its own, so it differs from decode(speed=1.3) of the concatenation -- which
    stretches it as one signal and blends the frames next to the boundary (293 frames as well, other samples) -- and matches
    the per-utterance restatement; the scalar call still matches ref_decode(speed=1.3)."""
    lengths, speeds = [100, 90], [1.3, 1.3]
    codes, text, ge, sl = _batch(dev, lengths, [30, 25], [1, 2], 13)
    hop = vq.samples_per_frame
    o, attn, bounds = vq.decode_segments(codes, text, ge, lengths, speeds, [0.0, 0.0], slice_indices=sl)
    o_r, attn_r, _ = _restate(vq, codes, text, ge, sl, lengths, speeds, [0.0, 0.0], [0, 0])
    assert bounds == [(0, 154 * hop), (154 * hop, 293 * hop)]
    e = float((o - o_r).abs().max())
    print("two utterances at 1.3 vs restatement: max %.2e" % e)
    assert o.shape == o_r.shape and e < 1e-4 and float((attn - attn_r).abs().max()) < 1e-5
    o_s, attn_s = vq.decode(codes, text, ge, noise_scale=0.0, speed=1.3, cuda_graph=False, slice_indices=sl)
    o_sr, attn_sr, _ = vq.ref_decode(codes, text, ge, speed=1.3, slice_indices=sl)
    assert o_s.shape == o_sr.shape == (1, 1, (int(380 / 1.3) + 1) * hop)
    assert float((o_s - o_sr).abs().max()) < 1e-4 and float((attn_s - attn_sr).abs().max()) < 1e-5
    # int(380 / 1.3) + 1 is 293 frames too: the lengths agree here, the samples do not
    assert o_s.shape == o.shape and not torch.equal(o_s, o)
    d = float((o_s - o).abs().max())
    print("segmented against scalar speed 1.3: max |diff| %.2e" % d)
    assert d > 1e-3


def test_argument_checks_through_the_abi(vq, dev):
    """a bad table is refused (GSV_ERR_ARG = 1, the message names the entry) before anything is launched -- the NaN-filled
    output stays NaN -- and the workspace query answers 0 for it"""
    L, h = N.lib(), vq._voc._h
    n, P = 12, 7
    codes, text, ge, _ = _batch(dev, [n], [P], [1], 14)
    c1, t1, g1 = codes.reshape(-1).contiguous(), text.reshape(-1).contiguous(), ge.float().reshape(1024, -1)[:, :1].contiguous()
    ws = torch.empty(L.gsv_voc_decode_workspace(h, n, P, 1, 2 * n, 0), dtype=torch.uint8, device=dev)
    buf = torch.full((4 * n * vq.samples_per_frame,), float("nan"), device=dev)

    def call(entries, count=None, Tg=1):
        table = (N.VocSegment * max(1, len(entries)))()
        for t, (l, f) in zip(table, entries):
            t.n_codes, t.out_frames, t.noise_scale, t.seed = l, f, 0.0, 0
        count = len(entries) if count is None else count
        assert L.gsv_voc_decode_segments_workspace(h, n, P, Tg, table, count) == 0
        rc = L.gsv_voc_decode_segments(h, c1.data_ptr(), n, t1.data_ptr(), P, g1.data_ptr(), Tg, 0, table, count, buf.data_ptr(), 0,
                                       ws.data_ptr(), ws.numel(), N.current_stream_ptr(dev))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), "a refused call wrote to the output"
        return rc, L.gsv_last_error().decode()

    rc, msg = call([], 0)
    assert rc == 1 and "0 segments" in msg
    rc, msg = call([(1, 2)] * 65)
    assert rc == 1 and "65 segments" in msg
    rc, msg = call([(5, 10), (6, 12)])                      # 11 codes for n_codes 12
    assert rc == 1 and "11 codes" in msg and "n_codes 12" in msg
    rc, msg = call([(5, 10), (8, 16)])                      # 13 codes
    assert rc == 1 and "segments 0..1" in msg and "13 codes" in msg
    rc, msg = call([(5, 10), (7, 0)])
    assert rc == 1 and "segment 1" in msg and "out_frames 0" in msg
    rc, msg = call([(0, 10), (12, 24)])
    assert rc == 1 and "segment 0" in msg and "n_codes 0" in msg
    rc, msg = call([(5, 10), (7, 14)], Tg=5)
    assert rc == 1 and "Tg 5" in msg
    with pytest.raises(ValueError):
        vq.decode_segments(codes, text, ge[:, :, :1], [5, 6], [1.0, 1.0], [0.0, 0.0])
    with pytest.raises(ValueError):
        vq.decode_segments(codes, text, ge[:, :, :1], [5, 7], [1.0], [0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------- facade
def _word_frontend(text):
    import re
    words = re.findall(r"[A-Za-z]+|[^\sA-Za-z]", text)
    ids = [1 + (ord(c) * 7) % 690 for w in words for c in w]
    return ids, {"word": words, "ph": [len(w) for w in words]}, None, text


TEXTS = ["First one is here. Second follows!", "Another text", "Third, with a comma."]
SPEEDS = [1.0, 1.25, 0.8]
MUTE_SCALE = {".": 1.5, "!": 1.5, ",": 1.0}


@pytest.fixture(scope="module")
def tts(dev):
    """the tiny models of test_hip_tts.py; the GPT is replaced by fixed token lists (request k gets 30 + 5 k tokens, returned in
    another order than requested), the vocoder is the real one"""
    from gsv_tts import TTS
    t = TTS(gpt_cache=[(1, 128), (1, 160), (4, 160)], sovits_cache=[50, 55], device=str(dev), dtype="float32")
    t.load_gpt_model("synthetic://gpt?seed=1234&n_layer=6&eos_gain=1.0")
    t.load_sovits_model("synthetic://sovits?version=v2Pro&seed=1234")
    t.set_text_frontend(_word_frontend)
    t.cache_spk_audio("spk.wav", ge=torch.from_numpy(synth.synth_ge(0, 1024)))
    x, y, _, _ = synth.synth_request(0, 12, 0, 30)
    t.cache_prompt_audio("prompt.wav", "prompt text.", prompt=torch.from_numpy(y)[None], phones1=x.tolist())
    t2s = next(iter(t.gpt_models.values())).t2s_model
    rng = np.random.default_rng(5)
    t.fixed_tokens = [torch.from_numpy(rng.integers(0, 1024, 30 + 5 * k)).to(dev) for k in range(8)]

    def fake_gpt(ids, prompts, berts, **kw):
        order = list(range(len(ids)))[::-1]
        return [t.fixed_tokens[k] for k in order], torch.tensor(order)
    t2s.infer_batched = fake_gpt
    return t


def _facade_batch(tts, dev):
    """the one vocoder batch infer_batched forms of TEXTS (cut_minlen 8), restated: segments, their texts, the balance order and
    the concatenated inputs"""
    from gsv_tts_lite_amd.tts import cut_text
    segs, seg2orig = [], []
    for i, t in enumerate(TEXTS):
        for c in cut_text(t if t[-1] in ".!" else t + ".", 8):      # infer_batched ends every text on a pause mark
            segs.append(c)
            seg2orig.append(i)
    assert seg2orig == [0, 0, 1, 2]
    vq = next(iter(tts.sovits_models.values())).vq_model
    ge = tts._ge_for("spk.wav", next(iter(tts.sovits_models))).squeeze(0)
    lengths = torch.tensor([len(tts.fixed_tokens[k]) for k in range(len(segs))])
    oi = balance_order(lengths).tolist()
    ln = [int(lengths[o]) for o in oi]
    phones = [_word_frontend(segs[o])[0] for o in oi]
    codes = torch.cat([tts.fixed_tokens[o] for o in oi])[None, None]
    ph_cat = torch.tensor([p for ph in phones for p in ph], dtype=torch.int64, device=dev)[None]
    ge_cat = torch.cat([ge.expand(-1, l) for l in ln], 1)[None]
    ends = np.cumsum([len(p) for p in phones])
    sl = torch.tensor([[int(e) - len(p), int(e)] for l, p, e in zip(ln, phones, ends) for _ in range(2 * l)], device=dev)
    return vq, segs, seg2orig, oi, ln, codes, ph_cat, ge_cat, sl


def _assemble(tts, segs, seg2orig, oi, audio, ranges, mutes):
    """cut `audio` at `ranges` (batch order), trim as infer_batched does, append each segment's mute, join per text"""
    peak = audio.abs().max()
    if peak > 1.0:
        audio = audio / peak
    per_seg = {}
    for o, (lo, hi) in zip(oi, ranges):
        a = audio[lo:hi]
        h, t = tts._find_head_threshold_offsets(a), tts._find_tail_threshold_offsets(a)
        per_seg[o] = a[h:-t].float().cpu().numpy()
    out = [[] for _ in TEXTS]
    for k, s in enumerate(segs):
        out[seg2orig[k]] += [per_seg[k], np.zeros(int(mutes[seg2orig[k]] * MUTE_SCALE[s[-1]] * 32000), np.float32)]
    return [np.concatenate(p) for p in out]


def test_facade_per_text_speed(tts, dev):
    """infer_batched(speed=[...], noise_scale=[...]): every clip is its segments' exact frame ranges of one decode_segments call,
    trimmed and followed by cut_mute / speed of its text; a scalar speed still is decode() + split_bounds, sample for sample;
    a list of the wrong length raises."""
    vq, segs, seg2orig, oi, ln, codes, ph_cat, ge_cat, sl = _facade_batch(tts, dev)
    hop = vq.samples_per_frame
    clips = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, speed=SPEEDS, noise_scale=[0.0] * 3)
    sp = [SPEEDS[seg2orig[o]] for o in oi]
    audio, _, bounds = vq.decode_segments(codes, ph_cat, ge_cat, ln, sp, [0.0] * len(oi), slice_indices=sl)
    assert bounds == _int_bounds(ln, sp, hop)
    for (lo, hi), l, s in zip(bounds, ln, sp):
        assert hi - lo == (2 * l if s == 1 else int(2 * l / s) + 1) * hop
    want = _assemble(tts, segs, seg2orig, oi, audio[0, 0], bounds, [0.4 / s for s in SPEEDS])
    assert len(clips) == 3
    for c, w in zip(clips, want):
        assert c.audio_data.shape == w.shape and np.array_equal(c.audio_data, w)
        assert abs(c.audio_len_s - len(w) / 32000) < 1e-9
    # a number: the path of the parent commit
    clips = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, speed=1.25, noise_scale=0.0)
    audio, _ = vq.decode(codes, ph_cat, ge_cat, noise_scale=0.0, speed=1.25, cuda_graph=False, slice_indices=sl)
    want = _assemble(tts, segs, seg2orig, oi, audio[0, 0], split_bounds(ln, hop, 1.25), [0.4 / 1.25] * 3)
    for c, w in zip(clips, want):
        assert c.audio_data.shape == w.shape and np.array_equal(c.audio_data, w)
    with pytest.raises(ValueError):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, speed=[1.0, 1.25])
    with pytest.raises(ValueError):
        tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, noise_scale=[0.0] * 4)


def test_facade_per_text_speed_subtitles(tts, dev, monkeypatch):
    """return_subtitles on the segmented path: each segment is aligned on its own rows and phoneme columns with its own speed.
    Random weights give no usable attention, so decode_segments' attention is replaced by a diagonal per segment (frame f of
    a segment of T frames and P phonemes looks at phoneme floor(f P / T)); the audio is the real one.  Each text's last
    end_s is its clip length minus the trailing mute to within one frame, 1 / 50 / speed s; the spans are ordered."""
    vq = next(iter(tts.sovits_models.values())).vq_model
    real = vq.decode_segments

    def diagonal(codes, text, ge, lengths, speeds, noise_scales, slice_indices=None, generator=None):
        audio, attn, bounds = real(codes, text, ge, lengths, speeds, noise_scales, slice_indices=slice_indices, generator=generator)
        pairs = slice_indices.cpu().numpy()
        syn = np.full(tuple(attn.shape), 1e-3, np.float32)
        row = 0
        for l in lengths:
            T, (p0, p1) = 2 * int(l), pairs[row]
            for f in range(T):
                syn[:, row + f, p0 + min(f * (p1 - p0) // T, p1 - p0 - 1)] = 1.0
            row += T
        return audio, torch.from_numpy(syn).to(attn.device), bounds
    monkeypatch.setattr(vq, "decode_segments", diagonal)
    clips = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, speed=SPEEDS, noise_scale=[0.0] * 3,
                              return_subtitles=True)
    plain = tts.infer_batched("spk.wav", "prompt.wav", "prompt text.", TEXTS, top_k=1, cut_minlen=8, speed=SPEEDS, noise_scale=[0.0] * 3)
    last_mark = ["!", ".", "."]                      # "Another text" gets its "." appended
    for c, p, t, s, mark in zip(clips, plain, TEXTS, SPEEDS, last_mark):
        assert np.array_equal(c.audio_data, p.audio_data) and p.subtitles == []
        assert c.subtitles
        prev = 0.0
        for e in c.subtitles:
            assert set(e) >= {"text", "start_s", "end_s", "orig_idx_start", "orig_idx_end"}
            assert e["start_s"] >= prev - 1e-9 and e["end_s"] >= e["start_s"] - 1e-9
            prev = e["end_s"]
        mute = int(0.4 / s * MUTE_SCALE[mark] * 32000) / 32000
        body_s = c.audio_len_s - mute
        print("text %r speed %.2f: last end_s %.4f, clip minus mute %.4f" % (t, s, c.subtitles[-1]["end_s"] - 0.4 / s * MUTE_SCALE[mark], body_s))
        assert abs(c.subtitles[-1]["end_s"] - 0.4 / s * MUTE_SCALE[mark] - body_s) <= 1 / 50 / s
