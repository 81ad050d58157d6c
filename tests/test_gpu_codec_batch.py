"""GPU: batched streamed vocoding (fm_codec_stream_decode_batch) against the per-stream path.

Every output row of every codec kernel depends only on its own input rows, which is why streamed
chunks already equal the one-shot decode bit for bit (test_gpu_codec_stream.py).  A batched pass
puts several stream contexts' chunks into the same launches, so it must not change a single bit:
every comparison here is assert_array_equal against decode_codes / decode_chunk, no tolerance.
"""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAXF, T = 320, 150  # 150 frames: every stream crosses the 128-frame window (the npre clamp engages)


def _codes(m, rng, n):
    C1 = m.cfg.n_codebooks + 1
    c = np.zeros((C1, n), np.int32)
    c[0] = rng.integers(0, m.cfg.semantic_codebook_size, n)
    c[1:] = rng.integers(0, m.cfg.codebook_size, (C1 - 1, n))
    return c


@pytest.fixture(scope="module", params=["bf16", "fp32"])
def rig(request, golden):
    """One codec per precision for the module, four streams' codes and their one-shot waveforms
    (computed once, never modified)."""
    from fishmi.codec import FishMICodec
    from fishmi.config import CodecConfig

    g = golden("codec_full.npz")
    cfg = CodecConfig.from_spec(json.loads(str(g["spec"])))
    m = FishMICodec.synthetic(cfg, int(g["synth_seed"]), 0, request.param, MAXF)
    rng = np.random.default_rng(41)
    codes = [_codes(m, rng, T) for _ in range(4)]
    full = [m.decode_codes(c) for c in codes]
    for f in full:
        f.setflags(write=False)
    yield m, codes, full
    m.close()


def _run(m, ctx, codes, schedules, order=None):
    """One batched call per step: stream i's next schedules[i][step] frames; returns each stream's PCM."""
    n = len(ctx)
    pos, pcm = [0] * n, [[] for _ in range(n)]
    for step in range(max(len(s) for s in schedules)):
        ids = [i for i in (order or range(n)) if step < len(schedules[i])]
        chunks = [codes[i][:, pos[i]:pos[i] + schedules[i][step]] for i in ids]
        for i, p in zip(ids, m.decode_chunks([ctx[i] for i in ids], chunks)):
            pcm[i].append(p)
            pos[i] += schedules[i][step]
    return [np.concatenate(p) for p in pcm]


RAGGED = [(1, 7, 22, 120), (22, 22, 22, 84), (3, 127, 19, 1)]


def test_ragged_schedules_equal_one_shot(rig):
    """T = 1 (shorter than every site's carried rows), T >= 127 (K/V state fully replaced), T just
    below the window, different positions inside one call."""
    m, codes, full = rig
    gap = m.batch_gap
    assert gap >= 1 and all(sum(s[k] for s in RAGGED) + 2 * gap <= MAXF for k in range(4))  # one native call per step
    ctx = [m.open_stream() for _ in range(3)]
    got = _run(m, ctx, codes, RAGGED)
    for i in range(3):
        np.testing.assert_array_equal(got[i], full[i])
    for c in ctx:
        c.close()


def test_batched_single_and_own_stream_share_state(rig):
    """Batched calls, single-stream decode_chunk calls and batches of one alternate on the same
    contexts; stream 2 is the handle's own (id 0); stream 3 starts late, at position 0 beside
    positions past the window."""
    m, codes, full = rig
    ctx = [m.open_stream(), m.open_stream(), None, m.open_stream()]
    m.stream_reset()
    pos, pcm = [0] * 4, [[] for _ in range(4)]

    def batch(ids, ns):
        chunks = [codes[i][:, pos[i]:pos[i] + k] for i, k in zip(ids, ns)]
        for i, k, p in zip(ids, ns, m.decode_chunks([ctx[i] for i in ids], chunks)):
            pcm[i].append(p)
            pos[i] += k

    def batch1(i, k):  # a native batch of one (decode_chunks itself hands a lone chunk to the single-stream call)
        sid = ctx[i].sid if ctx[i] is not None else 0
        pcm[i].append(_native_batch(m, [sid], [codes[i][:, pos[i]:pos[i] + k]])[0])
        pos[i] += k

    def single(i, k):
        c = np.ascontiguousarray(codes[i][:, pos[i]:pos[i] + k])
        pcm[i].append(ctx[i].decode_chunk(c) if ctx[i] is not None else m.decode_chunk(c))
        pos[i] += k

    batch([0, 1, 2], [40, 3, 64])
    single(0, 30)
    single(2, 1)
    batch1(1, 90)
    batch([2, 0], [70, 65])       # both past the 128-frame window now
    single(1, 50)
    batch([3, 0, 2, 1], [5, 15, 15, 7])   # stream 3 at position 0 beside 135, 135, 143
    single(3, 100)
    batch1(3, 40)
    batch([3], [5])
    assert pos == [T] * 4
    for i in range(4):
        np.testing.assert_array_equal(np.concatenate(pcm[i]), full[i])
    for c in ctx:
        if c is not None:
            c.close()


def test_segment_order_does_not_matter(rig):
    m, codes, full = rig
    ctx = [m.open_stream() for _ in range(3)]
    got = _run(m, ctx, codes, RAGGED, order=[2, 0, 1])
    for i in range(3):
        np.testing.assert_array_equal(got[i], full[i])
    for c in ctx:
        c.close()


def test_stale_work_buffers_do_not_leak(rig):
    """A full-length one-shot decode of unrelated codes right before every batched call leaves
    non-zero rows in every work buffer and gap; the batched PCM is unchanged, and a second run
    from rewound contexts repeats it bit for bit."""
    m, codes, full = rig
    junk = _codes(m, np.random.default_rng(5), MAXF)
    ctx = [m.open_stream() for _ in range(3)]
    runs = []
    for _ in range(2):
        pos, pcm = [0] * 3, [[] for _ in range(3)]
        for step in range(4):
            m.decode_codes(junk)
            chunks = [codes[i][:, pos[i]:pos[i] + RAGGED[i][step]] for i in range(3)]
            for i, p in enumerate(m.decode_chunks(ctx, chunks)):
                pcm[i].append(p)
                pos[i] += RAGGED[i][step]
        runs.append([np.concatenate(p) for p in pcm])
        for c in ctx:
            c.rewind()
    for i in range(3):
        np.testing.assert_array_equal(runs[0][i], full[i])
        np.testing.assert_array_equal(runs[1][i], runs[0][i])
    for c in ctx:
        c.close()


def _native_batch(m, sids, chunks):
    return m._decode_batch(sids, [np.ascontiguousarray(c, dtype=np.int32) for c in chunks])


def test_rejections_leave_contexts_usable(rig):
    from fishmi.native import FishMIError

    m, codes, full = rig
    gap = m.batch_gap
    ctx = [m.open_stream() for _ in range(3)]
    sid = [c.sid for c in ctx]
    got = [list() for _ in range(3)]
    for i, p in enumerate(m.decode_chunks(ctx, [c[:, :10] for c in codes[:3]])):
        got[i].append(p)
    neg = codes[1][:, 10:20].copy()
    neg[3, 4] = -1
    over = MAXF - 2 * gap - 20 + 1  # one frame past sum(T) + gap * (n - 1) <= max_frames
    bad = [
        ([sid[0], sid[0]], [codes[0][:, 10:20], codes[0][:, 20:30]]),           # duplicate id
        ([sid[0], 9999], [codes[0][:, 10:20], codes[1][:, 10:20]]),             # unknown id
        ([sid[0], sid[1]], [codes[0][:, 10:20], codes[1][:, 10:10]]),           # T = 0
        ([sid[0], sid[1]], [codes[0][:, 10:20], neg]),                          # negative code
        (sid, [codes[0][:, 10:20], codes[1][:, 10:20], np.zeros((codes[0].shape[0], over), np.int32)]),  # capacity
    ]
    for ids, chunks in bad:
        with pytest.raises(FishMIError):
            _native_batch(m, ids, chunks)
    # exactly at the limit: accepted (on a context of its own)
    extra = m.open_stream()
    fit = np.zeros((codes[0].shape[0], over - 1), np.int32)
    tmp = [m.open_stream(), m.open_stream()]
    out = _native_batch(m, [tmp[0].sid, tmp[1].sid, extra.sid], [codes[0][:, :10], codes[1][:, :10], fit])
    np.testing.assert_array_equal(out[0], full[0][:10 * m.frame_length])
    for c in tmp + [extra]:
        c.close()
    # the refused calls changed nothing: the streams go on and still equal the one-shot decode
    for i, p in enumerate(m.decode_chunks(ctx, [c[:, 10:T] for c in codes[:3]])):
        got[i].append(p)
    for i in range(3):
        np.testing.assert_array_equal(np.concatenate(got[i]), full[i])
    for c in ctx:
        c.close()


def test_batched_call_is_one_pass(rig):
    """Launch counts (fm_codec_profile_read): 4 segments in one call issue fewer than twice the
    launches of ONE single-stream chunk of the same length -- a loop over segments would issue 4x."""
    m, codes, full = rig
    ctx = [m.open_stream() for _ in range(4)]
    n0 = m.profile()[1]
    ctx[0].decode_chunk(np.ascontiguousarray(codes[0][:, :8]))
    n1 = m.profile()[1]
    ctx[0].rewind()
    out = m.decode_chunks(ctx, [c[:, :8] for c in codes])
    n2 = m.profile()[1]
    single, batched = n1 - n0, n2 - n1
    print(f"launches: single chunk {single}, 4-segment batch {batched}")
    assert single > 0 and 0 < batched < 2 * single
    for i in range(4):
        np.testing.assert_array_equal(out[i], full[i][:8 * m.frame_length])
    for c in ctx:
        c.close()


def test_decode_chunks_splits_into_native_calls(rig):
    """Three 140-frame chunks and a 10-frame one on max_frames 320: 140 + gap + 140 fits, a third
    does not, so the list takes three native calls: a batched pass of two, then the third context
    and its repeated chunk one at a time (a lone chunk goes to the single-stream call)."""
    m, codes, full = rig
    ctx = [m.open_stream() for _ in range(3)]
    streams = [ctx[0], ctx[1], ctx[2], ctx[2]]
    chunks = [codes[0][:, :140], codes[1][:, :140], codes[2][:, :140], codes[2][:, 140:150]]
    calls = []
    real = m._decode_batch
    real1 = m._decode_one
    m._decode_batch = lambda sids, ch: (calls.append(list(sids)), real(sids, ch))[1]
    m._decode_one = lambda sid, cd: (calls.append([sid]), real1(sid, cd))[1]
    try:
        out = m.decode_chunks(streams, chunks)
    finally:
        del m._decode_batch, m._decode_one
    assert calls == [[ctx[0].sid, ctx[1].sid], [ctx[2].sid], [ctx[2].sid]]
    for i in range(3):
        np.testing.assert_array_equal(out[i], full[i][:140 * m.frame_length])
    np.testing.assert_array_equal(out[3], full[2][140 * m.frame_length:])
    for c in ctx:
        c.close()


def test_stream_vocoder_batched_equals_one_shot(golden):
    """The four-request, two-wave scenario of test_gpu_codec_stream's StreamVocoder test with
    batch=4: every request's PCM is the one-shot decode's, contexts pooled as before."""
    from fishmi import scheduler as S
    from fishmi.codec import FishMICodec
    from fishmi.config import CodecConfig

    g = golden("codec_full.npz")
    cfg = CodecConfig.from_spec(json.loads(str(g["spec"])))
    m = FishMICodec.synthetic(cfg, int(g["synth_seed"]), 0, "bf16", 160)
    rng = np.random.default_rng(33)
    C1, Tn = m.cfg.n_codebooks + 2, 150  # a frame column: the main token, then the codec's rows
    streams = []
    for _ in range(4):
        c = np.zeros((C1, Tn + 1), np.int32)  # + the column serve() drops at the end
        c[0] = rng.integers(0, 1000, Tn + 1)
        c[1] = rng.integers(0, m.cfg.semantic_codebook_size, Tn + 1)
        c[2:] = rng.integers(0, m.cfg.codebook_size, (C1 - 2, Tn + 1))
        streams.append(c)
    full = [m.decode_codes(np.ascontiguousarray(c[1:, :Tn])) for c in streams]
    batches = []
    real = m.decode_chunks
    m.decode_chunks = lambda st, ch: (batches.append(len(st)), real(st, ch))[1]
    for chunk in (1, 32, 96):
        voc = S.StreamVocoder(m, chunk, batch=4)
        assert voc.batch == 4
        for w0 in (0, 2):  # the second wave reuses the first wave's contexts
            wave = streams[w0:w0 + 2]
            reqs = [S.Request(i, np.zeros((C1, 1), np.int32), Tn, 0) for i in range(len(wave))]
            cols = [[] for _ in wave]
            for t in range(0, Tn + 1, 17):  # a tick: 17 new columns per live stream
                for i, c in enumerate(wave):
                    cols[i] += [c[:, j] for j in range(t, min(t + 17, Tn + 1))]
                    voc.progress(i, reqs[i], cols[i])
            for i, c in enumerate(wave):
                pcm = voc.finish(i, reqs[i], np.stack(cols[i], 1)[:, :-1])
                np.testing.assert_array_equal(pcm, full[w0 + i])
        assert len(voc.ctxs) == 2
        voc.close()
    assert batches and max(batches) <= 4
    m.close()
