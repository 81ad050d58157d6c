"""CPU: scheduler.StreamVocoder(codec, chunk, batch=N) on a fake codec that records its calls.

What the vocoder thread may put into one decode_chunks call: chunk items standing next to each
other in its FIFO, of distinct requests, at most `batch` of them; a request's chunks keep their
order; an exception fails that batch's requests only; batch=0 or a codec without decode_chunks is
the per-chunk path.
"""
import threading

import numpy as np
import pytest

from fishmi import scheduler as S

C1 = 4  # rows of a frame column: the main token, then three codec rows


class _Ctx:
    def __init__(self, codec, sid):
        self.codec, self.sid, self.n = codec, sid, 0

    def decode_chunk(self, codes):
        self.codec.log.append(("chunk", self.sid, codes.shape[1]))
        return self.codec._pcm(self, codes)

    def rewind(self):
        self.n = 0

    def close(self):
        pass


class _PerChunkCodec:
    """No decode_chunks: today's interface."""
    max_frames = 64

    def __init__(self):
        self.log, self.nctx = [], 0

    def open_stream(self):
        self.nctx += 1
        return _Ctx(self, self.nctx)

    def _pcm(self, ctx, codes):
        # a "waveform" that encodes which codes came in which order: sample = first codec row
        ctx.n += codes.shape[1]
        return codes[0].astype(np.float32)


class _BatchCodec(_PerChunkCodec):
    def __init__(self, fail_on=None):
        super().__init__()
        self.fail_on = fail_on

    def decode_chunks(self, streams, codes_list):
        self.log.append(("batch", [s.sid for s in streams], [c.shape[1] for c in codes_list]))
        if self.fail_on is not None and any(int(c[0, 0]) == self.fail_on for c in codes_list):
            raise RuntimeError("codec failed")
        return [self._pcm(s, c) for s, c in zip(streams, codes_list)]


def _cols(rid, n):
    """n + 1 frame columns of request rid (the last one is the column serve() drops); the first codec
    row counts rid * 1000 + t, so PCM order shows chunk order."""
    c = np.zeros((C1, n + 1), np.int32)
    c[1] = rid * 1000 + np.arange(n + 1)
    return c


def _drive(voc, nreq, n, tick):
    reqs = [S.Request(i, np.zeros((C1, 1), np.int32), n, 0) for i in range(nreq)]
    data = [_cols(i, n) for i in range(nreq)]
    cols = [[] for _ in range(nreq)]
    for t in range(0, n + 1, tick):
        for i in range(nreq):
            cols[i] += [data[i][:, j] for j in range(t, min(t + tick, n + 1))]
            voc.progress(i, reqs[i], cols[i])
    return reqs, data, cols


def _finish(voc, reqs, cols):
    return [voc.finish(i, reqs[i], np.stack(cols[i], 1)[:, :-1]) for i in range(len(reqs))]


def _hold_thread(voc):
    """Park the vocoder thread in a plain FIFO item until the returned event is set, so the chunk
    items submitted meanwhile are all queued when it looks at them."""
    gate = threading.Event()
    voc.submit(gate.wait)
    return gate


def test_batches_hold_distinct_requests_in_order_up_to_batch():
    codec = _BatchCodec()
    voc = S.StreamVocoder(codec, chunk=4, batch=3)
    assert voc.batch == 3
    gate = _hold_thread(voc)
    reqs, data, cols = _drive(voc, nreq=5, n=40, tick=4)  # FIFO: r0 r1 r2 r3 r4 r0 r1 ...
    gate.set()
    pcm = _finish(voc, reqs, cols)
    voc.close()
    for i in range(5):  # every request's chunks arrived in order, nothing lost or repeated
        np.testing.assert_array_equal(pcm[i], (i * 1000 + np.arange(40)).astype(np.float32))
    batches = [e for e in codec.log if e[0] == "batch"]
    assert not [e for e in codec.log if e[0] == "chunk"]
    assert all(len(set(b[1])) == len(b[1]) for b in batches), "a request twice in one batch"
    assert all(1 <= len(b[1]) <= 3 for b in batches)
    assert [len(b[1]) for b in batches[:3]] == [3, 3, 3], "queued chunks of distinct requests were not batched"
    assert sum(sum(b[2]) for b in batches) == 5 * 40


def test_same_request_never_shares_a_batch():
    codec = _BatchCodec()
    voc = S.StreamVocoder(codec, chunk=4, batch=4)
    gate = _hold_thread(voc)
    reqs, data, cols = _drive(voc, nreq=2, n=16, tick=8)  # FIFO: r0 r1, then r0 r0 r1 r1, then r0 r1
    gate.set()
    pcm = _finish(voc, reqs, cols)
    voc.close()
    for i in range(2):
        np.testing.assert_array_equal(pcm[i], (i * 1000 + np.arange(16)).astype(np.float32))
    batches = [e[1] for e in codec.log if e[0] == "batch"]
    assert all(len(set(b)) == len(b) for b in batches)
    # a repeated request ends the batch and opens the next: r0 r1 | r0 | r0 r1 | r1 r0 | r1
    assert batches == [[1, 2], [1], [1, 2], [2, 1], [2]]


def test_exception_fails_only_that_batch():
    codec = _BatchCodec(fail_on=1000)  # the first chunk of request 1
    voc = S.StreamVocoder(codec, chunk=5, batch=2)
    gate = _hold_thread(voc)
    reqs, data, cols = _drive(voc, nreq=3, n=20, tick=5)  # FIFO: r0 r1 | r2 r0 | r1 r2 | ...
    gate.set()
    for i in (0, 1):  # the failing batch held requests 0 and 1
        with pytest.raises(RuntimeError):
            voc.finish(i, reqs[i], np.stack(cols[i], 1)[:, :-1])
    pcm = voc.finish(2, reqs[2], np.stack(cols[2], 1)[:, :-1])
    np.testing.assert_array_equal(pcm, (2000 + np.arange(20)).astype(np.float32))
    batches = [e[1] for e in codec.log if e[0] == "batch"]
    assert batches[0] == [1, 2]  # (context ids: request 0 opened 1, request 1 opened 2)
    assert all(b == [3] for b in batches[1:]), "a failed request's later chunks still reached the codec"
    voc.close()


def test_batch_zero_and_plain_codec_take_the_per_chunk_path():
    for codec, batch in ((_BatchCodec(), 0), (_BatchCodec(), 1), (_PerChunkCodec(), 4)):
        voc = S.StreamVocoder(codec, chunk=4, batch=batch)
        assert voc.batch == 0
        reqs, data, cols = _drive(voc, nreq=2, n=10, tick=3)
        pcm = _finish(voc, reqs, cols)
        voc.close()
        for i in range(2):
            np.testing.assert_array_equal(pcm[i], (i * 1000 + np.arange(10)).astype(np.float32))
        assert codec.log and all(e[0] == "chunk" for e in codec.log)
        assert [e[2] for e in codec.log if e[1] == 1] == [4, 4, 2]
    # and the default is batch = 0
    voc = S.StreamVocoder(_BatchCodec(), chunk=4)
    assert voc.batch == 0
    voc.close()


def test_server_vocode_batch_reaches_the_stream_vocoder():
    """fishmi.server: --vocode-batch (default 0) is the batch of every StreamVocoder the process
    builds through server.stream_vocoder."""
    from fishmi import server

    assert server.VOCODE_BATCH == 0
    voc = server.stream_vocoder(_BatchCodec(), chunk=4)
    assert voc.batch == 0
    voc.close()
    server.VOCODE_BATCH = 8
    try:
        voc = server.stream_vocoder(_BatchCodec(), chunk=4)
        assert voc.batch == 8 and voc.chunk == 4
        voc.close()
    finally:
        server.VOCODE_BATCH = 0
