"""Voice prefix cache (fishmi.prefix_cache.PrefixCache) through the serial and the batched LLM
workers, on CPU with the scripted model of tests/test_batching.py: every slot's next column hashes
the slot's whole token history, so a prefix that is wrong, short or loaded into the wrong slot
changes every later column.  The GPU counterpart is tests/test_gpu_prefix_cache.py."""
import queue

import numpy as np
import pytest

from test_batching import C, CB, ScriptedModel, _requests, _summary

ROW_BYTES = 64  # the scripted model's bytes per cached position


class CachingModel(ScriptedModel):
    """ScriptedModel with the prefix calls of DualARModel on its per-slot histories."""

    def __init__(self, max_slots=1, oom=False):
        super().__init__(max_slots)
        self.prefixes, self.next_pid, self.oom = {}, 1, oom

    def prefix_bytes(self, npos):
        return ROW_BYTES * int(npos)

    def save_prefix(self, slot, npos):
        from fishmi import native

        assert 1 <= npos <= len(self.hist[slot])
        if self.oom:
            e = native.FishMIError("libfishmi error -4: prefix_save: hipMalloc failed")
            e.code = native.FM_ERR_OOM
            raise e
        pid, self.next_pid = self.next_pid, self.next_pid + 1
        self.prefixes[pid] = list(self.hist[slot][:npos])
        self.calls.append(("save_prefix", slot, npos, pid))
        return pid

    def load_prefix(self, pid, slots):
        slots = [int(s) for s in slots]
        assert len(set(slots)) == len(slots)
        rows = self.prefixes[pid]
        for s in slots:
            self.hist[s] = list(rows)  # the slot's cached position becomes npos
        self.calls.append(("load_prefix", pid, tuple(slots)))

    def drop_prefix(self, pid):
        del self.prefixes[pid]
        self.calls.append(("drop_prefix", pid))

    def prefix_info(self, pid):
        return len(self.prefixes[pid]), ROW_BYTES * len(self.prefixes[pid])

    def prefill(self, slot, prompt, sp, pos0=0):
        col = super().prefill(slot, prompt, sp, pos0)
        self.calls[-1] = ("prefill", slot, pos0)
        return col

    def prefill_batch(self, slots, prompts, sps, pos0=None):
        if pos0 is None:
            return super().prefill_batch(slots, prompts, sps)
        self.calls.append(("prefill_batch", tuple(slots), tuple(int(p) for p in pos0)))
        return np.stack([ScriptedModel.prefill(self, s, p, sp, int(p0))
                         for s, p, sp, p0 in zip(slots, prompts, sps, pos0)])

    def generate_at(self, suffix, pos0, *a, **k):
        self.calls.append(("generate_at", k.get("slot", 0), int(pos0)))
        return super().generate_at(suffix, pos0, *a, **k)


def _serial_reference(reqs):
    from fishmi import engine

    return [[engine.WrappedGenerateResponse("success", o) for o in engine.generate_long(model=ScriptedModel(1), **r)]
            for r in reqs]


def _same(got, ref, tag=""):
    a, b = _summary(got), _summary(ref)
    assert [x[0] for x in a] == [x[0] for x in b], tag
    for (_, ca), (_, cb) in zip(a, b):
        if ca is not None:
            np.testing.assert_array_equal(ca, cb, err_msg=str(tag))


def _serve(w, reqs):
    """Queue the requests on the batched worker, run it until idle, return each request's responses."""
    from fishmi import engine

    qs = [queue.Queue() for _ in reqs]
    for r, q in zip(reqs, qs):
        w.input.put(engine.GenerateRequest(request=r, response_queue=q))
    while True:
        w.tick(block=False)
        if not (w.active or w.pending) and w.input.empty():
            break
    return [[q.get() for _ in range(q.qsize())] for q in qs]


def _cache(model, max_bytes=1 << 20, min_positions=1):
    from fishmi.prefix_cache import PrefixCache

    return PrefixCache(model, max_bytes, min_positions)


def _base_len(model, req):
    from fishmi import engine

    return engine.ConversationJob(model, prefix_cache=_cache(CachingModel(1)), **req).base_len


def _voice(i, seed=0, text="<|speaker:0|>hello there. <|speaker:1|>and hello to you."):
    rng = np.random.default_rng(1000 + i)
    return dict(text=text, max_new_tokens=9, top_k=30, temperature=0.7, chunk_length=30, seed=seed,
                prompt_tokens=[rng.integers(0, CB, (C, 6 + i))], prompt_text=[f"voice {i} says this"])


def _pos0_after(calls, j, slot):
    """Start position of the first prefill of `slot` recorded after calls[j]."""
    for c in calls[j + 1:]:
        if c[0] == "prefill" and len(c) == 3 and c[1] == slot:
            return c[2]
        if c[0] == "prefill_batch" and len(c) == 3 and slot in c[1]:
            return c[2][c[1].index(slot)]
    return None


def test_batched_worker_with_cache_equals_serial_twice():
    """The nine requests of test_batching, served twice through a 4-slot BatchedWorker with a cache:
    exactly the serial generate_long responses both times; in the second round every batch of every
    voice request is a load_prefix of that voice's entry into its slot followed by a prefill of the
    slot at pos0 == base_len, and nothing is saved again."""
    from fishmi import engine
    from fishmi.batching import BatchedWorker

    reqs = _requests()
    serial = _serial_reference(reqs)
    mb = CachingModel(4)
    cache = _cache(mb)
    w = BatchedWorker(mb, 4, tick_frames=5, prefix_cache=cache)
    voiced = [i for i, r in enumerate(reqs) if "prompt_tokens" in r]
    assert voiced and len(voiced) < len(reqs)
    for rnd in range(2):
        mark = len(mb.calls)
        got = _serve(w, reqs)
        for i, (g, ref) in enumerate(zip(got, serial)):
            _same(g, ref, (rnd, i))
        assert cache.stats["inserts"] == len(voiced) == len(cache.entries)
    calls = mb.calls[mark:]
    assert not any(c[0] == "save_prefix" for c in calls)
    seen = 0
    for i in voiced:
        job = engine.ConversationJob(mb, prefix_cache=cache, **reqs[i])
        entry = cache._find(job.base_block)
        assert entry is not None and entry.P == job.base_len > 0
        loads = [(j, s) for j, c in enumerate(calls) if c[0] == "load_prefix" and c[1] == entry.pid for s in c[2]]
        assert len(loads) == sum(1 for a in _summary(serial[i]) if a[0] == "sample")  # every batch of every sample
        for j, s in loads:
            assert _pos0_after(calls, j, s) == job.base_len
        seen += len(loads)
    assert seen == sum(len(c[2]) for c in calls if c[0] == "load_prefix")
    cache.close()
    assert cache.stats["bytes"] == 0 and not mb.prefixes


def test_requests_without_references_never_touch_the_cache():
    from fishmi.batching import BatchedWorker

    mb = CachingModel(4)
    cache = _cache(mb)
    w = BatchedWorker(mb, 4, tick_frames=5, prefix_cache=cache)
    reqs = [r for r in _requests() if "prompt_tokens" not in r]
    for g, ref in zip(_serve(w, reqs), _serial_reference(reqs)):
        _same(g, ref)
    assert cache.stats == {"hits": 0, "misses": 0, "inserts": 0, "evictions": 0, "failures": 0, "bytes": 0}
    assert not any(c[0] in ("save_prefix", "load_prefix") for c in mb.calls)


def test_second_round_first_prefill_starts_at_base_len():
    """Each voice request of test_batching served alone after its voice is cached: its first model
    call is load_prefix(entry, [slot]) and its first prefill runs at pos0 == base_len."""
    from fishmi.batching import BatchedWorker

    for r in [r for r in _requests() if "prompt_tokens" in r]:
        mb = CachingModel(4)
        cache = _cache(mb)
        w = BatchedWorker(mb, 4, tick_frames=5, prefix_cache=cache)
        first = _serve(w, [r])
        base_len = _base_len(mb, r)
        assert base_len > 0 and cache.stats["inserts"] == 1
        entry = next(iter(cache.entries.values()))
        assert entry.P == base_len
        mark = len(mb.calls)
        second = _serve(w, [r])
        _same(second[0], first[0])
        calls = mb.calls[mark:]
        assert calls[0][:2] == ("load_prefix", entry.pid) and len(calls[0][2]) == 1
        assert calls[1] == ("prefill", calls[0][2][0], base_len)


def test_serial_generate_long_with_cache():
    """generate_long with a cache (slot 0), every request twice: the uncached responses both times;
    the second run of a voice request loads its entry and continues at pos0 == base_len."""
    from fishmi import engine

    reqs = _requests()
    serial = _serial_reference(reqs)
    m = CachingModel(1)
    cache = _cache(m)
    for rnd in range(2):
        for i, (r, ref) in enumerate(zip(reqs, serial)):
            mark = len(m.calls)
            got = [engine.WrappedGenerateResponse("success", o)
                   for o in engine.generate_long(model=m, prefix_cache=cache, **r)]
            _same(got, ref, (rnd, i))
            calls = m.calls[mark:]
            if "prompt_tokens" not in r:
                assert not any(c[0] in ("save_prefix", "load_prefix") for c in calls)
            elif rnd == 1:
                base_len = _base_len(m, r)
                assert calls[0][0] == "load_prefix" and calls[0][2] == (0,)
                first = next(c for c in calls if c[0] in ("prefill", "generate_at"))
                assert first[2] == base_len
                assert not any(c[0] == "save_prefix" for c in calls)
    assert cache.stats["inserts"] == len({i for i, r in enumerate(reqs) if "prompt_tokens" in r})


def test_same_voice_in_one_tick_shares_one_load_and_one_prefill_batch():
    from fishmi.batching import BatchedWorker

    mb = CachingModel(4)
    cache = _cache(mb)
    w = BatchedWorker(mb, 4, tick_frames=4, prefix_cache=cache)
    serial = _serial_reference([_voice(0, seed=s) for s in range(4)])
    # a new voice arriving twice in one tick: both miss, one entry (the second insert is the no-op)
    got = _serve(w, [_voice(0, seed=0), _voice(0, seed=1)])
    for g, ref in zip(got, serial[:2]):
        _same(g, ref)
    assert cache.stats["inserts"] == 1 and len(mb.prefixes) == 1
    assert [c[0] for c in mb.calls].count("save_prefix") == 1
    entry = next(iter(cache.entries.values()))
    mark = len(mb.calls)
    reqs = [_voice(0, seed=s) for s in range(4)] [1:] + [dict(text="no voice here", max_new_tokens=5, seed=9)]
    got = _serve(w, reqs)
    for g, ref in zip(got[:3], serial[1:]):
        _same(g, ref)
    calls = mb.calls[mark:]
    assert calls[0][:2] == ("load_prefix", entry.pid) and len(calls[0][2]) == 3  # one load for the three
    assert calls[1][0] == "prefill_batch" and len(calls[1][1]) == 4               # hits and the miss together
    by_slot = dict(zip(calls[1][1], calls[1][2]))
    assert sorted(by_slot.values()) == [0, entry.P, entry.P, entry.P]
    assert set(calls[0][2]) == {s for s, p in by_slot.items() if p == entry.P}
    first_tick = calls[:next(i for i, c in enumerate(calls) if c[0] == "decode")]
    assert [c[0] for c in first_tick].count("load_prefix") == 1
    assert [c[0] for c in first_tick].count("prefill_batch") == 1


def test_lru_eviction_with_room_for_one_entry():
    """max_bytes sized for one entry: a second voice evicts the first (drop_prefix), the first voice
    misses again afterwards, and every output is still the uncached one."""
    from fishmi.batching import BatchedWorker

    v0, v1 = _voice(0), _voice(1)
    serial = _serial_reference([v0, v1])
    mb = CachingModel(2)
    n0, n1 = _base_len(mb, v0), _base_len(mb, v1)
    cache = _cache(mb, max_bytes=ROW_BYTES * max(n0, n1))
    w = BatchedWorker(mb, 2, tick_frames=4, prefix_cache=cache)
    _same(_serve(w, [v0])[0], serial[0])
    pid0 = next(iter(cache.entries.values())).pid
    _same(_serve(w, [v1])[0], serial[1])
    assert ("drop_prefix", pid0) in mb.calls and cache.stats["evictions"] == 1 and pid0 not in mb.prefixes
    assert cache.stats["bytes"] == ROW_BYTES * n1 <= cache.max_bytes
    mark, misses = len(mb.calls), cache.stats["misses"]
    _same(_serve(w, [v0])[0], serial[0])
    calls = mb.calls[mark:]
    assert cache.stats["misses"] == misses + 1 and calls[0] == ("prefill", calls[0][1], 0)
    assert cache.stats["evictions"] == 2 and cache.stats["inserts"] == 3


@pytest.mark.parametrize("why", ["too_large", "oom"])
def test_block_not_stored_serves_uncached(why):
    from fishmi import engine
    from fishmi.batching import BatchedWorker

    v = _voice(0)
    serial = _serial_reference([v])
    mb = CachingModel(2, oom=(why == "oom"))
    cache = _cache(mb, max_bytes=ROW_BYTES * _base_len(mb, v) - (1 if why == "too_large" else 0))
    w = BatchedWorker(mb, 2, tick_frames=4, prefix_cache=cache)
    for _ in range(2):
        _same(_serve(w, [v])[0], serial[0])
    assert not cache.entries and cache.stats["inserts"] == 0 and cache.stats["hits"] == 0
    assert cache.stats["failures"] == (cache.stats["misses"] if why == "oom" else 0)
    assert not any(c[0] == "load_prefix" for c in mb.calls)
    m1 = CachingModel(1, oom=(why == "oom"))
    c1 = _cache(m1, max_bytes=cache.max_bytes)
    got = [engine.WrappedGenerateResponse("success", o) for o in engine.generate_long(model=m1, prefix_cache=c1, **v)]
    _same(got, serial[0])
    assert not c1.entries


def test_lookup_and_insert_rules():
    m = CachingModel(1)
    rng = np.random.default_rng(5)
    enc = rng.integers(0, CB, (C + 1, 40)).astype(np.int32)
    m.prefill(0, enc, m.sampling())
    cache = _cache(m, min_positions=8)
    assert cache.insert(0, enc[:, :7]) is None                       # shorter than min_positions
    e20 = cache.insert(0, enc[:, :20])
    assert cache.insert(0, enc[:, :20]) is e20 and cache.stats["inserts"] == 1  # already present
    e30 = cache.insert(0, enc[:, :30])
    assert cache.lookup(enc) is e30                                  # the longest
    assert cache.lookup(enc[:, :30]) is e20                          # at least one position to prefill
    assert cache.lookup(enc[:, :20]) is None
    other = enc.copy()
    other[3, 25] ^= 1
    assert cache.lookup(other) is e20                                # tokens compared, not the digest alone
    other[0, 0] ^= 1
    assert cache.lookup(other) is None
    assert cache.stats["hits"] == 3 and cache.stats["misses"] == 2
    assert cache.stats["bytes"] == ROW_BYTES * 50
    cache.close()
    assert not m.prefixes


def test_no_cache_call_log_is_todays():
    """prefix_cache=None: the model call log equals that of a worker built without the argument."""
    from fishmi.batching import BatchedWorker

    logs = []
    for kw in ({}, {"prefix_cache": None}):
        mb = ScriptedModel(4)
        w = BatchedWorker(mb, 4, tick_frames=5, **kw)
        got = _serve(w, _requests())
        logs.append((mb.calls, [_summary(g) for g in got]))
    assert logs[0][0] == logs[1][0]
    assert any(c[0] == "prefill_batch" for c in logs[0][0])
