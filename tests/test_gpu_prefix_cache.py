"""Voice prefix cache on the GPU: fm_llm_prefix_save / _load / _drop / _info (the copy kernel of
csrc/fm_prefix.hip), fm_llm_prefill_batch_at, and fishmi.prefix_cache.PrefixCache through the
engine.  The copy is checked bit for bit on slot 0's cache rows and through the tokens other slots
emit after a load; the engine flow against the reference's own generate_long goldens."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import tuned

pytestmark = pytest.mark.gpu

IM_END = 4


def _cfg(name):
    from fishmi.config import DualARConfig

    cfg = DualARConfig.from_pretrained(os.path.join(GOLDEN, name))
    cfg.im_end_id = IM_END
    return cfg


def _build(name, prec, max_slots, golden):
    """llm_a: the tiny checkpoint (head_dim 32, 2 kv heads, 4 layers); llm_b: synthetic (1 kv head, biases, 3
    layers); llm_wide: synthetic at the S2-Pro head geometry (head_dim 128, 8 kv heads), 2 layers, 128 positions."""
    from fishmi.checkpoint import load_llm_weights
    from fishmi.llm import DualARModel

    cfg = _cfg(name)
    if name == "llm_a":
        m = DualARModel(cfg, 0, prec, max_slots)
        m.load_weights(load_llm_weights(os.path.join(GOLDEN, name)))
        m.finalize()
        return m
    g = golden(f"{name}_bf16.npz")
    return DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, prec, max_slots)


@pytest.fixture(scope="module")
def models(golden):
    built = {}

    def get(name, prec, max_slots=1):
        k = (name, prec, max_slots)
        if k not in built:
            built[k] = _build(name, prec, max_slots, golden)
        return built[k]

    yield get
    for m in built.values():
        m.close()


def _prompt(cfg, T, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((cfg.num_codebooks + 1, T), np.int32)
    p[0] = rng.integers(16, cfg.semantic_begin_id, T)
    p[1:] = rng.integers(0, cfg.codebook_size, (cfg.num_codebooks, T))
    return p


def _greedy(seed=0):
    from fishmi.llm import DualARModel

    return DualARModel.sampling(top_k=1, seed=seed, mask_im_end=True)


def _read_all(m):
    """Slot 0's K and V rows of every slow layer: (n_layer, 2, nkv, S, hd), the stored values as floats."""
    return np.stack([np.stack(m.read_cache(layer)) for layer in range(m.cfg.n_layer)])


LEN_A, LEN_B = 61, 90


@pytest.mark.parametrize("npos", [1, 37, LEN_A])
@pytest.mark.parametrize("name", ["llm_a", "llm_wide"])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_copy_bit_for_bit(prec, name, npos, models):
    """save_prefix / load_prefix alone: after prompt A's rows [0, npos) are saved, a longer prompt B
    overwrites the slot, and the prefix is loaded back, rows [0, npos) are A's bit for bit, rows
    >= npos are B's bit for bit, and the slot's cached position is npos."""
    m = models(name, prec)
    a, b = _prompt(m.cfg, LEN_A, 1), _prompt(m.cfg, LEN_B, 2)
    m.prefill(0, a, _greedy())
    rows_a = _read_all(m)
    pid = m.save_prefix(0, npos)
    assert m.prefix_info(pid) == (npos, m.prefix_bytes(npos))
    np.testing.assert_array_equal(_read_all(m), rows_a)  # the save leaves the slot as it was
    assert m.slot_pos(0) == LEN_A
    m.prefill(0, b, _greedy())
    rows_b = _read_all(m)
    assert not np.array_equal(rows_a[:, :, :, :npos], rows_b[:, :, :, :npos])
    m.load_prefix(pid, [0])
    got = _read_all(m)
    np.testing.assert_array_equal(got[:, :, :, :npos], rows_a[:, :, :, :npos])
    np.testing.assert_array_equal(got[:, :, :, npos:], rows_b[:, :, :, npos:])
    assert m.slot_pos(0) == npos
    m.drop_prefix(pid)


def test_copy_scalar_path_bit_for_bit(models):
    """The copy's scalar path (taken where a run or a base is not 16-byte aligned; forced here by the
    prefix_vec knob) moves the same rows as the vector path."""

    m = models("llm_a", "bf16")
    a, b = _prompt(m.cfg, LEN_A, 1), _prompt(m.cfg, LEN_B, 2)
    npos = 37
    with tuned(prefix_vec=0):
        m.prefill(0, a, _greedy())
        rows_a = _read_all(m)
        pid = m.save_prefix(0, npos)
        m.prefill(0, b, _greedy())
        rows_b = _read_all(m)
        m.load_prefix(pid, [0])
        got = _read_all(m)
    np.testing.assert_array_equal(got[:, :, :, :npos], rows_a[:, :, :, :npos])
    np.testing.assert_array_equal(got[:, :, :, npos:], rows_b[:, :, :, npos:])
    m.drop_prefix(pid)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_load_across_slots(prec, models):
    """A prefix saved from slot 1 and loaded into slots 0 and 2 in one call (both held another, longer
    prompt) continues exactly as slot 1 itself does: the same suffix prefilled at pos0 = npos with the
    same greedy record gives identical first columns and 6 identical frames on the three slots.  Slot
    3, holding an unrelated prompt, decodes the same 6 frames as in a run without any of this."""
    m = models("llm_a", prec, 4)
    cfg = m.cfg
    a, suffix, c, d = _prompt(cfg, 50, 3), _prompt(cfg, 9, 4), _prompt(cfg, 44, 5), _prompt(cfg, 70, 6)
    npos = 37
    m.prefill(3, c, _greedy(7))
    undisturbed = m.decode_frames([3], 6)

    first3 = m.prefill(3, c, _greedy(7))
    for s in (0, 2):
        m.prefill(s, d, _greedy())
    m.prefill(1, a, _greedy())
    pid = m.save_prefix(1, npos)
    m.load_prefix(pid, [0, 2])
    assert [m.slot_pos(s) for s in range(4)] == [npos, 50, npos, 44]
    firsts = [m.prefill(s, suffix, _greedy(11), pos0=npos) for s in (0, 1, 2)]
    frames = m.decode_frames([0, 1, 2], 6)
    for s in (0, 2):
        np.testing.assert_array_equal(firsts[s], firsts[1])
        np.testing.assert_array_equal(frames[:, s], frames[:, 1])
    np.testing.assert_array_equal(m.decode_frames([3], 6), undisturbed)
    assert first3.shape == (cfg.num_codebooks + 1,)
    m.drop_prefix(pid)


def _hold_prefixes(m, prefixes, kinds, junk):
    """Give slot i a prefix of its own length: kind 0 none (the slot keeps whatever it held), 1 loaded
    from a snapshot taken on that slot before `junk` overwrote it, 2 prefilled by the slot itself."""
    pids = []
    for i, (p, k) in enumerate(zip(prefixes, kinds)):
        if k == 0:
            continue
        m.prefill(i, p, _greedy())
        if k == 1:
            pid = m.save_prefix(i, p.shape[1])
            m.prefill(i, junk, _greedy())
            m.load_prefix(pid, [i])
            pids.append(pid)
    for pid in pids:
        m.drop_prefix(pid)


@pytest.mark.parametrize("n", [3, 10])
def test_prefill_batch_at_matches_single(n, models):
    """fm_llm_prefill_batch_at gives every request the first column and the greedy continuation of
    its own fm_llm_prefill_at (fp32; n = 3 takes the batch-1 GEMV tail, n = 10 the batched one),
    with start positions 0, a loaded prefix's and a self-prefilled one's in one call; with every
    start position zero it is fm_llm_prefill_batch."""
    m = models("llm_b", "fp32", n)
    cfg = m.cfg
    rng = np.random.default_rng(57 + n)
    kinds = [i % 3 for i in range(n)]
    plen = [0 if k == 0 else int(rng.integers(3, 80)) for k in kinds]
    prefixes = [_prompt(cfg, max(P, 1), 100 + i) for i, P in enumerate(plen)]
    suffixes = [_prompt(cfg, int(rng.integers(1, 60)), 200 + i) for i in range(n)]
    junk = _prompt(cfg, 85, 99)
    sps = [_greedy(s) for s in range(n)]
    slots = list(range(n))
    assert {0, 1, 2} <= set(kinds)

    _hold_prefixes(m, prefixes, kinds, junk)
    single = [m.prefill(s, x, sp, pos0=P) for s, x, sp, P in zip(slots, suffixes, sps, plen)]
    single_fr = m.decode_frames(slots, 6)
    _hold_prefixes(m, prefixes, kinds, junk)
    batch = m.prefill_batch(slots[::-1], suffixes[::-1], sps[::-1], pos0=plen[::-1])[::-1]
    assert [m.slot_pos(s) for s in slots] == [P + x.shape[1] for P, x in zip(plen, suffixes)]
    batch_fr = m.decode_frames(slots, 6)
    np.testing.assert_array_equal(np.stack(single), batch)
    np.testing.assert_array_equal(single_fr, batch_fr)

    plain = m.prefill_batch(slots, suffixes, sps)
    plain_fr = m.decode_frames(slots, 6)
    zero = m.prefill_batch(slots, suffixes, sps, pos0=[0] * n)
    zero_fr = m.decode_frames(slots, 6)
    np.testing.assert_array_equal(plain, zero)
    np.testing.assert_array_equal(plain_fr, zero_fr)


def _ckpt(tmp_path):
    d = tmp_path / "ckpt"
    shutil.copytree(os.path.join(GOLDEN, "llm_a"), d)
    for f in ("tokenizer.json", "tokenizer_config.json"):
        shutil.copy(os.path.join(GOLDEN, "tok_tiny", f), d / f)
    return str(d)


def _request(g, **kw):
    r = dict(device="cuda", max_new_tokens=7, text=str(g["text"]), top_p=0.9, repetition_penalty=1.1,
             temperature=0.7, compile=False, iterative_prompt=True, chunk_length=30,
             prompt_tokens=[g["ptok0"], g["ptok1"]], prompt_text=["ref a", "<|speaker:1|>ref b"], top_k=1)
    r.update(kw)
    return r


def test_engine_fp32_codes_equal_reference(golden, tmp_path):
    """generate_long with a voice prefix cache, twice, on the reference's own request (engine.npz,
    fp32 greedy): both runs give the reference's codes; the first run inserts the voice once, and
    the second run's first batch loads it and prefills only the suffix at pos0 = base_len."""
    from fishmi import engine
    from fishmi.llm import DualARModel
    from fishmi.prefix_cache import PrefixCache

    g = golden("engine.npz")
    m = DualARModel.from_pretrained(_ckpt(tmp_path), device=0, precision="fp32", max_length=2560)
    cache = PrefixCache(m, 64 << 20, min_positions=1)
    calls = []
    gen, gen_at, load = m.generate, m.generate_at, m.load_prefix

    def spy_gen(prompt, *a, **k):
        calls.append(("generate", 0, prompt.shape[1]))
        return gen(prompt, *a, **k)

    def spy_at(suffix, pos0, *a, **k):
        calls.append(("generate_at", pos0, suffix.shape[1]))
        return gen_at(suffix, pos0, *a, **k)

    def spy_load(pid, slots):
        calls.append(("load", pid, tuple(slots)))
        return load(pid, slots)

    m.generate, m.generate_at, m.load_prefix = spy_gen, spy_at, spy_load
    req = _request(g)
    base_len = engine.ConversationJob(m, prefix_cache=cache, **req).base_len
    assert base_len > 0
    runs = []
    for _ in range(2):
        calls.append(("run",))
        runs.append([o.codes for o in engine.generate_long(model=m, prefix_cache=cache, **req) if o.action == "sample"])
        assert cache.stats["inserts"] == 1
    for codes in runs:
        assert len(codes) >= 3
        for i, c in enumerate(codes):
            np.testing.assert_array_equal(c, g[f"codes_{i}"])
    second = calls[len(calls) - 1 - calls[::-1].index(("run",)):]
    entry = next(iter(cache.entries.values()))
    assert second[1] == ("load", entry.pid, (0,)) and second[2][:2] == ("generate_at", base_len)
    assert calls[1][0] == "generate"  # the first run's first batch: the whole prompt, then the insert
    assert m.prefix_info(entry.pid)[0] == base_len
    cache.close()
    assert cache.stats["bytes"] == 0
    m.close()


def test_engine_bf16_within_reference_error(golden, tmp_path):
    """bf16: after one uncached pass has inserted the voice, batch 0 of the reference's bf16
    conversation (engine_bf16.npz) is teacher-forced through ConversationJob with the cache -- load
    the voice's rows, prefill the suffix at pos0, decode -- and its logits stay within 1.5x the
    reference's own bf16-vs-fp32 error (parity_util.bf16_vs_reference)."""
    from fishmi import engine
    from fishmi.llm import DualARModel
    from fishmi.prefix_cache import PrefixCache
    from parity_util import bf16_vs_reference

    g = golden("engine_bf16.npz")
    req = _request(golden("engine.npz"))
    m = DualARModel.from_pretrained(_ckpt(tmp_path), device=0, precision="bf16", max_length=2560)
    cache = PrefixCache(m, 64 << 20, min_positions=1)
    plan = engine.ConversationJob(m, prefix_cache=cache, **req).next_batch()
    assert plan.prefix is None and plan.L == 0 and plan.insert_len > 0
    m.prefill(0, plan.enc, plan.sp)
    assert cache.insert(0, plan.enc[:, :plan.insert_len]) is not None

    job = engine.ConversationJob(m, prefix_cache=cache, **req)
    plan = job.next_batch()
    np.testing.assert_array_equal(plan.enc, g["prompt_0"])
    assert plan.prefix is not None and plan.L == job.base_len == plan.prefix.P
    m.prefill(0, _prompt(m.cfg, plan.enc.shape[1] + 5, 8), m.sampling(top_k=1))  # the slot held something else
    m.load_prefix(plan.prefix.pid, [0])
    cols = g["cols_0"]
    n = cols.shape[1]
    slow = np.zeros((n, m.cfg.vocab_size), np.float32)
    fast = np.zeros((n, m.cfg.num_codebooks - 1, m.cfg.codebook_size), np.float32)
    sp = m.sampling(top_k=1)
    try:
        for j in range(n):
            m.force(0, cols[:, j])
            if j == 0:
                m.prefill(0, plan.enc[:, plan.L:], sp, pos0=plan.L)
            else:
                m.decode([0])
            slow[j], fast[j] = m.read_logits(0)
    finally:
        m.force(0, None)
    assert m.slot_pos() == plan.enc.shape[1] + n - 1
    bf16_vs_reference(slow, fast, g["slow_0"], g["fast_0"], g["slow32_0"], g["fast32_0"])
    cache.close()
    m.close()


def test_argument_errors(models):
    """Host-side argument checks raise with a message, and the handle serves a normal prefill afterwards."""
    from fishmi import native

    m = models("llm_a", "fp32", 4)
    cfg = m.cfg
    a = _prompt(cfg, 20, 12)
    first = m.prefill(0, a, _greedy())
    pid = m.save_prefix(0, 20)
    for call, word in [(lambda: m.load_prefix(pid + 1000, [0]), "prefix id"),
                       (lambda: m.save_prefix(0, 21), "npos"),
                       (lambda: m.save_prefix(0, 0), "npos"),
                       (lambda: m.load_prefix(pid, [1, 1]), "duplicate"),
                       (lambda: m.load_prefix(pid, [4]), "slot"),
                       (lambda: m.prefill_batch([0, 1], [a, a], [_greedy(), _greedy()], pos0=[21, 0]), "cached positions"),
                       (lambda: m.prefill_batch([0, 1], [a, a], [_greedy(), _greedy()], pos0=[0, cfg.max_seq_len - 20]),
                        "max_seq_len")]:
        with pytest.raises(native.FishMIError, match=word):
            call()
    m.drop_prefix(pid)
    for call in (lambda: m.load_prefix(pid, [0]), lambda: m.drop_prefix(pid), lambda: m.prefix_info(pid)):
        with pytest.raises(native.FishMIError, match="prefix id"):
            call()
    assert m.slot_pos(0) == 20
    np.testing.assert_array_equal(m.prefill(0, a, _greedy()), first)
