"""fm_tune slow_attn_wo: a batch-1 bf16 slow layer runs its attention and its wo as one
launch (fm_rowgemv.hip slow_attn_wo_kernel): attn_fd's blocks at 8 waves and one q head per block publish their output
as tagged words, wo's row blocks issue their weights and then poll those words.  The change claims bit identity, so
every comparison is array_equal: the fused launch against the two launches it replaces through fm_op_slow_attn_wo
(poisoned caches, stale tagged words, two slots at one position, a stream decoded twice), whole frames under knob 0, 1
and 2 (teacher-forced and sampled, eager and graph, three slots in permuted order, a cache of sixteen splits), the launch counts, and the
settings under which the knob must change nothing.  Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

import attn_ref as ar
import linear_ref as lr
from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced
from test_gpu_rowgemv import _biased_cfg

pytestmark = pytest.mark.gpu

# (nh, nkv, hd, dim): the smallest shape with a 4-q-head group and a wo run of more than one row block per group;
# S2-Pro's widths; one q head per kv head (the only head group is the one that stores K / V).  head_dim 64 has no
# instantiation: test_op_not_dispatchable_is_a_status
SHAPES = [(8, 2, 128, 256), (32, 8, 128, 2560), (2, 2, 128, 256)]
S = 1024
# the pass (128 positions), tile (16) and split (cap 256) edges of an 8-wave block
POSITIONS = [0, 1, 15, 16, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, S - 1]


def _tag(pos, gen):
    """slow_attn_wo_kernel's hand-off tag of launch index gen at position pos"""
    return (pos * 41 + gen) % 65535 + 1


def _stale(K, pos, gen):
    """tagged words an earlier launch could have left: NaN values under the generations one off the current one
    (even words one below, odd words one above), wrapped into the tag's range 1 .. 65535"""
    t = _tag(pos, gen)
    lo, hi = (t - 2) % 65535 + 1, t % 65535 + 1
    w = np.where(np.arange(K) % 2 == 0, lo, hi).astype(np.uint32)
    return (np.uint32(0x7FC0) << np.uint32(16)) | w


def _operands(shape, seed=5):
    nh, nkv, hd, dim = shape
    K = nh * hd
    rng = np.random.default_rng([seed, nh, nkv, hd, dim])
    return lr.mk(rng, (dim, K), "bf16", K ** -0.5), lr.mk(rng, (dim,), "bf16", 0.5), lr.mk(rng, (dim,), "bf16")


def native_get(key):
    from fishmi import native

    return native.tune_get(key)


def _run(c, w, res, **kw):
    from fishmi import ops

    return ops.slow_attn_wo(kw.pop("qkv", c["qkv"]), c["nh"], c["nkv"], c["hd"], kw.pop("slots", c["row_slot"]),
                            kw.pop("pos", c["pos"]), c["kc"], c["vc"], c["rope_base"], w, res, qn=c["qn"], kn=c["kn"],
                            layer=c["layer"], **kw)


def _same(a, b, msg=""):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(ar.bits(x), ar.bits(y), err_msg=msg)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_positions_on_poisoned_caches(shape, knob):
    """One fused launch per position (slot 1 of 2; the small shapes: layer 1 of 2) on caches whose every word the
    kernels must not read is NaN, the tagged-word buffer pre-filled with NaN values under the generations one below
    and one above the current one: dispatchable, err == 0, finite, and the output row and the written K / V rows
    equal those of attn_fd + row GEMV on the same operands, with 2 and with 4 wo rows per group under the default wait
    knobs, and with 4 rows and no wait control at all (slow_aw_delay 0, slow_aw_cheap 0: every wave's full reads start
    over the stale words, microseconds before the attention stores, so only the full read's tag compare keeps them
    out); q-norm on (diffuse) and off (rising)."""
    nh, nkv, hd, dim = shape
    w, bias, res = _operands(shape)
    layers = 1 if dim > 256 else 2
    waits = {k: native_get(k) for k in ("slow_aw_delay", "slow_aw_cheap")}
    for fam in ("diffuse",) if dim > 256 else ("diffuse", "rising"):
        for pos in POSITIONS:
            c = ar.make_case(fam, nh, nkv, hd, pos, S, "bf16", row_slot=[1], nslots=2, layers=layers, layer=layers - 1)
            ref = _run(c, w, res, bias=bias, fused=False)
            assert ref[4] == 0 and np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all()
            gen = 1 + pos % 40
            for rp, bare in ((2, False), (4, False), (4, True)):
                knob("slow_aw_delay", 0 if bare else waits["slow_aw_delay"])
                knob("slow_aw_cheap", 0 if bare else waits["slow_aw_cheap"])
                f = _run(c, w, res, bias=bias, rp=rp, gens=gen, xt_init=_stale(nh * hd, pos, gen))
                assert f[3] and f[4] == 0, (fam, pos, rp, bare, f[3], f[4])
                _same(f, ref, f"{fam} pos {pos} rp {rp} bare {bare}")


def test_op_sixteen_splits_and_a_grid_of_idle_attention_blocks():
    """S 4096 (maxsplit 16, as at max_seq_len 5120: nh x 16 attention blocks ahead of the wo blocks, most of which
    leave after their first round trip): one split with 15 idle blocks per head, two splits, and all sixteen; the
    default wait knobs (the delay estimate at its largest) and none.  The two launches' bits, err == 0."""
    nh, nkv, hd, dim = SHAPES[0]
    w, bias, res = _operands(SHAPES[0])
    for pos in (3, 300, 3840, 4095):
        c = ar.make_case("diffuse", nh, nkv, hd, pos, 4096, "bf16")
        ref = _run(c, w, res, bias=bias, fused=False)
        assert ref[4] == 0 and np.isfinite(ref[0]).all()
        for rp in (2, 4):
            f = _run(c, w, res, bias=bias, rp=rp, gens=9, xt_init=_stale(nh * hd, pos, 9))
            assert f[3] and f[4] == 0, (pos, rp, f[4])
            _same(f, ref, f"pos {pos} rp {rp}")


def test_op_two_slots_at_one_position_and_a_following_layer():
    """Four launches in a row on one tagged-word buffer, as two frames of two layers leave them: slot 0 then slot 1
    at the same position, launch indices 1, 2 each, every run with its own QKV row.  Each run's outputs equal the two
    launches' -- a run never takes its predecessor's words (another slot's under the same tag two launches back, or
    the previous layer's) for its own."""
    nh, nkv, hd, dim = SHAPES[0]
    w, bias, res = _operands(SHAPES[0])
    for pos in (129, 300):
        c = ar.make_case("diffuse", nh, nkv, hd, [pos, pos], S, "bf16", row_slot=[0, 1])
        qkv = np.stack([c["qkv"][0], -c["qkv"][0], c["qkv"][1], -c["qkv"][1]])
        kw = dict(qkv=qkv, slots=[0, 0, 1, 1], pos=[pos] * 4, gens=[1, 2, 1, 2], restore=True)
        ref = _run(c, w, res, fused=False, **kw)
        for rp in (2, 4):
            f = _run(c, w, res, rp=rp, **kw)
            assert f[3] and f[4] == 0
            _same(f, ref, f"pos {pos} rp {rp}")
        assert not np.array_equal(ref[0][0], ref[0][2]) and not np.array_equal(ref[0][0], ref[0][1])


def test_op_stream_decoded_twice():
    """300 positions of one stream (each run reads the rows the runs before it wrote, launch indices cycling as the
    layers of a frame do) decoded twice with the fused launch and once with the two launches: identical output rows
    and identical written K / V rows."""
    nh, nkv, hd, dim = SHAPES[0]
    w, bias, res = _operands(SHAPES[0])
    n, p0 = 300, 100
    c = ar.make_case("diffuse", nh, nkv, hd, p0, S, "bf16")
    rng = np.random.default_rng(9)
    qkv = ar.rb("bf16")(rng.standard_normal((n, (nh + 2 * nkv) * hd))).astype(np.float32)
    kw = dict(qkv=qkv, slots=0, pos=np.arange(p0, p0 + n), gens=1 + np.arange(n) % 36, restore=False)
    a = _run(c, w, res, **kw)
    b = _run(c, w, res, **kw)
    ref = _run(c, w, res, fused=False, **kw)
    assert a[3] and a[4] == 0 and b[4] == 0 and np.isfinite(a[0]).all()
    _same(a, b)
    _same(a, ref)


def test_op_wait_settings_change_no_bit(knob):
    """How the wo waves wait is speed only: a first-read delay of 100 and 300 per cent of the estimated attention time,
    sleeps of 4 and 16 between reads and the one-word-per-128 poll ahead of the full reads (over stale words one
    generation off) give the two launches' bits, at one split and past it, err == 0."""
    nh, nkv, hd, dim = SHAPES[0]
    w, bias, res = _operands(SHAPES[0])
    for pos in (16, 255, 513):
        c = ar.make_case("diffuse", nh, nkv, hd, pos, S, "bf16")
        ref = _run(c, w, res, bias=bias, fused=False)
        for delay, sleep, cheap in ((100, 1, 0), (300, 4, 0), (0, 16, 1), (100, 4, 1)):
            knob("slow_aw_delay", delay)
            knob("slow_aw_sleep", sleep)
            knob("slow_aw_cheap", cheap)
            for rp in (2, 4):
                f = _run(c, w, res, bias=bias, rp=rp, gens=7, xt_init=_stale(nh * hd, pos, 7))
                assert f[3] and f[4] == 0, (pos, delay, sleep, cheap, rp)
                _same(f, ref, f"pos {pos} delay {delay} sleep {sleep} cheap {cheap} rp {rp}")


def test_op_not_dispatchable_is_a_status(knob):
    """Where the frame would keep its two launches the hook reports it and launches nothing: a wo depth without an
    instantiation (K = nh hd = 2560: 3 chunks per wave), head_dim 64 and 32, fd_hpb 2, fd_nw 4, gemv_chain 1; the
    unfused composition still runs."""
    def ok(shape):
        nh, nkv, hd, dim = shape
        w, bias, res = _operands(shape)
        c = ar.make_case("diffuse", nh, nkv, hd, 40, 64, "bf16")
        return _run(c, w, res)[3], _run(c, w, res, fused=False)

    assert ok(SHAPES[0])[0]
    assert not ok((20, 5, 128, 256))[0] and not ok((8, 2, 64, 256))[0] and not ok((8, 2, 32, 256))[0]
    for key, val in (("fd_hpb", 2), ("fd_nw", 4), ("gemv_chain", 1)):
        knob(key, val)
        good, un = ok(SHAPES[0])
        assert not good and np.isfinite(un[0]).all(), key
        knob(key, {"fd_hpb": 1, "fd_nw": 8, "gemv_chain": 0}[key])


# ---- whole frames on a tiny model ---------------------------------------------------------------------------------

NL = 3       # slow layers
T0 = 250     # prompt rows: 40 frames on cross position 256 (the second split, the combiner) at frame 7


def _tiny_cfg(o_bias, **kw):
    """test_gpu_rowgemv's biased layout (dim 512) with slow heads 8 / 2 x 128 (the instantiated head_dim), 3 slow
    layers, qk-norm on, room for 320 positions, with or without attention_o_bias"""
    base = _biased_cfg()
    kw.setdefault("max_seq_len", 320)
    cfg = dataclasses.replace(base, n_layer=NL, head_dim=128, attention_qk_norm=True, attention_o_bias=o_bias, **kw)
    cfg.im_end_id = base.im_end_id
    return cfg


def _inputs(cfg, seed, nf, T=T0):
    rng = np.random.default_rng(seed)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, T), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, T)
    cols = np.zeros((C1, nf), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, nf)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, nf))
    return prompt, cols


def _launches(m, classes=("linear", "attn", "slow_attn_wo")):
    """Launch counts per profiler class of one eager frame on slot 0 (the host checks chain_err after it)."""
    m.profile(True)
    try:
        before = {c: m.profile_read(c)[1] for c in classes}
        m.decode([0])
        return {c: m.profile_read(c)[1] - before[c] for c in classes}
    finally:
        m.profile(False)


def _sampled(m, slot, prompt, nframes):
    from fishmi.llm import DualARModel

    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=1234, mask_im_end=True)
    first = m.prefill(slot, prompt, sp)
    return np.concatenate([first[None], m.decode_frames([slot], nframes)[:, 0]])


@pytest.mark.parametrize("o_bias", [False, True])
def test_whole_frames_teacher_forced_and_sampled(o_bias, knob):
    """42 teacher-forced frames from a 250-row prompt (positions 250 .. 291: one split, then two and the combiner):
    slow logits, fast logits and emitted columns equal under slow_attn_wo 0, 1 and 2, the graph re-captured per
    setting; 8 frames run eagerly equal their graph replay; 40 sampled frames give the same columns; the launch
    counts of a frame move by the layer count: attn -L, linear -L, slow_attn_wo +L."""
    from fishmi.llm import DualARModel

    cfg = _tiny_cfg(o_bias)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3, 42)
    try:
        out, smp, n = {}, {}, {}
        for v in (0, 1, 2):
            knob("slow_attn_wo", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols)
            smp[v] = _sampled(m, 0, prompt, 40)
            m.prefill(0, prompt, DualARModel.sampling(top_k=1))
            n[v] = _launches(m)
        assert np.isfinite(out[0][1]).all()
        for v in (1, 2):
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo {v}")
            np.testing.assert_array_equal(smp[0], smp[v])
            assert n[0]["attn"] - n[v]["attn"] == NL and n[0]["linear"] - n[v]["linear"] == NL, n
            assert n[0]["slow_attn_wo"] == 0 and n[v]["slow_attn_wo"] == NL, n
        assert len(np.unique(smp[1][:, 1:])) > 8  # a sampled stream, not one repeated code
        for v in (1, 2):
            knob("slow_attn_wo", v)
            res = {}
            for graph in (False, True):
                m.use_graph(graph)
                res[graph] = _forced(m, prompt, cols[:, :8])
            for a, b in zip(res[False], res[True]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo {v}")
    finally:
        m.use_graph(True)
        m.close()


def test_three_slots_one_at_a_time(knob):
    """A handle with 3 slots decoded one slot at a time in permuted slot order, the slots at equal and at different
    positions (the tagged words are one buffer for all of them): the streams agree under slow_attn_wo 0, 1 and 2."""
    from fishmi.llm import DualARModel

    cfg = _tiny_cfg(False)
    m = DualARModel.synthetic(cfg, 13, 5, 0, "bf16", 3)
    prompts = [_inputs(cfg, 5 + s, 1, T=(250, 250, 120)[s])[0] for s in range(3)]
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=77, mask_im_end=True)
    order = [(2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0)]
    try:
        single = {}
        for v in (0, 1, 2):
            knob("slow_attn_wo", v)
            m.use_graph(True)
            got = {s: [m.prefill(s, prompts[s], sp)] for s in range(3)}
            for k in range(12):
                for s in order[k % len(order)]:
                    got[s].append(m.decode([s])[0])
            single[v] = np.stack([np.stack(got[s]) for s in range(3)])
        np.testing.assert_array_equal(single[0], single[1])
        np.testing.assert_array_equal(single[0], single[2])
        assert len(np.unique(single[1][:, :, 1:])) > 8
    finally:
        m.close()


def test_frames_on_a_cache_of_sixteen_splits(knob):
    """max_seq_len 5120 (maxsplit 16: 8 x 16 attention blocks per fused launch, all but 8 or 16 of them idle): 12
    teacher-forced frames across position 256 and 12 sampled ones equal under slow_attn_wo 0, 1 and 2, graph
    replay, the default wait knobs."""
    from fishmi.llm import DualARModel

    cfg = _tiny_cfg(False, max_seq_len=5120)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3, 12)
    try:
        out, smp = {}, {}
        for v in (0, 1, 2):
            knob("slow_attn_wo", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols)
            smp[v] = _sampled(m, 0, prompt, 12)
        for v in (1, 2):
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo {v}")
            np.testing.assert_array_equal(smp[0], smp[v])
    finally:
        m.close()


@pytest.mark.parametrize("setting", [("fd_hpb", 2), ("fd_nw", 4), ("gemv_chain", 1), ("fp32", 0), ("int8", 0), ("n2", 0)])
def test_fallbacks_leave_the_frame_alone(setting, knob):
    """Where a precondition fails -- fd_hpb 2, fd_nw 4, gemv_chain 1, an fp32 handle, an int8 handle, two rows per
    frame -- the knob changes nothing: today's launches (none of the new class) and the same bits."""
    from fishmi.llm import DualARModel

    key, val = setting
    cfg = _tiny_cfg(False)
    extra = {"quant": "int8"} if key == "int8" else {}
    slots = 2 if key == "n2" else 1
    m = DualARModel.synthetic(cfg, 11, 5, 0, "fp32" if key == "fp32" else "bf16", slots, **extra)
    prompt, cols = _inputs(cfg, 3, 10)
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=5, mask_im_end=True)
    try:
        if key in ("fd_hpb", "fd_nw", "gemv_chain"):
            knob(key, val)
        out, n = {}, {}
        for v in (0, 1, 2):
            knob("slow_attn_wo", v)
            m.use_graph(True)
            if key == "n2":
                for s in range(2):
                    m.prefill(s, prompt, sp)
                out[v] = (m.decode_frames([0, 1], 10),)
                m.profile(True)
                before = m.profile_read("slow_attn_wo")[1]
                m.decode([0, 1])
                n[v] = {"slow_attn_wo": m.profile_read("slow_attn_wo")[1] - before}
                m.profile(False)
            else:
                out[v] = _forced(m, prompt, cols)
                m.prefill(0, prompt, DualARModel.sampling(top_k=1))
                n[v] = _launches(m)
        assert n[0] == n[1] == n[2] and n[1]["slow_attn_wo"] == 0, n
        for v in (1, 2):
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo {v}")
    finally:
        m.close()
