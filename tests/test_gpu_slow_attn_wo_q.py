"""fm_tune slow_attn_wo_q: a batch-1 slow layer of a weight-only int8 / int4 handle runs its
attention and its wo as one launch (fm_rowgemv.hip slow_attn_wo_kernel<U, HD, RP, QM>): attn_fd's blocks publish tagged
words, wo's row blocks issue their row-major codes (and row scales / group (scale, zero) words) and then poll those
words.  The claim is bit identity with the two launches it replaces, so every comparison is array_equal, fused against
attn_fd + row GEMV on the same codes through fm_op_slow_attn_wo_q (poisoned caches, stale tagged words, sixteen splits,
two slots at one position, a stream decoded twice) and whole frames under the knob's three values (teacher-forced and
sampled, eager and graph, compact handles, three slots in permuted order, a cache of sixteen splits), the launch
counts, and the settings under which the knob must change nothing.  The unfused halves are held to float64 references
elsewhere (test_gpu_attn_ops.py, test_gpu_linear_ops.py); this file pins only the fusion.  Every test sets
slow_attn_wo_q itself.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

import attn_ref as ar
from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced
from test_gpu_slow_attn_wo import NL, POSITIONS, S, _inputs, _operands, _sampled, _stale, _tiny_cfg

pytestmark = pytest.mark.gpu

# (nh, nkv, hd, N): K 1024 = two 512-k chunks, so two waves of each group own none (nmy == 0), a 4-head group and more
# than one wo block; K 2048, one chunk per wave; S2-Pro's K 4096, both chunks of every wave (depth 2); one q head per
# kv head: at 2 / 2 heads K is 256, half a 512-k chunk, which no code form of the row GEMV takes -- the hook refuses it
# (test_op_positions_on_poisoned_caches asserts that), and 4 / 4 heads (K 512: three waves of each group own no chunk)
# is the smallest one-q-head-per-kv-head shape that runs
SHAPES = [(8, 2, 128, 256), (16, 4, 128, 256), (32, 8, 128, 256), (2, 2, 128, 256), (4, 4, 128, 256)]
FM_ERR_ARG = -1
QUANTS = [("int8", 128), ("int4", 128)]
CLASSES = ("linear", "attn", "slow_attn_wo", "slow_attn_wo_q")


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v[0], int) else f"{v[0]}g{v[1]}" if v[0] == "int4" else v[0]


def _run(c, w, res, quant, gs, **kw):
    from fishmi import ops

    return ops.slow_attn_wo_q(kw.pop("qkv", c["qkv"]), c["nh"], c["nkv"], c["hd"], kw.pop("slots", c["row_slot"]),
                              kw.pop("pos", c["pos"]), c["kc"], c["vc"], c["rope_base"], w, res, quant=quant, gs=gs,
                              qn=c["qn"], kn=c["kn"], layer=c["layer"], **kw)


def _same(a, b, msg=""):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(ar.bits(x), ar.bits(y), err_msg=msg)


def _tune_get(key):
    from fishmi import native

    return native.tune_get(key)


def _poisoned(shape, quant, gs, positions, knob):
    nh, nkv, hd, N = shape
    w, _, res = _operands(shape)
    waits = {k: _tune_get(k) for k in ("slow_aw_delay", "slow_aw_cheap")}
    for pos in positions:
        c = ar.make_case("diffuse", nh, nkv, hd, pos, S, "bf16", row_slot=[1], nslots=2, layers=2, layer=1)
        ref = _run(c, w, res, quant, gs, fused=False)
        assert ref[4] == 0 and all(np.isfinite(r).all() for r in ref[:3])
        gen = 1 + pos % 40
        for rp, bare in ((2, False), (4, False), (4, True)):
            knob("slow_aw_delay", 0 if bare else waits["slow_aw_delay"])
            knob("slow_aw_cheap", 0 if bare else waits["slow_aw_cheap"])
            f = _run(c, w, res, quant, gs, rp=rp, gens=gen, xt_init=_stale(nh * hd, pos, gen))
            assert f[3] and f[4] == 0, (pos, rp, bare, f[3], f[4])
            assert all(np.isfinite(r).all() for r in f[:3])
            _same(f, ref, f"pos {pos} rp {rp} bare {bare}")


@pytest.mark.parametrize("qg", QUANTS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_op_positions_on_poisoned_caches(shape, qg, knob):
    """One fused launch per position (slot 1 of 2, layer 1 of 2) on caches whose every word the kernels must not read
    is NaN, the tagged-word buffer pre-filled with NaN values under the generations one below and one above the
    current one: dispatchable, err == 0, finite, and the output row and the written K / V rows equal those of attn_fd +
    row GEMV on the same codes, with 2 and with 4 wo rows per group under the shipped wait knobs, and with 4 rows and
    no wait control (slow_aw_delay 0, slow_aw_cheap 0).  The first shape at every pass, tile and split edge; the others
    at 0, 255, 256 and 513.  K 256 (2 / 2 heads) is no whole 512-k chunk: both compositions are an argument error."""
    from fishmi.native import FishMIError

    knob("slow_attn_wo_q", 2)
    if shape[0] * shape[2] % 512:
        nh, nkv, hd, N = shape
        w, _, res = _operands(shape)
        c = ar.make_case("diffuse", nh, nkv, hd, 255, S, "bf16", row_slot=[1], nslots=2, layers=2, layer=1)
        for fused in (False, True):
            with pytest.raises(FishMIError) as e:
                _run(c, w, res, *qg, fused=fused)
            assert e.value.code == FM_ERR_ARG
        return
    _poisoned(shape, qg[0], qg[1], POSITIONS if shape == SHAPES[0] else (0, 255, 256, 513), knob)


def test_op_int4_group_32(knob):
    """Groups of 32 along K (four (scale, zero) words per lane's chunk row, lanes 0 .. 3 sharing one): the row GEMV takes
    any group size in whole 8-code words that divides K, and so does the fused form."""
    knob("slow_attn_wo_q", 2)
    _poisoned(SHAPES[0], "int4", 32, (0, 255, 256, 513), knob)


@pytest.mark.parametrize("qg", QUANTS, ids=_ids)
def test_op_sixteen_splits(qg, knob):
    """S 4096 (maxsplit 16: nh x 16 attention blocks ahead of the wo blocks): one split with 15 idle blocks per head,
    two splits, and all sixteen; rp 2 and 4.  The two launches' bits, err == 0."""
    knob("slow_attn_wo_q", 2)
    nh, nkv, hd, N = SHAPES[0]
    w, _, res = _operands(SHAPES[0])
    for pos in (3, 300, 4095):
        c = ar.make_case("diffuse", nh, nkv, hd, pos, 4096, "bf16")
        ref = _run(c, w, res, *qg, fused=False)
        assert ref[4] == 0 and np.isfinite(ref[0]).all()
        for rp in (2, 4):
            f = _run(c, w, res, *qg, rp=rp, gens=9, xt_init=_stale(nh * hd, pos, 9))
            assert f[3] and f[4] == 0, (pos, rp, f[4])
            _same(f, ref, f"pos {pos} rp {rp}")


@pytest.mark.parametrize("qg", QUANTS, ids=_ids)
def test_op_two_slots_at_one_position_and_a_following_layer(qg, knob):
    """Four launches in a row on one tagged-word buffer, as two frames of two layers leave them: slot 0 then slot 1 at
    the same position, launch indices 1, 2 each, every run with its own QKV row.  Each run equals its two-launch
    result, and the runs differ from one another."""
    knob("slow_attn_wo_q", 2)
    nh, nkv, hd, N = SHAPES[0]
    w, _, res = _operands(SHAPES[0])
    for pos in (129, 300):
        c = ar.make_case("diffuse", nh, nkv, hd, [pos, pos], S, "bf16", row_slot=[0, 1])
        qkv = np.stack([c["qkv"][0], -c["qkv"][0], c["qkv"][1], -c["qkv"][1]])
        kw = dict(qkv=qkv, slots=[0, 0, 1, 1], pos=[pos] * 4, gens=[1, 2, 1, 2], restore=True)
        ref = _run(c, w, res, *qg, fused=False, **kw)
        for rp in (2, 4):
            f = _run(c, w, res, *qg, rp=rp, **kw)
            assert f[3] and f[4] == 0
            _same(f, ref, f"pos {pos} rp {rp}")
        assert not np.array_equal(ref[0][0], ref[0][2]) and not np.array_equal(ref[0][0], ref[0][1])


@pytest.mark.parametrize("qg", QUANTS, ids=_ids)
def test_op_stream_decoded_twice(qg, knob):
    """64 consecutive positions across 256 on one slot and one tagged buffer (each run reads the rows the runs before
    it wrote, launch indices cycling as the layers of a frame do), decoded twice with the fused launch and once with
    the two launches: identical output rows and written K / V rows."""
    knob("slow_attn_wo_q", 2)
    nh, nkv, hd, N = SHAPES[0]
    w, _, res = _operands(SHAPES[0])
    n, p0 = 64, 224
    c = ar.make_case("diffuse", nh, nkv, hd, p0, S, "bf16")
    rng = np.random.default_rng(9)
    qkv = ar.rb("bf16")(rng.standard_normal((n, (nh + 2 * nkv) * hd))).astype(np.float32)
    kw = dict(qkv=qkv, slots=0, pos=np.arange(p0, p0 + n), gens=1 + np.arange(n) % 36, restore=False)
    a = _run(c, w, res, *qg, rp=4, **kw)
    b = _run(c, w, res, *qg, rp=4, **kw)
    ref = _run(c, w, res, *qg, fused=False, **kw)
    assert a[3] and a[4] == 0 and b[4] == 0 and np.isfinite(a[0]).all()
    _same(a, b)
    _same(a, ref)


def test_op_not_vacuous(knob):
    """The codes were really used: y differs from the bf16-weight launch on the same operands, and the codes and
    scales the hook returns are the row GEMV hook's (int8) and the int4 quantizer hook's for the same w."""
    from fishmi import ops

    knob("slow_attn_wo_q", 2)
    knob("slow_attn_wo", 2)
    nh, nkv, hd, N = SHAPES[0]
    K = nh * hd
    w, _, res = _operands(SHAPES[0])
    c = ar.make_case("diffuse", nh, nkv, hd, 300, S, "bf16")
    plain = ops.slow_attn_wo(c["qkv"], nh, nkv, hd, c["row_slot"], c["pos"], c["kc"], c["vc"], c["rope_base"], w, res,
                             qn=c["qn"], kn=c["kn"], layer=c["layer"], rp=4)
    assert plain[3] and plain[4] == 0
    f8 = _run(c, w, res, "int8", 128, rp=4)
    f4 = _run(c, w, res, "int4", 128, rp=4)
    for f in (f8, f4):
        assert f[3] and f[4] == 0
        assert not np.array_equal(ar.bits(f[0]), ar.bits(plain[0]))
        np.testing.assert_array_equal(ar.bits(f[1]), ar.bits(plain[1]))  # the attention half does not see the weights
    assert not np.array_equal(ar.bits(f8[0]), ar.bits(f4[0]))
    y = np.zeros(N, np.float32)
    q8, s8 = ops.rowgemv(w, np.zeros((1, K), np.float32), y, 0, q8=True, res=res)  # (0: the FIN form)
    np.testing.assert_array_equal(f8[5], q8)
    np.testing.assert_array_equal(ar.bits(f8[6]), ar.bits(s8))
    assert len(np.unique(f8[5])) > 64
    q4, sc, zr, _ = ops.quant4(w, 128)
    np.testing.assert_array_equal(f4[5].astype(np.uint8), q4)
    np.testing.assert_array_equal(ar.bits(f4[6]), ar.bits(sc))
    np.testing.assert_array_equal(ar.bits(f4[7]), ar.bits(zr))
    assert set(np.unique(q4)) == set(range(16))


@pytest.mark.parametrize("qg", QUANTS, ids=_ids)
def test_op_not_dispatchable_is_a_status(qg, knob):
    """Where the frame would keep its two launches the hook reports it and launches nothing: a wo depth without an
    instantiation (K = 48 x 128 = 6144: 3 chunks per wave), head_dim 64, gemv_chain 1; the unfused composition still
    runs.  A bias, and a group size the row GEMV refuses, are argument errors."""
    from fishmi.native import FishMIError

    knob("slow_attn_wo_q", 2)

    def ok(shape):
        nh, nkv, hd, N = shape
        w, _, res = _operands(shape)
        c = ar.make_case("diffuse", nh, nkv, hd, 40, 64, "bf16")
        f = _run(c, w, res, *qg)
        return f, _run(c, w, res, *qg, fused=False)

    f, un = ok(SHAPES[0])
    assert f[3] and f[4] == 0
    _same(f, un)
    for shape in ((48, 12, 128, 256), (16, 4, 64, 256)):
        f, un = ok(shape)
        assert not f[3] and f[4] == 0 and not f[0].any(), shape  # nothing launched: y as the binding zeroed it
        assert np.isfinite(un[0]).all() and un[0].any()
    knob("gemv_chain", 1)
    f, un = ok(SHAPES[0])
    assert not f[3] and not f[0].any() and np.isfinite(un[0]).all()
    knob("gemv_chain", 0)
    nh, nkv, hd, N = SHAPES[0]
    w, bias, res = _operands(SHAPES[0])
    c = ar.make_case("diffuse", nh, nkv, hd, 40, 64, "bf16")
    bad = [(qg[1], dict(bias=bias))]
    if qg[0] == "int4":
        bad += [(gs, {}) for gs in (12, 384)]  # no whole 8-code words; does not divide K 1024
    for gs, kw in bad:
        for fused in (False, True):
            with pytest.raises(FishMIError) as e:
                _run(c, w, res, qg[0], gs, fused=fused, **kw)
            assert e.value.code == FM_ERR_ARG


# ---- whole frames on a tiny model ---------------------------------------------------------------------------------


def _launches(m, slots=(0,)):
    """Launch counts per profiler class of one eager frame (the host checks chain_err after it)."""
    m.profile(True)
    try:
        before = {c: m.profile_read(c)[1] for c in CLASSES}
        m.decode(list(slots))
        return {c: m.profile_read(c)[1] - before[c] for c in CLASSES}
    finally:
        m.profile(False)


def _model(quant, slots=1, compact=False, precision="bf16", **cfg_kw):
    from fishmi.llm import DualARModel

    if quant == "int4":  # the int4 rule takes bias-free linears only: the same layout with its QKV and fast biases off
        cfg_kw.update(attention_qkv_bias=False, fast_attention_qkv_bias=False, fast_attention_o_bias=False)
    cfg = _tiny_cfg(False, **cfg_kw)
    kw = {} if quant is None else dict(quant=quant, groupsize=128, compact=compact)
    return cfg, DualARModel.synthetic(cfg, 11, 5, 0, precision, slots, **kw)


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_whole_frames_teacher_forced_and_sampled(quant, knob):
    """42 teacher-forced frames from a 250-row prompt (positions 250 .. 291: one split, then two and the combiner):
    slow logits, fast logits and emitted columns equal under slow_attn_wo_q 0, 1 and 2, the graph re-captured per
    setting; 8 frames run eagerly equal their graph replay; 40 sampled frames give the same columns; the launch counts
    of a frame move by the layer count: attn -L, linear -L, slow_attn_wo_q +L, and the class slow_attn_wo stays 0."""
    from fishmi.llm import DualARModel

    cfg, m = _model(quant)
    prompt, cols = _inputs(cfg, 3, 42)
    try:
        out, smp, n = {}, {}, {}
        for v in (0, 1, 2):
            knob("slow_attn_wo_q", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols)
            smp[v] = _sampled(m, 0, prompt, 40)
            m.prefill(0, prompt, DualARModel.sampling(top_k=1))
            n[v] = _launches(m)
        assert np.isfinite(out[0][1]).all()
        for v in (1, 2):
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo_q {v}")
            np.testing.assert_array_equal(smp[0], smp[v])
            assert n[0]["attn"] - n[v]["attn"] == NL and n[0]["linear"] - n[v]["linear"] == NL, n
            assert n[0]["slow_attn_wo_q"] == 0 and n[v]["slow_attn_wo_q"] == NL, n
        assert all(n[v]["slow_attn_wo"] == 0 for v in (0, 1, 2)), n
        assert len(np.unique(smp[1][:, 1:])) > 8  # a sampled stream, not one repeated code
        for v in (1, 2):
            knob("slow_attn_wo_q", v)
            res = {}
            for graph in (False, True):
                m.use_graph(graph)
                res[graph] = _forced(m, prompt, cols[:, :8])
            for a, b in zip(res[False], res[True]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo_q {v}")
    finally:
        m.use_graph(True)
        m.close()


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_compact_handles(quant, knob):
    """A compact handle keeps the row GEMV's row-major codes, so the launch engages there too: the same bits under
    slow_attn_wo_q 0 and 2, and L launches of the new class."""
    from fishmi.llm import DualARModel

    cfg, m = _model(quant, compact=True)
    prompt, cols = _inputs(cfg, 3, 12)
    try:
        out, smp, n = {}, {}, {}
        for v in (0, 2):
            knob("slow_attn_wo_q", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols)
            smp[v] = _sampled(m, 0, prompt, 12)
            m.prefill(0, prompt, DualARModel.sampling(top_k=1))
            n[v] = _launches(m)
        for a, b in zip(out[0], out[2]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(smp[0], smp[2])
        assert n[0]["slow_attn_wo_q"] == 0 and n[2]["slow_attn_wo_q"] == NL and n[2]["slow_attn_wo"] == 0, n
        assert n[0]["attn"] - n[2]["attn"] == NL and n[0]["linear"] - n[2]["linear"] == NL, n
    finally:
        m.close()


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_three_slots_one_at_a_time(quant, knob):
    """A handle with 3 slots decoded one slot at a time in permuted slot order, the slots at equal and at different
    positions (the tagged words are one buffer for all of them): the streams agree under slow_attn_wo_q 0, 1 and 2."""
    from fishmi.llm import DualARModel

    cfg, m = _model(quant, slots=3)
    prompts = [_inputs(cfg, 5 + s, 1, T=(250, 250, 120)[s])[0] for s in range(3)]
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=77, mask_im_end=True)
    order = [(2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0)]
    try:
        single = {}
        for v in (0, 1, 2):
            knob("slow_attn_wo_q", v)
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


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_frames_on_a_cache_of_sixteen_splits(quant, knob):
    """max_seq_len 5120 (maxsplit 16: 8 x 16 attention blocks per fused launch, all but 8 or 16 of them idle): 12
    teacher-forced frames across position 256 and 12 sampled ones equal under slow_attn_wo_q 0, 1 and 2."""
    cfg, m = _model(quant, max_seq_len=5120)
    prompt, cols = _inputs(cfg, 3, 12)
    try:
        out, smp = {}, {}
        for v in (0, 1, 2):
            knob("slow_attn_wo_q", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols)
            smp[v] = _sampled(m, 0, prompt, 12)
        for v in (1, 2):
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"slow_attn_wo_q {v}")
            np.testing.assert_array_equal(smp[0], smp[v])
    finally:
        m.close()


def _sweep(m, cfg, key, knob, slots=(0,)):
    """Frames and one eager frame's launch counts under key 0, 1 and 2"""
    from fishmi.llm import DualARModel

    prompt, cols = _inputs(cfg, 3, 10)
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=5, mask_im_end=True)
    out, n = {}, {}
    for v in (0, 1, 2):
        knob(key, v)
        m.use_graph(True)
        if len(slots) > 1:
            for s in slots:
                m.prefill(s, prompt, sp)
            out[v] = (m.decode_frames(list(slots), 10),)
        else:
            out[v] = _forced(m, prompt, cols)
            m.prefill(0, prompt, DualARModel.sampling(top_k=1))
        n[v] = _launches(m, slots)
    for v in (1, 2):
        for a, b in zip(out[0], out[v]):
            np.testing.assert_array_equal(a, b, err_msg=f"{key} {v}")
    return n


def test_the_new_knob_is_inert_on_an_unquantised_handle(knob):
    """A bf16 unquantised handle runs the same launches -- slow_attn_wo's, none of the new class -- and gives the same
    bits under slow_attn_wo_q 0, 1 and 2."""
    knob("slow_attn_wo", 2)
    cfg, m = _model(None)
    try:
        n = _sweep(m, cfg, "slow_attn_wo_q", knob)
        assert n[0] == n[1] == n[2] and n[0]["slow_attn_wo_q"] == 0 and n[0]["slow_attn_wo"] == NL, n
    finally:
        m.close()


def test_the_old_knob_is_inert_on_an_int4_handle(knob):
    """An int4 handle is unmoved by slow_attn_wo 0, 1 and 2 (the int8 half: test_gpu_slow_attn_wo.py), with the new
    knob engaged: the same launches, L of them in the new class, none in the old one."""
    knob("slow_attn_wo_q", 2)
    cfg, m = _model("int4")
    try:
        n = _sweep(m, cfg, "slow_attn_wo", knob)
        assert n[0] == n[1] == n[2] and n[0]["slow_attn_wo"] == 0 and n[0]["slow_attn_wo_q"] == NL, n
    finally:
        m.close()


@pytest.mark.parametrize("quant", ["int8", "int4"])
@pytest.mark.parametrize("setting", [("fd_hpb", 2), ("fd_nw", 4), ("gemv_chain", 1), ("n2", 0), ("row_off", 0)])
def test_fallbacks_leave_the_frame_alone(setting, quant, knob):
    """Where a precondition fails -- fd_hpb 2, fd_nw 4, gemv_chain 1, two rows per frame, wo off the row-block GEMV
    (rowgemv / rowgemv_q4 bit 0 clear) -- the new knob changes nothing: today's launches, none in the new class, and
    the same bits."""
    key, val = setting
    cfg, m = _model(quant, slots=2 if key == "n2" else 1)
    try:
        if key == "row_off":
            rk = "rowgemv_q4" if quant == "int4" else "rowgemv"
            knob(rk, _tune_get(rk) & ~1)
        elif key != "n2":
            knob(key, val)
        n = _sweep(m, cfg, "slow_attn_wo_q", knob, slots=(0, 1) if key == "n2" else (0,))
        assert n[0] == n[1] == n[2] and n[1]["slow_attn_wo_q"] == 0 and n[1]["slow_attn_wo"] == 0, n
    finally:
        m.close()
