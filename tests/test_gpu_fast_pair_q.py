"""fm_tune fast_pair_q: on a weight-only handle a batch-1 frame runs the fast decoder's
codebook positions 0 and 1 as one two-row pass on the codes, as fast_pair does on unquantised bf16: bit 0 on int8
handles, bit 1 on int4 handles (group 128).  Whole frames run both modes; the per-op cases run every two-row code form:
the row FIN form on int8 and int4 codes, NORM_STORE and NORM_SWIGLU on int4 codes, the tile kernel's two-row prologue
on int8 codes (store and SwiGLU8), the fused attention + wo pair form on both.  The change claims bit identity, so
every comparison is array_equal; one case per quant mode and kernel family holds the two-row outputs to the float64
bound of the one-row kernel; S2-Pro widths with two fast layers run the pair against the one-row pass (int8, int4) and
the dequantised-weight model (int4); the reference's int8 golden has one fast layer, where the knob must be inert.
Run on the MI355X box: pytest -m gpu."""
import dataclasses
import os

import numpy as np
import pytest

import attn_ref as ar
import linear_ref as lr
from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced, _inputs
from test_gpu_fast_pair import _pair_cfg

pytestmark = pytest.mark.gpu

GS = 128
SENT = 320.0  # output sentinel (a bf16 value no test output takes: the operands are O(1))
CLASSES = ("linear", "attn")
BIT = {"int8": 1, "int4": 2}  # the mode's bit
QUANTS = ["int8", "int4"]


def _model(variant, quant="int4", seed=11, max_slots=1, compact=False):
    from fishmi.llm import DualARModel

    cfg = _pair_cfg(variant)
    kw = {} if quant is None else dict(quant=quant, groupsize=GS, compact=compact)
    return cfg, DualARModel.synthetic(cfg, seed, 5, 0, "bf16", max_slots, **kw)


def _profile(m, slots=(0,)):
    """(launches, bytes) per profiler class of one eager decode frame (the host checks chain_err after it)."""
    m.profile(True)
    try:
        before = {c: m.profile_read(c)[1:] for c in CLASSES}
        m.decode(list(slots))
        after = {c: m.profile_read(c)[1:] for c in CLASSES}
    finally:
        m.profile(False)
    return {c: (after[c][0] - before[c][0], after[c][1] - before[c][1]) for c in CLASSES}


def _sampling(seed=1234):
    from fishmi.llm import DualARModel

    return DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=seed, mask_im_end=True)


def _equal(a, b, msg=""):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=msg)


# ---- whole frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("variant", ["b", "c", "d"])
def test_whole_frame_identity_teacher_forced(variant, quant, knob):
    """Slow logits, fast logits and emitted columns of 7 teacher-forced frames (gathered codes 0 and cb - 1 among
    them) under fast_pair_q 0 and on, the graph re-captured per setting; one frame eager equals its graph replay;
    once more with fattn_ilp 0 and once with fast_dead_q 3.  The knob-on frame really is the paired pass: its
    launch count differs from the knob-off frame's."""
    ON = BIT[quant]
    cfg, m = _model(variant, quant)
    prompt, cols = _inputs(cfg, 3)
    assert 0 in cols[1] and cfg.codebook_size - 1 in cols[1]
    try:
        for key, val, nf in ((None, None, 7), ("fattn_ilp", 0, 3), ("fast_dead_q", 3, 3)):
            if key:
                knob(key, val)
            out = {}
            for v in (0, ON):
                knob("fast_pair_q", v)
                m.use_graph(True)
                out[v] = _forced(m, prompt, cols[:, :nf])
            assert np.isfinite(out[0][1]).all()
            _equal(out[0], out[ON], f"{key} {val}")
            if key:
                knob(key, 1)
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            res[graph] = _forced(m, prompt, cols[:, :2])
        _equal(res[False], res[True])
        n = {}
        for v in (0, ON):
            knob("fast_pair_q", v)
            m.prefill(0, prompt, _sampling())
            n[v] = _profile(m)
        assert n[0]["linear"][0] > n[ON]["linear"][0], n
    finally:
        m.use_graph(True)
        m.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_compact_handle_identity(quant, knob):
    """A compact handle (codes only) engages as well: the same bits under 0 and on, fewer launches under on."""
    ON = BIT[quant]
    cfg, m = _model("b", quant, compact=True)
    prompt, cols = _inputs(cfg, 3)
    try:
        out, n = {}, {}
        for v in (0, ON):
            knob("fast_pair_q", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols[:, :4])
            m.prefill(0, prompt, _sampling())
            n[v] = _profile(m)
        _equal(out[0], out[ON])
        assert n[0]["linear"][0] - n[ON]["linear"][0] == 3 * (cfg.n_fast_layer - 1), n
    finally:
        m.close()


@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("variant", ["b", "c"])
def test_sampled_streams_identical(variant, quant, knob):
    """32 sampled frames (top_k 30, top_p 0.8, temperature 0.8, fixed seed) without host syncs: the same columns
    under fast_pair_q 0 and on."""
    ON = BIT[quant]
    cfg, m = _model(variant, quant, seed=13)
    prompt, _ = _inputs(cfg, 5)
    try:
        out = {}
        for v in (0, ON):
            knob("fast_pair_q", v)
            m.use_graph(True)
            first = m.prefill(0, prompt, _sampling())
            out[v] = np.concatenate([first[None], m.decode_frames([0], 32)[:, 0]])
        np.testing.assert_array_equal(out[0], out[ON])
        assert len(np.unique(out[ON][:, 1:])) > 8  # a sampled stream, not one repeated code
    finally:
        m.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_three_slots_one_at_a_time_and_batched(quant, knob):
    """A 3-slot handle decoded one slot at a time in permuted slot order gives identical streams under 0 and on;
    decoded together (n = 3, where the pair is inert) the bits and the launch counts are unchanged."""
    ON = BIT[quant]
    cfg, m = _model("b", quant, seed=13, max_slots=3)
    prompts = [_inputs(cfg, 5 + s)[0] for s in range(3)]
    order = [(2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0)]
    try:
        single, batched, prof = {}, {}, {}
        for v in (0, ON):
            knob("fast_pair_q", v)
            m.use_graph(True)
            got = {s: [m.prefill(s, prompts[s], _sampling(77))] for s in range(3)}
            for k in range(8):
                for s in order[k % len(order)]:
                    got[s].append(m.decode([s])[0])
            single[v] = np.stack([np.stack(got[s]) for s in range(3)])
            for s in range(3):
                m.prefill(s, prompts[s], _sampling(77))
            batched[v] = m.decode_frames([0, 1, 2], 6)
            prof[v] = _profile(m, (0, 1, 2))
        np.testing.assert_array_equal(single[0], single[ON])
        np.testing.assert_array_equal(batched[0], batched[ON])
        assert prof[0] == prof[ON], prof
        assert len(np.unique(single[ON][:, :, 1:])) > 8
    finally:
        m.close()


@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("variant", ["b", "c"])
def test_the_launches_went_away(variant, quant, knob):
    """profile_read over one eager frame: from fast_pair_q 0 to on the "linear" class drops by exactly 3 (n - 1)
    launches (w1 || w3 and w2 of fast layers 0 .. n - 2, the K / V-only wqkv of layers 1 .. n - 1) and the "attn" class
    by exactly n (codebook 0's n - 1 fused launches and its last layer's K / V-only attention); the "linear" bytes
    drop; the frames ran without a hand-off timeout (the host checks chain_err after each)."""
    ON = BIT[quant]
    cfg, m = _model(variant, quant)
    nl = cfg.n_fast_layer
    prompt, _ = _inputs(cfg, 3)
    try:
        n = {}
        for v in (0, ON):
            knob("fast_pair_q", v)
            m.prefill(0, prompt, _sampling())
            n[v] = _profile(m)
        print("per frame (launches, bytes)", n)
        assert n[0]["linear"][0] - n[ON]["linear"][0] == 3 * (nl - 1), n
        assert n[0]["attn"][0] - n[ON]["attn"][0] == nl, n
        assert n[ON]["linear"][1] < n[0]["linear"][1], n
    finally:
        m.close()


INERT = ["fast_dead_q-0", "int8:fast_dead_q-0", "a-int8", "fattn_wo-0", "int8:fattn_wo-0", "fast_tail-0",
         "int8:fast_tail-0", "int4_stream-0", "rowgemv_q4-15", "int8:rowgemv-127", "int8:q_u-16", "bf16", "bit0-on-int4",
         "bit1-on-int8"]


@pytest.mark.parametrize("case", INERT)
def test_inert_where_it_must_be(case, knob):
    """Where a precondition fails the knob changes neither the bits nor the profiler's (launches, bytes): without
    the QKV table (fast_dead_q 0); the o-bias layout (a) with int8 (an int4 handle cannot be opened on it: its quantiser refuses biased linears);
    without the fused launch (fattn_wo 0); without fast_tail; an int4 handle on its dequantised weights (int4_stream 0) or with the first layer's wqkv off
    the row form (rowgemv_q4 15); an int8 handle with w1 || w3 on the row form (rowgemv 127) or 16 units in flight
    (q_u 16: no two-row SwiGLU8 form); an unquantised bf16 handle; bit 0 alone on an int4 handle and bit 1 alone on an
    int8 one.  (Cases prefixed int8: run an int8 handle, the others int4 unless named.)"""
    quant = {"a-int8": "int8", "bf16": None, "bit1-on-int8": "int8"}.get(case, "int8" if case.startswith("int8:") else "int4")
    on = {"bit0-on-int4": 1, "bit1-on-int8": 2, "a-int8": 3, "bf16": 3}.get(case, 3)
    setting = case.split(":")[-1]
    if "-" in setting and setting.rsplit("-", 1)[1].isdigit():
        key, val = setting.rsplit("-", 1)
        knob(key, int(val))
    cfg, m = _model("a" if case.startswith("a-") else "b", quant=quant)
    prompt, cols = _inputs(cfg, 3)
    try:
        bits, prof = {}, {}
        for v in (0, on):
            knob("fast_pair_q", v)
            m.use_graph(True)
            bits[v] = _forced(m, prompt, cols[:, :4])
            prof[v] = _profile(m)
        print(case, prof)
        _equal(bits[0], bits[on])
        assert prof[0]["linear"][0] > 0 and prof[0] == prof[on], prof
    finally:
        m.use_graph(True)
        m.close()


# ---- per op: each two-row code form against the one-row production launcher, row by row ---------------------------

def _operands(seed, N, K):
    rng = np.random.default_rng(seed)
    w = lr.mk(rng, (N, K), "bf16", K ** -0.5)
    x = lr.mk(rng, (2, K), "bf16")
    return rng, w, x


FIN_CASES = [("int8", 128, 512, True), ("int8", 128, 2560, True), ("int8", 128, 9728, False),
             ("int4", 128, 512, True), ("int4", 32, 512, True), ("int4", 128, 2560, True), ("int4", 128, 9728, False)]


@pytest.mark.parametrize("quant,gs,K,gather", FIN_CASES)
def test_op_two_row_fin(quant, gs, K, gather):
    """wo / w2 form (2 rows per block, N = 4: two blocks) on int8 and int4 codes at one chunk (three idle waves), five
    chunks (uneven shares, a tail slot) and the deep form (19 chunks): both rows equal the one-row launcher's, row 1's
    residual plain or gathered from a table (one index past its end: the clamp); the padding stays at the sentinel."""
    from fishmi import ops

    N, ld = 4, 12
    rng, w, x = _operands(K + gs, N, K)
    res0 = lr.mk(rng, (N,), "bf16")
    tab = lr.mk(rng, (5, N), "bf16")
    for idx in ([3, 1], [3, 9], None) if gather else (None,):
        res1 = tab if idx is not None else tab[:1]
        y2, y1 = np.full((2, ld), SENT, np.float32), np.full((2, ld), SENT, np.float32)
        ops.rowgemv_pair_q(w, x, y2, y1, 0, quant, gs=gs, res0=res0, res1=res1, idx=idx, idx_col=1 if idx is not None else 0)
        np.testing.assert_array_equal(ar.bits(y2), ar.bits(y1))
        assert (y2[:, N:] == SENT).all() and not (y2[:, :N] == SENT).any()
        if quant == "int8" and idx is None:  # the one-row launcher of the hook is the production one: ops.rowgemv's
            for r, res in ((0, res0[None]), (1, res1)):
                y = np.full(ld, SENT, np.float32)
                ops.rowgemv(w, x[r:r + 1], y, 0, q8=True, res=res)
                np.testing.assert_array_equal(ar.bits(y2[r]), ar.bits(y))


@pytest.mark.parametrize("K", [512, 2560])
@pytest.mark.parametrize("N,skip0", [(16, 8), (40, 20), (16, 0)])  # N = 2 RP | a count inside a block | none skipped
def test_op_two_row_norm_store(K, N, skip0):
    """wqkv form on int4 codes (RMSNorm prologue, 8 rows per block), x[1] = 3 x so that the two statistics differ:
    row 1 equals the one-row launcher's output everywhere, row 0 from skip0 on; row 0's outputs below skip0 and the
    padding stay at the sentinel."""
    from fishmi import ops

    ld = N + 8
    rng, w, x = _operands(K + N, N, K)
    x[1] = lr.rb("bf16")(x[1] * 3.0)
    nw = lr.rb("bf16")(1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2, y1 = np.full((2, ld), SENT, np.float32), np.full((2, ld), SENT, np.float32)
    ops.rowgemv_pair_q(w, x, y2, y1, 1, "int4", gs=GS, nw=nw, eps=1e-5, skip0=skip0)
    assert not (y1[:, :N] == SENT).any() and (y1[:, N:] == SENT).all()
    for r in range(2):
        lo = skip0 if r == 0 else 0
        np.testing.assert_array_equal(ar.bits(y2[r, lo:]), ar.bits(y1[r, lo:]))
        assert (y2[r, :lo] == SENT).all() and not (y2[r, lo:N] == SENT).any()
    assert not np.array_equal(y2[0, skip0:N], y2[1, skip0:N])


@pytest.mark.parametrize("K", [512, 2560])
def test_op_two_row_norm_swiglu(K):
    """w1 || w3 form on int4 codes (4 + 4 interleaved rows per block, N = 16: two blocks): each row equals the one-row
    launcher's; the padding stays at the sentinel."""
    from fishmi import ops

    N, ld = 16, 8 + 5
    rng, w, x = _operands(K + 1, N, K)
    x[1] = lr.rb("bf16")(x[1] * 0.25)
    nw = lr.rb("bf16")(1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2, y1 = np.full((2, ld), SENT, np.float32), np.full((2, ld), SENT, np.float32)
    ops.rowgemv_pair_q(w, x, y2, y1, 2, "int4", gs=GS, nw=nw, eps=1e-5)
    np.testing.assert_array_equal(ar.bits(y2), ar.bits(y1))
    assert (y2[:, N // 2:] == SENT).all() and not (y2[:, :N // 2] == SENT).any()
    assert not np.array_equal(y2[0, :N // 2], y2[1, :N // 2])


@pytest.mark.parametrize("K", [512, 2560])
@pytest.mark.parametrize("epi", ["store", "swiglu8"])
def test_op_two_row_tile_int8(epi, K):
    """The 16-row tile kernel on int8 codes with the statistic from the staged rows (ss_gran 1) at R = 2, wqkv's store
    epilogue and w1 || w3's SwiGLU8 (N = 32: two tiles): each row equals the R = 1 production launch of that row on the
    same device operands; the spare row and the padding columns stay at the sentinel."""
    from fishmi import ops

    N = 32
    No = N // 2 if epi == "swiglu8" else N
    rng, w, x = _operands(K + 7, N, K)
    x[1] = lr.rb("bf16")(x[1] * 0.25)
    nw = lr.rb("bf16")(1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2, y1 = np.full((3, No + 8), SENT, np.float32), np.full((2, No + 8), SENT, np.float32)
    ops.gemv_pair_q(w, x, y2, y1, ops.EPI_SWIGLU8 if epi == "swiglu8" else ops.EPI_STORE, nw, eps=1e-5)
    np.testing.assert_array_equal(ar.bits(y2[:2]), ar.bits(y1))
    assert (y2[2] == SENT).all() and (y2[:, No:] == SENT).all() and not (y2[:2, :No] == SENT).any()
    assert not np.array_equal(y2[0, :No], y2[1, :No])


@pytest.mark.parametrize("K", [512, 2560])
def test_two_row_int8_tile_within_float64_bound(K):
    """int8 tile family at two rows (store epilogue) against tests/linear_ref.py: the RMSNorm prologue's centre and
    band, the fp32 accumulation over the device's codes, round(round(acc) * scale); every element inside its bound."""
    from fishmi import ops

    N = 32
    rng, w, x = _operands(11 * K, N, K)
    x[1] = lr.rb("bf16")(x[1] * 3.0)
    nw = lr.rb("bf16")(1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2, y1 = np.full((2, N), SENT, np.float32), np.full((2, N), SENT, np.float32)
    q, sc = ops.gemv_pair_q(w, x, y2, y1, ops.EPI_STORE, nw, eps=1e-5)
    c, dx = lr.norm_ref(x, nw, 1e-5, "bf16")
    v = lr.v_q8(lr.v_acc(c, q.astype(np.float64), dx=dx), sc.astype(np.float64)[None, :], "bf16")
    err = np.abs(y2.astype(np.float64) - v.t)
    print(f"int8 two-row tile store K={K}: max |got - t| / e {float((err / (v.e + 1e-300)).max()):.3g}")
    assert (err <= v.e).all()


def test_int8_real_widths_vs_reference_with_the_knob_on(golden, knob):
    """S2-Pro widths at reduced depth (test_gpu_int8's wide model, llm_wide_int8) against the reference int8 model's
    logits through test_int8_wide_real_widths_vs_reference's path, with fast_pair_q 3: within the bf16 bound.  The
    golden model has ONE fast layer, and the pair needs two (the tag argument), so the knob is inert here: the case
    only shows that switching it on leaves the reference-pinned path as it was.  The paired int8 pass at these widths
    is held to the one-row pass, bit for bit, by test_int8_real_widths_pair_engaged below."""
    from test_gpu_int8 import _int8_wide

    knob("fast_pair_q", 3)
    _int8_wide(golden)


def _wide2(golden, quant):
    """llm_wide's widths (S2-Pro: dim 2560, inter 9728, heads x 128) with a second fast layer, so that the pair engages"""
    from conftest import GOLDEN
    from fishmi.config import DualARConfig
    from fishmi.llm import DualARModel

    g = golden("llm_wide_bf16.npz")
    base = DualARConfig.from_pretrained(os.path.join(GOLDEN, "llm_wide"))
    cfg = dataclasses.replace(base, n_fast_layer=2)
    cfg.im_end_id = 4
    T = g["prompt"].shape[1]
    m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", 1, quant=quant, groupsize=GS)
    return g, g["seq"][:, T:T + 5], m


def test_int8_real_widths_pair_engaged(golden, knob):
    """S2-Pro widths with two fast layers on int8 codes (fast dim 2560: five chunks, uneven shares; w2 at K = 9728:
    the deep FIN form; the tile pair at K = 2560): teacher-forced slow and fast logits under fast_pair_q 1 equal those
    under 0 bit for bit, and the pair engaged -- the frame drops exactly 3 "linear" and 2 "attn" launches."""
    g, cols, m = _wide2(golden, "int8")
    try:
        out, n = {}, {}
        for v in (0, 1):
            knob("fast_pair_q", v)
            m.use_graph(True)
            out[v] = m.teacher_decode(g["prompt"], cols)
            n[v] = _profile(m)
        assert n[0]["linear"][0] - n[1]["linear"][0] == 3 and n[0]["attn"][0] - n[1]["attn"][0] == 2, n
        assert np.isfinite(out[1][1]).all()
        _equal(out[0], out[1])
    finally:
        m.close()


@pytest.mark.parametrize("quant", [1, 2])
def test_op_fused_pair_forms(quant):
    """The fused attention + wo pair launch on int8 / int4 wo at test_gpu_attn_ops.test_fattn_wo_pair_forms's smallest
    dispatching shape (4 / 2 heads x 128, K = 512): pair 1, pair 2 and the table form against the two one-row launches
    they replace (the K / V-only form at 0, then the plain or gathered form at 1 on the cache the first left) and against
    the unfused composition; row 0's Q part is NaN; the tagged words pre-filled with stale neighbours' tags; status
    {depth > 0, err 0}."""
    from fishmi import ops

    shape = (4, 2, 128)
    nh, nkv, hd = shape
    K, ld, N = nh * hd, (nh + 2 * nkv) * hd, 64
    rng = np.random.default_rng([13, quant])
    w, res = lr.mk(rng, (N, K), "bf16", K ** -0.5), lr.mk(rng, (5, N), "bf16")
    gen, pos0 = 3, 5
    stale = ((rng.integers(0, 1 << 16, 2 * K).astype(np.uint32) << 16) | np.uint32((pos0 * 41 + gen - 1) % 65535 + 1)).astype(np.uint32)

    def fw(c, res, **kw):
        return ops.fattn_wo(kw.pop("qkv"), nh, nkv, hd, int(c["row_slot"][0]), int(c["pos"][0]), kw.pop("kc", c["kc"]),
                            kw.pop("vc", c["vc"]), c["rope_base"], w, res, qn=c["qn"], kn=c["kn"], layer=c["layer"],
                            quant=quant, gs=GS, pos0=pos0, **kw)

    for c in ar.fast_cases(shape, "bf16", 0, 16)[:3]:
        row1 = ar.rb("bf16")(rng.standard_normal((1, ld))).astype(np.float32)
        row0 = c["qkv"].copy()
        row0[:, :K] = np.nan
        res0 = res[4]
        a = fw(c, res0[None, :], qkv=row0, kv0=True, gen=1)
        c1 = dict(c, pos=np.array([1], np.int32))
        b = fw(c1, res, qkv=row1, kc=a[1], vc=a[2], gen=gen)
        bu = fw(c1, res, qkv=row1, kc=a[1], vc=a[2], gen=gen, fused=False)
        assert a[3] and b[3] and a[4] == 0 and b[4] == 0
        np.testing.assert_array_equal(ar.bits(b[0]), ar.bits(bu[0]))
        both = np.concatenate([row0, row1])
        p1 = fw(c1, res, qkv=both, pair=1, res0=res0, gen=gen, xt_init=stale)
        assert p1[3] and p1[4] == 0
        assert ops.fattn_wo.last_depth == 2  # K = 512: one chunk of 512 k, the depth-2 form (rowgemv_u)
        np.testing.assert_array_equal(ar.bits(p1[0]), ar.bits(np.stack([a[0], b[0]])))
        np.testing.assert_array_equal(ar.bits(p1[1]), ar.bits(b[1]))
        np.testing.assert_array_equal(ar.bits(p1[2]), ar.bits(b[2]))
        p2 = fw(c1, res, qkv=both, pair=2, gen=gen, xt_init=stale)
        assert p2[3] and p2[4] == 0
        for u, v in zip(p2[:3], b[:3]):
            np.testing.assert_array_equal(ar.bits(u), ar.bits(v))
        qtab = ar.rb("bf16")(rng.standard_normal((5, ld))).astype(np.float32)
        qtab[2] = row1[0]
        ix = np.array([2], np.int32)
        bt = fw(c1, res, qkv=row1, kc=a[1], vc=a[2], idx=ix, gen=gen)
        pt = fw(c1, res, qkv=np.concatenate([row0, np.full((1, ld), np.nan, np.float32)]), qtab=qtab, idx=ix, pair=1,
                res0=res0, gen=gen, xt_init=stale)
        assert pt[3] and pt[4] == 0
        np.testing.assert_array_equal(ar.bits(pt[0]), ar.bits(np.stack([a[0], bt[0]])))
        np.testing.assert_array_equal(ar.bits(pt[1]), ar.bits(bt[1]))
        np.testing.assert_array_equal(ar.bits(pt[2]), ar.bits(bt[2]))


def test_fused_pair_depth_not_instantiated_is_a_status():
    """A depth outside the resident forms (int8: K = 4608, 9 chunks, depth 3) is reported, not launched."""
    from fishmi import ops

    nh, nkv, hd = 36, 9, 128
    K, ld, N = nh * hd, (nh + 2 * nkv) * hd, 16
    c = ar.fast_cases((4, 2, 128), "bf16", 0, 16)[0]
    kc = np.zeros((1, 1, nkv, 16, hd), np.float32)
    y = ops.fattn_wo(np.zeros((2, ld), np.float32), nh, nkv, hd, 0, 1, kc, kc.copy(), c["rope_base"], np.zeros((N, K), np.float32),
                     np.zeros((1, N), np.float32), quant=1, pair=2, gen=3)
    assert y[3] is False and y[4] == 0


# ---- not only self-consistency: the two-row outputs inside the one-row kernel's float64 bound -------------------

@pytest.mark.parametrize("K", [512, 2560])
def test_two_row_int8_fin_within_float64_bound(K):
    """int8 row FIN at two rows against tests/linear_ref.py, as test_gpu_linear_ops holds the one-row int8 row GEMV:
    the kernel's own sum (q + 128) . x - 128 sum(x) on the device's codes and scales, round(round(acc) * scale),
    then round(res + round(.)), every element inside its bound."""
    from fishmi import ops

    N, ld = 8, 8
    rng, w, x = _operands(7 * K, N, K)
    res = lr.mk(rng, (2, N), "bf16")
    y2, y1 = np.full((2, ld), SENT, np.float32), np.full((2, ld), SENT, np.float32)
    q, sc, _ = ops.rowgemv_pair_q(w, x, y2, y1, 0, "int8", res0=res[0], res1=res[1:])
    q64 = q.astype(np.float64)
    a = lr.v_acc(x.astype(np.float64), q64, extra=lambda ax: ax @ np.abs(q64 + 128).T + 128 * ax.sum(-1, keepdims=True))
    a = lr.v_q8(a, sc.astype(np.float64)[None, :], "bf16")
    v = lr.v_rnd(lr.v_add(lr.v_rnd(a, "bf16"), res.astype(np.float64)), "bf16")
    err = np.abs(y2.astype(np.float64) - v.t)
    print(f"int8 two-row fin K={K}: max |got - t| / e {float((err / (v.e + 1e-300)).max()):.3g}")
    assert (err <= v.e).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_two_row_int4_within_streamed_bound(kind):
    """int4 row FIN (K = 2560) and NORM_STORE at two rows against float64 on the exactly dequantised weights
    ((q - 8) s + z from the device's codes and (scale, zero) words), DESIGN section 1's streamed-GEMV bound
    2e-6 max|y| sqrt(K) plus the one bf16 rounding of each stored value (FIN: two, of the product and of the sum;
    NORM_STORE: plus the RMSNorm prologue's band on x', linear_ref.norm_ref)."""
    from fishmi import ops

    N, K, ld = 16, 2560, 16
    rng, w, x = _operands(99 + kind, N, K)
    res = lr.mk(rng, (2, N), "bf16")
    nw = lr.rb("bf16")(1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2, y1 = np.full((2, ld), SENT, np.float32), np.full((2, ld), SENT, np.float32)
    if kind == 0:
        q, sc, zr = ops.rowgemv_pair_q(w, x, y2, y1, 0, "int4", gs=GS, res0=res[0], res1=res[1:])
        xin = x.astype(np.float64)
    else:
        q, sc, zr = ops.rowgemv_pair_q(w, x, y2, y1, 1, "int4", gs=GS, nw=nw, eps=1e-5)
        xin, dx = lr.norm_ref(x, nw, 1e-5, "bf16")
    wx = ((q.astype(np.float64) - 8).reshape(N, K // GS, GS) * sc[..., None] + zr[..., None]).reshape(N, K)
    y = xin @ wx.T
    tol = 2e-6 * np.abs(y).max() * np.sqrt(K) + np.abs(y) * 2.0 ** -8
    if kind == 1:  # the prologue's documented band on the statistic (linear_ref.norm_ref), as test_gpu_linear_ops carries it
        tol = tol + dx @ np.abs(wx).T
    if kind == 0:
        y = y + res
        tol = tol + np.abs(y) * 2.0 ** -8
    err = np.abs(y2.astype(np.float64) - y)
    print(f"int4 two-row kind {kind}: max err / tol {float((err / tol).max()):.3g}")
    assert (err <= tol).all()


def test_int4_real_widths_vs_dequantised_model(golden, knob):
    """S2-Pro widths (llm_wide with a second fast layer, so that the pair engages; group 128) with the knob on: the
    streamed int4 model against the same model on its dequantised bf16 weights (int4_stream 0, where the pair is
    inert), at test_gpu_int4's tolerance; and the knob-on logits equal the knob-off ones bit for bit."""
    g, cols, m = _wide2(golden, "int4")
    try:
        out, n = {}, {}
        for name, stream, v in (("off", 1, 0), ("on", 1, 2), ("deq", 0, 2)):
            knob("int4_stream", stream)
            knob("fast_pair_q", v)
            m.use_graph(True)
            out[name] = m.teacher_decode(g["prompt"], cols)
            n[name] = _profile(m)
        assert n["off"]["linear"][0] - n["on"]["linear"][0] == 3, n  # the pair engaged at these widths
        _equal(out["off"], out["on"])
        rows = g["slow_rows"]
        for k in (0, 1):
            a, b = out["on"][k], out["deq"][k]
            if k == 0:
                a, b = a[:, rows], b[:, rows]
            fin = np.isfinite(b)
            rel = np.sqrt(np.mean((a[fin] - b[fin]) ** 2)) / np.sqrt(np.mean(b[fin] ** 2))
            assert rel < 2e-2, (k, rel)
            assert np.array_equal(np.isfinite(a), fin)
    finally:
        m.close()
