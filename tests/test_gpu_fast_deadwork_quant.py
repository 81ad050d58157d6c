"""fm_tune fast_dead_q: weight-only int8 / int4 handles get the fast decoder's two
removals that rowgemv bits 5 / 6 give unquantised bf16 models -- bit 0, the first fast layer's QKV at codebooks
>= 1 read from the table of its codebook_size possible rows; bit 1, the K / V-only projection and the Q-free
attention at codebook 0.  Both must leave every bit of the frame as it was, so every comparison is array_equal;
that the work really went away is read from the profiler's launch counts and bytes; and the knob must change
nothing where it has to stay inert.  The layouts are test_gpu_fast_deadwork's (dim 512, 8 / 2 heads x 64, 2 fast
layers): (b), qk-norm and no biases, is where the feature engages; (a), configured with qkv / o biases, stays
on the launches it has.  Run on the MI355X box: pytest -m gpu.

No case covers an int8 model whose fast nq is no multiple of 16 (where bit 1 would have to stay inert on the
16-row tile kernel): the knob acts only inside the fused fast attention + wo launch, whose int8 wo needs
nq = n_head * head_dim to be a whole number of 512-k chunks (rowgemv_u), so no valid layout has nq % 16 != 0
there -- 7 heads x 8, say, never reaches the fused launch at all."""
import numpy as np
import pytest

from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced, _inputs, _variant_cfg

pytestmark = pytest.mark.gpu

SETTINGS = (0, 1, 2, 3)
GS = 128  # int4 group size
CLASSES = ("linear", "attn")


def _model(quant, variant="b", seed=11, max_slots=1, precision="bf16"):
    from fishmi.llm import DualARModel

    cfg = _variant_cfg(variant)
    return cfg, DualARModel.synthetic(cfg, seed, 5, 0, precision, max_slots, quant=quant, groupsize=GS)


def _profile(m, slots=(0,)):
    """(launches, bytes) per profiler class of one eager decode frame of `slots` (the host checks the hand-off's
    error word after it)."""
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


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_every_bit_stays(quant, knob):
    """Slow logits, fast logits and emitted columns of 7 teacher-forced frames (gathered codes 0 and cb - 1 among
    them) are array_equal under fast_dead_q 0, 1, 2 and 3, the graph re-captured per setting; under 3 one frame
    run eagerly equals its graph replay."""
    cfg, m = _model(quant)
    prompt, cols = _inputs(cfg, 3)
    assert 0 in cols[1:] and cfg.codebook_size - 1 in cols[1:]
    try:
        out = {}
        for v in SETTINGS:
            knob("fast_dead_q", v)
            m.use_graph(True)  # re-capture the frame under the knob
            out[v] = _forced(m, prompt, cols)
        assert np.isfinite(out[0][1]).all()
        for v in SETTINGS[1:]:
            for a, b in zip(out[0], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"fast_dead_q {v}")
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            res[graph] = _forced(m, prompt, cols[:, :2])
        for a, b in zip(res[False], res[True]):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(res[True], out[3]):
            np.testing.assert_array_equal(a, b[:2])
    finally:
        m.use_graph(True)
        m.close()


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_the_work_went_away(quant, knob):
    """profile_read over one decoded frame.  From fast_dead_q 0 to 1 the "linear" launches drop by exactly C - 1
    (the first fast layer's QKV at codebooks 1 .. C - 1); from 0 to 2 the count is unchanged and the bytes drop
    by exactly the Q rows of the n_fast codebook-0 projections -- int8 nq * dim code bytes each, int4 nq * dim / 2
    code bytes + nq * (dim / group) (scale, zero) words; from 0 to 3 both; the "attn" class (the fused launch is
    booked there) never moves.  An all-inert build fails the first assertion."""
    cfg, m = _model(quant)
    prompt, _ = _inputs(cfg, 3)
    dim, nq = cfg.fast_dim, cfg.fast_n_head * cfg.fast_head_dim
    C, n_fast = cfg.num_codebooks, cfg.n_fast_layer
    q_rows = nq * dim if quant == "int8" else nq * dim // 2 + nq * (dim // GS) * 4
    try:
        got = {}
        for v in SETTINGS:
            knob("fast_dead_q", v)
            m.prefill(0, prompt, _sampling())
            got[v] = _profile(m)
        print(quant, got)
        (n0, b0), (n1, b1), (n2, b2), (n3, b3) = (got[v]["linear"] for v in SETTINGS)
        assert n0 - n1 == C - 1 and C > 1, got
        assert b1 < b0, got
        assert n2 == n0 and b0 - b2 == n_fast * q_rows, (got, n_fast * q_rows)
        assert n0 - n3 == C - 1 and b0 - b3 == (b0 - b1) + (b0 - b2), got
        assert got[0]["attn"][0] > 0 and all(got[v]["attn"] == got[0]["attn"] for v in SETTINGS), got
    finally:
        m.close()


INERT = ["a-int8", "bf16", "int4-stream0", "int8-unfused", "three-slots"]


@pytest.mark.parametrize("case", INERT)
def test_inert_where_it_must_be(case, knob):
    """The knob changes neither the bits nor the profiler's launch counts and bytes on: the o-bias layout (a)
    with int8; an unquantised bf16 handle; an int4 handle on its dequantised weights (int4_stream 0); an int8
    handle without the fused launch (fattn_wo 0); a 3-slot int8 handle decoding its slots batched."""
    quant = {"a-int8": "int8", "bf16": None, "int4-stream0": "int4", "int8-unfused": "int8", "three-slots": "int8"}[case]
    if case == "int4-stream0":
        knob("int4_stream", 0)
    if case == "int8-unfused":
        knob("fattn_wo", 0)
    slots = (0, 1, 2) if case == "three-slots" else (0,)
    cfg, m = _model(quant, variant="a" if case == "a-int8" else "b", max_slots=len(slots))
    prompt, cols = _inputs(cfg, 3)
    try:
        bits, prof = {}, {}
        for v in (0, 3):
            knob("fast_dead_q", v)
            m.use_graph(True)
            if len(slots) == 1:
                bits[v] = _forced(m, prompt, cols[:, :4])
            else:
                first = [m.prefill(s, _inputs(cfg, 5 + s)[0], _sampling(77)) for s in slots]
                bits[v] = (np.stack(first), m.decode_frames(list(slots), 4))
            prof[v] = _profile(m, slots)
        print(case, prof)
        for a, b in zip(bits[0], bits[3]):
            np.testing.assert_array_equal(a, b)
        assert prof[0]["linear"][0] > 0 and prof[0] == prof[3], prof
    finally:
        m.use_graph(True)
        m.close()


@pytest.mark.parametrize("quant", ["int8", "int4"])
def test_sampled_stream_identical(quant, knob):
    """32 sampled frames (top_k 30, top_p 0.8, temperature 0.8, fixed seed) without host syncs: the same columns
    under fast_dead_q 0 and 3."""
    cfg, m = _model(quant, seed=13)
    prompt, _ = _inputs(cfg, 5)
    try:
        out = {}
        for v in (0, 3):
            knob("fast_dead_q", v)
            m.use_graph(True)
            first = m.prefill(0, prompt, _sampling())
            out[v] = np.concatenate([first[None], m.decode_frames([0], 32)[:, 0]])
        np.testing.assert_array_equal(out[0], out[3])
        assert len(np.unique(out[3][:, 1:])) > 8  # a sampled stream, not one repeated code
    finally:
        m.close()


def test_three_slots_one_at_a_time(knob):
    """A 3-slot int8 handle, its slots decoded one at a time in permuted order: the streams under fast_dead_q 3
    equal those under 0 (the table and the hand-off tags do not depend on the slot)."""
    cfg, m = _model("int8", seed=13, max_slots=3)
    prompts = [_inputs(cfg, 5 + s)[0] for s in range(3)]
    order = [(2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0)]
    try:
        out = {}
        for v in (0, 3):
            knob("fast_dead_q", v)
            m.use_graph(True)
            got = {s: [m.prefill(s, prompts[s], _sampling(77))] for s in range(3)}
            for k in range(8):
                for s in order[k % len(order)]:
                    got[s].append(m.decode([s])[0])
            out[v] = np.stack([np.stack(got[s]) for s in range(3)])
        np.testing.assert_array_equal(out[0], out[3])
        assert len(np.unique(out[3][:, :, 1:])) > 8
    finally:
        m.close()


def test_int8_checkpoint_vs_reference_with_both_bits(golden, knob):
    """The knob's default leaves bit 1 off (its gain did not clear three times the baseline's spread, DESIGN
    section 3), so the files that pin the quantised path to the reference do not run it: test_gpu_int8's
    bf16-vs-reference check on the int8 checkpoint once more, with fast_dead_q 3."""
    from test_gpu_int8 import _qmodel
    from test_gpu_llm import _bf16_vs_reference

    knob("fast_dead_q", 3)
    g = golden("llm_q_int8_bf16.npz")
    m = _qmodel("bf16")
    try:
        T = g["prompt"].shape[1]
        slow, fast = m.teacher_decode(g["prompt"], g["seq"][:, T:])
        st = _bf16_vs_reference(slow, fast, g)
        assert st["top1_checked"] > 20
    finally:
        m.close()


def test_int8_real_widths_vs_reference_with_both_bits(golden, knob):
    """The checkpoint above is too narrow for the fused launch, so neither bit engages on it; S2-Pro widths at
    reduced depth (test_gpu_int8's wide model, where both do) against the reference int8 model's logits, with
    fast_dead_q 3: within the bf16 bound."""
    from test_gpu_int8 import _int8_wide

    knob("fast_dead_q", 3)
    _int8_wide(golden)


def test_table_follows_its_kernel(knob):
    """int4: under row_qkv_rp 4, then 8 (any fm_tune call starts a new tuning epoch, so the table is rebuilt by the
    QKV launch in force), the logits with the table (fast_dead_q 1) equal those without it (0) at the same value."""
    cfg, m = _model("int4")
    prompt, cols = _inputs(cfg, 7)
    try:
        for rp in (4, 8):
            out = {}
            for v in (1, 0):
                knob("fast_dead_q", v)
                knob("row_qkv_rp", rp)
                m.use_graph(True)
                out[v] = _forced(m, prompt, cols[:, :4])
            for a, b in zip(out[0], out[1]):
                np.testing.assert_array_equal(a, b, err_msg=f"row_qkv_rp {rp}")
    finally:
        m.close()
