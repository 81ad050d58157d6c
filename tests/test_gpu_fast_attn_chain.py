"""The fused fast attention + wo launch's shortened attention chain (fm_tune
fattn_ilp): the q / k prep chains side by side, and score / softmax / PV over a compile-time
position count with the softmax one position per lane.
Scheduling only, so every check is exact: logits and emitted columns are array_equal with the knob
off and on, on three head layouts with 10 codebooks (every position count 1 .. 10) and on one with
16 (the FW_MAXJ limit, the rounded-up counts 12 and 16), and in a sampled stream; the fused launch
still runs, and the reference bound holds under the default.  Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced
from test_gpu_llm import _bf16_vs_reference, _cfg
from test_gpu_rowgemv import FW_TAG, _biased_cfg, _row_blocks_ran

pytestmark = pytest.mark.gpu

SETTINGS = (0, 1)  # fattn_ilp
NF = 7  # teacher-forced frames: the prefill's frame + 6 decoded ones


@pytest.fixture
def knobs(knob):
    def set_(ilp):
        knob("fattn_ilp", ilp)

    return set_


def _layout_cfg(layout, codebooks=10):
    """a: test_gpu_rowgemv's biased layout (8 / 2 heads x 64, biases, no qk-norm); b: the same widths
    with qk-norm and no biases; c: head_dim 128, 4 q heads per kv head, qk-norm (the S2-Pro head layout
    at dim 512).  2 fast layers, `codebooks` codebooks: a frame walks cpos 0 .. codebooks - 1."""
    base = _biased_cfg()
    kw = dict(num_codebooks=codebooks)
    if layout in ("b", "c"):
        kw.update(attention_qk_norm=True, attention_qkv_bias=False, attention_o_bias=False,
                  fast_attention_qk_norm=True, fast_attention_qkv_bias=False, fast_attention_o_bias=False)
    if layout == "c":
        kw.update(n_head=4, n_local_heads=1, head_dim=128, fast_n_head=4, fast_n_local_heads=1, fast_head_dim=128)
    cfg = dataclasses.replace(base, **kw)
    cfg.im_end_id = base.im_end_id
    assert cfg.n_fast_layer == 2 and cfg.num_codebooks == codebooks
    return cfg


def _inputs(cfg, seed, nf=NF, T=12):
    rng = np.random.default_rng(seed)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, T), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, T)
    cols = np.zeros((C1, nf), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, nf)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, nf))
    return prompt, cols


def _equal(ref, got, what):
    for a, b in zip(ref, got):
        np.testing.assert_array_equal(a, b, err_msg=what)


@pytest.mark.parametrize("layout", ["a", "b", "c"])
def test_knobs_leave_every_bit(layout, knobs):
    """Slow and fast logits and the emitted columns of 7 teacher-forced frames are array_equal with the
    knob off and on (graph re-captured per setting); under the default one frame run eagerly equals
    its graph replay."""
    from fishmi.llm import DualARModel

    cfg = _layout_cfg(layout)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3)
    try:
        out = {}
        for s in SETTINGS:
            knobs(s)
            m.use_graph(True)  # re-capture the frame under the knobs
            out[s] = _forced(m, prompt, cols)
        assert np.isfinite(out[0][1]).all()
        for s in SETTINGS[1:]:
            _equal(out[0], out[s], f"fattn_ilp {s}")
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            res[graph] = _forced(m, prompt, cols[:, :2])
        _equal(res[False], res[True], "eager vs graph replay")
        _equal(res[True], [x[:2] for x in out[1]], "second capture")
    finally:
        m.use_graph(True)
        m.close()


def test_knobs_leave_every_bit_at_the_position_limit(knobs):
    """16 codebooks: the fused launch reaches cpos 15 (FW_MAXJ), the rounded-up position counts 12 and
    16 included; 3 teacher-forced frames, knob off and on array_equal."""
    from fishmi.llm import DualARModel

    cfg = _layout_cfg("b", codebooks=16)
    m = DualARModel.synthetic(cfg, 17, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 9, nf=3)
    try:
        out = {}
        for s in SETTINGS:
            knobs(s)
            m.use_graph(True)
            out[s] = _forced(m, prompt, cols)
        assert np.isfinite(out[0][1]).all()
        for s in SETTINGS[1:]:
            _equal(out[0], out[s], f"fattn_ilp {s}")
        knobs(1)
        m.prefill(0, prompt, DualARModel.sampling(top_k=1))
        assert _row_blocks_ran(m, lambda: m.decode([0]), FW_TAG) > 0
    finally:
        m.use_graph(True)
        m.close()


def test_sampled_stream_identical(knobs):
    """12 sampled frames (top_k 30, top_p 0.8, temperature 0.8, fixed seed): the same columns with the
    knob off and on."""
    from fishmi.llm import DualARModel

    cfg = _layout_cfg("c")
    m = DualARModel.synthetic(cfg, 13, 5, 0, "bf16", 1)
    prompt, _ = _inputs(cfg, 5)
    try:
        out = {}
        for s in SETTINGS:
            knobs(s)
            m.use_graph(True)
            sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=1234, mask_im_end=True)
            first = m.prefill(0, prompt, sp)
            out[s] = np.concatenate([first[None], m.decode_frames([0], 12)[:, 0]])
        for s in SETTINGS[1:]:
            np.testing.assert_array_equal(out[0], out[s], err_msg=str(s))
        assert len(np.unique(out[1][:, 1:])) > 8  # a sampled stream, not one repeated code
    finally:
        m.close()


@pytest.mark.parametrize("layout", ["a", "c"])
def test_the_fused_launch_still_runs(layout, knobs):
    """debug_ts records of one eager frame under the defaults: one attention-wave record per q head
    for each fused launch (every fast layer of every codebook but codebook 0's K / V-only last one)."""
    from fishmi.llm import DualARModel

    cfg = _layout_cfg(layout)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, _ = _inputs(cfg, 3)
    try:
        knobs(1)
        m.prefill(0, prompt, DualARModel.sampling(top_k=1))
        waves = _row_blocks_ran(m, lambda: m.decode([0]), FW_TAG)
        assert waves == cfg.fast_n_head * (cfg.n_fast_layer * cfg.num_codebooks - 1), waves
    finally:
        m.use_graph(True)
        m.close()


def test_wide_bf16_vs_reference_under_defaults(golden, knobs):
    """S2-Pro widths (2 + 1 layers, qk-norm) under the defaults: teacher-forced logits within the bf16
    bound of the reference."""
    from fishmi.llm import DualARModel

    knobs(1)
    g = golden("llm_wide_bf16.npz")
    cfg = _cfg("llm_wide")
    m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", 1)
    try:
        T = g["prompt"].shape[1]
        slow, fast = m.teacher_decode(g["prompt"], g["seq"][:, T:])
        _bf16_vs_reference(slow, fast, g, rows=g["slow_rows"])
    finally:
        m.close()
