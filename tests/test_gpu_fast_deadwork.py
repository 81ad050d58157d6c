"""The fast decoder's two removals (fm_tune rowgemv bits 5 and 6): the first fast
layer's QKV at codebooks >= 1 read from the table of its codebook_size possible rows, and the
K / V-only projection + Q-free attention at codebook 0.  Both must leave every bit of the frame as
it was, so the checks are exact: logits and emitted columns under rowgemv 27 (neither), 59 (table),
91 (codebook 0) and 123 (both) are array_equal, the launches really went away (debug_ts block
counts), sampled streams agree, the reference bound holds under 123, and the table follows a knob
that changes the kernel it is built with.  Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_llm import _bf16_vs_reference, _cfg
from test_gpu_rowgemv import FW_TAG, ROW_TAG, _biased_cfg, _row_blocks_ran

pytestmark = pytest.mark.gpu

SETTINGS = (27, 59, 91, 123)
NF = 7  # teacher-forced frames: the prefill's frame + 6 decoded ones


@pytest.fixture
def rowgemv(knob):
    """set_(v): the rowgemv bits; set_.knob: the shared fixture, for the other knobs a test sets"""
    def set_(v):
        knob("rowgemv", v)

    set_.knob = knob
    return set_


def _variant_cfg(variant):
    """(a) test_gpu_rowgemv's biased layout: dim 512, 8 / 2 heads x 64, qkv / o biases, no qk-norm,
    2 fast layers (codebook 0 runs the fused form and the K / V-only last layer); (b) the same
    widths with qk-norm and no biases."""
    cfg = _biased_cfg()
    if variant == "b":
        cfg = dataclasses.replace(cfg, attention_qk_norm=True, attention_qkv_bias=False, attention_o_bias=False,
                                  fast_attention_qk_norm=True, fast_attention_qkv_bias=False,
                                  fast_attention_o_bias=False)
        cfg.im_end_id = _biased_cfg().im_end_id
    assert cfg.n_fast_layer == 2
    return cfg


def _inputs(cfg, seed):
    rng = np.random.default_rng(seed)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, 12), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, 12)
    cols = np.zeros((C1, NF), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, NF)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, NF))
    cols[1:, 1] = 0                      # the clamp's edges: every gathered code 0 ...
    cols[1:, 2] = cfg.codebook_size - 1  # ... and cb - 1
    cols[1::2, 3] = 0
    cols[2::2, 3] = cfg.codebook_size - 1
    return prompt, cols


def _forced(m, prompt, cols, slot=0):
    """Teacher-forced frames on the production path: slow logits, fast logits, emitted columns."""
    from fishmi.llm import DualARModel

    sp = DualARModel.sampling(top_k=1)
    sl, fl, em = [], [], []
    try:
        for k in range(cols.shape[1]):
            m.force(slot, cols[:, k])
            em.append(m.prefill(slot, prompt, sp) if k == 0 else m.decode([slot])[0])
            s, f = m.read_logits(slot)
            sl.append(s)
            fl.append(f)
    finally:
        m.force(slot, None)
    return np.stack(sl), np.stack(fl), np.stack(em)


@pytest.mark.parametrize("variant", ["a", "b"])
def test_bits_5_and_6_leave_every_bit(variant, rowgemv):
    """Slow and fast logits and the emitted columns of 7 teacher-forced frames are array_equal under
    rowgemv 27, 59, 91 and 123 (graph re-captured per setting), codes 0 and cb - 1 included; under
    123 one frame run eagerly equals its graph replay."""
    from fishmi.llm import DualARModel

    cfg = _variant_cfg(variant)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3)
    try:
        out = {}
        for v in SETTINGS:
            rowgemv(v)
            m.use_graph(True)  # re-capture the frame under the knob
            out[v] = _forced(m, prompt, cols)
        assert np.isfinite(out[27][1]).all()
        for v in SETTINGS[1:]:
            for a, b in zip(out[27], out[v]):
                np.testing.assert_array_equal(a, b, err_msg=f"rowgemv {v}")
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            res[graph] = _forced(m, prompt, cols[:, :2])
        for a, b in zip(res[False], res[True]):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(res[True], out[123]):
            np.testing.assert_array_equal(a, b[:2])
    finally:
        m.use_graph(True)
        m.close()


def test_the_launches_went_away(rowgemv):
    """debug_ts records of one eager frame: from 27 to 123 the row-GEMV block count drops by exactly
    (C - 1) * nqkv / 8 (the nine-fold first-layer QKV, here five-fold) + n_fast * nq / 8 (the Q rows of
    codebook 0's projections); each bit alone drops its own share; the fused launch's attention waves
    are unchanged."""
    from fishmi.llm import DualARModel

    cfg = _variant_cfg("a")
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3)
    sp = DualARModel.sampling(top_k=1)
    nq = cfg.fast_n_head * cfg.fast_head_dim
    nqkv = nq + 2 * cfg.fast_n_local_heads * cfg.fast_head_dim
    tab = (cfg.num_codebooks - 1) * nqkv // 8
    kv0 = cfg.n_fast_layer * nq // 8
    try:
        rows, waves = {}, {}
        for v in SETTINGS:
            rowgemv(v)
            m.prefill(0, prompt, sp)
            rows[v] = _row_blocks_ran(m, lambda: m.decode([0]))
            waves[v] = _row_blocks_ran(m, lambda: m.decode([0]), FW_TAG)
        print("row blocks", rows, "attention waves", waves)
        assert rows[27] - rows[59] == tab, rows
        assert rows[27] - rows[91] == kv0, rows
        assert rows[27] - rows[123] == tab + kv0, rows
        assert waves[27] > 0 and all(waves[v] == waves[27] for v in SETTINGS), waves
    finally:
        m.use_graph(True)
        m.close()


def test_sampled_stream_identical(rowgemv):
    """32 sampled frames (top_k 30, top_p 0.8, temperature 0.8, fixed seed) without host syncs:
    the same columns under 27 and 123."""
    from fishmi.llm import DualARModel

    cfg = _variant_cfg("b")
    m = DualARModel.synthetic(cfg, 13, 5, 0, "bf16", 1)
    prompt, _ = _inputs(cfg, 5)
    try:
        out = {}
        for v in (27, 123):
            rowgemv(v)
            m.use_graph(True)
            sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=1234, mask_im_end=True)
            first = m.prefill(0, prompt, sp)
            out[v] = np.concatenate([first[None], m.decode_frames([0], 32)[:, 0]])
        np.testing.assert_array_equal(out[27], out[123])
        assert len(np.unique(out[123][:, 1:])) > 8  # a sampled stream, not one repeated code
    finally:
        m.close()


def test_wide_bf16_vs_reference_under_default(golden, rowgemv):
    """S2-Pro widths (2 + 1 layers, qk-norm) under rowgemv 123: teacher-forced logits within the
    bf16 bound of the reference, as test_wide_bf16_variants_vs_reference checks the other knobs."""
    from fishmi.llm import DualARModel

    rowgemv(123)  # the default, whatever the process runs under
    g = golden("llm_wide_bf16.npz")
    cfg = _cfg("llm_wide")
    m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", 1)
    try:
        T = g["prompt"].shape[1]
        slow, fast = m.teacher_decode(g["prompt"], g["seq"][:, T:])
        _bf16_vs_reference(slow, fast, g, rows=g["slow_rows"])
    finally:
        m.close()


def test_table_follows_the_kernel_it_is_built_with(rowgemv):
    """row_qkv_rp picks another wqkv kernel (4, then 8 rows per block): with bit 5 on, the table is
    rebuilt under each value and the logits equal the bit-5-off logits of the same value."""
    from fishmi.llm import DualARModel

    cfg = _variant_cfg("a")
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 7)
    try:
        for rp in (4, 8):
            out = {}
            for v in (123, 91):
                rowgemv(v)
                rowgemv.knob("row_qkv_rp", rp)
                m.use_graph(True)
                out[v] = _forced(m, prompt, cols[:, :4])
            for a, b in zip(out[91], out[123]):
                np.testing.assert_array_equal(a, b, err_msg=f"row_qkv_rp {rp}")
    finally:
        m.close()
