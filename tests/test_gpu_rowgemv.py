"""The batch-1 row-block GEMV (fm_rowgemv.hip: wo / w2 with the residual epilogue, wqkv with the
RMSNorm prologue; fm_tune rowgemv bits 0 / 1) against the reference goldens at S2-Pro shapes and
against the 16-row MFMA tile path on a model with qkv / o biases.  Run on the MI355X box:
pytest -m gpu."""
import json
import os

import numpy as np
import pytest

from parity_util import bf16_vs_golden, knob  # noqa: F401  (knob: the shared fixture)

pytestmark = pytest.mark.gpu

IM_END = 4
ROW_TAG = 0xFFFA  # fm_rowgemv.hip's debug_ts record tags: row-block GEMV blocks
FW_TAG = 0xFFF9   # fused fast attention + wo: attention waves


@pytest.fixture
def rowgemv_mode(knob):
    def set_(v, fused=1):
        knob("rowgemv", v)
        knob("fattn_wo", fused)

    return set_


def _row_blocks_ran(m, step, tag=ROW_TAG):
    """Number of row-GEMV block records of one eager step (debug_ts): proves the path ran."""
    from fishmi import native

    m.use_graph(False)
    native.tune("debug_ts", 1)
    try:
        step()
        rec = native.debug_ts_read().astype(np.int64)
    finally:
        native.tune("debug_ts", 0)
        m.use_graph(True)
    return int(((rec[:, 0] >> 32) == tag).sum())


@pytest.mark.parametrize("mode,fused", [(1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (3, 1), (7, 1), (8, 0), (18, 0), (31, 1)])
def test_rowgemv_full_depth_bf16_vs_reference(golden, rowgemv_mode, mode, fused):
    """Config 2 at full depth (36 + 4 layers, S2-Pro shapes), graph-replayed frames, with wo / w2
    (bit 0), wqkv (bit 1) or both on the row-block GEMV, the fast model's attention + wo fused or
    not: within the bf16 bound of the reference."""
    from fishmi.config import DualARConfig
    from fishmi.llm import DualARModel

    rowgemv_mode(mode, fused)
    g = golden("llm_full_bf16.npz")
    cfg = DualARConfig._from_fish_qwen3_omni(json.loads(str(g["config"])))
    cfg.im_end_id = IM_END
    m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", 1)
    try:
        T = g["prompt"].shape[1]
        slow, fast = m.teacher_decode(g["prompt"], g["seq"][:, T:])
        m.prefill(0, g["prompt"], DualARModel.sampling(top_k=1))
        nrec = _row_blocks_ran(m, lambda: m.decode([0]))
        m.prefill(0, g["prompt"], DualARModel.sampling(top_k=1))
        nfw = _row_blocks_ran(m, lambda: m.decode([0]), FW_TAG)
    finally:
        m.close()
    # per frame: wo + w2 of 36 slow layers and 10 x 4 - 1 fast layers at 1280 blocks each (bit 0;
    # codebook 0's last fast layer stops after its K / V write, fm_tune fast_tail; the fast wo inside
    # the fused launch when on); wqkv of 35 slow + 10 x 3 fast layers at 768 blocks (bit 1; the
    # first layers' too with bit 4, the fast one gathering its row at codebook > 0); w1 || w3 of
    # 36 + 39 layers at 2432 blocks (bit 2); the 9 codebook heads at 512 blocks (bit 3); fused: 32
    # attention waves x 39 fast layers
    fw = fused and (mode & 1)
    want = (1280 * (2 * 36 + 39 + (0 if fw else 39)) if mode & 1 else 0) + \
        (768 * (35 + 30 + (1 + 10 if mode & 16 else 0)) if mode & 2 else 0) + \
        (2432 * (36 + 39) if mode & 4 else 0) + (512 * 9 if mode & 8 else 0)
    assert nrec == want, (nrec, want)
    assert nfw == (32 * 39 if fw else 0), nfw
    st = bf16_vs_golden(slow, fast, g, rows=g["slow_rows"])
    # coverage floor of the top-1 check: its margin threshold is twice the larger max error, the
    # build's included, so the count moves with the build's rounding (mode 7 fused with the skinny
    # prompt GEMM: fast max 0.265 against the reference's 0.203, inside the 1.5x bound, 8 clear
    # positions, all agreeing)
    assert st["top1_checked"] >= 8


def _biased_cfg():
    """llm_b's layout (qkv and o biases, no qk-norm, untied head) at widths the row path takes."""
    from conftest import GOLDEN
    from fishmi.config import DualARConfig

    c = json.load(open(os.path.join(GOLDEN, "llm_b", "config.json")))
    c.update(dim=512, n_head=8, n_local_heads=2, head_dim=64, intermediate_size=1024, n_layer=2,
             max_seq_len=96)
    c = {k: v for k, v in c.items() if k in DualARConfig.__dataclass_fields__}
    for k in ("fast_dim", "fast_n_head", "fast_n_local_heads", "fast_head_dim", "fast_intermediate_size"):
        c.pop(k, None)
    cfg = DualARConfig(**c)
    cfg.im_end_id = IM_END
    return cfg


def test_rowgemv_matches_tile_path_with_biases(rowgemv_mode):
    """Teacher-forced frames of a biased model, row-block GEMV (rowgemv 31) vs the 16-row MFMA tiles
    (rowgemv 0): logits agree to bf16 rounding-order level (relative RMS < 2e-2, argmax equal where
    the margin is clear), the row path really ran, and its graph replay equals its eager frame bit
    for bit."""
    from fishmi.llm import DualARModel

    cfg = _biased_cfg()
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 2)
    rng = np.random.default_rng(3)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, 12), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, 12)
    cols = np.zeros((C1, 6), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, 6)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, 6))
    sp = DualARModel.sampling(top_k=1)
    try:
        out = {}
        for slot, mode in ((0, 0), (1, 31)):
            rowgemv_mode(mode, 1 if mode else 0)
            sl, fl = [], []
            for k in range(cols.shape[1]):
                m.force(slot, cols[:, k])
                if k == 0:
                    m.prefill(slot, prompt, sp)
                else:
                    m.decode([slot])
                s, f = m.read_logits(slot)
                sl.append(s)
                fl.append(f)
            out[mode] = (np.stack(sl), np.stack(fl))
        for a, b in zip(out[0], out[31]):
            fin = np.isfinite(a)  # (the constrained head's masked rows are -inf in both)
            assert np.array_equal(fin, np.isfinite(b))
            rel = np.sqrt(np.mean((a[fin] - b[fin]) ** 2)) / np.sqrt(np.mean(a[fin] ** 2))
            assert rel < 2e-2, rel
            srt = np.sort(a, axis=-1)
            clear = (srt[..., -1] - srt[..., -2]) > 0.1
            assert np.array_equal(np.argmax(a, -1)[clear], np.argmax(b, -1)[clear])
        rowgemv_mode(31, 1)
        m.force(1, cols[:, 1])
        assert _row_blocks_ran(m, lambda: m.decode([1])) > 0
        m.force(1, cols[:, 2])
        assert _row_blocks_ran(m, lambda: m.decode([1]), FW_TAG) > 0
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            m.force(0, cols[:, 0])
            m.prefill(0, prompt, sp)
            m.force(0, cols[:, 1])
            m.decode([0])
            res[graph] = m.read_logits(0)
        for a, b in zip(res[False], res[True]):
            np.testing.assert_array_equal(a, b)
    finally:
        for s in (0, 1):
            m.force(s, None)
        m.use_graph(True)
        m.close()


def test_fused_fast_attention_tags_stay_fresh_across_toggles(rowgemv_mode):
    """The fused fast attention + wo hands its attention rows over by tagged words (fattn_wo_kernel):
    teacher-forced frames with the fusion switched on, off and on again between frames (the words
    left in the buffer by an earlier frame must never pass for the current one) track the same
    frames without the fusion -- logits within bf16 rounding-order level, argmax equal where clear."""
    from fishmi.llm import DualARModel

    cfg = _biased_cfg()
    m = DualARModel.synthetic(cfg, 12, 5, 0, "bf16", 1)
    rng = np.random.default_rng(5)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, 10), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, 10)
    nf = 7
    cols = np.zeros((C1, nf), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, nf)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, nf))
    sp = DualARModel.sampling(top_k=1)
    try:
        out = {}
        for run, plan in (("off", [0] * nf), ("toggled", [1, 1, 0, 0, 1, 0, 1])):
            fl = []
            for k in range(nf):
                rowgemv_mode(27, plan[k])
                m.use_graph(True)  # re-capture the frame under the knob
                m.force(0, cols[:, k])
                if k == 0:
                    m.prefill(0, prompt, sp)
                else:
                    m.decode([0])
                fl.append(m.read_logits(0)[1])
            out[run] = np.stack(fl)
        a, b = out["off"], out["toggled"]
        rel = np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(a ** 2))
        assert rel < 2e-2, rel
        srt = np.sort(a, axis=-1)
        clear = (srt[..., -1] - srt[..., -2]) > 0.1
        assert np.array_equal(np.argmax(a, -1)[clear], np.argmax(b, -1)[clear])
    finally:
        m.force(0, None)
        m.use_graph(True)
        m.close()
