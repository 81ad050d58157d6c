"""Weight-only int8 models on the batched decode path (9..32 slots, bf16): with fm_tune "bstream_q8" 1
the batched linears (bsacc_kernel) stream the int8 codes instead of their bf16 fragment copy.  The
arithmetic is the same, so everything must be bit-equal to "bstream_q8" 0, which tests/test_gpu_int8.py
pins to the reference's own int8 model; only the bytes read change.  Run on the MI355X box:
pytest -m gpu."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from parity_util import tuned
from test_gpu_llm import IM_END, _bf16_vs_reference, _cfg

pytestmark = pytest.mark.gpu



def _prompts(g, cfg, n):
    """The golden prompt in slot 0, perturbed ones in the others (test_int8_batched_slots_match_single's)."""
    rng = np.random.default_rng(5)
    out = []
    for s in range(n):
        p = g["prompt"].copy()
        if s:
            p[0, 1:5] = rng.integers(16, cfg.semantic_begin_id, 4)
        out.append(p)
    return out


def _linear_bytes(m, slots):
    """The "linear" class bytes of one profiled (eager) decode frame of `slots`."""
    m.profile(True)
    m.decode(slots)
    _, launches, b = m.profile_read("linear")
    m.profile(False)
    assert launches > 0
    return b


def _tiny_run(g, prec, n, q8, extra=None):
    """A fresh llm_q_int8 model with the knob set before its first frame: greedy mask_im_end prefill +
    8 decode_frames of n slots, then one frame with slot 0 forced (its logits), then one profiled frame."""
    from fishmi.llm import DualARModel

    with tuned(bstream_q8=q8, **(extra or {})):
        m = DualARModel.from_pretrained(os.path.join(GOLDEN, "llm_q_int8"), 0, prec, n, im_end_id=IM_END)
        assert m.quant == "int8"
        slots = list(range(n))
        sp = DualARModel.sampling(top_k=1, mask_im_end=True)
        firsts = [m.prefill(s, p, sp) for s, p in enumerate(_prompts(g, m.cfg, n))]
        fr = m.decode_frames(slots, 8)
        cols = np.concatenate([np.stack(firsts)[None], fr], axis=0)  # (9, n, C+1)
        T = g["prompt"].shape[1]
        m.force(0, g["seq"][:, T + 9])
        try:
            m.decode(slots)
            slow, fast = m.read_logits(0)
        finally:
            m.force(0, None)
        b = _linear_bytes(m, slots)
        m.close()
    return cols, slow, fast, b


@pytest.mark.parametrize("n", [9, 32])
def test_int8_bf16_batched_codes_equal_fragment_copy(n, golden):
    """Tiny int8 checkpoint, bf16, 9 and 32 slots: every slot's columns, and slot 0's forced-frame slow
    and fast logits, are bit-equal between bstream_q8 0 and 1 -- and the knob is live there (the frame's
    linear bytes shrink)."""
    g = golden("llm_q_int8_bf16.npz")
    c0, s0, f0, b0 = _tiny_run(g, "bf16", n, 0)
    c1, s1, f1, b1 = _tiny_run(g, "bf16", n, 1)
    np.testing.assert_array_equal(c1, c0)
    assert np.isfinite(f0).all() and np.isfinite(s0).any()
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(f1, f0)
    print(f"n={n}: linear bytes per frame {b0} -> {b1}")
    assert b1 < b0


@pytest.mark.parametrize("case", ["bstream_acc0", "fp32"])
def test_bstream_q8_inert_on_the_other_paths(case, golden):
    """bstream_kernel (bstream_acc 0) and fp32 models keep reading the T copy of the codes: the knob
    changes neither the columns, nor slot 0's logits, nor the profiled bytes."""
    prec = "fp32" if case == "fp32" else "bf16"
    extra = {"bstream_acc": 0} if case == "bstream_acc0" else None
    g = golden(f"llm_q_int8_{prec}.npz")
    c0, s0, f0, b0 = _tiny_run(g, prec, 12, 0, extra)
    c1, s1, f1, b1 = _tiny_run(g, prec, 12, 1, extra)
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(f1, f0)
    assert b1 == b0


_WIDE = {}


def _wide_runs(golden):
    """llm_wide synthetic int8 (the golden's seed), bf16, 12 slots, once per knob value on a fresh model:
    slot 0 teacher-forced with the reference int8 model's columns while 11 other slots decode beside it
    (so every frame is the batched one), then one profiled frame.  Computed once, shared by the tests."""
    if _WIDE:
        return _WIDE
    from fishmi.llm import DualARModel

    path = os.path.join(GOLDEN, "llm_wide_int8_bf16.npz")
    if not os.path.exists(path):
        pytest.skip("llm_wide_int8_bf16.npz not generated")
    g = golden("llm_wide_int8_bf16.npz")
    cfg = _cfg("llm_wide")
    n = 12
    slots = list(range(n))
    T = g["prompt"].shape[1]
    cols = g["seq"][:, T:]
    nf = cols.shape[1]
    runs = {}
    for q8 in (0, 1):
        with tuned(bstream_q8=q8):
            m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", n, quant="int8")
            slow = np.zeros((nf, cfg.vocab_size), np.float32)
            fast = np.zeros((nf, cfg.num_codebooks - 1, cfg.codebook_size), np.float32)
            sp = DualARModel.sampling(top_k=1, mask_im_end=True)
            try:
                for i in range(nf):
                    m.force(0, cols[:, i])
                    if i == 0:
                        for s, p in enumerate(_prompts(g, cfg, n)):
                            m.prefill(s, p, sp)
                    else:
                        m.decode(slots)
                    slow[i], fast[i] = m.read_logits(0)
            finally:
                m.force(0, None)
            runs[q8] = (slow, fast, _linear_bytes(m, slots))
            m.close()
    _WIDE.update(g=g, cfg=cfg, runs=runs)
    return _WIDE


def test_int8_wide_batched_codes_vs_reference(golden):
    """S2-Pro widths, int8, the 12-slot batched frame streaming the codes: slot 0's teacher-forced logits
    pass test_int8_wide_real_widths_vs_reference's bar against the reference's own int8 model, and are
    bit-equal to the same run on the bf16 fragment copy."""
    w = _wide_runs(golden)
    slow1, fast1, _ = w["runs"][1]
    slow0, fast0, _ = w["runs"][0]
    _bf16_vs_reference(slow1, fast1, w["g"], rows=w["g"]["slow_rows"])
    np.testing.assert_array_equal(slow1, slow0)
    np.testing.assert_array_equal(fast1, fast0)


def test_int8_wide_batched_profile_bytes(golden):
    """The profiled "linear" bytes of one 12-slot frame shrink by exactly sum(N K - 2 N) over the
    quantised linears of the frame (each goes from N K 2 bytes of bf16 fragments to N K codes + N bf16
    scales): wqkv, wo, w1 || w3 and w2 of every slow layer once and of every fast layer once per codebook
    pass, the codebook head once per codebook >= 1, fast_project_in and the LM head where the model has
    them as linears (the tied LM head is an embedding and stays bf16)."""
    w = _wide_runs(golden)
    cfg = w["cfg"]
    b0, b1 = w["runs"][0][2], w["runs"][1][2]

    def saved(N, K):
        return N * K - 2 * N

    def stack(dim, nh, nkv, hd, inter):
        nqkv = (nh + 2 * nkv) * hd
        return saved(nqkv, dim) + saved(dim, nh * hd) + saved(2 * inter, dim) + saved(dim, inter)

    C = cfg.num_codebooks
    want = cfg.n_layer * stack(cfg.dim, cfg.n_head, cfg.n_local_heads, cfg.head_dim, cfg.intermediate_size)
    want += cfg.n_fast_layer * C * stack(cfg.fast_dim, cfg.fast_n_head, cfg.fast_n_local_heads, cfg.fast_head_dim,
                                         cfg.fast_intermediate_size)
    want += (C - 1) * saved(cfg.codebook_size, cfg.fast_dim)
    if cfg.fast_dim != cfg.dim:
        want += saved(cfg.fast_dim, cfg.dim)
    if not cfg.tie_word_embeddings:
        want += saved(cfg.semantic_end_id - cfg.semantic_begin_id + 2, cfg.dim)
    print(f"linear bytes per 12-slot frame: bstream_q8 0 {b0}, 1 {b1}, difference {b0 - b1}, expected {want}")
    assert b1 < b0
    assert b0 - b1 == want
