"""Weight-only int4 models (group size 128) on the batched decode path (9..32 slots, bf16): with fm_tune
"bstream_q4" 1 the batched linears (bsacc_kernel) stream the 4-bit codes and their group (scale, zero) words
instead of the dequantised bf16 fragment copy.  The register expansion is the copy's own arithmetic, so
everything must be bit-equal to "bstream_q4" 0 -- the path tests/test_gpu_int4.py ties to the reference's
quantiser; only the bytes read change.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

from parity_util import tuned
from test_gpu_int8_batched import _linear_bytes, _prompts
from test_gpu_llm import _cfg

pytestmark = pytest.mark.gpu

N_SLOTS = 12


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(golden, q4, nf, extra=None, groupsize=128, frames=0):
    """A fresh llm_wide synthetic int4 model (the bf16 golden's seed), bf16, 12 slots, the knob set before its
    first frame: slot 0 teacher-forced with the golden's columns for nf frames while 11 perturbed-prompt slots
    decode beside it (every frame is the batched one, replayed from its graph), then `frames` greedy
    decode_frames of all slots, then one profiled eager frame.  Returns (slow [nf][V], fast [nf][C-1][cb],
    columns [frames][12][C+1], linear bytes of the profiled frame, cfg)."""
    from fishmi.llm import DualARModel

    g = golden("llm_wide_bf16.npz")
    cfg = _cfg("llm_wide")
    slots = list(range(N_SLOTS))
    T = g["prompt"].shape[1]
    cols = g["seq"][:, T:]
    assert cols.shape[1] >= nf
    with tuned(bstream_q4=q4, **(extra or {})):
        m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", N_SLOTS, quant="int4",
                                  groupsize=groupsize)
        try:
            slow = np.zeros((nf, cfg.vocab_size), np.float32)
            fast = np.zeros((nf, cfg.num_codebooks - 1, cfg.codebook_size), np.float32)
            sp = DualARModel.sampling(top_k=1, mask_im_end=True)
            try:
                for i in range(nf):
                    m.force(0, cols[:, i])
                    if i == 0:
                        for s, p in enumerate(_prompts(g, cfg, N_SLOTS)):
                            m.prefill(s, p, sp)
                    else:
                        m.decode(slots)
                    slow[i], fast[i] = m.read_logits(0)
            finally:
                m.force(0, None)
            fr = m.decode_frames(slots, frames) if frames else None
            b = _linear_bytes(m, slots)
        finally:
            m.close()
    return slow, fast, fr, b, cfg


_MAIN = {}


def _main_runs(golden):
    """bstream_q4 0 and 1 at the default knobs, 5 forced frames + 8 greedy frames: computed once, shared"""
    if not _MAIN:
        _MAIN.update({q4: _run(golden, q4, 5, frames=8) for q4 in (0, 1)})
    return _MAIN


def test_int4_wide_batched_codes_equal_fragment_copy(golden):
    """slot 0's slow and fast logits of every teacher-forced frame are bit-equal between bstream_q4 0 and 1, with
    the same non-finite mask (the masked vocabulary rows), and all 12 slots' greedy columns agree over the 8
    frames that follow"""
    r = _main_runs(golden)
    s0, f0, c0, _, _ = r[0]
    s1, f1, c1, _, _ = r[1]
    assert np.isfinite(f0).all() and np.isfinite(s0).any() and np.any(f0 != 0)
    assert np.array_equal(np.isfinite(s1), np.isfinite(s0)) and np.array_equal(np.isfinite(f1), np.isfinite(f0))
    assert np.array_equal(_bits(s1), _bits(s0))
    assert np.array_equal(_bits(f1), _bits(f0))
    assert c0.shape == (8, N_SLOTS, c0.shape[2])
    np.testing.assert_array_equal(c1, c0)


def test_int4_wide_batched_profile_bytes(golden):
    """The profiled "linear" bytes of one 12-slot frame shrink by exactly the sum over the frame's quantised
    linears of N K 2 - (N K / 2 + N (K / 128) 4) (bf16 fragments -> 4-bit codes + one (scale, zero) word per row
    and 128-k unit): test_int8_wide_batched_profile_bytes's enumeration -- wqkv, wo, w1 || w3 and w2 of every slow
    layer once and of every fast layer once per codebook pass, the codebook head once per codebook >= 1,
    fast_project_in and the LM head where the model has them as linears (the tied head stays bf16)."""
    r = _main_runs(golden)
    b0, b1, cfg = r[0][3], r[1][3], r[0][4]

    def saved(N, K):
        assert K % 128 == 0
        return N * K * 2 - (N * K // 2 + N * (K // 128) * 4)

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
    print(f"linear bytes per 12-slot frame: bstream_q4 0 {b0}, 1 {b1}, difference {b0 - b1}, expected {want}")
    assert b1 < b0
    assert b0 - b1 == want


@pytest.mark.parametrize("case", ["bstream_acc0", "groupsize64", "int4_stream0"])
def test_bstream_q4_inert_on_the_other_paths(case, golden):
    """bstream_kernel (bstream_acc 0), groups of 64 (no 128-k (scale, zero) table) and the model on its
    dequantised weights (int4_stream 0) keep reading the bf16 copy: the knob changes neither slot 0's logits nor
    the profiled bytes"""
    extra = {"bstream_acc0": {"bstream_acc": 0}, "int4_stream0": {"int4_stream": 0}}.get(case)
    gs = 64 if case == "groupsize64" else 128
    s0, f0, _, b0, _ = _run(golden, 0, 2, extra, gs)
    s1, f1, _, b1, _ = _run(golden, 1, 2, extra, gs)
    assert np.isfinite(f0).all() and np.any(f0 != 0)
    assert np.array_equal(_bits(s1), _bits(s0))
    assert np.array_equal(_bits(f1), _bits(f0))
    assert b1 == b0


def test_int4_batched_graph_replay_equals_eager(golden):
    """bstream_q4 1: one 12-slot frame replayed from the captured graph (every bsacc_kernel attribute was set
    before the capture) is bit-equal to the same frame launched eagerly"""
    from fishmi.llm import DualARModel

    g = golden("llm_wide_bf16.npz")
    cfg = _cfg("llm_wide")
    slots = list(range(N_SLOTS))
    T = g["prompt"].shape[1]
    cols = g["seq"][:, T:]
    res = {}
    with tuned(bstream_q4=1):
        m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", N_SLOTS, quant="int4",
                                  groupsize=128)
        try:
            sp = DualARModel.sampling(top_k=1, mask_im_end=True)
            for graph in (False, True):
                m.use_graph(graph)
                try:
                    m.force(0, cols[:, 0])
                    for s, p in enumerate(_prompts(g, cfg, N_SLOTS)):
                        m.prefill(s, p, sp)
                    m.force(0, cols[:, 1])
                    out = m.decode(slots)
                    res[graph] = (out,) + m.read_logits(0)
                finally:
                    m.force(0, None)
        finally:
            m.use_graph(True)
            m.close()
    np.testing.assert_array_equal(res[True][0], res[False][0])
    assert np.isfinite(res[False][2]).all() and np.any(res[False][2] != 0)
    assert np.array_equal(_bits(res[True][1]), _bits(res[False][1]))
    assert np.array_equal(_bits(res[True][2]), _bits(res[False][2]))
