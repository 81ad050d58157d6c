"""fm_tune fast_pair: a batch-1 bf16 frame runs the fast decoder's codebook
positions 0 and 1 as one two-row pass, so each fast weight is read once for the two.  The change claims bit
identity, so every comparison is array_equal: whole frames (teacher-forced and sampled) under fast_pair 0 and 1,
the launches that must have gone away, the settings under which the knob must change nothing, each two-row
kernel form against the one-row production launcher per output row, and the reference bound under the default.
Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _forced, _inputs, _variant_cfg
from test_gpu_llm import _bf16_vs_reference, _cfg

pytestmark = pytest.mark.gpu

SENT = 320.0  # output sentinel (a bf16 value no test output takes: the operands are O(1))


def _pair_cfg(variant):
    """a / b: test_gpu_fast_deadwork's two layouts (dim 512, 8 / 2 heads x 64, biases | qk-norm, 2 fast layers);
    c: b with 3 fast layers, the smallest depth with a middle layer (the two-row wqkv whose Q blocks take one row);
    d: b with fast heads 4 / 2 x 128, S2-Pro's head layout (every lane's second RoPE pair masked)."""
    if variant in "ab":
        return _variant_cfg(variant)
    base = _variant_cfg("b")
    if variant == "c":
        cfg = dataclasses.replace(base, n_fast_layer=3)
    else:
        cfg = dataclasses.replace(base, fast_n_head=4, fast_n_local_heads=2, fast_head_dim=128)
    cfg.im_end_id = base.im_end_id
    return cfg


def _launches(m, classes=("linear", "attn")):
    """Launch counts per profiler class of one eager frame on slot 0 (the host checks chain_err after it)."""
    m.profile(True)
    try:
        before = {c: m.profile_read(c)[1] for c in classes}
        m.decode([0])
        return {c: m.profile_read(c)[1] - before[c] for c in classes}
    finally:
        m.profile(False)


@pytest.mark.parametrize("variant", ["a", "b", "c", "d"])
def test_whole_frame_identity_teacher_forced(variant, knob):
    """Slow logits, fast logits and emitted columns of 7 teacher-forced frames (codes 0 and cb - 1 at codebook 0
    among them) under fast_pair 0 and 1, the graph re-captured per setting; one frame run eagerly equals its graph
    replay; once more with fattn_ilp 0 (the pair form keeps the block form of the attention, which is bit-identical
    to the loops)."""
    from fishmi.llm import DualARModel

    cfg = _pair_cfg(variant)
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, cols = _inputs(cfg, 3)
    assert 0 in cols[1] and cfg.codebook_size - 1 in cols[1]
    try:
        for ilp in (1, 0):
            knob("fattn_ilp", ilp)
            out = {}
            for v in (0, 1):
                knob("fast_pair", v)
                m.use_graph(True)
                out[v] = _forced(m, prompt, cols if ilp else cols[:, :3])
            assert np.isfinite(out[0][1]).all()
            for a, b in zip(out[0], out[1]):
                np.testing.assert_array_equal(a, b, err_msg=f"fattn_ilp {ilp}")
        knob("fattn_ilp", 1)
        res = {}
        for graph in (False, True):
            m.use_graph(graph)
            res[graph] = _forced(m, prompt, cols[:, :2])
        for a, b in zip(res[False], res[True]):
            np.testing.assert_array_equal(a, b)
    finally:
        m.use_graph(True)
        m.close()


def _sampled(m, slot, prompt, nframes=32):
    from fishmi.llm import DualARModel

    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=1234, mask_im_end=True)
    first = m.prefill(slot, prompt, sp)
    return np.concatenate([first[None], m.decode_frames([slot], nframes)[:, 0]])


@pytest.mark.parametrize("variant", ["b", "c"])
def test_sampled_streams_identical(variant, knob):
    """32 sampled frames (top_k 30, top_p 0.8, temperature 0.8, fixed seed) without host syncs: the same columns
    under fast_pair 0 and 1."""
    from fishmi.llm import DualARModel

    cfg = _pair_cfg(variant)
    m = DualARModel.synthetic(cfg, 13, 5, 0, "bf16", 1)
    prompt, _ = _inputs(cfg, 5)
    try:
        out = {}
        for v in (0, 1):
            knob("fast_pair", v)
            m.use_graph(True)
            out[v] = _sampled(m, 0, prompt)
        np.testing.assert_array_equal(out[0], out[1])
        assert len(np.unique(out[1][:, 1:])) > 8  # a sampled stream, not one repeated code
    finally:
        m.close()


def test_three_slots_one_at_a_time_and_batched(knob):
    """A handle with 3 slots: decoded one slot at a time in permuted slot order (the fast cache and the tagged
    words are per slot and per frame) the streams agree under fast_pair 0 and 1; decoded together (n = 3, where
    the pair is inert) the batched frames are unchanged by the knob."""
    from fishmi.llm import DualARModel

    cfg = _pair_cfg("b")
    m = DualARModel.synthetic(cfg, 13, 5, 0, "bf16", 3)
    prompts = [_inputs(cfg, 5 + s)[0] for s in range(3)]
    sp = DualARModel.sampling(temperature=0.8, top_p=0.8, top_k=30, seed=77, mask_im_end=True)
    order = [(2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0)]
    try:
        single, batched = {}, {}
        for v in (0, 1):
            knob("fast_pair", v)
            m.use_graph(True)
            got = {s: [m.prefill(s, prompts[s], sp)] for s in range(3)}
            for k in range(8):
                for s in order[k % len(order)]:
                    got[s].append(m.decode([s])[0])
            single[v] = np.stack([np.stack(got[s]) for s in range(3)])
            for s in range(3):
                m.prefill(s, prompts[s], sp)
            batched[v] = m.decode_frames([0, 1, 2], 6)
        np.testing.assert_array_equal(single[0], single[1])
        np.testing.assert_array_equal(batched[0], batched[1])
        assert len(np.unique(single[1][:, :, 1:])) > 8
    finally:
        m.close()


@pytest.mark.parametrize("variant", ["a", "c"])
def test_the_launches_went_away(variant, knob):
    """profile_read launch counts of one eager frame: from fast_pair 0 to 1 the "linear" class drops by the two-row
    pass's saved launches -- w1 || w3 and w2 of fast layers 0 .. n - 2 and the K / V-only wqkv of layers 1 .. n - 1,
    3 (n - 1) -- and the "attn" class by the n - 1 fused launches of codebook 0 plus its last layer's K / V-only
    attention, n.  The frames ran without a hand-off timeout (the host checks chain_err after each)."""
    from fishmi.llm import DualARModel

    cfg = _pair_cfg(variant)
    nl = cfg.n_fast_layer
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1)
    prompt, _ = _inputs(cfg, 3)
    sp = DualARModel.sampling(top_k=1)
    try:
        n = {}
        for v in (0, 1):
            knob("fast_pair", v)
            m.prefill(0, prompt, sp)
            n[v] = _launches(m)
        print("launches per frame", n)
        assert n[0]["linear"] - n[1]["linear"] == 3 * (nl - 1), n
        assert n[0]["attn"] - n[1]["attn"] == nl, n
    finally:
        m.close()


@pytest.mark.parametrize("setting", [("fast_tail", 0), ("fattn_wo", 0), ("rowgemv", 27), ("rowgemv", 59), ("rowgemv", 91),
                                     ("int8", 0)])
def test_fallbacks_leave_the_frame_alone(setting, knob):
    """Where a precondition of the pair fails -- fast_tail 0, fattn_wo 0, rowgemv without bit 5 or 6, an int8
    handle -- the knob changes nothing: the same launch counts and the same bits."""
    from fishmi.llm import DualARModel

    key, val = setting
    cfg = _pair_cfg("a")
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", 1, **({"quant": "int8"} if key == "int8" else {}))
    prompt, cols = _inputs(cfg, 3)
    sp = DualARModel.sampling(top_k=1)
    try:
        if key != "int8":
            knob(key, val)
        out, n = {}, {}
        for v in (0, 1):
            knob("fast_pair", v)
            m.use_graph(True)
            out[v] = _forced(m, prompt, cols[:, :4])
            m.prefill(0, prompt, sp)
            n[v] = _launches(m)
        assert n[0] == n[1], n
        for a, b in zip(out[0], out[1]):
            np.testing.assert_array_equal(a, b)
    finally:
        m.close()


# ---- per-op: each two-row kernel form against the one-row production launcher, row by row ------------------

def _operands(seed, N, K, rows=2):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    x = rng.standard_normal((rows, K)).astype(np.float32)
    return rng, w, x


# K: one chunk per wave | uneven shares, a tail slot | the deep (w2) form, which has no gathered instantiation
@pytest.mark.parametrize("K,gather", [(1024, False), (1024, True), (2560, False), (2560, True), (10240, False)])
def test_op_two_row_fin(K, gather):
    """wo / w2 form (2 rows per block, N = 2 RP): both rows of the two-row launch equal the one-row launcher's
    outputs, row 1's residual gathered from a table (with an index past its end: the clamp) or not; the padding
    past N stays untouched."""
    from fishmi import ops

    N, ld = 4, 12
    rng, w, x = _operands(K, N, K)
    bias = rng.standard_normal(N).astype(np.float32)
    res0 = rng.standard_normal(N).astype(np.float32)
    tab = rng.standard_normal((5, N)).astype(np.float32)
    for idx in ([3, 1], [3, 9]) if gather else (None,):
        res1 = tab if gather else tab[:1]
        y2 = np.full((2, ld), SENT, np.float32)
        ops.rowgemv_pair(w, x, y2, 0, bias=bias, res0=res0, res1=res1, idx=idx, idx_col=1 if gather else 0)
        y0 = np.full(ld, SENT, np.float32)
        ops.rowgemv(w, x[0], y0, 0, bias=bias, res=res0[None])
        y1 = np.full(ld, SENT, np.float32)
        ops.rowgemv(w, x[1], y1, 0, bias=bias, res=res1, idx=idx, idx_col=1 if gather else 0)
        np.testing.assert_array_equal(y2[0], y0)
        np.testing.assert_array_equal(y2[1], y1)
        assert (y2[:, N:] == SENT).all() and not (y2[:, :N] == SENT).any()


@pytest.mark.parametrize("K", [1024, 2560])
@pytest.mark.parametrize("N,skip0", [(16, 8), (40, 20), (16, 0)])  # N = 2 RP | a count inside a block | none skipped
def test_op_two_row_norm_store(K, N, skip0):
    """wqkv form (RMSNorm prologue, 8 rows per block): row 1 equals the one-row launcher's output everywhere, row 0
    from skip0 on; row 0's outputs below skip0 (the Q rows) and the padding past N stay untouched."""
    from fishmi import ops

    ld = N + 8
    rng, w, x = _operands(K + N, N, K)
    x[1] *= 3.0  # two different statistics
    nw = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    for bias in (None, rng.standard_normal(N).astype(np.float32)):
        y2 = np.full((2, ld), SENT, np.float32)
        ops.rowgemv_pair(w, x, y2, 1, bias=bias, nw=nw, eps=1e-5, skip0=skip0)
        for r in range(2):
            y = np.full(ld, SENT, np.float32)
            ops.rowgemv(w, x[r], y, 1, bias=bias, nw=nw, eps=1e-5)
            lo = skip0 if r == 0 else 0
            np.testing.assert_array_equal(y2[r, lo:], y[lo:])
            assert (y2[r, :lo] == SENT).all() and not (y2[r, lo:N] == SENT).any()


@pytest.mark.parametrize("K", [512, 2560])
def test_op_two_row_tile_swiglu(K):
    """w1 || w3 on the 16-row tile kernel with the statistic from the staged rows (ss_gran 1) at R = 2: each row
    equals the R = 1 launch of that row; the spare row and the padding columns stay untouched."""
    from fishmi import ops

    N = 32
    rng, w, x = _operands(K + 7, N, K)
    x[1] *= 0.25
    nw = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y2 = np.full((3, N // 2 + 8), SENT, np.float32)
    ops.gemv(w, x, y2, pro=ops.PRO_PRENORM, epi=ops.EPI_SWIGLU8, nw=nw, eps=1e-5, ss_gran=1)
    for r in range(2):
        y = np.full((2, N // 2 + 8), SENT, np.float32)
        ops.gemv(w, x[r:r + 1], y, pro=ops.PRO_PRENORM, epi=ops.EPI_SWIGLU8, nw=nw, eps=1e-5, ss_gran=1)
        np.testing.assert_array_equal(y2[r], y[0])
    assert (y2[2] == SENT).all() and (y2[:, N // 2:] == SENT).all() and not (y2[:2, :N // 2] == SENT).any()


def test_wide_bf16_vs_reference_under_default(golden, knob):
    """S2-Pro widths (2 + 1 layers, qk-norm) under the default (fast_pair 1, rowgemv 123): teacher-forced logits
    within the bf16 bound of the reference."""
    from fishmi.llm import DualARModel

    knob("rowgemv", 123)
    knob("fast_pair", 1)
    g = golden("llm_wide_bf16.npz")
    cfg = _cfg("llm_wide")
    m = DualARModel.synthetic(cfg, int(g["synth_seed"]), int(g["log2_half"]), 0, "bf16", 1)
    try:
        T = g["prompt"].shape[1]
        slow, fast = m.teacher_decode(g["prompt"], g["seq"][:, T:])
        _bf16_vs_reference(slow, fast, g, rows=g["slow_rows"])
    finally:
        m.close()
