"""Compact weight-only handles (fm_llm_set_quant_compact): a quantised handle that keeps only
its codes must compute, bit for bit, what the same handle computes with the bf16 fragment copy of every
quantised linear beside them -- the 16-row MFMA tile kernel's code-reading forms rebuild each bf16 fragment
from the step-granular codes (Frag::dq8s / dq4s) and run the steps, the reductions and the epilogues of the
bf16 form, so every comparison between the two is array_equal.  Model level on test_gpu_fast_deadwork_quant's
layout (dim 512, 8 / 2 heads x 64, 2 + 2 layers, untied head, int4 groups of 128; max_seq_len raised to 128 for
the 100-token prompt), op level through fm_op_linear_q, the byte accounting of fm_llm_memory_info, and the
host-side refusals.  Run on the MI355X box: pytest -m gpu."""
import ctypes
import dataclasses

import numpy as np
import pytest

from fishmi import native, ops
from linear_ref import mk as _mk, v_acc, v_add, v_q8, v_rnd
from parity_util import knob  # noqa: F401  (fixture)
from test_gpu_fast_deadwork import _variant_cfg
from test_gpu_linear_ops import _buf, _check, _linear_ref, _same, _sentinel

pytestmark = pytest.mark.gpu

GS = 128
QUANTS = ["int8", "int4"]
FM_ERR_ARG, FM_ERR_STATE = -1, -3


def _cfg():
    return dataclasses.replace(_variant_cfg("b"), max_seq_len=128)


def _pair(quant, max_slots=1, seed=11):
    """(config, non-compact handle, compact handle) from the same seed"""
    from fishmi.llm import DualARModel

    cfg = _cfg()
    mk = lambda c: DualARModel.synthetic(cfg, seed, 5, 0, "bf16", max_slots, quant=quant, groupsize=GS, compact=c)  # noqa: E731
    return cfg, mk(False), mk(True)


def _tokens(cfg, T, nf, seed):
    """a T-token text prompt and nf forced columns (codes 0 and cb - 1 among them)"""
    rng = np.random.default_rng(seed)
    C1 = cfg.num_codebooks + 1
    prompt = np.zeros((C1, T), np.int32)
    prompt[0] = rng.integers(16, cfg.semantic_begin_id, T)
    cols = np.zeros((C1, nf), np.int32)
    cols[0] = rng.integers(cfg.semantic_begin_id, cfg.semantic_end_id + 1, nf)
    cols[1:] = rng.integers(0, cfg.codebook_size, (C1 - 1, nf))
    cols[1::2, 1] = 0
    cols[2::2, 1] = cfg.codebook_size - 1
    return prompt, cols


def _forced(m, prompt, cols, slot=0):
    """teacher-forced prefill + frames on the production path: slow logits, fast logits, emitted columns"""
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


def _equal(a, b, msg):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=msg)


# ------------------------------------------------------------------------------------------ 1. one slot
@pytest.mark.parametrize("quant", QUANTS)
def test_one_slot_every_bit(quant):
    """Teacher-forced prefill + 4 frames at prompt lengths 5 (the GEMV path), 20 (<2, .>), 40 and 64 (one 64-row
    group of <4, .>), 65 and 100 (a second group with a ragged tail): slow logits, fast logits and emitted columns
    equal between the handles; slot 0's K / V rows of slow layer 0 equal after the 100-token prompt; an eager frame
    equals its graph replay on the compact handle."""
    cfg, ref, cmp_ = _pair(quant)
    try:
        assert cmp_.memory_info()["quant_fragments"] == 0 < ref.memory_info()["quant_fragments"]
        for T in (5, 20, 40, 64, 65, 100):
            prompt, cols = _tokens(cfg, T, 5, 100 + T)
            a, b = _forced(ref, prompt, cols), _forced(cmp_, prompt, cols)
            assert np.isfinite(a[1]).all() and np.isfinite(a[0][:, cfg.semantic_begin_id:cfg.semantic_end_id + 1]).all()
            _equal(a, b, f"{quant} T={T}")
        for x, y in zip(ref.read_cache(0), cmp_.read_cache(0)):
            np.testing.assert_array_equal(x[:, :104], y[:, :104])
            assert np.abs(x[:, :104]).max() > 0
        prompt, cols = _tokens(cfg, 20, 3, 7)
        res = {}
        for graph in (False, True):
            cmp_.use_graph(graph)
            res[graph] = _forced(cmp_, prompt, cols)
        _equal(res[False], res[True], "eager vs graph")
    finally:
        cmp_.use_graph(True)
        ref.close()
        cmp_.close()


def test_int8_checkpoint_compact(golden):
    """The int8 checkpoint quantize.py writes (FM_DT_I8 tensors + scales, never expanded to bf16 on a compact handle),
    loaded with and without compact=True: the teacher-forced logits of its golden stream are equal, no fragment copy
    is held, and a bf16 checkpoint refuses the flag (ValueError, no quant)."""
    import os

    from conftest import GOLDEN
    from fishmi.llm import DualARModel
    from test_gpu_int8 import IM_END

    path = os.path.join(GOLDEN, "llm_q_int8")
    g = golden("llm_q_int8_bf16.npz")
    T = g["prompt"].shape[1]
    out = []
    for compact in (False, True):
        m = DualARModel.from_pretrained(path, 0, "bf16", 1, im_end_id=IM_END, compact=compact)
        try:
            assert m.quant == "int8" and m.compact is compact
            assert (m.memory_info()["quant_fragments"] == 0) is compact
            out.append(m.teacher_decode(g["prompt"], g["seq"][:, T:T + 6]))
        finally:
            m.close()
    _equal(out[0], out[1], "int8 checkpoint")
    with pytest.raises(ValueError):
        DualARModel.from_pretrained(os.path.join(GOLDEN, "llm_a"), 0, "bf16", 1, im_end_id=IM_END, compact=True)


@pytest.mark.parametrize("quant", QUANTS)
def test_prompt_pass_books_code_bytes(quant):
    """profile_read over a 40-token prefill: the same "linear" launches on both handles, and on the compact one
    every slow-stack linear of the prompt chunk (the tile kernel's code form) is booked at its code bytes -- int8
    N K + 2 N, int4 N K / 2 + 4 N K / 128 -- instead of 2 N K; the one-row launches after it stream codes on both."""
    from fishmi.llm import DualARModel

    cfg, ref, cmp_ = _pair(quant)
    prompt, _ = _tokens(cfg, 40, 2, 9)
    try:
        got = []
        for m in (ref, cmp_):
            m.profile(True)
            try:
                m.prefill(0, prompt, DualARModel.sampling(top_k=1))
                got.append(m.profile_read("linear")[1:])
            finally:
                m.profile(False)
        (n0, b0), (n1, b1) = got
        d, nq, inter = cfg.dim, cfg.n_head * cfg.head_dim, cfg.intermediate_size
        shapes = cfg.n_layer * [((cfg.n_head + 2 * cfg.n_local_heads) * cfg.head_dim, d), (d, nq), (2 * inter, d), (d, inter)]
        code = (lambda N, K: N * K + 2 * N) if quant == "int8" else (lambda N, K: N * K // 2 + N * (K // 128) * 4)
        assert n0 == n1 > 0 and b0 - b1 == sum(2 * N * K - code(N, K) for N, K in shapes), (got, shapes)
    finally:
        ref.close()
        cmp_.close()


# ------------------------------------------------------------------------------------------ 2. twelve slots
NS = 12


def _batched(m, cfg, prompts, cols):
    """prefill_batch of the ragged prompts, then 4 batched frames, every slot teacher-forced: per frame the slow
    and fast logits of every slot, and the emitted columns"""
    from fishmi.llm import DualARModel

    slots = list(range(NS))
    sps = [DualARModel.sampling(top_k=1) for _ in slots]
    sl, fl, em = [], [], []
    try:
        for k in range(cols[0].shape[1]):
            for s in slots:
                m.force(s, cols[s][:, k])
            em.append(m.prefill_batch(slots, prompts, sps) if k == 0 else m.decode(slots))
            lg = [m.read_logits(s) for s in slots]
            sl.append(np.stack([x[0] for x in lg]))
            fl.append(np.stack([x[1] for x in lg]))
    finally:
        for s in slots:
            m.force(s, None)
    return np.stack(sl), np.stack(fl), np.stack(em)


@pytest.mark.parametrize("quant", QUANTS)
def test_twelve_slots_every_bit_and_knobs(quant, knob):
    """12 ragged prompts of 3-90 tokens through prefill_batch, then 4 batched frames: equal to the non-compact
    handle; and on the compact handle each knob that would pick a reader of the bf16 copy (the graph re-captured
    under it) gives finite outputs equal to the compact handle's own default-knob output."""
    cfg, ref, cmp_ = _pair(quant, max_slots=NS)
    rng = np.random.default_rng(5)
    lens = [3, 90] + [int(t) for t in rng.integers(3, 91, NS - 2)]
    toks = [_tokens(cfg, T, 5, 300 + i) for i, T in enumerate(lens)]
    prompts, cols = [t[0] for t in toks], [t[1] for t in toks]
    sem = slice(cfg.semantic_begin_id, cfg.semantic_end_id + 1)
    try:
        base = _batched(cmp_, cfg, prompts, cols)
        assert np.isfinite(base[1]).all() and np.isfinite(base[0][:, :, sem]).all()
        _equal(_batched(ref, cfg, prompts, cols), base, f"{quant} compact vs non-compact")
        qk = "bstream_q8" if quant == "int8" else "bstream_q4"
        for key, val in (("bstream", 0), ("bstream_acc", 0), (qk, 0), ("int4_stream", 0), ("bstream_chain", 1)):
            default = native.tune_get(key)
            knob(key, val)
            cmp_.use_graph(True)  # re-capture the frame under the knob
            got = _batched(cmp_, cfg, prompts, cols)
            knob(key, default)
            assert np.isfinite(got[1]).all() and np.isfinite(got[0][:, :, sem]).all(), key
            _equal(got, base, f"{quant} {key} {val}")
    finally:
        ref.close()
        cmp_.close()


@pytest.mark.parametrize("max_slots", [1, NS])
@pytest.mark.parametrize("quant", QUANTS)
def test_decode_frames_run_the_same_launches(quant, max_slots):
    """profile_read over one eager decode frame of all the handle's slots: the compact handle's "linear" and "attn"
    launch counts and booked bytes are the non-compact handle's (the decode frames read codes on both)."""
    from fishmi.llm import DualARModel

    cfg, ref, cmp_ = _pair(quant, max_slots=max_slots)
    slots = list(range(max_slots))
    prompts = [_tokens(cfg, 6 + s, 2, 40 + s)[0] for s in slots]
    sps = [DualARModel.sampling(top_k=1) for _ in slots]
    try:
        got = []
        for m in (ref, cmp_):
            m.prefill_batch(slots, prompts, sps)
            m.profile(True)
            try:
                before = {c: m.profile_read(c)[1:] for c in ("linear", "attn")}
                m.decode(slots)
                after = {c: m.profile_read(c)[1:] for c in ("linear", "attn")}
            finally:
                m.profile(False)
            got.append({c: (after[c][0] - before[c][0], after[c][1] - before[c][1]) for c in after})
        assert got[0]["linear"][0] > 0 and got[0] == got[1], got
    finally:
        ref.close()
        cmp_.close()


HANDLES = {"bf16": (None, False), "int8": ("int8", False), "int4": ("int4", False),
           "int8_compact": ("int8", True), "int4_compact": ("int4", True)}
MEM = ("quant_fragments", "gemv_codes", "step_codes", "row_major", "other_weights", "kv_cache", "activations", "total")
# (handle, max_slots) -> memory_info() in MEM's order, then [launches, bytes] of prefill "linear", prefill "attn",
# decode "linear", decode "attn"
BOOKED = {
    ("bf16", 1): ((0, 0, 0, 17891328, 19442688, 137216, 84685920, 122157152),
                  [40, 45156352], [12, 5242880], [40, 45012992], [12, 5242880]),
    ("bf16", 12): ((0, 0, 0, 17891328, 19442688, 1646592, 86859072, 125839680),
                   [62, 70390832], [36, 0], [62, 67521584], [14, 0]),
    ("int8", 1): ((17973248, 9075776, 0, 8962048, 1469440, 137216, 84685920, 122303648),
                  [43, 29376640], [14, 2894848], [43, 24780928], [14, 2894848]),
    ("int8", 12): ((17973248, 9075776, 8986624, 8962048, 1469440, 1646592, 86859072, 134972800),
                   [62, 42884402], [36, 0], [62, 35463474], [14, 0]),
    ("int4", 1): ((17973248, 4774144, 0, 4752384, 1469440, 137216, 84685920, 113792352),
                  [43, 19872256], [14, 1531904], [43, 13183488], [14, 1531904]),
    ("int4", 12): ((17973248, 4774144, 4493312, 4752384, 1469440, 1646592, 86859072, 121968192),
                   [62, 30165312], [36, 0], [62, 20640064], [14, 0]),
    ("int8_compact", 1): ((0, 9075776, 8986624, 8962048, 977920, 137216, 84685920, 112825504),
                          [43, 24935552], [14, 2894848], [43, 24780928], [14, 2894848]),
    ("int8_compact", 12): ((0, 9075776, 8986624, 8962048, 977920, 1646592, 86859072, 116508032),
                           [62, 38443314], [36, 0], [62, 35463474], [14, 0]),
    ("int4_compact", 1): ((0, 4774144, 4493312, 4752384, 977920, 137216, 84685920, 99820896),
                          [43, 13326848], [14, 1531904], [43, 13183488], [14, 1531904]),
    ("int4_compact", 12): ((0, 4774144, 4493312, 4752384, 977920, 1646592, 86859072, 103503424),
                           [62, 23619904], [36, 0], [62, 20640064], [14, 0]),
}


def _booked(handle, max_slots):
    """the handle's memory_info() and the profile_read deltas [launches, bytes] of "linear" and "attn" over
    prefill_batch of the slots' 6 + s-token prompts, then over one eager decode of all slots"""
    from fishmi.llm import DualARModel

    quant, compact = HANDLES[handle]
    cfg = _cfg()
    m = DualARModel.synthetic(cfg, 11, 5, 0, "bf16", max_slots, quant=quant, groupsize=GS, compact=compact)
    slots = list(range(max_slots))
    prompts = [_tokens(cfg, 6 + s, 2, 40 + s)[0] for s in slots]
    sps = [DualARModel.sampling(top_k=1) for _ in slots]
    read = lambda: {c: m.profile_read(c)[1:] for c in ("linear", "attn")}  # noqa: E731
    delta = lambda a, b: {c: [b[c][0] - a[c][0], b[c][1] - a[c][1]] for c in a}  # noqa: E731
    try:
        out = {"memory": m.memory_info()}
        m.profile(True)
        try:
            r0 = read()
            m.prefill_batch(slots, prompts, sps)
            r1 = read()
            m.decode(slots)
            r2 = read()
        finally:
            m.profile(False)
        out["prefill"], out["decode"] = delta(r0, r1), delta(r1, r2)
        return out
    finally:
        m.close()


@pytest.mark.parametrize("max_slots", [1, NS])
@pytest.mark.parametrize("handle", list(HANDLES))
def test_booked_figures(handle, max_slots):
    """The absolute figures the handle books: every memory_info() class, and the "linear" / "attn" launch counts and
    bytes of a batched prefill and of one eager decode frame, equal to the integers recorded on the MI355X from
    commit 471cf80 (compact weight-only handles), the last one before each linear became one Linear record: the
    weight-byte formula of every layout and the byte class of every buffer are unchanged."""
    got = _booked(handle, max_slots)
    print(handle, max_slots, got)
    mem, pl, pa, dl, da = BOOKED[(handle, max_slots)]
    assert got == {"memory": dict(zip(MEM, mem)), "prefill": {"linear": pl, "attn": pa},
                   "decode": {"linear": dl, "attn": da}}


# ------------------------------------------------------------------------------------------ 3. op level
EPIS = {"store": ops.EPI_STORE, "resid": ops.EPI_RESID, "f32": ops.EPI_F32}


def _dequant4(q, scale, zero):
    """bf16(fma(q - 8, scale, zero)) of the returned codes and group tables: exact in float64, rounded once to
    fp32 (the fma) and then to bf16 (RNE), as Frag::dq4 does"""
    from fishmi.synth import round_bf16

    g = q.shape[1] // scale.shape[1]
    exact = (q.astype(np.float64) - 8.0) * np.repeat(scale, g, 1).astype(np.float64) + np.repeat(zero, g, 1)
    return round_bf16(exact.astype(np.float32))


def _ref_q(quant, epi, x, q, scale, zero, res):
    """test_gpu_linear_ops's bound over the returned codes and scales (int8: round(round(acc) * scale), then the
    epilogue's roundings; int4: the plain bf16 linear on the dequantised weights)"""
    if quant == "int4":
        return _linear_ref(epi, x, _dequant4(q, scale, zero), None, None, res, "bf16")
    a = v_q8(v_acc(x, q.astype(np.float32)), scale[None, :].astype(np.float64), "bf16")
    if epi == ops.EPI_RESID:
        return v_rnd(v_add(a, res.astype(np.float64)), "bf16")
    return a  # (store / fp32 of an already rounded value: no further rounding)


def _op_case(quant, epi_name, R, N, K, seed, split=False):
    rng = np.random.default_rng(seed)
    epi = EPIS[epi_name]
    ldx, ldy, ldr = K + 8, N + 5, N + 3
    x = _mk(rng, (R, ldx), "bf16")
    w = _mk(rng, (N, K), "bf16", K ** -0.5)
    res = _mk(rng, (R, ldr), "bf16") if epi == ops.EPI_RESID else None
    tag = f"linear_q {quant} {epi_name} R={R} N={N} K={K} split={int(split)}"
    outs = []
    for reps in (1, 3):
        yq, yb = _buf(R + 2, ldy), _buf(R + 2, ldy)
        ksb, dirty, q, sc, zr = ops.linear_q(w, x, yq, yb, quant, epi, gs=GS, res=res, split=split, reps=reps)
        assert dirty == 0, (tag, reps, dirty)
        _same(tag + " codes vs bf16", yq, yb)
        _sentinel(tag, yq, R, N)
        _sentinel(tag, yb, R, N)
        outs.append(yb)
    _same(tag + " reps", outs[0], outs[1])
    v = _ref_q(quant, epi, x[:, :K], q, sc, zr, None if res is None else res[:, :N])
    _check(tag, f"linear_q/{quant}/{epi_name}", outs[0][:R, :N], v)
    return ksb


@pytest.mark.parametrize("epi_name", list(EPIS))
@pytest.mark.parametrize("quant", QUANTS)
def test_op_codes_equal_bf16(quant, epi_name):
    """fm_op_linear_q: N 16 / 40 (a ragged last tile) / 272, K 128 / 384 / 1024, R across the 1 / 2 / 4 column-group
    kernels and the second 64-row group: the code form's output equals the bf16 form's, the sentinel padding is
    untouched, reps = 3 is bit-identical with no ticket left, and the output lies within test_gpu_linear_ops's
    bound of the float64 product over the returned codes and scales."""
    i = 0
    for N in (16, 40, 272):
        for K in (128, 384, 1024):
            for R in (9, 16, 17, 32, 33, 64, 65, 100):
                i += 1
                ksb = _op_case(quant, epi_name, R, N, K, 1000 * i + R)
                assert ksb == 1


@pytest.mark.parametrize("quant", QUANTS)
def test_op_split_k(quant, knob):
    """split K (8 < R <= 64, fm_tune linear_fill raised until K = 1024 really splits): the partials, the ticketed
    last-slice reduction and the ticket reset are the bf16 form's, so the same assertions hold with ksb > 1."""
    for N, fill in ((40, 6), (272, 34)):
        knob("linear_fill", fill)
        for j, epi_name in enumerate(EPIS):
            for R in (9, 16, 17, 32, 33, 64):
                ksb = _op_case(quant, epi_name, R, N, 1024, 77 * R + N + j, split=True)
                assert ksb > 1, (N, R, ksb)


# ------------------------------------------------------------------------------------------ 4. accounting
def _quant_linears(cfg):
    """(N, K) of every quantised linear as the handle holds it: per layer wqkv, wo, w1 || w3 (one 2 * inter-row
    matrix) and w2 of both stacks, the codebook head, and the untied slow head's constrained rows"""
    def stack(n, dim, nh, nkv, hd, inter):
        return n * [((nh + 2 * nkv) * hd, dim), (dim, nh * hd), (2 * inter, dim), (dim, inter)]

    out = stack(cfg.n_layer, cfg.dim, cfg.n_head, cfg.n_local_heads, cfg.head_dim, cfg.intermediate_size)
    out += stack(cfg.n_fast_layer, cfg.fast_dim, cfg.fast_n_head, cfg.fast_n_local_heads, cfg.fast_head_dim,
                 cfg.fast_intermediate_size)
    out.append((cfg.codebook_size, cfg.fast_dim))
    assert not cfg.tie_word_embeddings and cfg.fast_dim == cfg.dim  # an untied head; no fast_project_in
    out.append((cfg.semantic_end_id - cfg.semantic_begin_id + 2, cfg.dim))
    return out


@pytest.mark.parametrize("max_slots", [1, 12])
@pytest.mark.parametrize("quant", QUANTS)
def test_memory_accounting(quant, max_slots):
    cfg, ref, cmp_ = _pair(quant, max_slots=max_slots)
    try:
        a, b = ref.memory_info(), cmp_.memory_info()
        print(quant, max_slots, a, b)
        pad = lambda n: (n + 15) // 16 * 16  # noqa: E731
        weights = sum(pad(N) * K for N, K in _quant_linears(cfg))
        assert a["quant_fragments"] == 2 * weights and b["quant_fragments"] == 0
        assert a["gemv_codes"] == b["gemv_codes"] > 0 and a["row_major"] == b["row_major"] > 0
        assert b["step_codes"] == (weights if quant == "int8" else weights // 2)
        assert a["step_codes"] == (b["step_codes"] if max_slots > 8 else 0)
        assert a["kv_cache"] == b["kv_cache"] > 0 and a["activations"] == b["activations"] > 0
        for d in (a, b):
            assert d["total"] == sum(v for k, v in d.items() if k != "total")
        assert b["total"] < a["total"]
    finally:
        ref.close()
        cmp_.close()


def test_memory_info_unquantised():
    from fishmi.llm import DualARModel

    m = DualARModel.synthetic(_cfg(), 11, 5, 0, "bf16", 1)
    try:
        d = m.memory_info()
        assert d["quant_fragments"] == d["gemv_codes"] == d["step_codes"] == 0
        assert d["other_weights"] > 2 * sum(N * K for N, K in _quant_linears(_cfg()))  # the packed weights
        assert d["total"] == sum(v for k, v in d.items() if k != "total")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 5. refusals
def _open(cfg, precision):
    L = native.lib()
    c = cfg.to_c()
    h = ctypes.c_void_p()
    native.check(L.fm_llm_open(ctypes.byref(c), 0, native.FM_PREC_BF16 if precision == "bf16" else native.FM_PREC_FP32,
                               1, ctypes.byref(h)))
    return L, h


def test_refusals():
    """All on the host, nothing launched: compact on fp32 (FM_ERR_ARG); before set_quant and after a set_tensor
    (FM_ERR_STATE); int4 group 64 at finalize (FM_ERR_ARG, the tensor named, the handle left as it was); compact
    without quant from Python (ValueError)."""
    from fishmi.llm import DualARModel

    cfg = _cfg()
    L, h = _open(cfg, "fp32")
    try:
        native.check(L.fm_llm_set_quant(h, native.FM_QUANT_INT8))
        assert L.fm_llm_set_quant_compact(h, 1) == FM_ERR_ARG
    finally:
        L.fm_llm_close(h)
    L, h = _open(cfg, "bf16")
    try:
        assert L.fm_llm_set_quant_compact(h, 1) == FM_ERR_STATE  # unquantised
        native.check(L.fm_llm_set_quant(h, native.FM_QUANT_INT8))
        native.check(L.fm_llm_synth_tensor(h, b"norm.weight", cfg.dim, 1, 1.0, 5))
        assert L.fm_llm_set_quant_compact(h, 1) == FM_ERR_STATE  # after a tensor
    finally:
        L.fm_llm_close(h)
    m = DualARModel(cfg, 0, "bf16", 1, quant="int4", groupsize=64, compact=True)
    try:
        m.synth(11, 5)
        with pytest.raises(native.FishMIError) as e:
            m.finalize()
        assert e.value.code == FM_ERR_ARG and ".weight" in str(e.value) and "group size 64" in str(e.value)
        out = (ctypes.c_int64 * 8)()
        assert L.fm_llm_memory_info(m.h, out) == FM_ERR_STATE  # still not finalized
    finally:
        m.close()
    with pytest.raises(ValueError):
        DualARModel(cfg, 0, "bf16", 1, compact=True)
    with pytest.raises(ValueError):
        DualARModel.synthetic(cfg, 11, compact=True)
