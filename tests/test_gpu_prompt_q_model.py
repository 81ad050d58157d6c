"""Weight-only int8 / int4 handles on the skinny prompt GEMM (fm_tune prompt_skinny_q; linears of 33 .. 64 rows),
model level, on test_gpu_quant_compact's layout (dim 512, 8 / 2 heads x 64, 2 + 2 layers, int4 groups of 128,
max_seq_len 128).  The code forms rebuild the bf16 copy's bits and keep mode 0's slices and steps, so every handle
kind -- bf16 copy only, codes under either knob value, compact -- must give the same bits; against the old routing
(prompt_skinny_q 2: the 16-row tile kernel) only the order of the fp32 sums differs, which is held to parity_util's
bf16 bound with the handle's own fp32-mode run as the truth.  Run on the MI355X box: pytest -m gpu."""
import dataclasses

import numpy as np
import pytest

from parity_util import bf16_vs_reference, knob  # noqa: F401  (knob: fixture)
from test_gpu_fast_deadwork import _variant_cfg
from test_gpu_quant_compact import GS, QUANTS, _equal, _forced, _tokens

pytestmark = pytest.mark.gpu


def _cfg():
    return dataclasses.replace(_variant_cfg("b"), max_seq_len=128)


def _open(cfg, quant, max_slots=1, compact=False, precision="bf16"):
    from fishmi.llm import DualARModel

    return DualARModel.synthetic(cfg, 11, 5, 0, precision, max_slots, quant=quant, groupsize=GS, compact=compact)


def _prompt_q(m, prompt):
    """the code-streaming skinny launches of one prefill"""
    from fishmi.llm import DualARModel

    m.profile(True)
    try:
        m.prefill(0, prompt, DualARModel.sampling(top_k=1))
        return m.profile_read("prompt_q")[1]
    finally:
        m.profile(False)


@pytest.mark.parametrize("T", [40, 64])
@pytest.mark.parametrize("quant", QUANTS)
def test_every_handle_kind_every_bit(quant, T, knob):
    """Teacher-forced prefill + 3 frames: (1) a 1-slot handle (no step-granular copy: mode 0 on the bf16 copy, int8
    with the row scales in the epilogues), (2) a 12-slot handle on its codes, (3) the same handle on its bf16 copy,
    (4) a compact handle -- equal slow logits, fast logits and columns.  The "prompt_q" class counts the four
    linears of every slow layer on (2) and (4), nothing on (1), and nothing anywhere under the old routing."""
    cfg = _cfg()
    one, twelve, compact = _open(cfg, quant), _open(cfg, quant, 12), _open(cfg, quant, 1, True)
    prompt, cols = _tokens(cfg, T, 4, 500 + T)
    sem = slice(cfg.semantic_begin_id, cfg.semantic_end_id + 1)
    try:
        knob("prompt_skinny_q", 1)
        base = _forced(one, prompt, cols)
        assert np.isfinite(base[1]).all() and np.isfinite(base[0][:, sem]).all()
        _equal(_forced(twelve, prompt, cols), base, f"{quant} T={T}: codes (12 slots)")
        _equal(_forced(compact, prompt, cols), base, f"{quant} T={T}: compact")
        assert [_prompt_q(m, prompt) for m in (one, twelve, compact)] == [0, 4 * cfg.n_layer, 4 * cfg.n_layer]
        knob("prompt_skinny_q", 0)
        _equal(_forced(twelve, prompt, cols), base, f"{quant} T={T}: bf16 copy (12 slots)")
        _equal(_forced(compact, prompt, cols), base, f"{quant} T={T}: compact ignores 0")
        assert [_prompt_q(m, prompt) for m in (one, twelve, compact)] == [0, 0, 4 * cfg.n_layer]
        knob("prompt_skinny_q", 2)
        assert [_prompt_q(m, prompt) for m in (one, twelve, compact)] == [0, 0, 0]
        old = _forced(twelve, prompt, cols)
        _equal(_forced(compact, prompt, cols), old, f"{quant} T={T}: old routing, compact vs not")
    finally:
        for m in (one, twelve, compact):
            m.close()


@pytest.mark.parametrize("T", [40, 64])
def test_new_route_against_old_route(T, knob):
    """int8: the skinny route and the old routing differ by reordered fp32 sums only.  Truth: the same int8 model in
    fp32 compute; the skinny route's error against it is held to 1.5 x the old routing's own (RMS and max), with
    the argmax equal wherever the truth's top-2 margin exceeds twice the larger error (parity_util)."""
    cfg = _cfg()
    prompt, cols = _tokens(cfg, T, 4, 600 + T)
    f32, m = _open(cfg, "int8", precision="fp32"), _open(cfg, "int8", 12)
    try:
        ts, tf, _ = _forced(f32, prompt, cols)
        knob("prompt_skinny_q", 2)
        rs, rf, _ = _forced(m, prompt, cols)
        knob("prompt_skinny_q", 1)
        slow, fast, _ = _forced(m, prompt, cols)
        assert _prompt_q(m, prompt) == 4 * cfg.n_layer
        out = bf16_vs_reference(slow, fast, rs, rf, ts, tf)
        assert out["top1_checked"] > 0
    finally:
        f32.close()
        m.close()


def test_forty_slot_batched_frame(knob):
    """A batched decode frame of 40 slots reaches the same linears with 40 rows (both stacks): after 40 short
    prefills, one teacher-forced frame on the codes equals the same frame on the bf16 copy, and the route ran."""
    from fishmi.llm import DualARModel

    cfg, NS = _cfg(), 40
    m = _open(cfg, "int8", NS)
    slots = list(range(NS))
    toks = [_tokens(cfg, 3 + s % 4, 2, 700 + s) for s in slots]
    prompts, cols = [t[0] for t in toks], [t[1] for t in toks]
    sps = [DualARModel.sampling(top_k=1) for _ in slots]

    def frame():
        m.use_graph(True)  # re-capture the frame under the knob in force
        try:
            for s in slots:
                m.force(s, cols[s][:, 0])
            m.prefill_batch(slots, prompts, sps)
            for s in slots:
                m.force(s, cols[s][:, 1])
            em = m.decode(slots)
            lg = [m.read_logits(s) for s in slots]
        finally:
            for s in slots:
                m.force(s, None)
        return np.stack([x[0] for x in lg]), np.stack([x[1] for x in lg]), em

    try:
        knob("prompt_skinny_q", 1)
        a = frame()
        m.profile(True)
        try:
            m.decode(slots)
            assert m.profile_read("prompt_q")[1] >= 4 * cfg.n_layer
        finally:
            m.profile(False)
        knob("prompt_skinny_q", 0)
        b = frame()
        assert np.isfinite(a[1]).all()
        _equal(a, b, "40-slot frame: codes vs bf16 copy")
    finally:
        m.close()


def test_decode_written_kv_rows_int8(knob):
    """test_gpu_engine.test_decode_written_kv_rows on the int8 handle at 40 positions: the K / V rows ten decode
    frames wrote after a 30-token prompt against the rows one 40-row prompt pass (the code-streaming skinny route)
    writes -- at most 1 % of the elements differ, by at most 2 bf16 ulps (that test's bound: the K order of the
    accumulation differs between the one-row kernels and any prompt GEMM)."""
    cfg = _cfg()
    T, n = 30, 11
    prompt, cols = _tokens(cfg, T, n, 800)
    m = _open(cfg, "int8", 12)
    sp = m.sampling(top_k=1)
    knob("prompt_skinny_q", 1)
    try:
        for i in range(n):
            m.force(0, cols[:, i])
            if i == 0:
                m.prefill(0, prompt, sp)
            else:
                m.decode([0])
        dec = [m.read_cache(l) for l in range(cfg.n_layer)]
        m.force(0, cols[:, n - 1])
        assert _prompt_q(m, np.concatenate([prompt, cols[:, : n - 1]], axis=1)) == 4 * cfg.n_layer
        m.force(0, None)
        pro = [m.read_cache(l) for l in range(cfg.n_layer)]
    finally:
        m.close()
    d = [(x[:, T:T + n - 1], y[:, T:T + n - 1]) for a, b in zip(dec, pro) for x, y in zip(a, b)]
    cnt = sum(int((x != y).sum()) for x, y in d)
    ulp = max(int((np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64)) >> 16).max()) for x, y in d)
    tot = sum(x.size for x, _ in d)
    print(f"int8, skinny route on codes: {cnt} of {tot} decode-written elements differ (max {ulp} ulp)")
    assert all(np.abs(x).max() > 0 for x, _ in d)
    assert cnt <= tot // 100 and ulp <= 2
